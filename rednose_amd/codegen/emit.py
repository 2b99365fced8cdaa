"""Assemble a generated filter library: `{name}.hip` (kernels + C ABI) and `{name}.h` (prototypes).

This is the replacement for the BACK half of the reference's gen_code
(/root/reference/rednose/helpers/ekf_sym.py:118-217).  What is kept from it is the contract:
  * `{name}.h` holds one prototype per line; every reference symbol is there with the reference's
    exact signature -- {name}_update_{kind} (:149), the sympy routine wrappers {name}_f_fun ... (:155-161),
    {name}_predict (:162), {name}_set_{var} (:166-171) -- so `load_code` style loaders keep working;
  * `lib{name}.so` is self-contained and lives beside the header.
What is new: `int {name}_batch_*` entry points over DEVICE pointers (include/rednose_amd_filter.h),
and every symbol, scalar ones included, executes on the GPU.  The C++ plugin hook of the reference
(:186-203: `const EKF {name} = {...}` + `ekf_lib_init` -> `extern "C" void *ekf_get()`, rednose/helpers/ekf.h:14-42)
is emitted too (plugin_text below, templates/ekf_plugin.h), so the reference's `ekf_load_and_register`
(ekf_load.cc:22-39) and through it `EKFSym` can load a rednose_amd library unmodified.

Where things are: emit() -> _library() puts the file together from functions that each return one piece of it -- _select (family, fused run,
smoother and trace structures under the tuning and the fallbacks), _kernels, _routines (the sympy routines and their host wrappers), _rts_model,
_augment_kernel, and the C ABI in file order: _abi_model, _abi_debug, _abi_batched, _abi_tri, _abi_rts, _abi_scalar.  Every exported function is
defined through _Abi.fn, which writes the definition and the prototype of `{name}.h` from ONE signature; the checks every batched entry point
makes in front of its launch are _batched().  The launch texts belong to the kernel emitters (emit_common.launch_*, emit_small / emit_run2 /
emit_wide3 .launch_run, emit_rts4.launch).  This module imports the kernel emitters; emit_small and emit_wide2 ask it for step_kinds() and the
fallbacks in progress and import it where they do (the one cycle among the emitters).
"""
import types

from rednose_amd.codegen import emit_common, emit_rts4, emit_run2, emit_small, emit_wide2, emit_wide3, tuning
from rednose_amd.codegen.emit_common import routine_device_function, NOISE_MODES, TABLE, ENTRY, DIAG
from rednose_amd.codegen.lower import NULLSPACE_RESIDUAL, SINCOS_FAST

SMALL_MAX_E = 7    # lane-per-filter register budget: x, P and the update's temporaries in VGPRs/AGPRs without spilling.  At 8
                   # error states hipcc spills (12 VGPRs in a step kernel, 58 in the fused run) and the fused run's trace came out
                   # wrong for single filters on some runs (tools/stress_run_trace.py); 8 goes to the lane-group kernels


# Fallback structures gen_code may ask for when the first build of a model does not fit the register file (they are arguments
# of ONE emit() call, not process state: nothing about a model survives its gen_code call):
#   force_wide         the lane-per-filter build spilled registers -> lane-group family
#   no_model_defaults  the per-model tuning defaults (two wavefronts per SIMD) spilled -> general structure
#   rts_one_wave       the smoother spilled under the two-wavefronts-per-SIMD budget -> full register file
#   no_rts             the smoother still touches scratch -> library without batch_rts (forward filter unaffected)
#   no_rts4            the smoother with register-broadcast operands (emit_rts4, two wavefronts per SIMD) spilled, or one of its DPP reads follows
#                      the write of its source too closely (build.dpp_hazards) -> rn::k_rts_group
#   no_run_blk         the blocked fused run of a lane-per-filter model (emit_small.run_kernel_blk) spilled -> k_run serves untraced runs too
#   no_tri             one of the packed-triangle trace kernels (k_run2_tri / k_rts4_tri) spilled -> library without batch_run_tri / batch_rts_tri
#   no_run2            the fused run with a scalar wavefront beside the matrix wavefront (emit_run2, two wavefronts per SIMD) spilled -> k_run (emit_wide3)
#   no_run             the fused multi-step run of a model above 32 error states touches scratch -> library without batch_run
#                      (status ERR_UNSUPPORTED, the step-granular entry points cover such models)
#   no_kinds           the mixed-kind step kernel (k_kinds: a kind per filter in one launch) touches scratch memory or spills -> library without
#                      it ({name}_has_step_kinds() == 0, its entry points return ERR_UNSUPPORTED; one `_masked` launch per kind serves such a call)
#   no_run_pf          the fused run with a schedule per filter (k_run_pf / k_run_pf_tr) touches scratch memory or spills -> library without it
#                      ({name}_has_batch_run_pf() == 0, batch_run_pf returns ERR_UNSUPPORTED; BatchedEKF.run_logs walks such logs step by step)
#   no_run_pf_r        the fused run with a schedule per filter and a noise matrix per entry (k_run_rpf / k_run_rpf_tr) touches scratch memory or spills ->
#                      library without it ({name}_has_batch_run_pf_r() == 0, batch_run_pf_r returns ERR_UNSUPPORTED); k_run_pf and everything else stay
#   no_run_pf_rd       the same run with a DIAGONAL noise per entry (k_run_dpf / k_run_dpf_tr) touches scratch memory or spills -> library without it
#                      ({name}_has_batch_run_pf_rd() == 0, batch_run_pf_rd returns ERR_UNSUPPORTED); k_run_pf, k_run_rpf and everything else stay
#   no_run_pf_ea       the fused run with a schedule per filter of an MSCKF model (k_run_epf: extra arguments per entry, a window shift per filter) touches
#                      scratch memory or spills -> library without it ({name}_has_batch_run_pf_ea() == 0, batch_run_pf_ea returns ERR_UNSUPPORTED;
#                      BatchedEKF.run_logs walks such logs step by step)
#   no_rts4_pf         k_rts4_pf (emit_rts4.kernel(pf=True), two wavefronts per SIMD) spilled, or one of its DPP reads follows the write of its source
#                      too closely -> rn::k_rts_group<RtsModel, true> serves batch_rts_pf, as rn::k_rts_group serves batch_rts behind no_rts4
#   no_rts_pf          the smoother with a schedule per filter (the PF = true instantiation of rn::k_rts / rn::k_rts_group) touches scratch memory or
#                      spills -> library without it ({name}_has_batch_rts_pf() == 0, batch_rts_pf returns ERR_UNSUPPORTED); batch_rts and everything else stay
FALLBACKS = ("force_wide", "no_model_defaults", "no_rts4", "rts_one_wave", "no_rts", "no_run2", "no_run", "no_run_blk", "no_tri", "no_kinds") + tuple(
  m.fallback for m in NOISE_MODES) + ("no_rts4_pf", "no_rts_pf", "no_run_pf_ea")
KINDS_MAX = 16      # kinds of a model with a mixed-kind step: the Z table rn::k_timeline_push takes by value
_active = frozenset()      # fallbacks of the emit() call in progress


def family(spec, fallbacks=None):
  """Lane-per-filter kernels up to SMALL_MAX_E error states; lane-group kernels above, and for every MSCKF model
  (the null-space projection of feature-track kinds is emitted for the lane-group family only)."""
  fb = _active if fallbacks is None else fallbacks
  if any(k.He_sym is not None for k in spec.kinds) or "force_wide" in fb:
    return "wide"
  return "small" if spec.dim_err <= min(SMALL_MAX_E, tuning.current().small_max_e) else "wide"


def step_kinds(spec, fallbacks=None):
  """Does this library get the mixed-kind step kernel k_kinds?  Not MSCKF models, and not models with a kind that takes extra arguments or
  keeps its innovation covariance in LDS (emit_wide2.WIDE_Z_LDS): those kinds have per-kind buffers the mixed kernel does not carry."""
  fb = _active if fallbacks is None else fallbacks
  if "no_kinds" in fb or spec.N > 0 or len(spec.kinds) > KINDS_MAX:
    return False
  return all(k.ea_sym is None and k.He_sym is None and k.zdim < emit_wide2.WIDE_Z_LDS and k.kind > 0 for k in spec.kinds)


def has_run_pf(spec, noise, fallbacks=None):
  """Does this library get the fused run with a schedule per filter in this noise flavour (emit_common.NoiseMode; the kernels are
  emit_small.run_pf_kernel's and emit_wide3.run_pf_kernel's)?  Models with a fused run whose kinds take no extra arguments, MSCKF models excepted; the
  per-entry flavours at most where the table's k_run_pf is, and not tied to one another: a row of k_run_dpf is zmax doubles where k_run_rpf's is
  zmax^2.  (Lane-group models whose batch_run is emit_run2's k_run2 get emit_wide3's single-wavefront kernel, with the functions it needs emitted
  beside emit_run2's.)"""
  fb = _active if fallbacks is None else fallbacks
  if noise.fallback in fb or "no_run_pf" in fb or "no_run" in fb or spec.N > 0 or spec.dim_err > 64:
    return False
  return all(k.ea_sym is None and k.He_sym is None and k.kind > 0 for k in spec.kinds)


def has_run_pf_ea(spec, fallbacks=None):
  """Does this library get the fused run with a schedule per filter of MSCKF models (emit_wide3.run_epf_kernel: k_run_epf, with extra arguments
  per entry, the predicated null-space projection and a window shift per filter)?  MSCKF models with a fused run; every other model is served by
  has_run_pf()'s kernels (a model outside the MSCKF family that has a kind with extra arguments takes BatchedEKF.run_logs' step walk)."""
  fb = _active if fallbacks is None else fallbacks
  if "no_run_pf_ea" in fb or "no_run" in fb or spec.N <= 0 or spec.dim_err > 64 or family(spec, fb) != "wide":
    return False
  return all(k.kind > 0 for k in spec.kinds)


def run_pf(spec, fallbacks=None):
  """has_run_pf() of the run with one R per kind (k_run_pf)."""
  return has_run_pf(spec, TABLE, fallbacks)


def run_pf_r(spec, fallbacks=None):
  """has_run_pf() of the run with a noise matrix per entry (k_run_rpf)."""
  return has_run_pf(spec, ENTRY, fallbacks)


def run_pf_rd(spec, fallbacks=None):
  """has_run_pf() of the run with a DIAGONAL noise per entry (k_run_dpf)."""
  return has_run_pf(spec, DIAG, fallbacks)


def rts_pf(spec, fallbacks=None):
  """Does this library get the smoother with a schedule per filter (batch_rts_pf)?  Every model with a smoother and without an MSCKF window, in the
  structure its batch_rts has: rn::k_rts<RtsModel, true> for lane-per-filter models, k_rts4_pf (emit_rts4.kernel(pf=True)) where batch_rts launches
  k_rts4 (fallback no_rts4_pf: rn::k_rts_group's), rn::k_rts_group<RtsModel, true> for the other lane-group models."""
  fb = _active if fallbacks is None else fallbacks
  if "no_rts_pf" in fb or "no_rts" in fb or spec.N > 0 or any(k.He_sym is not None for k in spec.kinds):
    return False
  return spec.dim_main == spec.dim_x and spec.dim_main_err == spec.dim_err and spec.dim_err <= 64


def _align2(n):
  return n + (n & 1)


ea_len = emit_common.ea_count


def ea_req(k):
  return " && ea" if ea_len(k) else ""


def emit(spec, fallbacks=()):
  """-> (header_text, hip_text).  `fallbacks`: see FALLBACKS."""
  global _active      # pylint: disable=global-statement
  assert set(fallbacks) <= set(FALLBACKS), fallbacks
  _active = frozenset(fallbacks)
  try:
    with tuning.using_model(spec, enabled="no_model_defaults" not in _active):
      return _library(spec)
  finally:
    _active = frozenset()


def plugin_text(spec):
  """The reference's plugin descriptor (ekf_sym.py:186-203): name, kinds, feature kinds and the scalar entry points by kind /
  by name, published through ekf_get() and, when the host defines it, ekf_register() at load time (ekf.h:35-42)."""
  name = spec.name
  feat = [k.kind for k in spec.kinds if k.He_sym is not None]
  L = ["", "// ---- C++ plugin hook (/root/reference/rednose/helpers/ekf.h:14-42, emitted by the reference at ekf_sym.py:186-203) ----",
       '#include "ekf_plugin.h"', "namespace {", "const EKF& rn_plugin_descriptor() {", "  static const EKF e = [] {", "    EKF d;",
       f'    d.name = "{name}";', f"    d.kinds = {{ {', '.join(str(k.kind) for k in spec.kinds)} }};",
       f"    d.feature_kinds = {{ {', '.join(str(k) for k in feat)} }};"]
  for fn in ("f_fun", "F_fun", "err_fun", "inv_err_fun", "H_mod_fun", "predict"):
    L.append(f"    d.{fn} = {name}_{fn};")
  for k in spec.kinds:
    L.append(f"    d.hs[{k.kind}] = {name}_h_{k.kind}; d.Hs[{k.kind}] = {name}_H_{k.kind}; d.updates[{k.kind}] = {name}_update_{k.kind};")
  for k in feat:
    L.append(f"    d.Hes[{k}] = {name}_He_{k};")
  for var in spec.global_vars:
    L.append(f'    d.sets["{var.name}"] = {name}_set_{var.name};')
  for r in spec.extra_routines:
    L.append(f'    d.extra_routines["{r[0]}"] = reinterpret_cast<extra_routine_t>({name}_{r[0]});')
  L += ["    return d;", "  }();", "  return e;", "}", "}  // namespace",
        'extern "C" void *ekf_get() { return (void *)&rn_plugin_descriptor(); }',
        "static void __attribute__((constructor)) rn_plugin_register(void) { if (ekf_register) ekf_register(&rn_plugin_descriptor()); }", ""]
  return "\n".join(L)


class _Abi:
  """Part of the `extern "C"` block together with its part of `{name}.h`.  Every exported function goes through fn(): its signature is
  written once, and definition and prototype come out in the same order."""

  def __init__(self, name):
    self.name, self.src, self.hdr = name, [], []

  def fn(self, ret, suffix, params, body):
    """`ret {name}_suffix(params)`.  A body of indented statement lines is set between the braces' lines, anything else beside them."""
    sig = f"{ret}{'' if ret.endswith('*') else ' '}{self.name}_{suffix}({params})"
    self.src.append(f"{sig} {{\n{body}\n}}" if body.startswith("  ") else f"{sig} {{ {body} }}")
    self.hdr.append(sig + ";")

  def text(self, line):
    self.src.append(line)


def _aligned16(ptrs):
  """The 16-byte condition on device pointers (R only where it is per filter: a shared R is read with scalar loads; "R per entry": the
  entry point has no such switch, its R is always per entry)."""
  return " && ".join("(!r_per_filter || rn::aligned16(R))" if p == "R" else f"rn::aligned16({p.split()[0]})" for p in ptrs)


def _batched(require, aligned, launch, require2=None, empty="n == 0", decl="", hip_check=True):
  """Body of a batched entry point: the argument check(s), the empty batch, the alignment check, declarations the launch text needs (the
  `active = nullptr` of the unmasked twins), the launch and its error check (hip_check=False: a library without the kernel, whose `launch`
  is _unsupported(); the line stays, empty)."""
  return "\n".join([f"  RN_REQUIRE({require}, rn::ERR_ARG);"] + ([f"  RN_REQUIRE({require2}, rn::ERR_ARG);"] if require2 else []) +
                   [f"  if ({empty}) return rn::OK;"] + ([f"  RN_REQUIRE({_aligned16(aligned)}, rn::ERR_ALIGN);"] if aligned else []) +
                   [decl + launch, "  " + ("RN_HIP(hipGetLastError());" if hip_check else ""), "  return rn::OK;"])


# launch geometry of the runtime's bookkeeping kernels: a thread per filter; a wavefront per filter
GRID_256 = "dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, (hipStream_t)stream"
GRID_PUSH = "dim3((unsigned)((n + 3) / 4 < 16384 ? (n + 3) / 4 : 16384)), dim3(256), 0, (hipStream_t)stream"
# parameters of batch_run / batch_run_tri and of batch_rts / batch_rts_tri
RUN_PARAMS = ("double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, "
              "uint8_t *flags, double *trace_x, double *trace_P, const double *ea, const int32_t *augment, void *stream")
RUN_PF_PARAMS = ("double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, "
                 "uint8_t *flags, double *trace_x, double *trace_P, void *stream")
RUN_PF_EA_PARAMS = RUN_PF_PARAMS.replace("void *stream", "const double *ea, const int32_t *augment, void *stream")
RTS_PF_PARAMS = ("const double *xf, const double *Pf, const double *dts, const uint8_t *act, int64_t T, const double *Q, int64_t n, int norm_quats, double *xs, "
                 "double *Ps, const double *x_last, const double *P_last, void *stream")
RTS_PARAMS = ("const double *xf, const double *Pf, const double *ts, int64_t T, const double *Q, int64_t n, int norm_quats, double *xs, double *Ps, "
              "const double *x_last, const double *P_last, void *stream")


def _run_body(launch, hip_check=True, r_per_entry=False, ea=False):
  """r_per_entry: R is (T, n, zmax^2) (batch_run_pf_r) or (T, n, zmax) (batch_run_pf_rd), read by the lanes and 16-byte aligned like x, P and z.
  ea: the extra arguments are required (batch_run_pf_ea)."""
  return _batched("n >= 0 && T >= 0 && x && P && Q && kinds && dts && z && R" + (" && ea" if ea else ""), ["x", "P", "z", "trace_x", "trace_P"] + (["R per entry"] if r_per_entry else []),
                  launch, empty="n == 0 || T == 0", hip_check=hip_check)


def _unsupported(why, unused=""):
  return f'  {unused}return rn::fail(rn::ERR_UNSUPPORTED, 0, "{why}", __LINE__);'


def _select(spec):
  """What this library is made of (family, tuning and the fallbacks of the emit() call in progress) -> namespace:
    fam       "small" / "wide";  step: the module whose launch_predict / launch_step / launch_step_ckpt / launch_kinds / launch_maha serve it
    has_run   fused multi-step run (rows of P stay in VGPRs; emit_wide3: several rows per lane up to 32 error states, one above);
              use_run2: as two wavefronts per tile (emit_run2)
    has_rts   smoother.  Lane-per-filter models: rn::k_rts (state and covariance of a filter in one lane's registers).  Lane-group models: k_rts4
              (use_rts4; emit_rts4: 8 .. 22 error states) or rn::k_rts_group (MSCKF models -- their main block is smoothed, ekf_sym.py:675-686 --,
              larger models, and the fallback of k_rts4)
    use_tri   packed-triangle trace: both structures or neither (batch_run_tri writes what batch_rts_tri reads)
    has_kinds the mixed-kind step kernel k_kinds  (the fused runs with a schedule per filter: has_run_pf(spec, noise), asked where they are emitted)"""
  if spec.dim_err > 64:
    raise NotImplementedError(f"{spec.dim_err} error states: the lane-group kernels hold one row of P per lane of a wavefront (<= 64)")
  tune = tuning.current()
  s = types.SimpleNamespace(fam=family(spec), has_run="no_run" not in _active, has_kinds=step_kinds(spec))
  wide = s.fam == "wide"
  s.step = emit_wide2 if wide else emit_small
  s.use_run2 = wide and s.has_run and tune.run2 and "no_run2" not in _active and emit_run2.applicable(spec)
  s.use_rts4 = wide and emit_rts4.applicable(spec) and tune.rts4 and "no_rts4" not in _active and "no_rts" not in _active
  s.use_tri = bool(s.use_run2 and s.use_rts4 and emit_run2.tri_trace(spec) and "no_tri" not in _active)
  s.has_rts = (wide or (spec.dim_main == spec.dim_x and spec.dim_main_err == spec.dim_err)) and "no_rts" not in _active
  s.use_rts4_pf = bool(s.use_rts4 and s.has_rts and rts_pf(spec) and "no_rts4_pf" not in _active)
  return s


def _kernels(spec, s):
  """The family's kernels.  Lane-group models: step-granular kernels in the three-phase structure (emit_wide2), the fused multi-step run with
  the state resident in registers (emit_wide3; emit_run2 beside it where it applies), the smoother's kernels of emit_rts4."""
  if s.fam == "small":
    return [emit_small.kernels(spec) + "\n" + emit_small.maha_kernels(spec)]
  parts = [emit_wide2.kernels(spec)]
  if s.has_run:
    parts.append(emit_wide3.kernels(spec, with_run=not s.use_run2))
    if s.use_run2:
      parts.append(emit_run2.kernels(spec, tri=s.use_tri))
  parts.append(emit_wide2.maha_kernels(spec))
  return (["\n".join(parts)] + ([emit_rts4.kernel(spec)] if s.use_rts4 else []) + ([emit_rts4.kernel(spec, tri=True)] if s.use_tri else []) +
          ([emit_rts4.kernel(spec, pf=True)] if s.use_rts4_pf else []))


def _routines(spec):
  """The reference's per-routine functions (scalar ABI + used by the smoother) -> (device text, their host wrappers).
  A wrapper packs its arguments into the pinned staging buffer; one single-thread launch works on it in place; the output is unpacked."""
  dev, a = [], _Abi(spec.name)
  for r in spec.routines():
    text, params, n_out = routine_device_function(r)
    dev.append(text)
    ptr_params = [(n, sz) for kind, n, sz in params if kind == "ptr"]
    c_sig = ", ".join((f"double *{n}" if kind == "ptr" else f"double {n}") for kind, n, _ in params)
    k_sig = ", ".join((f"const double* {n}" if kind == "ptr" else f"double {n}") for kind, n, _ in params)
    call = ", ".join(n for _, n, _ in params)
    dev.append(f"__global__ void k_fn_{r.name}({k_sig}, double* out) {{ {r.name}({call}, out); }}")
    offs, cur = {}, 0
    for n, sz in ptr_params:
      offs[n] = cur
      cur += _align2(sz)
    kargs = ", ".join((f"s.dev + {offs[n]}" if kind == "ptr" else n) for kind, n, _ in params)
    a.fn("void", r.name, f"{c_sig}, double *out", "\n".join(
      ["  rn::Scratch& s = rn::scratch();", "  std::lock_guard<std::mutex> hold(s.mu);", f"  if (s.ensure({cur + _align2(n_out)}) != rn::OK) return;"] +
      [f"  s.put({offs[n]}, {n}, {sz});" for n, sz in ptr_params if not n.startswith("unused")] +
      [f"  hipLaunchKernelGGL(k_fn_{r.name}, dim3(1), dim3(1), 0, 0, {kargs}, s.dev + {cur});",
       f"  if (s.wait(\"{r.name}\", __LINE__) != rn::OK) return;", f"  s.get(out, {cur}, {n_out});"]))
  return dev, a


def _rts_model(spec, s):
  """The adapter handed to the hand-written smoother kernels."""
  D, E, M = spec.dim_x, spec.dim_err, spec.dim_main_err
  quat = "".join(f" rn::normalize_quat<{D}>(x, {q});" for q in spec.quaternion_idxs)
  grp = f"""
  // lane-group smoother (k_rts_group): slot layout and phase functions of the three-phase step kernels
  static constexpr int DM = {spec.dim_main};
  static constexpr int EM = {M};
  static constexpr int SLOT = ::SLOT;
  static constexpr int OFF_X = SLOT_OFF_X;
  static constexpr int OFF_DT = SLOT_OFF_DT;
  static __device__ __forceinline__ void scal(const double* xin, double dt, double* sl, int norm) {{ scal_predict(xin, dt, sl, norm); }}
  static constexpr int WAVES = {2 if (M <= 22 and "rts_one_wave" not in _active) else 1};       // wavefronts per SIMD the register budget is set for (see k_rts_group)
  static __device__ __forceinline__ void mat_predict(const double (&row)[{M}], double* sB, const double* gQc, const double* sl, int cc, bool act,
                                                     double (&y)[{M}]) {{ mat_predict_rts(row, sB, gQc, sl, cc, act, y); }}""" if s.fam == "wide" else ""
  return f"""
// adapter handed to the hand-written smoother kernels (templates/ekf_hip_rts.h)
struct RtsModel {{
  static constexpr int D = {D};
  static constexpr int E = {E};
  static constexpr bool ID0 = {'true' if emit_rts4.dt0_path(spec) else 'false'};      // predict(dt = 0) is the identity: such steps take Ck = I (ekf_hip_rts.h)
  static __device__ __forceinline__ void f(const double* x, double dt, double* out) {{ f_fun(x, dt, out); }}
  static __device__ __forceinline__ void F(const double* x, double dt, double* out) {{ F_fun(x, dt, out); }}
  static __device__ __forceinline__ void err(const double* nom, const double* delta, double* out) {{ err_fun(nom, delta, out); }}
  static __device__ __forceinline__ void inv_err(const double* nom, const double* tru, double* out) {{ inv_err_fun(nom, tru, out); }}
  static __device__ __forceinline__ void normalize(double (&x)[{D}]) {{{quat} (void)x; }}
{grp}
}};
"""


def _augment_kernel(spec):
  D, E, EE = spec.dim_x, spec.dim_err, spec.dim_err * spec.dim_err
  d1, d2, d3, d4 = spec.dim_main, spec.dim_main_err, spec.dim_augment, spec.dim_augment_err
  return f"""
// ---- MSCKF window shift (/root/reference/rednose/helpers/ekf_sym.py:365-391): the oldest augmented state drops out, the
// first {d3} main states become the newest one; P follows with rows/columns [{d2}, {d2 + d4}) deleted and the first {d4}
// re-appended.  One wavefront per filter, state staged through LDS (the permutation reads what it overwrites).
__device__ __forceinline__ int aug_src_err(int i) {{
  const int r = i < {E - d4} ? i : i - {E - d4};
  return r < {d2} ? r : r + {d4};
}}
__global__ __launch_bounds__(64) void k_augment(double* __restrict__ gx, double* __restrict__ gP, const int64_t n) {{
  __shared__ double s_P[{EE}];
  __shared__ double s_x[{D}];
  const int lane = threadIdx.x;
  for (int64_t f = blockIdx.x; f < n; f += gridDim.x) {{
    for (int i = lane; i < {D}; i += 64) s_x[i] = gx[f * {D} + i];
    for (int i = lane; i < {EE}; i += 64) s_P[i] = gP[f * {EE} + i];
    rn::wave_lds_sync();
    for (int i = lane; i < {D}; i += 64) {{
      const int src = i < {d1} ? i : (i < {D - d3} ? i + {d3} : i - {D - d3});
      gx[f * {D} + i] = s_x[src];
    }}
    for (int i = lane; i < {EE}; i += 64) {{
      const int r = i / {E}, c = i % {E};
      gP[f * {EE} + i] = s_P[aug_src_err(r) * {E} + aug_src_err(c)];
    }}
    rn::wave_lds_sync();
  }}
}}
// ---- the same shift for the filters with active[f] != 0 (active == nullptr: every filter); the others are neither read nor written ----
__global__ __launch_bounds__(64) void k_augment_m(double* __restrict__ gx, double* __restrict__ gP, const uint8_t* __restrict__ active, const int64_t n) {{
  __shared__ double s_P[{EE}];
  __shared__ double s_x[{D}];
  const int lane = threadIdx.x;
  for (int64_t f = blockIdx.x; f < n; f += gridDim.x) {{
    if (active != nullptr && active[f] == 0) continue;      // (uniform over the workgroup)
    for (int i = lane; i < {D}; i += 64) s_x[i] = gx[f * {D} + i];
    for (int i = lane; i < {EE}; i += 64) s_P[i] = gP[f * {EE} + i];
    rn::wave_lds_sync();
    for (int i = lane; i < {D}; i += 64) {{
      const int src = i < {d1} ? i : (i < {D - d3} ? i + {d3} : i - {D - d3});
      gx[f * {D} + i] = s_x[src];
    }}
    for (int i = lane; i < {EE}; i += 64) {{
      const int r = i / {E}, c = i % {E};
      gP[f * {EE} + i] = s_P[aug_src_err(r) * {E} + aug_src_err(c)];
    }}
    rn::wave_lds_sync();
  }}
}}
"""


def _switch(spec, value):
  return "switch (kind) { " + " ".join(f"case {k.kind}: return {value(k)};" for k in spec.kinds) + " default: return -1; }"


def _abi_model(spec):
  """What a caller asks a library about its model, the error state, and the setters of the model's run-time scalars."""
  a = _Abi(spec.name)
  a.fn("void", "dims", "int *dims", f"dims[0] = {spec.dim_x}; dims[1] = {spec.dim_err}; dims[2] = {spec.dim_main_err};")
  a.fn("int", "kind_zdim", "int kind", _switch(spec, lambda k: k.zdim))
  a.fn("int", "kind_maha", "int kind", _switch(spec, lambda k: int(k.maha_test)))
  a.fn("int", "num_kinds", "void", f"return {len(spec.kinds)};")
  a.fn("void", "kinds", "int *out", " ".join(f"out[{i}] = {k.kind};" for i, k in enumerate(spec.kinds)))
  a.fn("int", "last_error", "void", "return rn::err().code;")
  a.fn("const char *", "last_error_string", "void", "return rn::err().msg;")
  a.fn("void", "clear_error", "void", "rn::err() = rn::ErrorState();")
  a.text("")
  for var in spec.global_vars:
    a.fn("void", f"set_{var.name}", "double x", f"""  if (hipMemcpyToSymbol(HIP_SYMBOL({var.name}), &x, sizeof(double), 0, hipMemcpyHostToDevice) != hipSuccess)
    rn::fail(rn::ERR_HIP, (int)hipGetLastError(), "{spec.name}_set_{var.name}", __LINE__);""")
  return a


def _abi_debug(spec, s):
  """Read-back of the debug timelines (tuning knobs small_timeline / wide_timeline; tools/timeline.py)."""
  a = _Abi(spec.name)

  def read_back(suffix, symbol, count):
    a.fn("int", suffix, "unsigned long long *out", f"""  RN_HIP(hipDeviceSynchronize());
  RN_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL({symbol}), sizeof(unsigned long long) * {count}, 0, hipMemcpyDeviceToHost));
  return rn::OK;""")
  if s.fam == "small" and tuning.current().small_timeline:      # 256 workgroups x 8 slots x (shader cycles, 100 MHz wall clock)
    read_back("debug_timeline", "g_tl", "256 * 8 * 2")
  if s.fam == "wide" and tuning.current().wide_timeline:
    read_back("debug_timeline", "g_tl", "256 * 64 * 2")
    read_back("debug_rts_timeline", "rn::g_rts_tl", "256 * 16")
    read_back("debug_blocks", "g_tlb", "4096 * 2")
  return a


def _abi_batched(spec, s):
  """The batched entry points over device pointers, up to the fused run."""
  name, a = spec.name, _Abi(spec.name)
  zmax = max(k.zdim for k in spec.kinds)
  # Every step-granular entry point exists twice: plain, and `_masked` with a per-filter `active` byte (0 = this filter has no
  # observation in this call: its x, P and z pass through untouched and flag bit 4 is set) -- what a batch of filters on
  # INDEPENDENT timelines needs (each filter of the reference is its own instance with its own filter_time, ekf_sym.cc:83-117);
  # together with the per-filter dt vector a call then advances exactly the filters that have something to do.
  predict = "const double *Q, const double *dt_vec, double dt, "
  obs = "double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, "
  no_mask = "  const uint8_t *active = nullptr;\n"
  for sfx, act_param, decl in (("", "", no_mask), ("_masked", "const uint8_t *active, ", "")):
    a.fn("int", f"batch_predict{sfx}", f"double *x, double *P, {predict}int64_t n, int norm_quats, {act_param}void *stream",
         _batched("n >= 0 && x && P && Q", ["x", "P"], s.step.launch_predict(), decl=decl))
    for k in spec.kinds:
      a.fn("int", f"batch_update_{k.kind}{sfx}", f"double *x, double *P, {obs}{act_param}void *stream",
           _batched(f"n >= 0 && x && P && z && R{ea_req(k)}", ["x", "P", "z", "R"], s.step.launch_step(k.kind, False), decl=decl))
      a.fn("int", f"batch_predict_update_{k.kind}{sfx}", f"double *x, double *P, {predict}{obs}{act_param}void *stream",
           _batched(f"n >= 0 && x && P && Q && z && R{ea_req(k)}", ["x", "P", "z", "R"], s.step.launch_step(k.kind, True), decl=decl))

  # the fused step that also writes the call's checkpoint (k_stepc_{kind}): what a rewind ring keeps of a call -- the observations as they came and the
  # filtered pair (ekf_sym.cc:142-156, 191) -- leaves with the step's own stores instead of three copies behind it
  for k in spec.kinds:
    a.fn("int", f"batch_predict_update_{k.kind}_ckpt", f"double *x, double *P, {predict}{obs}double *ckpt_x, double *ckpt_P, double *ckpt_z, void *stream",
         _batched(f"n >= 0 && x && P && Q && z && R && ckpt_x && ckpt_P && ckpt_z{ea_req(k)}", ["x", "P", "z", "R", "ckpt_x", "ckpt_P", "ckpt_z"],
                  s.step.launch_step_ckpt(k.kind), require2="ckpt_x != x && ckpt_P != P && ckpt_z != z", decl=no_mask))

  a.fn("int", "batch_ring_copy", "double *ring, int64_t ring_stride, double *flat, int64_t flat_stride, int64_t rec, const int32_t *slot, const uint8_t *active, "
       "int64_t n, int to_ring, void *stream",
       _batched("n >= 0 && rec >= 0 && rec <= ring_stride && rec <= flat_stride && ring && flat && slot", [], empty="n == 0 || rec == 0", launch=(
         "  hipLaunchKernelGGL(rn::k_ring_copy, dim3((unsigned)(n < 65536 ? n : 65536)), dim3(64), 0, (hipStream_t)stream, "
         "ring, ring_stride, flat, flat_stride, rec, slot, active, n, to_ring);")))
  a.fn("int", "batch_flags_set", "uint8_t *flags, const uint8_t *mask, int value, int64_t n, void *stream",
       _batched("n >= 0 && flags && mask", [], f"  hipLaunchKernelGGL(rn::k_flags_set, {GRID_256}, flags, mask, value, n);"))

  # per-filter timelines with the in-order bookkeeping on the device (rn::k_timeline_plan / k_timeline_push, include/rednose_amd_filter.h):
  # what every filter does in this call before the step, the call's checkpoint behind it
  a.fn("int", "batch_timeline_plan", "const double *t, const uint8_t *active, const double *ft, int64_t n, double *dt_out, uint8_t *act_out, uint8_t *late_out, "
       "int32_t *n_late, const double *z_src, double *z_keep, int64_t z_count, void *stream",
       _batched("n >= 0 && t && ft && dt_out && act_out && late_out && n_late", [], require2="z_count >= 0 && (z_keep == nullptr || z_count == 0 || (z_src != nullptr && z_src != z_keep))",
                launch=f"""  hipLaunchKernelGGL(rn::k_timeline_plan, {GRID_256},
                     t, active, ft, n, dt_out, act_out, late_out, n_late, z_src, z_count > 0 ? z_keep : nullptr, z_count);"""))
  push = ("const double *t, const uint8_t *act, double *ft, const double *x, const double *P, int64_t n, int64_t K, int64_t nmax, "
          "double *ring_t, double *ring_x, double *ring_P, int32_t *ring_kind, int32_t *ring_nobs, double *ring_z, double *ring_R, double *ring_ea, "
          "int64_t *ring_head, int64_t *ring_length, ")
  ring = "rn::TimelineRing{K, nmax, ring_t, ring_x, ring_P, ring_kind, ring_nobs, ring_z, ring_R, ring_ea, ring_head, ring_length}"
  rings = "ring_t && ring_x && ring_P && ring_kind && ring_nobs && ring_z && ring_R && ring_ea && ring_head && ring_length"
  eamax = max([ea_len(k) for k in spec.kinds] + [1])
  sizes = f"{spec.dim_x}, {spec.dim_err * spec.dim_err}"
  tl_ea = " ".join(f"case {k.kind}: EA = {ea_len(k)}; break;" for k in spec.kinds)
  a.fn("int", "batch_timeline_push", push + "int kind, int nobs, const double *z_obs, int64_t z_stride_f, int64_t z_stride_o, "
       "const double *R, int r_per_filter, int64_t r_stride_f, int64_t r_stride_o, const double *ea, int64_t ea_stride_f, int64_t ea_stride_o, "
       "void *stream", f"""  RN_REQUIRE(n >= 0 && K >= 0 && t && act && ft, rn::ERR_ARG);
  const int Z = {name}_kind_zdim(kind);
  int EA = -1;
  switch (kind) {{ {tl_ea} default: break; }}
  rn::TimelineRing r{{}};
  rn::TimelineObs o{{}};
  if (K > 0) {{
    RN_REQUIRE(Z > 0 && EA >= 0 && nmax >= 1 && nobs >= 1 && nobs <= nmax, rn::ERR_ARG);
    RN_REQUIRE(x && P && {rings}, rn::ERR_ARG);
    RN_REQUIRE(z_obs && R && (EA == 0 || ea) && z_stride_f >= 0 && z_stride_o >= 0 && r_stride_f >= 0 && r_stride_o >= 0 && ea_stride_f >= 0 && ea_stride_o >= 0, rn::ERR_ARG);
    r = {ring};
    o = rn::TimelineObs{{z_obs, R, ea, z_stride_f, z_stride_o, r_per_filter ? r_stride_f : 0, r_stride_o, ea_stride_f, ea_stride_o}};
  }}
  if (n == 0) return rn::OK;
  hipLaunchKernelGGL(rn::k_timeline_push, {GRID_PUSH},
                     t, act, ft, x, P, n, {sizes}, r, kind, nobs, Z, EA, {zmax}, {eamax}, o, rn::TimelineKinds{{}});
  RN_HIP(hipGetLastError());
  return rn::OK;""")

  # A kind per filter in one launch (k_kinds): the step of a call on per-filter timelines in which the filters bring different kinds, and the
  # checkpoint of such a call.  The symbols exist in every library; without the kernel they return ERR_UNSUPPORTED.
  a.fn("int", "has_step_kinds", "void", f"return {int(s.has_kinds)};")
  no_kinds = _unsupported("mixed-kind step: not generated for this model (MSCKF model, a kind with extra arguments or a wide "
                          "observation, or the kernel did not fit the register file)")
  mixed = "const int32_t *kinds, double *z, const double *R, int r_per_filter, "
  step_tail = "int64_t n, int norm_quats, uint8_t *flags, const uint8_t *active, void *stream"
  for sym, params, req, do_p in (("batch_predict_update_kinds", f"double *x, double *P, {predict}{mixed}{step_tail}", "x && P && Q && kinds && z && R", True),
                                 ("batch_update_kinds", f"double *x, double *P, {mixed}{step_tail}", "x && P && kinds && z && R", False)):
    a.fn("int", sym, params, _batched(f"n >= 0 && {req}", ["x", "P", "z", "R"], s.step.launch_kinds(do_p)) if s.has_kinds else no_kinds)
  tab = ", ".join(f"{{{k.kind}, {k.zdim}}}" for k in spec.kinds)
  a.fn("int", "batch_timeline_push_kinds", push + "const int32_t *kinds, const double *z_obs, const double *R, int r_per_filter, void *stream",
       f"""  RN_REQUIRE(n >= 0 && K >= 0 && t && act && ft && kinds, rn::ERR_ARG);
  rn::TimelineRing r{{}};
  rn::TimelineObs o{{}};
  if (K > 0) {{
    RN_REQUIRE(nmax >= 1 && x && P && {rings} && z_obs && R, rn::ERR_ARG);
    r = {ring};
    o = rn::TimelineObs{{z_obs, R, nullptr, {zmax}, 0, r_per_filter ? {zmax * zmax} : 0, 0, 0, 0}};
  }}
  if (n == 0) return rn::OK;
  const rn::TimelineKinds tk{{kinds, {len(spec.kinds)}, {{{tab}}}}};
  hipLaunchKernelGGL(rn::k_timeline_push, {GRID_PUSH},
                     t, act, ft, x, P, n, {sizes}, r, 0, 1, 0, 0, {zmax}, {eamax}, o, tk);
  RN_HIP(hipGetLastError());
  return rn::OK;""" if s.has_kinds else no_kinds)

  # The late observation of per-filter timelines on the device (rn::k_rewind_locate / k_rewind_fetch, include/rednose_amd_filter.h): the rewind of
  # every late filter in its own ring, then one replay position of all rewound filters gathered into the buffers of the mixed-kind step
  rw_ring = "rn::RewindRing{{K, {nmax}, ring_t, {x}, {P}, {kind}, {z}, {R}, {head}, {length}}}"
  a.fn("int", "batch_rewind_locate", "const uint8_t *late, const double *t, int64_t n, int64_t K, double *ring_t, double *ring_x, double *ring_P, "
       "int64_t *ring_head, int64_t *ring_length, double max_rewind_age, double *x, double *P, double *ft, double *dt_out, uint8_t *act_out, "
       "int32_t *rep_slot, int32_t *rep_n, uint8_t *drop_out, int32_t *counts, void *stream",
       _batched("n >= 0 && K >= 1 && late && t && ring_t && ring_x && ring_P && ring_head && ring_length", [],
                require2="x && P && ft && dt_out && act_out && rep_slot && rep_n && drop_out && counts",
                launch=f"""  hipLaunchKernelGGL(rn::k_rewind_locate, {GRID_PUSH},
                     late, t, n, {sizes}, {rw_ring.format(nmax=1, x="ring_x", P="ring_P", kind="nullptr", z="nullptr", R="nullptr", head="ring_head", length="ring_length")}, max_rewind_age,
                     x, P, ft, dt_out, act_out, rep_slot, rep_n, drop_out, counts);"""))
  if len(spec.kinds) <= KINDS_MAX:
    fetch = f"""  const rn::TimelineKinds tk{{nullptr, {len(spec.kinds)}, {{{tab}}}}};
  hipLaunchKernelGGL(rn::k_rewind_fetch, {GRID_PUSH},
                     rep_slot, rep_n, q, t_prev, n, {rw_ring.format(nmax="nmax", x="nullptr", P="nullptr", kind="ring_kind", z="ring_z", R="ring_R", head="nullptr", length="nullptr")}, {zmax}, tk,
                     t_out, dt_out, kinds_out, act_out, z_out, z_keep, R_out);"""
  else:
    fetch = _unsupported(f"batch_rewind_fetch: the model has more than {KINDS_MAX} kinds", unused="(void)stream; ")
  a.fn("int", "batch_rewind_fetch", "const int32_t *rep_slot, const int32_t *rep_n, int64_t q, const double *t_prev, int64_t n, int64_t K, int64_t nmax, "
       "double *ring_t, int32_t *ring_kind, double *ring_z, double *ring_R, double *t_out, double *dt_out, int32_t *kinds_out, uint8_t *act_out, "
       "double *z_out, double *z_keep, double *R_out, void *stream",
       _batched("n >= 0 && K >= 1 && nmax >= 1 && q >= 0 && rep_slot && rep_n && t_prev && ring_t && ring_kind && ring_z && ring_R", [],
                require2="t_out && dt_out && kinds_out && act_out && z_out && z_keep && R_out", launch=fetch, hip_check=len(spec.kinds) <= KINDS_MAX))

  for k in spec.kinds:
    a.fn("int", f"batch_maha_{k.kind}", "const double *x, const double *P, const double *z, const double *R, int r_per_filter, const double *ea, int64_t n, double *d2, void *stream",
         _batched(f"n >= 0 && x && P && z && R && d2{ea_req(k)}", ["x", "P", "z", "R"], s.step.launch_maha(k.kind)))
  if spec.N > 0:
    a.fn("int", "batch_augment", "double *x, double *P, int64_t n, void *stream",
         _batched("n >= 0 && x && P", [], "  hipLaunchKernelGGL(k_augment, dim3(rn::grid_for_tiles(n)), dim3(64), 0, (hipStream_t)stream, x, P, n);"))
    a.fn("int", "batch_augment_masked", "double *x, double *P, const uint8_t *active, int64_t n, void *stream",
         _batched("n >= 0 && x && P", [], "  hipLaunchKernelGGL(k_augment_m, dim3(rn::grid_for_tiles(n)), dim3(64), 0, (hipStream_t)stream, x, P, active, n);"))
  a.fn("void", "msckf_dims", "int *dims",
       f"dims[0] = {spec.dim_main}; dims[1] = {spec.dim_main_err}; dims[2] = {spec.dim_augment}; dims[3] = {spec.dim_augment_err}; dims[4] = {spec.N};")
  a.fn("int", "kind_eadim", "int kind", _switch(spec, ea_len))
  a.fn("int", "zmax", "void", f"return {zmax};")
  # steps per loop iteration of the kernel an untraced batch_run launches (instruction accounting of bench.py)
  unroll = (emit_small.run_block(spec) or emit_small.run_unroll(spec)) if s.fam == "small" else 1
  a.fn("int", "run_unroll", "void", f"return {unroll};")
  # 0: this model's fused multi-step kernel did not fit the register file (fallback no_run) -- {name}_batch_run returns ERR_UNSUPPORTED
  # and callers walk a schedule with the step-granular entry points (BatchedEKF.run does)
  a.fn("int", "has_batch_run", "void", f"return {int(s.has_run)};")
  # 1: predict(dt = 0) is the identity on (x, P) for this model, symbolically (FilterSpec.identity_at_dt0) -- a batch_run step with dt = 0 is
  # then an update alone, which is how the orchestrators serve the n observations of ONE predict_and_update_batch call (the reference predicts
  # once and updates n times, ekf_sym.cc:172-180) in one launch; 0: they issue batch_update_k launches instead
  a.fn("int", "predict_identity_at_dt0", "void", f"return {int(spec.identity_at_dt0())};")
  if not s.has_run:
    launch = _unsupported("batch_run: not generated for this model (its fused run did not fit the register file)",
                          unused="(void)norm_quats; (void)flags; (void)stream; (void)ea; (void)augment; ")
  else:
    launch = emit_small.launch_run(spec) if s.fam == "small" else (emit_run2.launch_run() if s.use_run2 else emit_wide3.launch_run())
  a.fn("int", "batch_run", RUN_PARAMS, _run_body(launch, hip_check=s.has_run))
  # The fused run with a schedule per filter (k_run_pf): kinds (T, n), dts (T, n), R the per-kind table of batch_predict_update_kinds.  The
  # symbols exist in every library; without the kernel batch_run_pf returns ERR_UNSUPPORTED.  The same run with a noise matrix per entry
  # (batch_run_pf_r, k_run_rpf): R (T, n, zmax^2), row (t, i) the `r_per_filter != 0` row of filter i in step t; with a diagonal noise per entry
  # (batch_run_pf_rd, k_run_dpf): R (T, n, zmax), the leading Z doubles of row (t, i) the variances of filter i's entry t.
  for noise in NOISE_MODES:
    has, sym = has_run_pf(spec, noise), f"batch_run_pf{noise.sfx}"
    a.fn("int", f"has_{sym}", "void", f"return {int(has)};")
    launch = (emit_small if s.fam == "small" else emit_wide3).launch_run_pf(noise)
    a.fn("int", sym, RUN_PF_PARAMS, _run_body(launch, r_per_entry=noise.per_entry) if has else _unsupported(
      f"{sym}: not generated for this model (MSCKF model, a kind with extra arguments, no fused run, or the kernel did not fit the register file)"))
  # The same run for MSCKF models (k_run_epf): batch_run_pf with `ea` (T, n, EA), EA the largest kind_eadim, and `augment` (T, n) or NULL -- a
  # window shift of filter i after its entry t.  The symbols exist in every library; without the kernel batch_run_pf_ea returns ERR_UNSUPPORTED.
  has = has_run_pf_ea(spec)
  a.fn("int", "has_batch_run_pf_ea", "void", f"return {int(has)};")
  a.fn("int", "batch_run_pf_ea", RUN_PF_EA_PARAMS, _run_body(emit_wide3.launch_run_epf(), ea=True) if has else _unsupported(
    "batch_run_pf_ea: not generated for this model (not an MSCKF model, no fused run, or the kernel did not fit the register file)"))
  return a


def _abi_tri(spec, s):
  """Packed-triangle trace (opt-in; models with k_run2 AND k_rts4): batch_run_tri writes the lower triangle of every filtered covariance
  (row-major, E (E + 1) / 2 doubles) where batch_run writes E^2, batch_rts_tri (_abi_rts) smooths such a trace into packed smoothed covariances; the
  fused run's covariance is symmetric by contract and batch_rts reads lower triangles only (include/rednose_amd_filter.h), so nothing is lost."""
  a = _Abi(spec.name)
  a.fn("int", "has_tri_trace", "void", f"return {int(s.use_tri)};")
  if s.use_tri:
    a.fn("int", "batch_run_tri", RUN_PARAMS, _run_body(emit_run2.launch_run(tri=True)))
    for suffix, params, kernel, args in (("batch_tri_unpack", "const double *tri, double *full", "k_tri_unpack", "tri, full"),
                                         ("batch_tri_pack", "const double *full, double *tri", "k_tri_pack", "full, tri")):
      a.fn("int", suffix, params + ", int64_t count, void *stream", _batched("count >= 0 && tri && full", [], empty="count == 0", launch=(
        f"  hipLaunchKernelGGL(rn::{kernel}<{spec.dim_err}>, dim3(8192), dim3(256), 0, (hipStream_t)stream, {args}, count);")))
  return a


def _abi_rts(spec, s):
  """The smoother: batch_rts, and batch_rts_tri on a packed-triangle trace."""
  a = _Abi(spec.name)

  def rts(suffix, launch):
    a.fn("int", suffix, RTS_PARAMS, _batched("n >= 0 && T >= 0 && xf && Pf && ts && Q && xs && Ps", ["xf", "Pf", "xs", "Ps", "x_last", "P_last"], launch,
                                             empty="n == 0 || T == 0"))
  if s.has_rts:
    if s.use_rts4:
      launch = emit_rts4.launch(spec)
    else:
      M = spec.dim_main_err
      fpw = (64 // (16 if M <= 16 else (32 if M <= 32 else 64))) if s.fam == "wide" else 2      # filters per wavefront
      tiles = f"(n + {fpw - 1}) / {fpw}"
      launch = f"""  const int64_t tiles = {tiles};
  hipLaunchKernelGGL(rn::{'k_rts_group' if s.fam == 'wide' else 'k_rts'}<RtsModel>, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     xf, Pf, ts, T, Q, n, norm_quats, xs, Ps, x_last, P_last);"""
    rts("batch_rts", launch)
    if s.use_tri:
      rts("batch_rts_tri", emit_rts4.launch(spec, tri=True))
  # The smoother with a schedule per filter: dts (T, n) and act (T, n) in place of ts (T).  The symbols exist in every library; without the
  # kernel batch_rts_pf returns ERR_UNSUPPORTED.  The kernel has the structure of the library's batch_rts: k_rts4_pf beside k_rts4, else the
  # PF = true instantiation of the hand-written smoother of the model's family (templates/ekf_hip_rts.h).
  has = s.has_rts and rts_pf(spec)
  a.fn("int", "has_batch_rts_pf", "void", f"return {int(has)};")
  if has and s.use_rts4_pf:
    body = _batched("n >= 0 && T >= 0 && xf && Pf && dts && act && Q && xs && Ps", ["xf", "Pf", "xs", "Ps", "x_last", "P_last"], emit_rts4.launch_pf(), empty="n == 0 || T == 0")
  elif has:
    M = spec.dim_main_err
    fpw = (64 // (16 if M <= 16 else (32 if M <= 32 else 64))) if s.fam == "wide" else 2      # filters per wavefront
    launch = f"""  const int64_t tiles = (n + {fpw - 1}) / {fpw};
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rn::{'k_rts_group' if s.fam == 'wide' else 'k_rts'}<RtsModel, true>), dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     xf, Pf, dts, T, Q, n, norm_quats, xs, Ps, x_last, P_last, act);"""
    body = _batched("n >= 0 && T >= 0 && xf && Pf && dts && act && Q && xs && Ps", ["xf", "Pf", "xs", "Ps", "x_last", "P_last"], launch, empty="n == 0 || T == 0")
  else:
    body = _unsupported("batch_rts_pf: not generated for this model (MSCKF model, no smoother, or the kernel did not fit the register file)")
  a.fn("int", "batch_rts_pf", RTS_PF_PARAMS, body)
  return a


def _abi_scalar(spec):
  """The reference's scalar host-pointer ABI, executed as a batch of one on the GPU."""
  name, a = spec.name, _Abi(spec.name)
  D, EE = spec.dim_x, spec.dim_err * spec.dim_err
  xo, Po, Qo = 0, _align2(D), _align2(D) + _align2(EE)
  a.text("")
  a.text("// ---- reference scalar ABI (/root/reference/rednose/helpers/ekf_sym.py:149-165): HOST pointers, in place ----")
  a.fn("void", "predict", "double *in_x, double *in_P, double *in_Q, double dt", f"""  rn::Scratch& s = rn::scratch();
  std::lock_guard<std::mutex> hold(s.mu);
  if (s.ensure({Qo + _align2(EE)}) != rn::OK) return;
  s.put({xo}, in_x, {D}); s.put({Po}, in_P, {EE}); s.put({Qo}, in_Q, {EE});
  if ({name}_batch_predict(s.dev + {xo}, s.dev + {Po}, s.dev + {Qo}, nullptr, dt, 1, 0, nullptr) != rn::OK) return;
  if (s.wait("{name}_predict", __LINE__) != rn::OK) return;
  s.get(in_x, {xo}, {D}); s.get(in_P, {Po}, {EE});""")
  for k in spec.kinds:
    Z = k.zdim
    zo = Po + _align2(EE)
    Ro = zo + _align2(Z)
    eo = Ro + _align2(Z * Z)
    EA = ea_len(k)
    ea_put = f" s.put({eo}, in_ea, {EA});" if EA else ""
    ea_arg = f"s.dev + {eo}" if EA else "nullptr"
    a.fn("void", f"update_{k.kind}", "double *in_x, double *in_P, double *in_z, double *in_R, double *in_ea", f"""  (void)in_ea;
  rn::Scratch& s = rn::scratch();
  std::lock_guard<std::mutex> hold(s.mu);
  if (s.ensure({eo + _align2(EA)}) != rn::OK) return;
  s.put({xo}, in_x, {D}); s.put({Po}, in_P, {EE}); s.put({zo}, in_z, {Z}); s.put({Ro}, in_R, {Z * Z});{ea_put}
  if ({name}_batch_update_{k.kind}(s.dev + {xo}, s.dev + {Po}, s.dev + {zo}, s.dev + {Ro}, 0, {ea_arg}, 1, 0, nullptr, nullptr) != rn::OK) return;
  if (s.wait("{name}_update_{k.kind}", __LINE__) != rn::OK) return;
  s.get(in_x, {xo}, {D}); s.get(in_P, {Po}, {EE}); s.get(in_z, {zo}, {Z});""")
  return a


def _library(spec):
  """-> (header_text, hip_text): the pieces above in the order of the file."""
  name, tune = spec.name, tuning.current()
  s = _select(spec)
  src = [f"// GENERATED by rednose_amd.helpers.ekf_sym.gen_code for filter '{name}' -- do not edit.",
         f"// DIM={spec.dim_x} EDIM={spec.dim_err} MEDIM={spec.dim_main_err} kinds={[k.kind for k in spec.kinds]} family={s.fam}",
         *(["#define RN_RTS_TL 1"] if (s.fam == "wide" and tune.wide_timeline) else []),
         *(["#define RN_EXACT_MATH 1"] if tune.exact_math else []),
         '#include "ekf_hip_rt.h"', '#include "ekf_hip_rts.h"', "", "namespace {",
         f"constexpr int DIM = {spec.dim_x};", f"constexpr int EDIM = {spec.dim_err};", f"constexpr int MEDIM = {spec.dim_main_err};", ""]
  # run-time scalars of the model (reference: file-scope doubles + set_{var}, ekf_sym.py:129-132,166-171): device
  # globals written by {name}_set_{var}; like the reference they are per LIBRARY, not per filter instance
  src += [f"__device__ double {var.name} = 0.0;" for var in spec.global_vars]
  routines, wrappers = _routines(spec)
  src += routines + _kernels(spec, s)
  if s.has_rts:
    src.append(_rts_model(spec, s))
  if spec.N > 0:
    src.append(_augment_kernel(spec))
  src += ["}  // namespace\n", 'extern "C" {', ""]
  # the wrappers of the routines: first in the header (as in the reference's), last in the source (they call nothing of the ABI)
  abi = [_abi_model(spec), _abi_debug(spec, s), _abi_batched(spec, s), _abi_tri(spec, s), _abi_rts(spec, s), _abi_scalar(spec)]
  for a in abi + [wrappers]:
    src += a.src
  src += ['}  // extern "C"', plugin_text(spec)]
  hdr = ["#pragma once", "#include <stdint.h>", "#ifdef __cplusplus", 'extern "C" {', "#endif"]
  for a in [wrappers] + abi:
    hdr += a.hdr
  hdr += ["#ifdef __cplusplus", "}", "#endif", ""]
  text = "\n".join(src) + "\n"
  # helpers codegen/lower.py printed calls of: the residual of feature-track kinds in the reference's null-space basis, the fast sin / cos
  for call, helper in (("rn::nullspace_residual<", NULLSPACE_RESIDUAL), ("rn::sincos_fast(", SINCOS_FAST)):
    if call in text:
      text = text.replace('#include "ekf_hip_rts.h"\n', '#include "ekf_hip_rts.h"\n' + helper, 1)
  return "\n".join(hdr), text
