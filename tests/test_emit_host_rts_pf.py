"""k_rts4_pf (codegen/emit_rts4.kernel(pf=True): the register-broadcast smoother with a schedule per filter) run WHOLE on the host in the fiber
emulation of tests/test_emit_host.py -- `_rts4_host_library`'s recipe restated for the new kernel name -- against yardstick (a), the numpy
restatement of the reference's rts_smooth on the oracle's functions applied filter by filter to the contract of RN_DECLARE_BATCH_RTS_PF
(tests/rts_pf_cases.py), 1e-7 relative on states and covariances.  rand8 (one row slot), randaff11 (affine: predict(0) is not the identity, and an
idle entry must still be an identity step) and rand17 (two row slots: the branches of the emitter that no shipped library takes, since the
two-slot models' k_rts4_pf spills and falls back), T = 7, n = 7: one full tile plus a ragged one, the schedule builder's logs.  Guard rows in front of and
behind both outputs, pass-through rows bit for bit, in place and not, x_last / P_last passed and NULL."""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import test_emit_host as H
from rts_pf_cases import OracleModel, forward_dts, restate, schedule

BOUND = 1e-7


@H._once
def _rts4_pf_host_library(tmp_path, spec):
  from rednose_amd.codegen import emit_rts4, tuning
  from rednose_amd.codegen.emit_common import routine_device_function
  hdr = open(H.HDR, encoding="utf-8").read()
  helpers = "\n".join(H._function_text(hdr, f) for f in ("rsqrt_pow", "sincos_fast", "normalize_quat"))
  with tuning.using_model(spec):
    assert emit_rts4.applicable(spec)
    text = emit_rts4.kernel(spec) + "\n" + emit_rts4.kernel(spec, pf=True)      # (k_rts4 brings the macros and the scalar phase both kernels use)
  routines = "\n".join(routine_device_function(r)[0] for r in spec.routines() if r.name in ("err_fun", "inv_err_fun"))
  text = re.sub(r'asm volatile\("" : ((?:"\+v"\(\w+\)(?:, )?)+)\);', ";", text)
  text = text.replace("__builtin_amdgcn_sched_barrier", "rn::sched_barrier_")
  text = text.replace("__attribute__((ext_vector_type(2)))", "__attribute__((vector_size(16), aligned(8)))")
  text = text.replace("(const __attribute__((address_space(1))) void*)", "(const void*)")
  text = re.sub(r"(__device__ \w+ (?:void|int) scal_\w+\(.*?\n}\n)", lambda m: m.group(1).replace("rn::wave_lds_sync();", ";"), text, flags=re.S)
  entry = """
extern "C" __attribute__((visibility("default"))) void host_rts4_pf(int grid, const double* xf, const double* Pf, const double* dts, const unsigned char* act, int64_t T,
    const double* Q, int64_t n, int norm_quats, double* xs, double* Ps, const double* xl, const double* Pl) {
  run_grid(grid, [&] { k_rts4_pf(xf, Pf, dts, T, Q, n, norm_quats, xs, Ps, xl, Pl, act); });
}"""
  prelude = H._KERNEL_PRELUDE.replace("inline void pin(double&) {}", "inline void pin(double&) {}\n" + H._WIDE_COPIES + "inline void* lds_offset_ptr(double* p) { return p; }\n")
  prelude = prelude.replace("namespace rn {", H._WAVE_VOTES + H._RTS4_HOST + "namespace rn {", 1)
  src = "\n".join([prelude, helpers, "}  // namespace rn", routines, text, H._RUN_GRID, entry])
  cpp, lib = tmp_path / f"{spec.name}_rts4_pf_host.cpp", tmp_path / f"lib{spec.name}_rts4_pf_host.so"
  cpp.write_text(H._fiberize(src) if "#include <pthread.h>" in src else src, encoding="utf-8")
  res = subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fno-gnu-unique", "-fvisibility=hidden", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-ffp-contract=off", str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  dll = ctypes.CDLL(str(lib))
  fn = dll.host_rts4_pf
  fn.set_lds_fill = lambda bits: H.set_lds_fill(dll, bits)
  dp, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)
  fn.argtypes = [ctypes.c_int, dp, dp, dp, bp, ctypes.c_int64, dp, ctypes.c_int64, ctypes.c_int, dp, dp, dp, dp]
  return fn


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("name", ["rand8", "randaff11", "rand17"])
def test_per_filter_register_broadcast_smoother_on_the_host(tmp_path, name):
  from oracle_lib import OracleLib
  from rednose_amd.codegen.spec import build_spec
  import examples.random_kf as R
  M = {"rand8": R.Random8Kalman, "randaff11": R.RandomAffine11Kalman, "rand17": R.Random17Kalman}[name]
  spec = build_spec(**M.model())
  id0 = name != "randaff11"
  assert spec.identity_at_dt0() == id0
  fn = _rts4_pf_host_library(tmp_path, spec)
  D = E = spec.dim_x
  model = OracleModel(OracleLib(M.name), D, E)
  n, T = 7, 7
  rng = np.random.default_rng(D)
  sch = schedule(n, T, sorted(M.obs_noise), seed=17)
  act = (sch["kinds_rts"] > 0) & (sch["kinds_rts"] < 9999)
  assert sch["unknown"] is not None and not act[sch["unknown"]]
  dts = np.ascontiguousarray(forward_dts(sch["ts"], sch["kinds_rts"], np.full(n, 0.9)))
  act = np.ascontiguousarray(act.astype(np.uint8))
  # which rows of a tile are at an identity step (Ck = I) in backward step k: no entry at k + 1, an entry with dt == 0 behind which another one
  # follows (only where predict(0) is the identity), or nothing at or behind k + 1 at all
  ident = lambda k, i: not act[k + 1, i] or (id0 and dts[k + 1, i] == 0.0 and act[k + 2:, i].any()) or not act[k + 1:, i].any()      # noqa: E731
  tiles = [[[ident(k, i) for i in range(b0, min(n, b0 + 4))] for k in range(T - 1)] for b0 in (0, 4)]
  assert any(not all(r) and any(r) for r in tiles[0]), "the first tile needs a step whose rows differ"
  assert any(all(r) for r in tiles[0 if id0 else 1]), "a tile needs a step with every row at an identity step (the affine model's full log never is)"
  X = M.initial_x[None, None] + rng.normal(size=(T, n, D)) * 0.3
  A = rng.normal(size=(T, n, D, D)) * 0.2
  P = np.diag(M.initial_P_diag)[None, None] + A @ A.transpose(0, 1, 3, 2)
  for t in range(1, T):      # the trace is dense: the row of an entry that did not step its filter is the pair the filter already had
    idle = act[t] == 0
    X[t, idle], P[t, idle] = X[t - 1, idle], P[t - 1, idle]
  iu = np.triu_indices(E, 1)
  P[:, 0, iu[0], iu[1]] += 0.05      # the contract: lower triangles are read (filter 0: something else above the diagonal)
  X, P = np.ascontiguousarray(X), np.ascontiguousarray(P)
  xl = np.ascontiguousarray(X[-1] + rng.normal(size=(n, D)) * 1e-3)
  Pl = np.ascontiguousarray(1.5 * np.tril(P[-1]) + 1.5 * np.tril(P[-1], -1).transpose(0, 2, 1))
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  dp, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a: a.ctypes.data_as(dp)      # noqa: E731
  got = {}
  for fill_name, bits in H.LDS_FILLS:      # what LDS held at workgroup entry: the NaN pattern, then a large finite number (a select hides a NaN, not 1e30)
    fn.set_lds_fill(bits)
    for inplace, last in itertools.product((False, True), (False, True)):
      bx, bP = np.full((T + 4, n, D), 7.0), np.full((T + 4, n, E, E), 7.0)
      xs, Ps = bx[2:T + 2], bP[2:T + 2]
      if inplace:
        xs[:], Ps[:] = X, P
      xf, Pf = (xs, Ps) if inplace else (X.copy(), P.copy())
      fn(2, ptr(xf), ptr(Pf), ptr(dts), act.ctypes.data_as(bp), T, ptr(Q), n, 0, ptr(xs), ptr(Ps), ptr(xl) if last else None, ptr(Pl) if last else None)
      what = f"{name} inplace={inplace} newest pair passed={last} (LDS starts as {fill_name})"
      assert (bx[:2] == 7.0).all() and (bx[T + 2:] == 7.0).all() and (bP[:2] == 7.0).all() and (bP[T + 2:] == 7.0).all(), what + ": a guard row was written"
      if not inplace:
        assert np.array_equal(xf, X) and np.array_equal(Pf, P), what + ": the trace was written"
      assert np.isfinite(xs).all() and np.isfinite(Ps).all(), what
      r = restate(model, X, P, dts, act, xs, Ps, Q, x_last=xl if last else None, P_last=Pl if last else None)
      print(f"{what}: x {r['worst']['x']:.3e} P {r['worst']['P']:.3e} pass-through rows {len(r['passed'])}")
      assert r["bits"], what + ": a pass-through row changed"
      assert len(r["passed"]) >= 10
      assert r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, (what, r["worst"])
      if last:
        for i in range(n):
          st = np.nonzero(act[:, i])[0]
          if len(st):
            assert np.array_equal(xs[st[-1], i], xl[i]) and np.array_equal(Ps[st[-1], i], Pl[i]), (what, i)
      got[fill_name, inplace, last] = (xs.copy(), Ps.copy())
  fn.set_lds_fill(H.LDS_FILLS[0][1])
  for inplace, last in itertools.product((False, True), (False, True)):
    for a, b, label in zip(got["NaN", inplace, last], got["1e30", inplace, last], ("xs", "Ps")):
      assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} inplace={inplace} newest pair passed={last} {label}: the result depends on what LDS held at workgroup entry"
