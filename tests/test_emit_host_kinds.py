"""The generated mixed-kind step kernels (k_kinds<true> / <false>: a different observation kind per filter in one launch) as WHOLE kernels
on the host, in the fiber emulation of tests/test_emit_host.py: a workgroup is 64 lanes that meet at every wave_lds_sync().  Both families --
lane per filter (emit_small.kinds_kernel) and lane group (emit_wide2, the structure each model ships with) -- against the oracle's predict +
update of each filter's own kind."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_close
from test_emit_host import HDR, _KERNEL_PRELUDE, _RUN_GRID, _WIDE_COPIES, _fiberize, _function_text, _model, _once, _wide_model

_GXX = ["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fno-gnu-unique", "-fvisibility=hidden", "-Wno-unknown-pragmas", "-Wno-attributes"]
_SOLVERS = ("spd_factor", "spd_forward", "spd_solve", "ldu_factor", "ldu_forward", "ldu_forward_t", "ldu_solve", "rsqrt_pow", "sincos_fast", "normalize_quat")
_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_kinds(int grid, int do_predict, double* x, double* P, double* z, const double* R, int r_per_filter,
    const int32_t* kinds, const double* Q, const double* dt_vec, double dt, int64_t n, int norm_quats, uint8_t* flags, const uint8_t* active) {
  if (do_predict) run_grid(grid, [&] { k_kinds<true>(x, P, z, R, r_per_filter, kinds, Q, dt_vec, dt, n, norm_quats, flags, active); });
  else run_grid(grid, [&] { k_kinds<false>(x, P, z, R, r_per_filter, kinds, nullptr, nullptr, 0.0, n, norm_quats, flags, active); });
}
"""


def _compile(tmp_path, name, src):
  cpp, lib = tmp_path / f"{name}_kinds_host.cpp", tmp_path / f"lib{name}_kinds_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


@_once
def _small_library(tmp_path, spec):
  from rednose_amd.codegen import emit_small, tuning
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in ("lds_stride", "tile_g2l", "tile_l2g", "lds_to_regs", "regs_to_lds") + _SOLVERS)
  with tuning.using_model(spec):      # the text a library ships with: the model's tuning decides e.g. which flavour of update_{k}_regs the kernel calls
    text = emit_small.kernels(spec)
  funcs = text[:text.index("// ---- predict only")]      # predict_regs, update_{k}_regs[_split], and the host forms of wait_but_tile / lane_dt
  at = text.index("// ---- a kind per filter")
  kern = text[at:text.index("\n}\n", text.index("void k_kinds(", at)) + 3]
  assert "void k_kinds(" in kern and "_regs_split(" in kern
  src = "\n".join([_KERNEL_PRELUDE, helpers,
                   "template <int EPF> inline void tile_g2l_async(const double* g, int cnt, double* lds, int lane) { tile_g2l<EPF>(g, cnt, lds, lane); }",
                   "}  // namespace rn", funcs, kern, _RUN_GRID, _ENTRY])
  return _compile(tmp_path, spec.name, src), 64


@_once
def _wide_library(tmp_path, spec):
  from rednose_amd.codegen import emit_wide2, tuning
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in _SOLVERS)
  with tuning.using_model(spec):
    text = emit_wide2.kernels(spec)
    FT = emit_wide2.tile_filters(spec)
  assert "void k_kinds(" in text
  text = re.sub(r'asm volatile\("" : "\+v"\((\w+)\)( :: "memory")?\);', ";", text)
  text = text.replace("__builtin_amdgcn_sched_barrier", "rn::sched_barrier_")
  # (the scalar-phase functions run on the lanes that own a filter only: their wave_lds_sync() calls are scheduling boundaries, not rendezvous points)
  text = re.sub(r"(__device__ \w+ (?:void|int) scal_\w+\(.*?\n}\n)", lambda m: m.group(1).replace("rn::wave_lds_sync();", ";"), text, flags=re.S)
  prelude = _KERNEL_PRELUDE.replace("inline void pin(double&) {}", "inline void pin(double&) {}\n" + _WIDE_COPIES)
  src = "\n".join([prelude, helpers, "}  // namespace rn", text, _RUN_GRID, _ENTRY])
  return _compile(tmp_path, spec.name, src), FT


def _attitude():
  from examples.attitude_kf import AttitudeKalman as M
  return M, M.model(), {"quaternion_idxs": [0]}, 0


CASES = [("attitude", "small"), ("rand5", "small"), ("kinematic6_maha", "small"), ("kinematic9", "wide"), ("rand11", "wide"), ("live", "wide")]


@pytest.mark.parametrize("name,family", CASES)
def test_mixed_kind_step_kernel_on_the_host(tmp_path, name, family):
  from oracle_lib import OracleLib
  from rednose_amd.codegen import emit
  from rednose_amd.codegen.spec import build_spec
  if name == "attitude":
    M, mdl, kw, quat_idx = _attitude()
  elif family == "small":
    M, mdl, kw = _model(name)
    quat_idx = -1
  else:
    M, mdl, kw, quat_idx = _wide_model(name)
  mdl = dict(mdl)
  mdl["name"] = name
  for key in ("quaternion_idxs", "maha_test_kinds"):
    if key in mdl and key in kw:
      kw = {k_: v for k_, v in kw.items() if k_ != key}
  spec = build_spec(**mdl, **kw)
  assert emit.family(spec, ()) == family and emit.step_kinds(spec, ())
  lib, FT = (_small_library if family == "small" else _wide_library)(tmp_path, spec)
  o = OracleLib(name)
  tol = 1e-11 if family == "small" else 1e-10
  D, E = spec.dim_x, spec.dim_err
  rng = np.random.default_rng(100 + E)
  n, grid = 2 * FT + max(1, FT // 2) + (FT > 2), 2               # two full tiles and a ragged third one, on two workgroups
  kinds = spec.kinds                                            # drawn per filter over ALL kinds of the model
  zdim = {k.kind: k.zdim for k in spec.kinds}
  zmax = max(zdim.values())
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  x_init = np.asarray(M.initial_x, dtype=np.float64)
  P_init = np.diag(M.initial_P_diag)
  Rs = {k.kind: np.ascontiguousarray(np.atleast_2d(M.obs_noise.get(k.kind, 0.01 * np.eye(k.zdim))), dtype=np.float64) for k in spec.kinds}
  x0 = np.tile(x_init, (n, 1)) + rng.normal(size=(n, D)) * 0.01 * np.maximum(1.0, np.abs(x_init))[None] * (np.abs(x_init)[None] < 10.0)
  if quat_idx >= 0:
    x0[:, quat_idx:quat_idx + 4] /= np.linalg.norm(x0[:, quat_idx:quat_idx + 4], axis=1, keepdims=True)
  A = rng.normal(size=(n, E, E)) * 0.1 * np.sqrt(np.diag(P_init))[None, :, None]
  P0 = P_init[None] + A @ A.transpose(0, 2, 1)
  kd = rng.choice(np.array([k.kind for k in kinds], dtype=np.int32), size=n).astype(np.int32)
  kd[:FT] = kinds[-1].kind                                      # one uniform tile; every other tile / pass is mixed
  act = (rng.uniform(size=n) >= 0.4).astype(np.uint8)
  unknown = FT + 1
  kd[unknown], act[unknown] = 4242, 1
  for j, k in enumerate(kinds):                                 # every kind has at least one active filter in a mixed pass
    kd[FT + 2 + j], act[FT + 2 + j] = k.kind, 1
  z0 = rng.normal(size=(n, zmax))
  for k in kinds:                                               # observations near h(x), a third of them far out (the gate, where the model has one)
    m = np.nonzero(kd == k.kind)[0]
    for i in m:
      hx = np.zeros(k.zdim)
      o.call(f"h_{k.kind}", x0[i].copy(), np.zeros(4), hx)
      z0[i, :k.zdim] = hx + rng.normal(size=k.zdim) * np.sqrt(np.diag(Rs[k.kind]))
    far = m[rng.uniform(size=m.size) < 0.34]
    z0[far, :k.zdim] += rng.normal(size=(far.size, k.zdim)) * 40.0 * np.sqrt(P_init.max())
  dtv = rng.uniform(0.0, 0.02, size=n)
  Rtab = np.zeros((len(spec.kinds), zmax * zmax))
  for i, k in enumerate(spec.kinds):
    Rtab[i, :k.zdim ** 2] = Rs[k.kind].reshape(-1)
  scale = rng.uniform(0.5, 2.0, size=n)
  Rpf = np.zeros((n, zmax * zmax))
  for i, k in enumerate(spec.kinds):
    Rpf[kd == k.kind] = Rtab[i][None] * scale[kd == k.kind, None]
  dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a, t=dp: a.ctypes.data_as(t)      # noqa: E731
  lib.host_kinds.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, ctypes.c_int, ip, dp, dp, ctypes.c_double, ctypes.c_int64, ctypes.c_int, bp, bp]
  on = (act != 0) & np.isin(kd, [k.kind for k in spec.kinds])
  assert on.sum() >= n // 2
  gated = 0
  for mode in ("per-filter dt", "update only, per-filter R"):
    pred, per = mode == "per-filter dt", mode != "per-filter dt"
    G = 2
    xg, Pg, zg = np.full((n + 2 * G, D), 7.5), np.full((n + 2 * G, E, E), 7.5), np.full((n + 2 * G, zmax), 7.5)
    fg = np.full(n + 2 * G, 99, dtype=np.uint8)
    xg[G:G + n], Pg[G:G + n], zg[G:G + n] = x0, P0, z0
    Rin = np.ascontiguousarray(Rpf if per else Rtab)
    lib.host_kinds(grid, int(pred), ptr(xg[G]), ptr(Pg[G]), ptr(zg[G]), ptr(Rin), int(per), ptr(kd, ip), ptr(Q), ptr(dtv), 0.0, n, int(quat_idx >= 0),
                   ptr(fg[G:], bp), ptr(act, bp))
    for a, fill in ((xg, 7.5), (Pg, 7.5), (zg, 7.5), (fg, 99)):
      assert (a[:G] == fill).all() and (a[-G:] == fill).all(), f"{name} {mode}: guard rows"
    xh, Ph, zh, fl = xg[G:G + n], Pg[G:G + n], zg[G:G + n], fg[G:G + n]
    what = f"{name} {mode}"
    assert np.array_equal(xh[~on], x0[~on]) and np.array_equal(Ph[~on], P0[~on]) and np.array_equal(zh[~on], z0[~on]), what + ": untouched filters"
    assert (fl[act == 0] == 16).all() and fl[unknown] == 8, what + ": flags of untouched filters"
    for k in kinds:
      Z = k.zdim
      sel = np.nonzero(on & (kd == k.kind))[0]
      assert sel.size > 0
      xr, Pr, zr = x0[sel].copy(), P0[sel].copy(), np.ascontiguousarray(z0[sel, :Z])
      fr = np.zeros(sel.size, dtype=np.uint8)
      Ro = np.ascontiguousarray(Rpf[sel, :Z * Z].reshape(-1, Z, Z)) if per else Rs[k.kind]
      o.batch_step(k.kind, xr, Pr, zr, Ro, Q, dtv[sel] if pred else 0.0, quat_idx=quat_idx, flags=fr, do_predict=pred)
      assert np.array_equal(fl[sel] & 1, fr & 1), what + f" kind {k.kind}: gate flags"
      gated += int((fl[sel] & 1).sum())
      for got, want, label in ((xh[sel], xr, "x"), (Ph[sel].reshape(sel.size, -1), Pr.reshape(sel.size, -1), "P")):
        err = np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)
        assert err.max() <= tol, f"{what} kind {k.kind} {label}: {err.max():.3e} of the row maximum (bound {tol:.0e})"
      assert_close(zh[sel, :Z], zr, rtol=tol, atol=tol * 1e-2 * max(1.0, np.abs(z0).max()), what=what + f" kind {k.kind} y")
      assert np.array_equal(zh[sel, Z:], z0[sel, Z:]), what + f" kind {k.kind}: z columns beyond Z"
  assert (gated > 0) == any(k.maha_test for k in spec.kinds)
