"""The fused run with a schedule per filter of MSCKF models (k_run_epf, emit_wide3.run_epf_kernel) as a WHOLE kernel on the host, in the fiber
emulation of tests/test_emit_host.py (machinery of tests/test_emit_host_run_pf.py): the `feature` model, 8 filters per wavefront, every filter with
its own kinds, dts, idle entries, landmarks and window shifts.  The predicated null-space projection (`update_2_rows_epf`) and the shift per group
are walked by every lane; the rows of idle groups, of groups of another kind and of groups that do not shift must come out unchanged.  Against
OracleLib.batch_step(..., ea=) per filter plus the window shift restated in numpy (run_pf_ea_cases).  Emulated LDS starts poisoned; the case
runs under the NaN pattern and under 1e30 and must give the same bits."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_close
from run_pf_cases import UNKNOWN, expected_flags_untouched, make_schedule, r_table, stepped_mask
from run_pf_ea_cases import FEATURE, oracle_walk_ea
from test_emit_host import HDR, LDS_FILLS, _KERNEL_PRELUDE, _RUN_GRID, _WAVE_VOTES, _WIDE_COPIES, _fiberize, _function_text, _once, set_lds_fill
from test_emit_host_kinds import _GXX, _SOLVERS

pytestmark = pytest.mark.timeout(240, method="thread")

_PROJECTION = ("householder_qr", "apply_reflectors", "project_noise")      # plain C++ of the runtime header, like _SOLVERS
_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_run_epf(int grid, double* x, double* P, const double* Q, const int32_t* kinds,
    const double* dts, int64_t T, double* z, const double* R, int64_t n, int norm_quats, uint8_t* flags, double* tx, double* tP,
    const double* ea, const int32_t* augs) {
  run_grid(grid, [&] { k_run_epf(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, tx, tP, ea, augs); });
}
"""


@_once
def _library(tmp_path, spec):
  from rednose_amd.codegen import emit_wide3, tuning
  from rednose_amd.codegen.lower import NULLSPACE_RESIDUAL
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in _SOLVERS + _PROJECTION)
  with tuning.using_model(spec):
    text = emit_wide3.kernels(spec)
  assert "void k_run_epf(" in text and "_rows_epf(" in text
  text = re.sub(r'asm volatile\("" : "\+v"\((\w+)\)( :: "memory")?\);', ";", text)
  text = text.replace("__builtin_amdgcn_sched_barrier", "rn::sched_barrier_")
  # (the scalar-phase functions run on the lanes that own a filter only: their wave_lds_sync() calls are scheduling boundaries, not rendezvous points)
  text = re.sub(r"(__device__ \w+ (?:void|int) scal_\w+\(.*?\n}\n)", lambda m: m.group(1).replace("rn::wave_lds_sync();", ";"), text, flags=re.S)
  prelude = _KERNEL_PRELUDE.replace("inline void pin(double&) {}", "inline void pin(double&) {}\n" + _WIDE_COPIES).replace("namespace rn {", _WAVE_VOTES + "namespace rn {", 1)
  src = "\n".join([prelude, helpers, "}  // namespace rn", "using std::fabs; using std::sqrt;", NULLSPACE_RESIDUAL, text, _RUN_GRID, _ENTRY])
  cpp, lib = tmp_path / f"{spec.name}_run_epf_host.cpp", tmp_path / f"lib{spec.name}_run_epf_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


def test_msckf_per_filter_run_on_the_host(tmp_path):
  from examples.feature_kf import FeatureKalman as M
  from oracle_lib import OracleLib
  from rednose_amd.codegen import emit, emit_wide3
  from rednose_amd.codegen.spec import build_spec
  name = "feature"
  spec = build_spec(**M.model())
  assert emit.family(spec, ()) == "wide" and emit.has_run_pf_ea(spec, ()) and not emit.run_pf(spec, ())
  lib = _library(tmp_path, spec)
  o = OracleLib(name)
  tol = 1e-8      # of the row maximum: the lane-group multi-step emulations' bound
  D, E = spec.dim_x, spec.dim_err
  FT = emit_wide3.layout(spec)[2]
  assert FT == 8, "8 lanes x 2 rows: the predicates diverge inside a wavefront"
  n, T, grid = 2 * FT + FT // 2 + 1, 6, 2                       # two full tiles and a ragged third one, on two workgroups
  dims = (spec.dim_main, spec.dim_main_err, spec.dim_augment, spec.dim_augment_err)
  rng = np.random.default_rng(415)
  kset = [k.kind for k in spec.kinds]
  zdim = {k.kind: k.zdim for k in spec.kinds}
  zmax = max(zdim.values())
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  Rs = {k: np.ascontiguousarray(M.obs_noise[k], dtype=np.float64) for k in kset}
  Rtab = r_table([(k.kind, k.zdim) for k in spec.kinds], Rs, zmax)
  kd, info = make_schedule(rng, T, n, kset, FT)
  on = stepped_mask(kd, kset)
  nv = info["never"]
  assert not on[:, nv].any() and kd[info["unknown"]] == UNKNOWN and len(set(kd[:, :FT][kd[:, :FT] > 0])) == 1
  assert all((kd[:, FT:2 * FT] == k).any() for k in kset), "every kind appears in the mixed tile"
  assert abs((kd <= 0).mean() - 0.3) < 0.12, "about 30 % of the entries are idle"
  dts = rng.uniform(0.0, 0.05, size=(T, n))
  dts[rng.uniform(size=(T, n)) < 0.1] = 0.0
  # the planted landmark: a feature entry with an entry of its filter in front of it, dt = 0 (predict is the identity: the entry must leave x and P as they are)
  tp, ip = next((int(t), int(i)) for t, i in zip(*np.nonzero(kd == FEATURE)) if t >= 1 and i >= FT and i != nv)
  dts[tp, ip] = 0.0
  dts[kd <= 0] = np.nan                                         # ignored at idle entries
  aug = (on & (rng.uniform(size=(T, n)) < 1.0 / 3.0)).astype(np.int32)
  aug[:tp, ip] = 0                                              # (the trace row in front of the planted entry is then the state it meets)
  assert abs(aug[on].mean() - 1.0 / 3.0) < 0.12 and (aug[:, :FT].sum(axis=0) > 0).any() and (aug.sum(axis=0)[on.any(axis=0)] == 0).any()
  ignored = aug.copy()
  idle_at = np.argwhere(kd <= 0)
  for t, i in idle_at[rng.permutation(len(idle_at))[:6]]:       # set at a few idle entries, one of the never-stepped filter's, and at the unknown entry: ignored
    ignored[t, i] = 1
  ignored[0, nv] = 1
  ignored[info["unknown"]] = 1
  ea = np.full((T, n, 3), np.nan)                               # never read but at the entries of the feature kind
  feat = kd == FEATURE
  ea[feat] = np.array([2.0, 1.0, 8.0]) + rng.normal(size=(int(feat.sum()), 3))
  ea[tp, ip] = [1.0, 1.0, 1e200]                                # d h / d landmark underflows to zero: the projection is rank deficient
  x_init = np.asarray(M.initial_x, dtype=np.float64)
  P_init = np.diag(M.initial_P_diag)
  x0 = np.tile(x_init, (n, 1)) + rng.normal(size=(n, D)) * 0.1
  A = rng.normal(size=(n, E, E)) * 0.1 * np.sqrt(np.diag(P_init))[None, :, None]
  P0 = P_init[None] + A @ A.transpose(0, 2, 1)
  Wk = rng.normal(size=(n, E, E))                               # asymmetric: the fused runs are specified on (P + P^T) / 2
  P0 = P0 + 1e-3 * np.abs(P0).max(axis=(1, 2), keepdims=True) * (Wk - Wk.transpose(0, 2, 1))
  zs = rng.normal(size=(T, n, zmax))
  for k in spec.kinds:                                          # observations near h(x0, landmark)
    for t, i in zip(*np.nonzero(kd == k.kind)):
      hx = np.zeros(k.zdim)
      o.call(f"h_{k.kind}", x0[i].copy(), np.ascontiguousarray(ea[t, i]) if k.kind == FEATURE else np.zeros(4), hx)
      zs[t, i, :k.zdim] = hx + rng.normal(size=k.zdim) * np.sqrt(np.diag(Rs[k.kind]))
  zs[tp, ip] = 0.0
  xr, Pr, zr = x0.copy(), 0.5 * (P0 + P0.transpose(0, 2, 1)), zs.copy()
  fr, txr, tPr = oracle_walk_ea(o, zdim, Rs, Q, kd, dts, xr, Pr, zr, ea, aug, dims)
  assert np.array_equal(fr[~on], expected_flags_untouched(kd, kset)[~on])
  # The oracle restates the reference's C path, which has no rank test: with Hea = 0 (and H = 0: the rays are ~1e200 long) its update of the planted
  # entry changes nothing either, unflagged.  The kernel ignores such a measurement and says so: flag 4 there, and nowhere else.
  assert not (fr[on] & 4).any()
  fr[tp, ip] |= 4

  dp, ip_, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a, t=dp: a.ctypes.data_as(t)      # noqa: E731
  lib.host_run_epf.argtypes = [ctypes.c_int, dp, dp, dp, ip_, dp, ctypes.c_int64, dp, dp, ctypes.c_int64, ctypes.c_int, bp, dp, dp, dp, ip_]
  G, got = 2, {}
  for fill_name, bits in LDS_FILLS:      # what LDS held at workgroup entry: the NaN pattern, then a large finite number (a select hides a NaN, not 1e30)
    set_lds_fill(lib, bits)
    xg, Pg = np.full((n + 2 * G, D), 7.5), np.full((n + 2 * G, E, E), 7.5)
    xg[G:G + n], Pg[G:G + n] = x0, P0
    zg = np.full((T + 2, n, zmax), 777.0)
    zg[1:T + 1] = zs
    fg = np.full((T + 2, n), 99, dtype=np.uint8)
    tx, tP = np.full((T + 2, n, D), 5.0), np.full((T + 2, n, E, E), 5.0)
    lib.host_run_epf(grid, ptr(xg[G]), ptr(Pg[G]), ptr(Q), ptr(kd, ip_), ptr(dts), T, ptr(zg[1]), ptr(Rtab), n, 0, ptr(fg[1], bp), ptr(tx[1]), ptr(tP[1]),
                     ptr(ea), ptr(ignored, ip_))
    what = f"{name} k_run_epf (LDS starts as {fill_name})"
    for a, fill in ((xg, 7.5), (Pg, 7.5)):
      assert (a[:G] == fill).all() and (a[-G:] == fill).all(), what + ": guard filters"
    for a, fill in ((zg, 777.0), (fg, 99), (tx, 5.0), (tP, 5.0)):
      assert (a[0] == fill).all() and (a[T + 1] == fill).all(), what + ": guard rows"
    xh, Ph, zh, fl = xg[G:G + n], Pg[G:G + n], zg[1:T + 1], fg[1:T + 1]
    for a in (xh, Ph, zh, tx, tP):
      assert np.isfinite(a).all(), what + ": an output is not finite"
    assert np.array_equal(fl, fr), what + ": flags (16 idle, 8 unknown kind, 4 the planted landmark)"
    assert np.array_equal(zh[~on], zs[~on]), what + ": z rows of idle entries pass through bit for bit"
    assert np.array_equal(xh[nv], x0[nv]) and np.array_equal(Ph[nv], P0[nv]), what + ": the never-stepped filter is not written back (its augment entry is ignored)"
    # final state: AFTER the last shift of every filter; trace rows: BEFORE the shift of their entry
    for g_, w_, label in ((np.delete(xh, nv, 0), np.delete(xr, nv, 0), "x"), (np.delete(Ph, nv, 0).reshape(n - 1, -1), np.delete(Pr, nv, 0).reshape(n - 1, -1), "P"),
                          (tx[1:T + 1].reshape(T * n, -1), txr.reshape(T * n, -1), "trace x"), (tP[1:T + 1].reshape(T * n, -1), tPr.reshape(T * n, -1), "trace P")):
      err = np.abs(g_ - w_) / np.abs(w_).max(axis=1, keepdims=True)
      assert err.max() <= tol, f"{what} {label}: {err.max():.3e} of the row maximum (bound {tol:.0e})"
    for k in spec.kinds:
      Zy = k.zdim - 3 if k.kind == FEATURE else k.zdim      # feature kinds write Z - 3 residual rows, in the reference's basis
      m = kd == k.kind
      assert_close(zh[m][:, :Zy], zr[m][:, :Zy], rtol=tol, atol=tol * 1e-2 * max(1.0, np.abs(zs).max()), what=what + f" kind {k.kind} y")
      assert np.array_equal(zh[m][:, Zy:], zs[m][:, Zy:]), what + f" kind {k.kind}: z columns beyond the residual"
    # the planted entry: flag 4, x and P as the entry met them (its dt is 0), bit for bit
    assert np.array_equal(tx[1 + tp, ip], tx[tp, ip]) and np.array_equal(tP[1 + tp, ip], tP[tp, ip]), what + ": the rank-deficient entry changed x or P"
    # dense trace: an idle entry's row repeats the row before it unless that entry shifted the window
    rep = ~on[1:] & ~((aug[:-1] != 0) & on[:-1])
    assert np.array_equal(tx[2:T + 1][rep], tx[1:T][rep]) and np.array_equal(tP[2:T + 1][rep], tP[1:T][rep]), what + ": trace rows of idle entries"
    last_sh = np.array([bool(aug[np.nonzero(on[:, i])[0][-1], i]) if on[:, i].any() else False for i in range(n)])
    keep = on.any(axis=0) & ~last_sh
    assert last_sh.any() and keep.any()
    assert np.array_equal(tx[T][keep], xh[keep]) and np.array_equal(tP[T][keep], Ph[keep]), what + ": last trace row of filters whose last entry does not shift"
    assert not np.array_equal(tx[T][last_sh], xh[last_sh]), what + ": the trace row of a shifting entry is the estimate BEFORE the shift"
    got[fill_name] = (xh.copy(), Ph.copy(), zh.copy(), fl.copy(), tx.copy(), tP.copy())
    if fill_name == "NaN":      # augs == NULL: no shifts; the filters that never shift come out bit for bit as above
      xg2, Pg2, zg2 = x0.copy(), P0.copy(), zs.copy()
      lib.host_run_epf(grid, ptr(xg2), ptr(Pg2), ptr(Q), ptr(kd, ip_), ptr(dts), T, ptr(zg2), ptr(Rtab), n, 0, None, None, None, ptr(ea), None)
      calm = aug.sum(axis=0) == 0
      assert calm.any() and not calm.all()
      assert np.array_equal(xg2[calm], xh[calm]) and np.array_equal(Pg2[calm], Ph[calm]) and np.array_equal(zg2[:, calm], zh[:, calm]), what + ": augment == NULL"
      assert not np.array_equal(xg2[~calm], xh[~calm])
  set_lds_fill(lib, LDS_FILLS[0][1])
  for a, b, label in zip(got["NaN"], got["1e30"], ("x", "P", "y", "flags", "trace x", "trace P")):
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} {label}: the result depends on what LDS held at workgroup entry"


def _window_shift_statements(kernel_text):
  """The statements of a fused run's MSCKF window shift that move numbers: lane 0's permutation of x, the row index of every row slot and the
  rows re-read out of the image -- without indentation and without the guard `if (sh)` of the per-group variant."""
  lines = kernel_text.split("// MSCKF window shift after this step", 1)[1].split("\n    }\n", 1)[0].splitlines()      # up to the end of the step loop
  lines = [re.sub(r"^if \(sh\) (?=\{ const int sr\b)", "", line.strip()) for line in lines]
  return [line for line in lines if re.match(r"sl\[\d+\] = xo\[\d+\];$|row\d+\[\d+\] = sP\[srow \* \d+ \+ \d+\];$|\{ const int sr = ", line)]


@pytest.mark.parametrize("name", ["feature", "feature36"])
def test_both_fused_runs_shift_the_window_with_the_same_statements(name):
  """k_run shifts every filter of the wavefront at once, k_run_epf each group under its own predicate: one builder (emit_wide3._window_shift)
  prints both blocks, and whatever its parameters change, the permutation of x and the rows taken out of the image are the same statements."""
  from examples.feature_kf import FeatureKalman, WideFeatureKalman
  from rednose_amd.codegen import emit_wide3, tuning
  from rednose_amd.codegen.spec import build_spec
  spec = build_spec(**{"feature": FeatureKalman, "feature36": WideFeatureKalman}[name].model())
  with tuning.using_model(spec):
    shared, per_group = emit_wide3.run_kernel(spec), emit_wide3.run_epf_kernel(spec)
  assert "void k_run(" in shared and "void k_run_epf(" in per_group
  a, b = _window_shift_statements(shared), _window_shift_statements(per_group)
  R, D, E = emit_wide3.layout(spec)[1], spec.dim_x, spec.dim_err
  assert sum(s.startswith("row") for s in a) == R * E and sum(s.startswith("{ const int sr") for s in a) == R
  assert 0 < sum(s.startswith("sl[") for s in a) <= D
  assert a == b
  assert sum("if (sh) { const int sr" in line for line in per_group.splitlines()) == R and "if (sh)" not in shared
