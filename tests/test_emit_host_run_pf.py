"""The fused run with a schedule per filter (k_run_pf / k_run_pf_tr, emit_small.run_pf_kernel) as WHOLE kernels on the host, in the fiber
emulation of tests/test_emit_host.py: a workgroup is 64 lanes that meet at every wave_lds_sync().  Every filter has its own kinds, its own
dts and its own idle entries; the oracle steps each filter through its own entries.  Both families: lane per filter (emit_small.run_pf_kernel)
and lane group (emit_wide3.run_pf_kernel: every lane walks the predicated matrix phases of every kind present and meets every barrier; the
rows of idle groups and of groups of another kind must come out unchanged).  Emulated LDS starts poisoned (test_emit_host._poison_shared); every case
runs under the NaN pattern and under 1e30 and must give the same bits."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_close
from run_pf_cases import UNKNOWN, expected_flags_untouched, make_schedule, oracle_walk, r_table, stepped_mask
from test_emit_host import HDR, LDS_FILLS, _KERNEL_PRELUDE, _RUN_GRID, _WAVE_VOTES, _WIDE_COPIES, _fiberize, _function_text, _model, _once, _wide_model, set_lds_fill
from test_emit_host_kinds import _GXX, _SOLVERS, _attitude

pytestmark = pytest.mark.timeout(180, method="thread")

_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_run_pf(int grid, int traced, double* x, double* P, const double* Q, const int32_t* kinds,
    const double* dts, int64_t T, double* z, const double* R, int64_t n, int norm_quats, uint8_t* flags, double* tx, double* tP) {
  if (traced) run_grid(grid, [&] { k_run_pf_tr(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, tx, tP); });
  else run_grid(grid, [&] { k_run_pf(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags); });
}
"""


@_once
def _library(tmp_path, spec):
  from rednose_amd.codegen import emit_small, tuning
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in ("lds_stride", "tile_g2l", "tile_l2g", "lds_to_regs", "regs_to_lds") + _SOLVERS)
  with tuning.using_model(spec):
    text = emit_small.kernels(spec)
  funcs = text[:text.index("// ---- predict only")]      # predict_regs_sym, update_{k}_regs_sym, symmetrize_regs
  kern = text[text.index("__device__ __forceinline__ void pin_k("):]
  assert "void k_run_pf(" in kern and "void k_run_pf_tr(" in kern and "v_readlane" not in kern and "lane_bcast" not in kern
  kern = kern.replace('asm volatile("" : "+v"(v));', ";")
  src = "\n".join([_KERNEL_PRELUDE, helpers, "}  // namespace rn", funcs, kern, _RUN_GRID, _ENTRY])
  cpp, lib = tmp_path / f"{spec.name}_run_pf_host.cpp", tmp_path / f"lib{spec.name}_run_pf_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


_WIDE_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_run_pf(int grid, int traced, double* x, double* P, const double* Q, const int32_t* kinds,
    const double* dts, int64_t T, double* z, const double* R, int64_t n, int norm_quats, uint8_t* flags, double* tx, double* tP) {
  (void)traced;      // one kernel: the trace pointers decide
  run_grid(grid, [&] { k_run_pf(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, tx, tP); });
}
"""


@_once
def _wide_library(tmp_path, spec):
  from rednose_amd.codegen import emit_wide3, tuning
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in _SOLVERS)
  with tuning.using_model(spec):
    text = emit_wide3.kernels(spec)
  assert "void k_run_pf(" in text and "_rows_pf(" in text
  text = re.sub(r'asm volatile\("" : "\+v"\((\w+)\)( :: "memory")?\);', ";", text)
  text = text.replace("__builtin_amdgcn_sched_barrier", "rn::sched_barrier_")
  # (the scalar-phase functions run on the lanes that own a filter only: their wave_lds_sync() calls are scheduling boundaries, not rendezvous points)
  text = re.sub(r"(__device__ \w+ (?:void|int) scal_\w+\(.*?\n}\n)", lambda m: m.group(1).replace("rn::wave_lds_sync();", ";"), text, flags=re.S)
  prelude = _KERNEL_PRELUDE.replace("inline void pin(double&) {}", "inline void pin(double&) {}\n" + _WIDE_COPIES).replace("namespace rn {", _WAVE_VOTES + "namespace rn {", 1)
  src = "\n".join([prelude, helpers, "}  // namespace rn", text, _RUN_GRID, _WIDE_ENTRY])
  cpp, lib = tmp_path / f"{spec.name}_run_pf_host.cpp", tmp_path / f"lib{spec.name}_run_pf_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


def _spec(name, family):
  """-> (model class, spec, quaternion index) of a case (the model lookup of tests/test_emit_host_run_pf_rd.py)"""
  from rednose_amd.codegen import emit
  from rednose_amd.codegen.spec import build_spec
  if name == "attitude":
    M, mdl, kw, quat_idx = _attitude()
  elif family == "small":
    M, mdl, kw = _model(name)
    quat_idx = -1
  elif name == "randz10":
    import examples.random_kf as R
    M, kw, quat_idx = R.RandomWideObs10Kalman, {}, -1
    mdl = M.model()
  else:
    M, mdl, kw, quat_idx = _wide_model(name)
  mdl = dict(mdl)
  mdl["name"] = name
  for key in ("quaternion_idxs", "maha_test_kinds"):
    if key in mdl and key in kw:
      kw = {k_: v for k_, v in kw.items() if k_ != key}
  spec = build_spec(**mdl, **kw)
  assert emit.family(spec, ()) == family and emit.run_pf(spec, ())
  return M, spec, quat_idx


@pytest.mark.parametrize("name,family", [("attitude", "small"), ("rand5", "small"), ("kinematic9", "wide"), ("rand11", "wide"), ("live", "wide"),
                                         ("randz10", "wide")])      # (randz10: a 9-dimensional kind, two observation entries per lane)
def test_per_filter_schedule_run_on_the_host(tmp_path, name, family):
  from oracle_lib import OracleLib
  from rednose_amd.codegen import emit_small
  M, spec, quat_idx = _spec(name, family)
  lib = (_library if family == "small" else _wide_library)(tmp_path, spec)
  o = OracleLib(name)
  # of the row maximum, DESIGN section 4: lane-per-filter emulations 1e-10, lane-group multi-step runs 1e-8
  tol = 1e-10 if family == "small" else 1e-8
  D, E = spec.dim_x, spec.dim_err
  if family == "small":
    T, FT = 2 * emit_small.run_pf_block(spec) + 1, 64
  else:
    from rednose_amd.codegen import emit_wide3
    T, FT = 5, emit_wide3.layout(spec)[2]
  n, grid = 2 * FT + FT // 2 + 1, 2                             # two full tiles and a ragged third one, on two workgroups
  rng = np.random.default_rng(311 if name == "randz10" else 300 + E)      # (randz10: the seed of tests/test_emit_host_run_pf_rd.py, at which the draw below has its ~30 % of idle entries)
  kset = [k.kind for k in spec.kinds]
  zdim = {k.kind: k.zdim for k in spec.kinds}
  zmax = max(zdim.values())
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  x_init = np.asarray(M.initial_x, dtype=np.float64)
  P_init = np.diag(M.initial_P_diag)
  Rs = {k.kind: np.ascontiguousarray(np.atleast_2d(M.obs_noise.get(k.kind, 0.01 * np.eye(k.zdim))), dtype=np.float64) for k in spec.kinds}
  Rtab = r_table([(k.kind, k.zdim) for k in spec.kinds], Rs, zmax)
  kd, info = make_schedule(rng, T, n, kset, FT)
  on = stepped_mask(kd, kset)
  assert on.sum() * 2 >= T * n, "at least half of all entries are stepped"
  assert not on[:, info["never"]].any() and kd[info["unknown"]] == UNKNOWN and len(set(kd[:, :FT][kd[:, :FT] > 0])) == 1
  assert all((kd[:, FT:2 * FT] == k).any() for k in kset), "every kind appears in the mixed tile"
  assert abs((kd <= 0).mean() - 0.3) < 0.12, "about 30 % of the entries are idle (T = 5: one or two entries per filter)"
  dts = rng.uniform(0.0, 0.02, size=(T, n))
  dts[rng.uniform(size=(T, n)) < 0.1] = 0.0                     # (predict(dt = 0): skipped where it is the identity, the renormalisation stays)
  dts[kd <= 0] = np.nan                                         # ignored at idle entries
  x0 = np.tile(x_init, (n, 1)) + rng.normal(size=(n, D)) * 0.01 * np.maximum(1.0, np.abs(x_init))[None] * (np.abs(x_init)[None] < 10.0)
  if quat_idx >= 0:
    x0[:, quat_idx:quat_idx + 4] /= np.linalg.norm(x0[:, quat_idx:quat_idx + 4], axis=1, keepdims=True)
  A = rng.normal(size=(n, E, E)) * 0.1 * np.sqrt(np.diag(P_init))[None, :, None]
  P0 = P_init[None] + A @ A.transpose(0, 2, 1)
  Wk = rng.normal(size=(n, E, E))                               # asymmetric: the fused runs are specified on (P + P^T) / 2
  P0 = P0 + 1e-3 * np.abs(P0).max(axis=(1, 2), keepdims=True) * (Wk - Wk.transpose(0, 2, 1))
  zs = rng.normal(size=(T, n, zmax))
  for k in spec.kinds:                                          # observations near h(x0), a fifth of them far out (the gate, where the model has one)
    for t, i in zip(*np.nonzero(kd == k.kind)):
      hx = np.zeros(k.zdim)
      o.call(f"h_{k.kind}", x0[i].copy(), np.zeros(4), hx)
      zs[t, i, :k.zdim] = hx + rng.normal(size=k.zdim) * np.sqrt(np.diag(Rs[k.kind])) * (40.0 if rng.uniform() < 0.2 else 1.0)
  xr, Pr, zr = x0.copy(), 0.5 * (P0 + P0.transpose(0, 2, 1)), zs.copy()
  fr, txr, tPr = oracle_walk(o, zdim, Rs, Q, kd, dts, xr, Pr, zr, quat_idx=quat_idx, trace=True)
  assert np.array_equal(fr[~on], expected_flags_untouched(kd, kset)[~on])

  dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a, t=dp: a.ctypes.data_as(t)      # noqa: E731
  lib.host_run_pf.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, ip, dp, ctypes.c_int64, dp, dp, ctypes.c_int64, ctypes.c_int, bp, dp, dp]
  G, got = 2, {}
  for fill_name, bits in LDS_FILLS:      # what LDS held at workgroup entry: the NaN pattern, then a large finite number (a select hides a NaN, not 1e30)
    set_lds_fill(lib, bits)
    for traced in (0, 1):
      xg, Pg = np.full((n + 2 * G, D), 7.5), np.full((n + 2 * G, E, E), 7.5)
      xg[G:G + n], Pg[G:G + n] = x0, P0
      zg = np.full((T + 2, n, zmax), 777.0)
      zg[1:T + 1] = zs
      fg = np.full((T + 2, n), 99, dtype=np.uint8)
      tx, tP = np.full((T + 2, n, D), 5.0), np.full((T + 2, n, E, E), 5.0)
      lib.host_run_pf(grid, traced, ptr(xg[G]), ptr(Pg[G]), ptr(Q), ptr(kd, ip), ptr(dts), T, ptr(zg[1]), ptr(Rtab), n, int(quat_idx >= 0), ptr(fg[1], bp),
                      ptr(tx[1]) if traced else None, ptr(tP[1]) if traced else None)
      what = f"{name} {'k_run_pf_tr' if traced else 'k_run_pf'} (LDS starts as {fill_name})"
      for a, fill in ((xg, 7.5), (Pg, 7.5)):
        assert (a[:G] == fill).all() and (a[-G:] == fill).all(), what + ": guard filters"
      for a, fill in ((zg, 777.0), (fg, 99), (tx, 5.0), (tP, 5.0)):
        assert (a[0] == fill).all() and (a[T + 1] == fill).all(), what + ": guard rows"
      if not traced:
        assert (tx == 5.0).all() and (tP == 5.0).all()
      xh, Ph, zh, fl = xg[G:G + n], Pg[G:G + n], zg[1:T + 1], fg[1:T + 1]
      assert np.array_equal(fl, fr), what + ": flags (16 idle, 8 unknown kind, the gate bit of stepped entries)"
      assert np.array_equal(zh[~on], zs[~on]), what + ": z rows of idle entries pass through bit for bit"
      nv = info["never"]
      assert np.array_equal(xh[nv], x0[nv]) and np.array_equal(Ph[nv], P0[nv]), what + ": the never-stepped filter is not written back"
      for g_, w_, label in ((xh, xr, "x"), (Ph.reshape(n, -1), Pr.reshape(n, -1), "P")):
        err = np.abs(np.delete(g_, nv, 0) - np.delete(w_, nv, 0)) / np.abs(np.delete(w_, nv, 0)).max(axis=1, keepdims=True)
        assert err.max() <= tol, f"{what} {label}: {err.max():.3e} of the row maximum (bound {tol:.0e})"
      for k in spec.kinds:
        Z = k.zdim
        m = kd == k.kind
        assert_close(zh[m][:, :Z], zr[m][:, :Z], rtol=tol, atol=tol * 1e-2 * max(1.0, np.abs(zs).max()), what=what + f" kind {k.kind} y")
        assert np.array_equal(zh[m][:, Z:], zs[m][:, Z:]), what + f" kind {k.kind}: z columns beyond Z"
      if traced:
        for g_, w_, label in ((tx[1:T + 1].reshape(T * n, -1), txr.reshape(T * n, -1), "trace x"), (tP[1:T + 1].reshape(T * n, -1), tPr.reshape(T * n, -1), "trace P")):
          err = np.abs(g_ - w_) / np.abs(w_).max(axis=1, keepdims=True)
          assert err.max() <= tol, f"{what} {label}: {err.max():.3e} of the row maximum (bound {tol:.0e})"
        live = np.ones(n, dtype=bool)
        live[nv] = False
        assert np.array_equal(tx[T][live], xh[live]) and np.array_equal(tP[T][live], Ph[live]), what + ": last trace row"
        # dense trace: an idle entry's row repeats the row before it
        idle = ~on[1:]
        assert np.array_equal(tx[2:T + 1][idle], tx[1:T][idle]) and np.array_equal(tP[2:T + 1][idle], tP[1:T][idle]), what + ": trace rows of idle entries"
      got[fill_name, traced] = (xh.copy(), Ph.copy(), zh.copy(), fl.copy(), tx.copy(), tP.copy())
  set_lds_fill(lib, LDS_FILLS[0][1])
  for a, b in zip(got["NaN", 0][:4], got["NaN", 1][:4]):
    assert np.array_equal(a, b), f"{name}: traced and untraced kernels differ"
  for traced in (0, 1):
    for a, b, label in zip(got["NaN", traced], got["1e30", traced], ("x", "P", "y", "flags", "trace x", "trace P")):
      assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} traced={traced} {label}: the result depends on what LDS held at workgroup entry"
  if not any(k.maha_test for k in spec.kinds):
    assert not (fr[on] & 1).any()


@pytest.mark.parametrize("name", ["randz10", "rand11"])
def test_ragged_logs_run_on_the_host(tmp_path, name):
  """The logs of tests/rts_pf_cases.schedule, which make_schedule does not draw: filters without an entry, with a single one (at row 0, mid-log),
  late starts, early ends, about a third of the dts exactly 0 -- dts by forward_dts, as run_logs derives them.  T = 9, two full tiles and a ragged
  third one on two workgroups, against the oracle's walk at the lane-group bound (1e-8 of the row maximum); under both LDS fills, same bits."""
  from oracle_lib import OracleLib
  from rednose_amd.codegen import emit_wide3
  from rts_pf_cases import forward_dts, schedule
  M, spec, quat_idx = _spec(name, "wide")
  lib = _wide_library(tmp_path, spec)
  o = OracleLib(name)
  tol = 1e-8
  D, E = spec.dim_x, spec.dim_err
  FT = emit_wide3.layout(spec)[2]
  n, T, grid = 2 * FT + FT // 2 + 1, 9, 2
  kset = [k.kind for k in spec.kinds]
  zdim = {k.kind: k.zdim for k in spec.kinds}
  zmax = max(zdim.values())
  sch = schedule(n, T, kset, seed=3)
  kd = np.ascontiguousarray(sch["kinds"])
  on = stepped_mask(kd, kset)
  dts = np.ascontiguousarray(forward_dts(sch["ts_fwd"], kd, np.full(n, 0.9)))
  never = ~on.any(axis=0)
  assert never.any() and (on.sum(axis=0) == 1).any() and on.all(axis=0).any() and (dts[on] == 0.0).mean() > 0.2 and (dts[on] > 0.0).any()
  assert (~on[0] & ~never).any() and (~on[-1] & ~never).any(), "late starts and early ends"
  rng = np.random.default_rng(500 + E)
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  x_init = np.asarray(M.initial_x, dtype=np.float64)
  P_init = np.diag(M.initial_P_diag)
  Rs = {k.kind: np.ascontiguousarray(np.atleast_2d(M.obs_noise[k.kind]), dtype=np.float64) for k in spec.kinds}
  Rtab = r_table([(k.kind, k.zdim) for k in spec.kinds], Rs, zmax)
  x0 = np.tile(x_init, (n, 1)) + rng.normal(size=(n, D)) * 0.01 * np.maximum(1.0, np.abs(x_init))[None]
  A = rng.normal(size=(n, E, E)) * 0.1 * np.sqrt(np.diag(P_init))[None, :, None]
  P0 = P_init[None] + A @ A.transpose(0, 2, 1)
  Wk = rng.normal(size=(n, E, E))                               # asymmetric: the fused runs are specified on (P + P^T) / 2
  P0 = P0 + 1e-3 * np.abs(P0).max(axis=(1, 2), keepdims=True) * (Wk - Wk.transpose(0, 2, 1))
  zs = rng.normal(size=(T, n, zmax))
  for k in spec.kinds:
    for t, i in zip(*np.nonzero(kd == k.kind)):
      hx = np.zeros(k.zdim)
      o.call(f"h_{k.kind}", x0[i].copy(), np.zeros(4), hx)
      zs[t, i, :k.zdim] = hx + rng.normal(size=k.zdim) * np.sqrt(np.diag(Rs[k.kind]))
  xr, Pr, zr = x0.copy(), 0.5 * (P0 + P0.transpose(0, 2, 1)), zs.copy()
  fr, txr, tPr = oracle_walk(o, zdim, Rs, Q, kd, dts, xr, Pr, zr, quat_idx=quat_idx, trace=True)
  assert np.array_equal(fr[~on], np.full((~on).sum(), 16)) and not (fr[on] & 1).any()

  dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a, t=dp: a.ctypes.data_as(t)      # noqa: E731
  lib.host_run_pf.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, ip, dp, ctypes.c_int64, dp, dp, ctypes.c_int64, ctypes.c_int, bp, dp, dp]
  G, got = 2, {}
  for fill_name, bits in LDS_FILLS:
    set_lds_fill(lib, bits)
    xg, Pg = np.full((n + 2 * G, D), 7.5), np.full((n + 2 * G, E, E), 7.5)
    xg[G:G + n], Pg[G:G + n] = x0, P0
    zg = np.full((T + 2, n, zmax), 777.0)
    zg[1:T + 1] = zs
    fg = np.full((T + 2, n), 99, dtype=np.uint8)
    tx, tP = np.full((T + 2, n, D), 5.0), np.full((T + 2, n, E, E), 5.0)
    lib.host_run_pf(grid, 1, ptr(xg[G]), ptr(Pg[G]), ptr(Q), ptr(kd, ip), ptr(dts), T, ptr(zg[1]), ptr(Rtab), n, 0, ptr(fg[1], bp), ptr(tx[1]), ptr(tP[1]))
    what = f"{name} k_run_pf on ragged logs (LDS starts as {fill_name})"
    for a, fill in ((xg, 7.5), (Pg, 7.5)):
      assert (a[:G] == fill).all() and (a[-G:] == fill).all(), what + ": guard filters"
    for a, fill in ((zg, 777.0), (fg, 99), (tx, 5.0), (tP, 5.0)):
      assert (a[0] == fill).all() and (a[T + 1] == fill).all(), what + ": guard rows"
    xh, Ph, zh, fl = xg[G:G + n], Pg[G:G + n], zg[1:T + 1], fg[1:T + 1]
    for a in (xh, Ph, zh, tx, tP):
      assert np.isfinite(a).all(), what + ": an output is not finite"
    assert np.array_equal(fl, fr), what + ": flags (16 at idle entries)"
    assert np.array_equal(zh[~on], zs[~on]), what + ": z rows of idle entries pass through bit for bit"
    assert np.array_equal(xh[never], x0[never]) and np.array_equal(Ph[never], P0[never]), what + ": filters without an entry are not written back"
    live = ~never
    for g_, w_, label in ((xh[live], xr[live], "x"), (Ph[live].reshape(live.sum(), -1), Pr[live].reshape(live.sum(), -1), "P"),
                          (tx[1:T + 1].reshape(T * n, -1), txr.reshape(T * n, -1), "trace x"), (tP[1:T + 1].reshape(T * n, -1), tPr.reshape(T * n, -1), "trace P")):
      err = np.abs(g_ - w_) / np.abs(w_).max(axis=1, keepdims=True)
      assert err.max() <= tol, f"{what} {label}: {err.max():.3e} of the row maximum (bound {tol:.0e})"
    for k in spec.kinds:
      Z = k.zdim
      m = kd == k.kind
      assert_close(zh[m][:, :Z], zr[m][:, :Z], rtol=tol, atol=tol * 1e-2 * max(1.0, np.abs(zs).max()), what=what + f" kind {k.kind} y")
      assert np.array_equal(zh[m][:, Z:], zs[m][:, Z:]), what + f" kind {k.kind}: z columns beyond Z"
    assert np.array_equal(tx[T][live], xh[live]) and np.array_equal(tP[T][live], Ph[live]), what + ": last trace row"
    got[fill_name] = (xh.copy(), Ph.copy(), zh.copy(), fl.copy(), tx.copy(), tP.copy())
  set_lds_fill(lib, LDS_FILLS[0][1])
  for a, b, label in zip(got["NaN"], got["1e30"], ("x", "P", "y", "flags", "trace x", "trace P")):
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name} {label}: the result depends on what LDS held at workgroup entry"
