"""The fused run with a schedule per filter and a NOISE MATRIX PER ENTRY (k_run_rpf / k_run_rpf_tr: emit_small.run_pf_kernel and
emit_wide3.run_pf_kernel with r_entry=True) as WHOLE kernels on the host, in the fiber emulation of tests/test_emit_host_run_pf.py and on its
shapes.  Every entry brings its own R = s (R_kind + c v v^T); NaN fills every row of R that belongs to an idle entry or to an entry of an unknown
kind and every position beyond Z * Z of the others, and nothing of it may reach an output: in the lane-group kernel every lane walks the
predicated update of every kind present, with a pointer to its own group's row."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_close
from run_pf_cases import UNKNOWN, expected_flags_untouched, make_schedule, stepped_mask
from run_pf_r_cases import entry_matrix, entry_noise, gates_clear, oracle_walk_r
from test_emit_host import HDR, LDS_FILLS, _KERNEL_PRELUDE, _RUN_GRID, _WAVE_VOTES, _WIDE_COPIES, _fiberize, _function_text, _model, _once, _wide_model, set_lds_fill
from test_emit_host_kinds import _GXX, _SOLVERS, _attitude

pytestmark = pytest.mark.timeout(180, method="thread")

_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_run_rpf(int grid, int traced, double* x, double* P, const double* Q, const int32_t* kinds,
    const double* dts, int64_t T, double* z, const double* R, int64_t n, int norm_quats, uint8_t* flags, double* tx, double* tP) {
  if (traced) run_grid(grid, [&] { k_run_rpf_tr(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, tx, tP); });
  else run_grid(grid, [&] { k_run_rpf(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags); });
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
  assert "void k_run_rpf(" in kern and "void k_run_rpf_tr(" in kern
  rpf = kern[kern.index("R per entry"):]
  assert "s_R" not in rpf and "v_readlane" not in rpf, "no table in LDS, nothing broadcast"
  kern = kern.replace('asm volatile("" : "+v"(v));', ";")
  src = "\n".join([_KERNEL_PRELUDE, helpers, "}  // namespace rn", funcs, kern, _RUN_GRID, _ENTRY])
  cpp, lib = tmp_path / f"{spec.name}_run_rpf_host.cpp", tmp_path / f"lib{spec.name}_run_rpf_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


_WIDE_ENTRY = """
extern "C" __attribute__((visibility("default"))) void host_run_rpf(int grid, int traced, double* x, double* P, const double* Q, const int32_t* kinds,
    const double* dts, int64_t T, double* z, const double* R, int64_t n, int norm_quats, uint8_t* flags, double* tx, double* tP) {
  (void)traced;      // one kernel: the trace pointers decide
  run_grid(grid, [&] { k_run_rpf(x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, tx, tP); });
}
"""


@_once
def _wide_library(tmp_path, spec):
  from rednose_amd.codegen import emit_wide3, tuning
  hdr = open(HDR, encoding="utf-8").read()
  helpers = "\n".join(_function_text(hdr, f) for f in _SOLVERS)
  with tuning.using_model(spec):
    text = emit_wide3.kernels(spec)
  assert "void k_run_rpf(" in text and "_rows_rpf(" in text
  text = re.sub(r'asm volatile\("" : "\+v"\((\w+)\)( :: "memory")?\);', ";", text)
  text = text.replace("__builtin_amdgcn_sched_barrier", "rn::sched_barrier_")
  # (the scalar-phase functions run on the lanes that own a filter only: their wave_lds_sync() calls are scheduling boundaries, not rendezvous points)
  text = re.sub(r"(__device__ \w+ (?:void|int) scal_\w+\(.*?\n}\n)", lambda m: m.group(1).replace("rn::wave_lds_sync();", ";"), text, flags=re.S)
  prelude = _KERNEL_PRELUDE.replace("inline void pin(double&) {}", "inline void pin(double&) {}\n" + _WIDE_COPIES).replace("namespace rn {", _WAVE_VOTES + "namespace rn {", 1)
  src = "\n".join([prelude, helpers, "}  // namespace rn", text, _RUN_GRID, _WIDE_ENTRY])
  cpp, lib = tmp_path / f"{spec.name}_run_rpf_host.cpp", tmp_path / f"lib{spec.name}_run_rpf_host.so"
  cpp.write_text(_fiberize(src), encoding="utf-8")
  res = subprocess.run(_GXX + [str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-4000:]
  return ctypes.CDLL(str(lib))


# seeds at which every gate decision of the oracle's walk is clear of its threshold (run_pf_r_cases.gates_clear, asserted below)
SEED = {"attitude": 306, "rand5": 305, "kinematic9": 309, "rand11": 311, "live": 322}


@pytest.mark.parametrize("name,family", [("attitude", "small"), ("rand5", "small"), ("kinematic9", "wide"), ("rand11", "wide"), ("live", "wide")])
def test_per_entry_noise_run_on_the_host(tmp_path, name, family):
  from oracle_lib import OracleLib
  from rednose_amd.codegen import emit, emit_small
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
  assert emit.family(spec, ()) == family and emit.run_pf_r(spec, ())
  lib = (_library if family == "small" else _wide_library)(tmp_path, spec)
  o = OracleLib(name)
  # of the row maximum, DESIGN section 4: lane-per-filter emulations 1e-10, lane-group multi-step runs 1e-8
  tol = 1e-10 if family == "small" else 1e-8
  D, E = spec.dim_x, spec.dim_err
  if family == "small":
    T, FT = 2 * emit_small.run_pf_r_block(spec) + 1, 64
  else:
    from rednose_amd.codegen import emit_wide3
    T, FT = 5, emit_wide3.layout(spec)[2]
  n, grid = 2 * FT + FT // 2 + 1, 2                             # two full tiles and a ragged third one, on two workgroups
  rng = np.random.default_rng(SEED[name])
  kset = [k.kind for k in spec.kinds]
  zdim = {k.kind: k.zdim for k in spec.kinds}
  zmax = max(zdim.values())
  Q = np.ascontiguousarray(M.Q, dtype=np.float64)
  x_init = np.asarray(M.initial_x, dtype=np.float64)
  P_init = np.diag(M.initial_P_diag)
  Rs = {k.kind: np.ascontiguousarray(np.atleast_2d(M.obs_noise.get(k.kind, 0.01 * np.eye(k.zdim))), dtype=np.float64) for k in spec.kinds}
  kd, info = make_schedule(rng, T, n, kset, FT)
  on = stepped_mask(kd, kset)
  assert on.sum() * 2 >= T * n, "at least half of all entries are stepped"
  assert not on[:, info["never"]].any() and kd[info["unknown"]] == UNKNOWN and len(set(kd[:, :FT][kd[:, :FT] > 0])) == 1
  assert all((kd[:, FT:2 * FT] == k).any() for k in kset), "every kind appears in the mixed tile"
  assert abs((kd <= 0).mean() - 0.3) < 0.12, "about 30 % of the entries are idle"
  Re = entry_noise(rng, kd, zdim, Rs, zmax)
  assert np.isnan(Re[~on]).all() and np.isfinite(Re[on][:, :min(zdim.values()) ** 2]).all()
  for k in spec.kinds:
    assert np.isnan(Re[kd == k.kind][:, k.zdim ** 2:]).all()
  if zmax > 1:
    m = kd == max(zdim, key=zdim.get)
    assert (Re[m][:, 1] != 0.0).all() and np.array_equal(Re[m][:, 1], Re[m][:, zmax]), "symmetric, with off-diagonal entries"
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
  for k in spec.kinds:                                          # observations around h(x0) with the entry's own R, a fifth of them 40 sigma out
    for t, i in zip(*np.nonzero(kd == k.kind)):
      hx = np.zeros(k.zdim)
      o.call(f"h_{k.kind}", x0[i].copy(), np.zeros(4), hx)
      L = np.linalg.cholesky(entry_matrix(Re, t, i, k.zdim))
      zs[t, i, :k.zdim] = hx + L @ rng.normal(size=k.zdim) * (40.0 if rng.uniform() < 0.2 else 1.0)
  Psym = 0.5 * (P0 + P0.transpose(0, 2, 1))
  assert gates_clear(o, zdim, Re, Q, kd, dts, x0, Psym, zs, quat_idx=quat_idx), "a gate decision of the oracle within 1e-6 of the threshold: another seed"
  xr, Pr, zr = x0.copy(), Psym.copy(), zs.copy()
  fr, txr, tPr = oracle_walk_r(o, zdim, Re, Q, kd, dts, xr, Pr, zr, quat_idx=quat_idx, trace=True)
  assert np.array_equal(fr[~on], expected_flags_untouched(kd, kset)[~on])
  if any(k.maha_test for k in spec.kinds):
    assert (fr[on] & 1).any() and not (fr[on] & 1).all(), "the gate fires for some entries, not for all"

  dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_ubyte)
  ptr = lambda a, t=dp: a.ctypes.data_as(t)      # noqa: E731
  lib.host_run_rpf.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, ip, dp, ctypes.c_int64, dp, dp, ctypes.c_int64, ctypes.c_int, bp, dp, dp]
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
      Rg = Re.copy()                                                # exactly (T, n, zmax^2): a read past either end is not the kernel's to make
      lib.host_run_rpf(grid, traced, ptr(xg[G]), ptr(Pg[G]), ptr(Q), ptr(kd, ip), ptr(dts), T, ptr(zg[1]), ptr(Rg), n, int(quat_idx >= 0), ptr(fg[1], bp),
                       ptr(tx[1]) if traced else None, ptr(tP[1]) if traced else None)
      what = f"{name} {'k_run_rpf traced' if traced else 'k_run_rpf'} (LDS starts as {fill_name})"
      assert np.array_equal(Rg, Re, equal_nan=True), what + ": R is read only"
      for a in (xg, Pg, zg, tx, tP):
        assert not np.isnan(a).any(), what + ": NaN in an output (an unused row of R has reached it)"
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
