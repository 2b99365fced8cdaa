"""The fused run with a schedule per filter ({name}_batch_run_pf, BatchedEKF.run_logs): N logs replayed in one launch, against the step
walk it replaces (one batch_predict_update_kinds launch per step on a copy of the state), against batch_run on a shared schedule, against
the oracle stepping each filter through its own entries, and on the reference's logs (tests/golden/perfilter_timelines.npz), each sorted
by time.  Both kernel families: lane per filter (kinematic6, attitude) and lane group (kinematic9, live).  At the end of the file: the lane-group
kernels of randz10, randaff11, rand24 and rand8 on the ragged logs of tests/rts_pf_cases.py -- parity with the step walk and the oracle, the same bits
whatever LDS held before the call, randz10's shared table against its per-entry variances; measured maxima in profiles/run_pf_parity.json (written
under RN_WRITE_PARITY=1; the committed file is such a run's; every figure is a fraction of the tolerance it is held to)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import REPO, assert_close, golden
from run_pf_cases import expected_flags_untouched, make_schedule, oracle_walk, r_table, stepped_mask
from test_gpu_kinds import _case as _kinds_case

pytestmark = pytest.mark.gpu

SMALL = ("kinematic6", "attitude")


def _case(name):
  if name.startswith(("randaff", "randz")):      # (the seeded random filters tests/test_gpu_kinds.py does not look up)
    from examples import model_class_of
    R_ = model_class_of(name)
    Dr = int(R_.dim)

    def rstates(rng, n):
      x0 = R_.initial_x[None] + rng.normal(size=(n, Dr)) * 0.3
      A = rng.normal(size=(n, Dr, Dr)) * 0.2
      return x0, np.diag(R_.initial_P_diag)[None] + A @ A.transpose(0, 2, 1), None
    return R_, dict(dim=(Dr, Dr), quat=[]), -1, tuple(sorted(R_.obs_noise)), {k: np.atleast_2d(R_.obs_noise[k]) for k in R_.obs_noise}, rstates
  if name != "kinematic6":
    return _kinds_case(name)
  from examples.kinematic6_kf import Kinematic6Kalman as M

  def states(rng, n):
    x0 = M.initial_x[None] + rng.normal(size=(n, 6)) * 0.3
    A = rng.normal(size=(n, 6, 6)) * 0.2
    return x0, np.diag(M.initial_P_diag)[None] + A @ A.transpose(0, 2, 1), None
  return M, dict(dim=(6, 6), quat=[]), -1, (1,), {1: np.atleast_2d(M.obs_noise[1])}, states


def _filter(name, n, **more):
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  gen = ensure_generated([name])
  M, kw, qi, kinds, Rs, states = _case(name)
  D, E = kw["dim"]
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=kw["quat"], per_filter=True, **more)
  return f, M, qi, kinds, Rs, states


def _block(f):
  """Steps per block of the kernel (lane-per-filter models); 4 for the lane-group models."""
  return int(getattr(f._lib, f"{f.name}_run_unroll")()) if f.name in SMALL else 4      # pylint: disable=protected-access


def _fpw(name):
  return 64 if name in SMALL else 8


def _bounds(name):
  """(x, P) as (rtol, floor): tests/test_gpu_run_blk.py's fused-vs-fused bounds for the lane-per-filter models, tests/test_gpu_run.py's
  fused-vs-step bounds for the lane-group ones."""
  return ((1e-10, 1e-12), (1e-10, 1e-12)) if name in SMALL else ((1e-9, 1e-11), (1e-8, 1e-10))


def _times(rng, kd, t0=0.0):
  """ts (T, N) with NaN at idle entries, increasing per filter from t0, and the dts run_logs derives from them (the same subtraction)."""
  T, n = kd.shape
  ts, dts = np.full((T, n), np.nan), np.zeros((T, n))
  prev = np.full(n, t0)
  for t in range(T):
    has = kd[t] > 0
    ts[t] = np.where(has, prev + rng.uniform(0.0, 0.02, size=n), np.nan)
    dts[t] = np.where(has, ts[t] - prev, 0.0)
    prev = np.where(has, ts[t], prev)
  return ts, dts, prev


def _walk(f, x0, P0, kd, dts, zs, Rtab):
  """The path the kernel replaces, on its own copy of the state (symmetrised, the fused runs' contract): T batch_predict_update_kinds launches.
  -> (x, P, y, flags, trace_x, trace_P) as numpy arrays."""
  import torch
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  T, n = kd.shape
  x, P, Rd = t(x0), t(0.5 * (P0 + P0.transpose(0, 2, 1))), t(Rtab)
  y, fl = zs.copy(), np.zeros((T, n), dtype=np.uint8)
  tx, tP = np.zeros((T,) + x0.shape), np.zeros((T,) + P0.shape)
  for s in range(T):
    kt, a8, dt, zt, ft = t(kd[s], torch.int32), t(kd[s] > 0, torch.uint8), t(dts[s]), t(zs[s]), torch.zeros(n, dtype=torch.uint8, device=dev)
    f._call("batch_predict_update_kinds", f._p(x), f._p(P), f._p(f.Q), f._p(dt), 0.0, f._p(kt), f._p(zt), f._p(Rd), 0, n, f.norm_quats, f._p(ft), f._p(a8), f._stream())
    torch.cuda.synchronize()
    y[s], fl[s], tx[s], tP[s] = zt.cpu().numpy(), ft.cpu().numpy(), x.cpu().numpy(), P.cpu().numpy()
  return x.cpu().numpy(), P.cpu().numpy(), y, fl, tx, tP


def _inputs(name, n, T, seed, unknown=True):
  f, M, qi, kinds, Rs, states = _filter(name, n)
  rng = np.random.default_rng(seed)
  x0, P0, hx = states(rng, n)
  P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))      # symmetric to the last bit: the fused runs' (P + P^T) / 2 is then P itself
  zmax = max(f.zdims.values())      # the library's row stride of z
  kd, info = make_schedule(rng, T, n, kinds, _fpw(name))
  if not unknown and info["unknown"] is not None:
    kd[info["unknown"]] = 0
    info["unknown"] = None
  on = stepped_mask(kd, kinds)
  if T > 0:
    assert on.sum() * 2 >= T * n, "at least half of all entries are stepped"
  ts, dts, t_last = _times(rng, kd)
  zs = rng.normal(size=(T, n, zmax))
  if hx is not None:      # observations near h(x) of the state the filter starts from
    for k in kinds:
      Z = Rs[k].shape[0]
      tt_, ii_ = np.nonzero(kd == k)
      zs[tt_, ii_, :Z] = hx[k][ii_] + rng.normal(size=(tt_.size, Z)) * np.sqrt(np.diag(Rs[k]))
  return f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax


def _compare(name, what, got, want, on, zs, Rs, kd, never):
  (xb, Pb), n = _bounds(name), got[0].shape[0]
  x, P, y, fl, tx, tP = got
  xr, Pr, yr, flr, txr, tPr = want
  T = kd.shape[0]
  assert np.array_equal(fl, flr), what + ": flags (gate decisions included)"
  assert np.array_equal(y[~on], zs[~on]), what + ": z rows of idle entries, bit for bit"
  assert_close(x, xr, rtol=xb[0], floor=xb[1], what=what + " x")
  assert_close(P.reshape(n, -1), Pr.reshape(n, -1), rtol=Pb[0], floor=Pb[1], what=what + " P")
  for k, R in Rs.items():
    Z, m = R.shape[0], kd == k
    if m.any():
      assert_close(y[m][:, :Z], yr[m][:, :Z], rtol=xb[0], atol=xb[1] * 10 * max(1.0, np.abs(zs).max()), what=what + f" y kind {k}")
      assert np.array_equal(y[m][:, Z:], zs[m][:, Z:]), what + f" kind {k}: z columns beyond Z"
  if tx is not None and T > 0:
    assert_close(tx.reshape(T * n, -1), txr.reshape(T * n, -1), rtol=xb[0], floor=xb[1], what=what + " trace x")
    assert_close(tP.reshape(T * n, -1), tPr.reshape(T * n, -1), rtol=Pb[0], floor=Pb[1], what=what + " trace P")
    if never is None:
      assert np.array_equal(tx[-1], x) and np.array_equal(tP[-1], P), what + ": last trace row"


@pytest.mark.parametrize("n_case", ["1", "FPW+1", "203"])
@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9", "live"])
def test_shapes_against_the_step_walk(name, n_case):
  import torch
  n = {"1": 1, "FPW+1": _fpw(name) + 1, "203": 203}[n_case]
  probe = _filter(name, 1)[0]
  K = _block(probe)
  assert probe._has_batch_run_pf()
  for T in sorted({0, 1, K - 1, K, K + 1, 3 * K + 2}):
    f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 1000 * n + T)
    D, E = x0.shape[1], P0.shape[1]
    dev = f.device
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    Rtab = r_table([(k, f.zdims[k]) for k in f.kinds], Rs, zmax)
    want = _walk(f, x0, P0, kd, dts, zs, Rtab)
    # guard rows before and after z, the flags and both traces (two rows: the guarded views stay 16-byte aligned)
    G = 2
    zg = torch.full((T + 2 * G, n, zmax), 777.0, dtype=torch.float64, device=dev)
    txg = torch.full((T + 2 * G, n, D), 5.0, dtype=torch.float64, device=dev)
    tPg = torch.full((T + 2 * G, n, E, E), 5.0, dtype=torch.float64, device=dev)
    fg = torch.full((T + 2 * G, n), 99, dtype=torch.uint8, device=dev)
    zg[G:G + T] = t(zs)
    Ps = 0.5 * (P0 + P0.transpose(0, 2, 1))
    f.init_state(x0, Ps, 0.0)
    what = f"{name} n={n} T={T}"
    kdd, dtd, Rd = t(kd if T else np.zeros((1, n)), torch.int32), t(dts if T else np.zeros((1, n))), t(Rtab)      # (an empty tensor has no address: T == 0 still wants pointers)
    f._call("batch_run_pf", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(kdd), f._p(dtd), T, f._p(zg[G:]), f._p(Rd), n, f.norm_quats, f._p(fg[G:]),
            f._p(txg[G:]), f._p(tPg[G:]), f._stream())
    torch.cuda.synchronize()
    fl = fg[G:G + T].cpu().numpy()
    assert bool((fg[:G] == 99).all()) and bool((fg[G + T:] == 99).all()), what + ": guard rows of the flags"
    for a, fill in ((zg, 777.0), (txg, 5.0), (tPg, 5.0)):
      assert bool((a[:G] == fill).all()) and bool((a[G + T:] == fill).all()), what + ": guard rows"
    got = (f.state(), f.covs(), zg[G:G + T].cpu().numpy(), fl, txg[G:G + T].cpu().numpy(), tPg[G:G + T].cpu().numpy())
    if T == 0:
      assert np.array_equal(got[0], x0) and np.array_equal(got[1], Ps)
      continue
    assert np.array_equal(fl[~on], expected_flags_untouched(kd, kinds)[~on]), what + ": 16 at idle entries, 8 at the unknown kind"
    if info["unknown"] is not None:
      assert fl[info["unknown"]] == 8
    nv = info["never"]
    if nv is not None:
      assert np.array_equal(got[0][nv], x0[nv]) and np.array_equal(got[1][nv], Ps[nv]), what + ": the never-stepped filter, bit for bit"
    _compare(name, what, got, want, on, zs, Rs, kd, nv)


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9"])
def test_never_stepped_filter_keeps_an_asymmetric_covariance(name):
  """The kernel reads (P + P^T) / 2; a filter without a stepped entry is not written back, so its covariance leaves as it came, skew part included."""
  import torch
  n, T = _fpw(name) + 1, 3
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 77, unknown=False)
  rng = np.random.default_rng(1)
  W = rng.normal(size=P0.shape)
  Pa = P0 + 1e-3 * (W - W.transpose(0, 2, 1))
  f.init_state(x0, Pa, 0.0)
  f.run_logs(ts, kd, zs.copy(), Rs)
  torch.cuda.synchronize()
  nv = info["never"]
  assert np.array_equal(f.covs()[nv], Pa[nv]) and np.array_equal(f.state()[nv], x0[nv])
  stepped = on.any(axis=0)
  P = f.covs()[stepped]
  assert np.abs(P - P.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(P).max()


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9"])
def test_shared_schedule_is_a_special_case(name):
  """The same (T,) schedule replicated to (T, n) gives batch_run's x, P, y, flags and trace."""
  import torch
  n = 203
  f, M, qi, kinds, Rs, states = _filter(name, n)
  g = _filter(name, n)[0]
  K = _block(f)
  T = 2 * K + 1
  rng = np.random.default_rng(9)
  x0, P0, _ = states(rng, n)
  zmax = max(f.zdims.values())
  sched = np.array([kinds[t % len(kinds)] for t in range(T)], dtype=np.int32)
  ts = np.cumsum(rng.uniform(0.005, 0.03, size=T))
  zs = rng.normal(size=(T, n, zmax))
  f.init_state(x0, P0, 0.0)
  g.init_state(x0, P0, 0.0)
  ya, txa, tPa, fa = f.run(ts, sched, zs.copy(), Rs, trace=True, flags=True)
  yb, txb, tPb, fb = g.run_logs(np.tile(ts[:, None], (1, n)), np.tile(sched[:, None], (1, n)), zs.copy(), Rs, trace=True, flags=True)
  torch.cuda.synchronize()
  kd = np.tile(sched[:, None], (1, n))
  _compare(name, f"{name} shared schedule", (g.state(), g.covs(), yb.cpu().numpy(), fb.cpu().numpy(), txb.cpu().numpy(), tPb.cpu().numpy()),
           (f.state(), f.covs(), ya.cpu().numpy(), fa.cpu().numpy(), txa.cpu().numpy(), tPa.cpu().numpy()), np.ones((T, n), dtype=bool), zs, Rs, kd, None)
  assert np.array_equal(g.filter_times().cpu().numpy(), np.full(n, ts[-1]))


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9"])
def test_against_the_oracle(name):
  """256 filters stepped through their own entries with OracleLib.batch_step, at the tolerances tests/test_gpu_kinds.py uses for these models."""
  import torch
  from oracle_lib import OracleLib
  n = 300
  f0 = _filter(name, 1)[0]
  T = _block(f0) + 1
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 31, unknown=False)
  f.init_state(x0, P0, 0.0)
  y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), Rs, trace=True, flags=True)
  torch.cuda.synchronize()
  sub = np.arange(256)
  xo, Po, zo = x0[sub].copy(), P0[sub].copy(), np.ascontiguousarray(zs[:, sub])
  fr, txr, tPr = oracle_walk(OracleLib(name), {k: Rs[k].shape[0] for k in kinds}, Rs, M.Q, kd[:, sub], dts[:, sub], xo, Po, zo, quat_idx=qi, trace=True)
  what = f"{name} vs oracle"
  assert np.array_equal(fl.cpu().numpy()[:, sub], fr)
  assert_close(f.state()[sub], xo, rtol=1e-11, floor=1e-13, what=what + " x")
  assert_close(f.covs()[sub].reshape(256, -1), Po.reshape(256, -1), rtol=1e-11, floor=1e-13, what=what + " P")
  Y = y.cpu().numpy()[:, sub]
  for k in kinds:
    Z, m = Rs[k].shape[0], kd[:, sub] == k
    assert_close(Y[m][:, :Z], zo[m][:, :Z], rtol=1e-11, atol=1e-13 * max(1.0, np.abs(zs).max()), what=what + f" y kind {k}")
  assert_close(tx.cpu().numpy()[:, sub].reshape(T * 256, -1), txr.reshape(T * 256, -1), rtol=1e-11, floor=1e-13, what=what + " trace x")
  assert_close(tP.cpu().numpy()[:, sub].reshape(T * 256, -1), tPr.reshape(T * 256, -1), rtol=1e-11, floor=1e-13, what=what + " trace P")


def _sorted_logs(t, kind, z):
  """(N, J) arrival-ordered logs -> (T, N) time-ordered ones (stable), padded with idle entries behind each log's end."""
  N, J = t.shape
  T = int((kind > 0).sum(axis=1).max())
  ts, kd, zs = np.full((T, N), np.nan), np.zeros((T, N), dtype=np.int32), np.zeros((T, N) + z.shape[2:])
  for i in range(N):
    idx = np.nonzero(kind[i] > 0)[0]
    order = idx[np.argsort(t[i, idx], kind="stable")]
    ts[:order.size, i], kd[:order.size, i], zs[:order.size, i] = t[i, order], kind[i, order], z[i, order]
  return ts, kd, zs


def test_the_reference_logs_in_one_call_each():
  """tests/golden/perfilter_timelines.npz: the reference's rewind + replay of a log IS the in-order sequence, so each log sorted by time and
  run through run_logs in one call ends in the reference's final state.  Part B: 10 logs of the 9-state model; part A: 12 logs x 700
  observations of the 2-state model, minus the one observation the reference ignored."""
  import torch
  from examples import ensure_generated
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  gen = ensure_generated(["kinematic", "kinematic9"])
  g = golden("perfilter_timelines.npz")
  # part B
  NB = g["B_t"].shape[0]
  ts, kd, zs = _sorted_logs(g["B_t"], g["B_kind"], g["B_z"])
  f = BatchedEKF(gen, "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=NB, per_filter=True)
  Rs = {k: K9.obs_noise[k] for k in (1, 2, 3)}
  assert f._has_batch_run_pf()
  f.run_logs(ts, kd, zs.copy(), Rs)
  torch.cuda.synchronize()
  assert_close(f.state(), g["B_x"][:, -1], rtol=1e-8, floor=1e-10, what="part B final x")
  assert_close(f.covs().reshape(NB, -1), g["B_P"][:, -1].reshape(NB, -1), rtol=1e-8, floor=1e-10, what="part B final P")
  assert np.array_equal(f.filter_times().cpu().numpy(), np.nanmax(ts, axis=0))
  # part A
  NA = g["A_t"].shape[0]
  ts, kd, zs = _sorted_logs(g["A_t"], (~g["A_none"]).astype(np.int32), g["A_z"][:, :, None])
  assert (kd > 0).sum() == g["A_t"].size - 1 and g["A_t"].shape == (12, 700)
  f = BatchedEKF(gen, "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.eye(2), 2, 2, batch=NA, per_filter=True)
  assert f._has_batch_run_pf()
  f.run_logs(ts, kd, zs.copy(), {1: np.array([[0.1**2]])})
  torch.cuda.synchronize()
  assert_close(f.state(), g["A_x_final"], rtol=1e-8, floor=1e-10, what="part A final x")
  assert_close(f.covs().reshape(NA, -1), g["A_P_final"].reshape(NA, -1), rtol=1e-8, floor=1e-10, what="part A final P")
  assert np.array_equal(f.filter_times().cpu().numpy(), np.nanmax(ts, axis=0))
  # an unsorted log is refused, and so is one that starts before its filter's time
  bad_t = ts.copy()
  bad_t[[3, 4], 5] = bad_t[[4, 3], 5]
  f.init_state(np.array([0.5, 0.0]), np.eye(2), None)
  with pytest.raises(KalmanError, match=r"filter 5, step 4.*sort the log"):
    f.run_logs(bad_t, kd, zs.copy(), {1: np.array([[0.1**2]])})
  f.init_state(np.array([0.5, 0.0]), np.eye(2), np.full(NA, 1e9))
  with pytest.raises(KalmanError, match="sort the log"):
    f.run_logs(ts, kd, zs.copy(), {1: np.array([[0.1**2]])})
  with pytest.raises(KeyError):
    f.run_logs(ts, kd * 7, zs.copy(), {1: np.array([[0.1**2]])})


def test_run_logs_plumbing():
  """A library "without" the kernel and exact=True walk the same schedule to the same results; the rings are empty afterwards; a following
  in-order call continues from each filter's own time."""
  import torch
  name, n, T = "attitude", 131, 9
  out = {}
  for mode in ("kernel", "no kernel", "exact"):
    f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 5, unknown=False)
    f.init_state(x0, P0, 0.0)
    assert f._has_batch_run_pf()
    if mode == "no kernel":
      f._has_batch_run_pf = lambda: False
    y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), Rs, trace=True, flags=True, exact=mode == "exact")
    torch.cuda.synchronize()
    assert f.pf_stats == {"fast": 0, "legacy": 0} and f.rewind_stats == {"device": 0, "torch": 0}
    out[mode] = (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy())
    assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
  _compare(name, "kernel vs walk", out["kernel"], out["no kernel"], on, zs, Rs, kd, info["never"])
  for a, b in zip(out["no kernel"], out["exact"]):      # a symmetric P0: the two walks launch the same kernels on the same numbers
    assert np.array_equal(a, b)
  # rings, and the call after the run
  rng = np.random.default_rng(2)
  z_first, z_next = rng.normal(size=(n, zmax)), rng.normal(size=(n, zmax))
  k_first, k_next = rng.choice(np.array(kinds, dtype=np.int32), size=n), rng.choice(np.array(kinds + (0,), dtype=np.int32), size=n)
  res = []
  for fused in (True, False):
    f = _filter(name, n, rewind_to_keep=8, device_timeline=True)[0]
    f.init_state(x0, P0, np.full(n, -0.01))
    f.predict_and_update_kinds(np.zeros(n), k_first, z_first.copy(), Rs)
    assert int(f._ring["length"].sum()) == n
    if fused:
      f.run_logs(ts, kd, zs.copy(), Rs)
      assert int(f._ring["length"].sum()) == 0 and int(f._ring["head"].sum()) == 0
      assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
    else:
      for s in range(T):
        f.predict_and_update_kinds(np.nan_to_num(ts[s]), kd[s], zs[s].copy(), Rs)
    f.predict_and_update_kinds(t_last + 0.01, k_next, z_next.copy(), Rs)
    torch.cuda.synchronize()
    assert f.pf_stats["legacy"] == 0
    res.append((f.state(), f.covs(), f.filter_times().cpu().numpy()))
  (xb, Pb) = _bounds(name)
  assert_close(res[0][0], res[1][0], rtol=xb[0], floor=xb[1], what="state after the call behind the run")
  assert_close(res[0][1].reshape(n, -1), res[1][1].reshape(n, -1), rtol=Pb[0], floor=Pb[1], what="covariance after the call behind the run")
  assert np.array_equal(res[0][2], res[1][2])


# ---- the lane-group kernels no other test launches: randz10 (a 9-dimensional kind: 81-entry R / HPH / S / L per lane, two observation entries per
# lane), randaff11 (affine: predict(0) is not the identity), rand24 (16 lanes per filter), rand8 -- on the logs of tests/rts_pf_cases.schedule:
# filters without an entry, with a single one, late starts, early ends, about a third of the dts exactly 0 ------------------------------------------

WIDE_PF = ["randz10", "randaff11", "rand24", "rand8"]
T_LOG, T0_LOG = 9, 0.9
ORACLE_BOUND = (1e-11, 1e-13)      # test_against_the_oracle's (rtol, floor), x and P alike
_PARITY = {}


def _record(key, **figures):
  """The measured maxima, as fractions of the tolerance they are held to (assert_close's rtol |want| + floor max|row|): below 1 means within bounds."""
  _PARITY[key] = {k: float(v) for k, v in figures.items()}
  if os.environ.get("RN_WRITE_PARITY"):
    fn = os.path.join(REPO, "profiles", "run_pf_parity.json")
    old = {}
    if os.path.exists(fn):
      with open(fn, encoding="utf-8") as f:
        old = json.load(f)
    old.update(_PARITY)
    with open(fn, "w", encoding="utf-8") as f:
      json.dump(old, f, indent=1, sort_keys=True)
      f.write("\n")


def _of_tol(got, want, rtol, floor, atol=0.0):
  """max |got - want| / (assert_close's tolerance)"""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  if got.size == 0:
    return 0.0
  tol = rtol * np.abs(want) + floor * np.max(np.abs(want), axis=-1, keepdims=True) + atol + 1e-300
  return float(np.max(np.abs(got - want) / tol))


def _fpw_wide(name):
  """Filters per wavefront of the lane-group fused run, as the generated text states it."""
  from examples import GENERATED_DIR, ensure_generated
  ensure_generated([name])
  with open(os.path.join(GENERATED_DIR, f"{name}.hip"), encoding="utf-8") as fh:
    return int(re.search(r"constexpr int FPWR = (\d+);", fh.read()).group(1))


def _lds():
  """tools/liblds_poison.so (lds_poison: the NaN pattern conftest fills LDS with; lds_fill: any 64-bit pattern), None where it is not built."""
  fn = os.path.join(REPO, "tools", "liblds_poison.so")
  if not os.path.exists(fn):
    return None
  lib = ctypes.CDLL(fn)
  lib.lds_poison.argtypes, lib.lds_poison.restype = [ctypes.c_void_p], None
  lib.lds_fill.argtypes, lib.lds_fill.restype = [ctypes.c_uint64, ctypes.c_void_p], None
  return lib


_LOGS = {}


def _log_inputs(name, n, T=T_LOG, seed=3):
  """One seeded case per (model, n), shared by the tests below (which copy what a call consumes): states with a symmetric P0, the ragged logs, observations."""
  from rts_pf_cases import forward_dts, schedule
  if (name, n, T) not in _LOGS:
    M, kw, qi, kinds, Rs, states = _case(name)
    rng = np.random.default_rng(seed)
    x0, P0, hx = states(rng, n)
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    sch = schedule(n, T, kinds, seed=seed)
    kd = sch["kinds"]
    zmax = max(R.shape[0] for R in Rs.values())
    zs = rng.normal(size=(T, n, zmax)) * 0.5
    if hx is not None:      # observations near h(x) of the state the filter starts from
      for k in kinds:
        Z = Rs[k].shape[0]
        tt_, ii_ = np.nonzero(kd == k)
        zs[tt_, ii_, :Z] = hx[k][ii_] + rng.normal(size=(tt_.size, Z)) * np.sqrt(np.diag(Rs[k]))
    dts = forward_dts(sch["ts_fwd"], kd, np.full(n, T0_LOG))
    on = stepped_mask(kd, kinds)
    assert np.array_equal(on, kd > 0)
    if n >= 7:
      assert (~on.any(axis=0)).any() and (on.sum(axis=0) == 1).any() and (dts[on] == 0.0).any() and (dts[on] > 0.0).any()
    _LOGS[name, n, T] = dict(M=M, qi=qi, kinds=kinds, Rs=Rs, x0=x0, P0=P0, ts=sch["ts_fwd"], kd=kd, zs=zs, dts=dts, on=on)
  return _LOGS[name, n, T]


def _replay(f, c, Rs=None, exact=False):
  """run_logs(trace=True, flags=True) from the case's start -> ((x, P, y, flags, trace_x, trace_P) as numpy arrays, the entry points launched)"""
  import torch
  n = c["x0"].shape[0]
  f.init_state(c["x0"], c["P0"], np.full(n, T0_LOG))
  real, seen = f._call, []

  def spy(sym, *args):
    seen.append(sym)
    return real(sym, *args)
  f._call = spy
  y, tx, tP, fl = f.run_logs(c["ts"], c["kd"], c["zs"].copy(), c["Rs"] if Rs is None else Rs, trace=True, flags=True, exact=exact)
  torch.cuda.synchronize()
  del f._call
  return (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy()), seen


@pytest.mark.parametrize("n_case", ["1", "FPW+1", "130"])
@pytest.mark.parametrize("name", WIDE_PF)
def test_lane_group_logs_against_the_step_walk_and_the_oracle(name, n_case):
  """One batch_run_pf launch against run_logs(exact=True) on a second object at test_shapes_against_the_step_walk's lane-group bounds, and
  against the oracle stepping at most 16 filters (the first two tiles' worth and the ragged end) through their own entries at
  test_against_the_oracle's.  Flags equal; idle rows of y and the filters without an entry bit for bit."""
  from oracle_lib import OracleLib
  n = {"1": 1, "FPW+1": _fpw_wide(name) + 1, "130": 130}[n_case]
  c = _log_inputs(name, n)
  T, kd, on, zs, Rs, kinds = T_LOG, c["kd"], c["on"], c["zs"], c["Rs"], c["kinds"]
  f, g = _filter(name, n)[0], _filter(name, n)[0]
  assert f._has_batch_run_pf()
  got, seen = _replay(f, c)
  assert seen == ["batch_run_pf"], seen
  want, walked = _replay(g, c, exact=True)
  assert "batch_run_pf" not in walked and len(walked) >= T
  what = f"{name} n={n} T={T}"
  for a in got:
    assert np.isfinite(a.astype(np.float64)).all(), what + ": an output is not finite"
  never = ~on.any(axis=0)
  assert np.array_equal(got[0][never], c["x0"][never]) and np.array_equal(got[1][never], c["P0"][never]), what + ": filters without an entry, bit for bit"
  assert np.array_equal(got[3][~on], expected_flags_untouched(kd, kinds)[~on]), what + ": 16 at idle entries"
  (xb, Pb) = _bounds(name)
  fig = dict(x_walk=_of_tol(got[0], want[0], *xb), P_walk=_of_tol(got[1].reshape(n, -1), want[1].reshape(n, -1), *Pb),
             trace_x_walk=_of_tol(got[4].reshape(T * n, -1), want[4].reshape(T * n, -1), *xb),
             trace_P_walk=_of_tol(got[5].reshape(T * n, -1), want[5].reshape(T * n, -1), *Pb))
  # the oracle on a subset
  sub = np.unique(np.r_[np.arange(min(n, 8)), np.arange(max(0, n - 8), n)])
  assert sub.size <= 16
  m = sub.size
  xo, Po, zo = c["x0"][sub].copy(), c["P0"][sub].copy(), np.ascontiguousarray(zs[:, sub])
  fr, txr, tPr = oracle_walk(OracleLib(name), {k: Rs[k].shape[0] for k in kinds}, Rs, np.asarray(c["M"].Q, dtype=np.float64), np.ascontiguousarray(kd[:, sub]),
                             np.ascontiguousarray(c["dts"][:, sub]), xo, Po, zo, quat_idx=c["qi"], trace=True)
  ro, fo = ORACLE_BOUND
  fig.update(x_oracle=_of_tol(got[0][sub], xo, ro, fo), P_oracle=_of_tol(got[1][sub].reshape(m, -1), Po.reshape(m, -1), ro, fo),
             trace_x_oracle=_of_tol(got[4][:, sub].reshape(T * m, -1), txr.reshape(T * m, -1), ro, fo),
             trace_P_oracle=_of_tol(got[5][:, sub].reshape(T * m, -1), tPr.reshape(T * m, -1), ro, fo))
  Y = got[2][:, sub]
  fig["y_oracle"] = max([_of_tol(Y[kd[:, sub] == k][:, :Rs[k].shape[0]], zo[kd[:, sub] == k][:, :Rs[k].shape[0]], ro, 0.0, atol=fo * max(1.0, np.abs(zs).max()))
                         for k in kinds])
  print(what, {k: f"{v:.3e}" for k, v in fig.items()}, "(fractions of the tolerance)")
  _record(f"parity/{name}/n={n}", **fig)
  _compare(name, what + " vs the step walk", got, want, on, zs, Rs, kd, True)
  live = ~never
  assert np.array_equal(got[4][-1][live], got[0][live]) and np.array_equal(got[5][-1][live], got[1][live]), what + ": last trace row"
  assert np.array_equal(got[3][:, sub], fr), what + ": flags vs the oracle"
  assert_close(got[0][sub], xo, rtol=ro, floor=fo, what=what + " vs oracle x")
  assert_close(got[1][sub].reshape(m, -1), Po.reshape(m, -1), rtol=ro, floor=fo, what=what + " vs oracle P")
  for k in kinds:
    Z, sel = Rs[k].shape[0], kd[:, sub] == k
    if sel.any():
      assert_close(Y[sel][:, :Z], zo[sel][:, :Z], rtol=ro, atol=fo * max(1.0, np.abs(zs).max()), what=what + f" vs oracle y kind {k}")
  assert_close(got[4][:, sub].reshape(T * m, -1), txr.reshape(T * m, -1), rtol=ro, floor=fo, what=what + " vs oracle trace x")
  assert_close(got[5][:, sub].reshape(T * m, -1), tPr.reshape(T * m, -1), rtol=ro, floor=fo, what=what + " vs oracle trace P")


@pytest.mark.parametrize("name", WIDE_PF + ["kinematic9", "live"])
def test_same_call_same_bits_whatever_lds_held(name):
  """Three calls on identical inputs from a re-initialised object: behind the NaN pattern of lds_poison, behind lds_fill(1e30) and behind
  lds_fill(-0.0).  Every output finite and the same bits in all three: nothing the kernel computes comes from LDS (or a register) it did not write.
  A comparison of values -- three calls, no loop."""
  import torch
  n = 130
  c = _log_inputs(name, n)
  f = _filter(name, n)[0]
  assert f._has_batch_run_pf()
  lds = _lds()
  bits = lambda v: int(np.float64(v).view(np.uint64))      # noqa: E731
  out = []
  for label, refill in (("lds_poison", lambda: lds.lds_poison(None)), ("lds_fill(1e30)", lambda: lds.lds_fill(bits(1e30), None)),
                        ("lds_fill(-0.0)", lambda: lds.lds_fill(bits(-0.0), None))):
    if lds is not None:
      refill()
      torch.cuda.synchronize()
    got, seen = _replay(f, c)
    assert seen == ["batch_run_pf"], (label, seen)
    out.append((label, got))
  names = ("x", "P", "y", "flags", "trace_x", "trace_P")
  for label, got in out:
    for a, nm in zip(got, names):
      assert np.isfinite(a.astype(np.float64)).all(), f"{name} behind {label}: {nm} is not finite ({int((~np.isfinite(a.astype(np.float64))).sum())} entries)"
  for label, got in out[1:]:
    for a, b, nm in zip(out[0][1], got, names):
      diff = (a.view(np.uint64) != b.view(np.uint64)) if a.dtype == np.float64 else (a != b)
      assert not diff.any(), f"{name}: {nm} behind {label} differs from the call behind {out[0][0]} in {int(diff.sum())} of {diff.size} entries"


def test_randz10_shared_table_against_per_entry_variances():
  """The same log through batch_run_pf (the shared diagonal table) and through batch_run_pf_rd (the same variances per entry), at the bounds
  tests/test_gpu_run_pf_rd.py::test_against_batch_run_pf_r_on_the_expanded_rows holds two flavours to (the lane-per-filter ones, equal flags).
  With the parity test above: a defect of the TABLE flavour's compiled code fails here and there, one of the shared structure fails there only."""
  name, n = "randz10", 130
  c = _log_inputs(name, n)
  T, kd, on, Rs = T_LOG, c["kd"], c["on"], c["Rs"]
  f, g = _filter(name, n)[0], _filter(name, n)[0]
  assert f._has_batch_run_pf() and g._has_batch_run_pf_rd()
  for R in Rs.values():
    assert not (R - np.diag(np.diag(R))).any()
  Rv = {k: np.ascontiguousarray(np.broadcast_to(np.diag(Rs[k]), (T, n, Rs[k].shape[0]))) for k in Rs}
  tab, seen_t = _replay(f, c)
  var, seen_v = _replay(g, c, Rs=Rv)
  assert seen_t == ["batch_run_pf"] and seen_v == ["batch_run_pf_rd"], (seen_t, seen_v)
  assert np.array_equal(tab[3], var[3]), "flags"
  (xb, Pb) = _bounds("kinematic6")
  _record(f"flavours/{name}/n={n}", x=_of_tol(tab[0], var[0], *xb), P=_of_tol(tab[1].reshape(n, -1), var[1].reshape(n, -1), *Pb),
          trace_x=_of_tol(tab[4].reshape(T * n, -1), var[4].reshape(T * n, -1), *xb), trace_P=_of_tol(tab[5].reshape(T * n, -1), var[5].reshape(T * n, -1), *Pb))
  print(name, "table vs variances", _PARITY[f"flavours/{name}/n={n}"])
  _compare("kinematic6", f"{name} table vs variances per entry", tab, var, on, c["zs"], Rs, kd, True)
