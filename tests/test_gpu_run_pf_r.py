"""The fused run with a schedule per filter and a noise matrix per entry ({name}_batch_run_pf_r, BatchedEKF.run_logs with per-entry Rs), against
the step walk it replaces: T batch_predict_update_kinds launches with R[t] and r_per_filter = 1 on a copy of the state.  R is allocated at exactly
(T, n, zmax^2) and holds NaN wherever the contract says "never used": the rows of idle entries and of entries with an unknown kind, and the
positions beyond Z * Z of the others.  Both kernel families: lane per filter (kinematic6, attitude) and lane group (kinematic9, live)."""
import os
import re

import numpy as np
import pytest

from conftest import assert_close
from run_pf_cases import expected_flags_untouched, r_table
from run_pf_r_cases import entry_noise, oracle_walk_r, table_rows
from test_gpu_run_pf import SMALL, _bounds, _compare, _filter, _fpw, _inputs

pytestmark = pytest.mark.gpu


def _block(f):
  """Steps per block of k_run_rpf (lane-per-filter models: the title line of the generated kernel states it); 4 for the lane-group models."""
  if f.name not in SMALL:
    return 4
  from examples import GENERATED_DIR
  with open(os.path.join(GENERATED_DIR, f"{f.name}.hip"), encoding="utf-8") as fh:
    return int(re.search(r"R per entry \(gR \(T, n, \d+\)\): blocks of (\d+) steps", fh.read()).group(1))


def _noise(name, seed, kd, f, Rs, zmax):
  return entry_noise(np.random.default_rng(seed + 17), kd, {k: f.zdims[k] for k in Rs}, Rs, zmax)


def _walk_r(f, x0, P0, kd, dts, zs, Re):
  """The path the kernel replaces, on its own copy of the state (symmetrised): T batch_predict_update_kinds launches with R[t], r_per_filter = 1.
  -> (x, P, y, flags, trace_x, trace_P) as numpy arrays."""
  import torch
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  T, n = kd.shape
  x, P = t(x0), t(0.5 * (P0 + P0.transpose(0, 2, 1)))
  y, fl = zs.copy(), np.zeros((T, n), dtype=np.uint8)
  tx, tP = np.zeros((T,) + x0.shape), np.zeros((T,) + P0.shape)
  for s in range(T):
    kt, a8, dt, zt, Rt, ft = t(kd[s], torch.int32), t(kd[s] > 0, torch.uint8), t(dts[s]), t(zs[s]), t(Re[s]), torch.zeros(n, dtype=torch.uint8, device=dev)
    f._call("batch_predict_update_kinds", f._p(x), f._p(P), f._p(f.Q), f._p(dt), 0.0, f._p(kt), f._p(zt), f._p(Rt), 1, n, f.norm_quats, f._p(ft), f._p(a8), f._stream())
    torch.cuda.synchronize()
    y[s], fl[s], tx[s], tP[s] = zt.cpu().numpy(), ft.cpu().numpy(), x.cpu().numpy(), P.cpu().numpy()
  return x.cpu().numpy(), P.cpu().numpy(), y, fl, tx, tP


def _run_r(f, x0, Ps, kd, dts, zs, Re, G=2):
  """One batch_run_pf_r launch with guard rows around z, the flags and both traces; R at exactly (T, n, zmax^2).  -> (got, guards_ok)"""
  import torch
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  T, n = kd.shape
  D, E, zmax = x0.shape[1], Ps.shape[1], zs.shape[2]
  zg = torch.full((T + 2 * G, n, zmax), 777.0, dtype=torch.float64, device=dev)
  txg = torch.full((T + 2 * G, n, D), 5.0, dtype=torch.float64, device=dev)
  tPg = torch.full((T + 2 * G, n, E, E), 5.0, dtype=torch.float64, device=dev)
  fg = torch.full((T + 2 * G, n), 99, dtype=torch.uint8, device=dev)
  zg[G:G + T] = t(zs)
  f.init_state(x0, Ps, 0.0)
  # (an empty tensor has no address: T == 0 still wants pointers)
  kdd, dtd, Rd = t(kd if T else np.zeros((1, n)), torch.int32), t(dts if T else np.zeros((1, n))), t(Re if T else np.zeros((1, n, zmax * zmax)))
  assert Rd.numel() == max(T, 1) * n * zmax * zmax
  f._call("batch_run_pf_r", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(kdd), f._p(dtd), T, f._p(zg[G:]), f._p(Rd), n, f.norm_quats, f._p(fg[G:]),
          f._p(txg[G:]), f._p(tPg[G:]), f._stream())
  torch.cuda.synchronize()
  ok = bool((fg[:G] == 99).all()) and bool((fg[G + T:] == 99).all())
  for a, fill in ((zg, 777.0), (txg, 5.0), (tPg, 5.0)):
    ok = ok and bool((a[:G] == fill).all()) and bool((a[G + T:] == fill).all())
  return (f.state(), f.covs(), zg[G:G + T].cpu().numpy(), fg[G:G + T].cpu().numpy(), txg[G:G + T].cpu().numpy(), tPg[G:G + T].cpu().numpy()), ok


@pytest.mark.parametrize("n_case", ["1", "FPW+1", "203"])
@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9", "live"])
def test_shapes_against_the_step_walk(name, n_case):
  n = {"1": 1, "FPW+1": _fpw(name) + 1, "203": 203}[n_case]
  probe = _filter(name, 1)[0]
  K = _block(probe)
  assert probe._has_batch_run_pf_r()
  for T in sorted({0, 1, K - 1, K, K + 1, 3 * K + 2}):
    seed = 1000 * n + T
    f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, seed)
    Ps = 0.5 * (P0 + P0.transpose(0, 2, 1))
    Re = _noise(name, seed, kd, f, Rs, zmax)
    what = f"{name} n={n} T={T}"
    got, guards = _run_r(f, x0, Ps, kd, dts, zs, Re)
    assert guards, what + ": guard rows"
    if T == 0:
      assert np.array_equal(got[0], x0) and np.array_equal(got[1], Ps)
      continue
    assert np.isnan(Re[~on]).all() and (on.all() or np.isnan(Re).any())
    want = _walk_r(f, x0, P0, kd, dts, zs, Re)
    for a in got:
      assert not np.isnan(a.astype(np.float64)).any(), what + ": NaN in an output (an unused row of R has reached it)"
    fl = got[3]
    assert np.array_equal(fl[~on], expected_flags_untouched(kd, kinds)[~on]), what + ": 16 at idle entries, 8 at the unknown kind"
    if info["unknown"] is not None:
      assert fl[info["unknown"]] == 8
    nv = info["never"]
    if nv is not None:
      assert np.array_equal(got[0][nv], x0[nv]) and np.array_equal(got[1][nv], Ps[nv]), what + ": the never-stepped filter, bit for bit"
    _compare(name, what, got, want, on, zs, Rs, kd, nv)


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9", "live"])
def test_rows_filled_from_the_table_give_batch_run_pf(name):
  """The degenerate case: every entry's row holds its kind's row of the per-kind table.  The two kernels run the same arithmetic functions on the
  same numbers (they may contract FMAs differently): the lane-per-filter bounds, for both families."""
  import torch
  n = 203
  f0 = _filter(name, 1)[0]
  T = 2 * _block(f0) + 1
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 41)
  Ps = 0.5 * (P0 + P0.transpose(0, 2, 1))
  Re = table_rows(kd, [(k, f.zdims[k]) for k in kinds], Rs, zmax)
  got, guards = _run_r(f, x0, Ps, kd, dts, zs, Re)
  assert guards
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  zd, fd = t(zs), torch.zeros((T, n), dtype=torch.uint8, device=dev)
  txd, tPd = torch.zeros((T,) + x0.shape, dtype=torch.float64, device=dev), torch.zeros((T,) + Ps.shape, dtype=torch.float64, device=dev)
  kdd, dtd, Rd = t(kd, torch.int32), t(dts), t(r_table([(k, f.zdims[k]) for k in f.kinds], Rs, zmax))
  f.init_state(x0, Ps, 0.0)
  f._call("batch_run_pf", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(kdd), f._p(dtd), T, f._p(zd), f._p(Rd), n, f.norm_quats, f._p(fd), f._p(txd), f._p(tPd), f._stream())
  torch.cuda.synchronize()
  want = (f.state(), f.covs(), zd.cpu().numpy(), fd.cpu().numpy(), txd.cpu().numpy(), tPd.cpu().numpy())
  _compare("kinematic6", f"{name} table rows vs batch_run_pf", got, want, on, zs, Rs, kd, info["never"])      # (the lane-per-filter bounds)


@pytest.mark.parametrize("name", ["kinematic6_maha", "live_maha"])
def test_the_gate_reads_the_entry_noise(name):
  """The same observation, far from the prediction, in two filters in the same state whose entries differ in R by 10^4: the chi-square gate fires for
  the one with the small R and not for the other, in the kernel as in the step walk."""
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  from oracle_lib import OracleLib
  gen = ensure_generated([name])
  if name == "kinematic6_maha":
    from examples.kinematic6_kf import Kinematic6Kalman as M
    D, E, quat, kind = 6, 6, [], 1
    R0 = np.atleast_2d(M.obs_noise[1])
    x1 = np.asarray(M.initial_x, dtype=np.float64)
  else:
    from examples.live_kf import LiveKalman as M, ObservationKind as LK
    from conftest import golden
    D, E, quat, kind = 23, 22, [3], int(LK.ECEF_POS)
    R0 = np.atleast_2d(M.obs_noise[kind])
    x1 = golden("live_single_steps.npz")["x_in"][0]
  n, T = 2, 1
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat, per_filter=True,
                 maha_test_kinds=[kind])
  assert f._has_batch_run_pf_r()
  Z, zmax = f.zdims[kind], max(f.zdims.values())
  P1 = np.diag(M.initial_P_diag) * 1e-6      # a confident filter: the innovation covariance is R's
  hx = np.zeros(Z)
  OracleLib(name).call(f"h_{kind}", x1.copy(), np.zeros(4), hx)
  sig = np.sqrt(np.diag(R0))
  zs = np.zeros((T, n, zmax))
  zs[0, :, :Z] = hx + 10.0 * sig             # 10 sigma of the small R, 0.1 sigma of the large one
  Re = np.full((T, n, zmax * zmax), np.nan)
  Re[0, 0, :Z * Z] = R0.reshape(-1)
  Re[0, 1, :Z * Z] = (1e4 * R0).reshape(-1)
  kd, dts = np.full((T, n), kind, dtype=np.int32), np.zeros((T, n))
  x0, P0 = np.tile(x1, (n, 1)), np.tile(P1, (n, 1, 1))
  got, guards = _run_r(f, x0, P0, kd, dts, zs, Re)
  want = _walk_r(f, x0, P0, kd, dts, zs, Re)
  assert guards
  assert got[3][0, 0] & 1 and not got[3][0, 1] & 1, got[3]
  assert np.array_equal(got[3], want[3])
  assert np.abs(got[0][1] - x0[1]).max() > 0.0, "the accepted observation moves its filter"


def test_run_logs_plumbing():
  """run_logs with per-entry noise: a dict with one kind per entry and one shared, the (T, N, zmax, zmax) tensor, exact=True and a library "without"
  the kernel agree; filter_times() and the ring state are as documented; a (Z, Z)-only dict still launches batch_run_pf; wrong shapes are named."""
  import torch
  from rednose_amd.helpers import KalmanError
  name, n, T = "attitude", 131, 9
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 5, unknown=False)
  Z = {k: f.zdims[k] for k in kinds}
  k_entry, k_shared = kinds[0], kinds[1]
  Re = _noise(name, 5, kd, f, Rs, zmax)
  Re[kd == k_shared, :Z[k_shared] ** 2] = Rs[k_shared].reshape(-1)
  R4 = np.full((T, n, Z[k_entry], Z[k_entry]), np.nan)      # read only where that kind occurs
  R4[kd == k_entry] = Re[kd == k_entry][:, :Z[k_entry] ** 2].reshape(-1, Z[k_entry], Z[k_entry])
  as_dict = {k_entry: R4, k_shared: Rs[k_shared]}
  out = {}
  for mode in ("dict", "tensor", "flat array", "exact", "no kernel"):
    f = _filter(name, n)[0]
    f.init_state(x0, P0, 0.0)
    assert f._has_batch_run_pf_r()
    if mode == "no kernel":
      f._has_batch_run_pf_r = lambda: False
    elif mode != "exact":
      f._run_logs_stepwise = None            # the kernel serves these: the walk must not be entered
    if mode == "tensor":
      arg = torch.as_tensor(Re.reshape(T, n, zmax, zmax), device=f.device)
    else:
      arg = Re if mode == "flat array" else (as_dict if mode == "dict" else torch.as_tensor(Re, device=f.device))
    y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), arg, trace=True, flags=True, exact=mode == "exact")
    torch.cuda.synchronize()
    if mode == "tensor":
      assert f._keepalive[2].data_ptr() == arg.data_ptr(), "a device tensor in the kernel's layout is used without a copy"
    assert f.pf_stats == {"fast": 0, "legacy": 0} and f.rewind_stats == {"device": 0, "torch": 0}
    assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
    out[mode] = (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy())
  for mode in ("tensor", "flat array"):
    for a, b in zip(out["dict"], out[mode]):
      assert np.array_equal(a, b), f"dict vs {mode}: the same launch on the same numbers"
  for a, b in zip(out["no kernel"], out["exact"]):      # a symmetric P0: the two walks launch the same kernels on the same numbers
    assert np.array_equal(a, b)
  _compare(name, "kernel vs walk", out["dict"], out["no kernel"], on, zs, Rs, kd, info["never"])
  # the rewind rings are emptied, as by reset_rewind(), and the filters' times are their logs' last
  f = _filter(name, n, rewind_to_keep=8, device_timeline=True)[0]
  f.init_state(x0, P0, np.full(n, -0.01))
  rng = np.random.default_rng(2)
  f.predict_and_update_kinds(np.zeros(n), rng.choice(np.array(kinds, dtype=np.int32), size=n), rng.normal(size=(n, zmax)), Rs)
  assert int(f._ring["length"].sum()) == n
  f.run_logs(ts, kd, zs.copy(), as_dict)
  torch.cuda.synchronize()
  assert int(f._ring["length"].sum()) == 0 and int(f._ring["head"].sum()) == 0
  assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
  # (Z, Z) values only: batch_run_pf as before, the per-entry entry point is not called
  f = _filter(name, n)[0]
  f.init_state(x0, P0, 0.0)
  real = f._call

  def no_r(sym, *args):
    assert sym != "batch_run_pf_r", "a (Z, Z)-only dict must launch batch_run_pf"
    return real(sym, *args)
  f._call = no_r
  f._run_logs_stepwise = None
  f.run_logs(ts, kd, zs.copy(), Rs)
  torch.cuda.synchronize()
  # wrong shapes name the expected one
  f = _filter(name, n)[0]
  f.init_state(x0, P0, 0.0)
  with pytest.raises(KalmanError, match=rf"\(T, N, zmax, zmax\) = \({T}, {n}, {zmax}, {zmax}\)"):
    f.run_logs(ts, kd, zs.copy(), Re[:-1])
  with pytest.raises(KalmanError, match=rf"Rs\[{k_entry}\].*\(T, N, Z, Z\) = \({T}, {n}, {Z[k_entry]}, {Z[k_entry]}\)"):
    f.run_logs(ts, kd, zs.copy(), {k_entry: R4[:, :-1], k_shared: Rs[k_shared]})
  with pytest.raises(KalmanError, match=rf"Rs\[{k_shared}\] must be \(Z, Z\)"):
    f.run_logs(ts, kd, zs.copy(), {k_entry: R4, k_shared: np.eye(Z[k_shared] + 1)})
  with pytest.raises(KeyError):
    f.run_logs(ts, kd, zs.copy(), {k_entry: R4})


def test_masked_walk_with_entry_noise_against_the_oracle():
  """A library without the mixed-kind step kernel (randz10: a 9-dimensional observation) walks per-entry noise with one `_masked` launch per kind
  present, that kind's rows compacted to (N, Z^2): run_logs(exact=True) against the oracle stepping every filter through its own entries."""
  import torch
  from examples import ensure_generated, model_class_of
  from oracle_lib import OracleLib
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  from run_pf_cases import make_schedule, stepped_mask
  from test_gpu_run_pf import _times
  name, n, T = "randz10", 9, 5
  M = model_class_of(name)
  gen = ensure_generated([name])
  D = M.dim
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, D, batch=n, per_filter=True)
  assert not f._has_step_kinds()
  kinds = tuple(sorted(f.zdims))
  Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
  zmax = max(f.zdims.values())
  rng = np.random.default_rng(12)
  x0 = M.initial_x[None] + rng.normal(size=(n, D)) * 0.3
  A = rng.normal(size=(n, D, D)) * 0.2
  P0 = np.diag(M.initial_P_diag)[None] + A @ A.transpose(0, 2, 1)
  P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
  kd, info = make_schedule(rng, T, n, kinds, 2)      # (a "tile" of 2: the nine filters bring every kind)
  kd[info["unknown"]] = 0                      # (run_logs refuses a kind the model does not have)
  on = stepped_mask(kd, kinds)
  assert all((kd == k).any() for k in kinds) and not on[:, info["never"]].any()
  ts, dts, t_last = _times(rng, kd)
  zs = rng.normal(size=(T, n, zmax))
  Re = entry_noise(rng, kd, dict(f.zdims), Rs, zmax)
  f.init_state(x0, P0, 0.0)
  y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), Re, trace=True, flags=True, exact=True)
  torch.cuda.synchronize()
  xo, Po, zo = x0.copy(), P0.copy(), zs.copy()
  fr, txr, tPr = oracle_walk_r(OracleLib(name), {k: f.zdims[k] for k in kinds}, Re, M.Q, kd, dts, xo, Po, zo, trace=True)
  what = f"{name} masked walk vs oracle"
  for a in (f.state(), f.covs(), y.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy()):
    assert not np.isnan(a).any(), what + ": NaN in an output"
  assert np.array_equal(fl.cpu().numpy(), fr)
  assert np.array_equal(y.cpu().numpy()[~on], zs[~on])
  # tests/test_gpu_random.py's step-against-oracle bounds for the lane-group models
  assert_close(f.state(), xo, rtol=1e-9, floor=1e-11, what=what + " x")
  assert_close(f.covs().reshape(n, -1), Po.reshape(n, -1), rtol=1e-8, floor=1e-10, what=what + " P")
  assert_close(tP.cpu().numpy().reshape(T * n, -1), tPr.reshape(T * n, -1), rtol=1e-8, floor=1e-10, what=what + " trace P")
  assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
