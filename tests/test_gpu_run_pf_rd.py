"""The fused run with a schedule per filter and a DIAGONAL noise per entry ({name}_batch_run_pf_rd, BatchedEKF.run_logs with variances per
entry), against the step walk on the expanded matrices (T batch_predict_update_kinds launches with R[t] = diag(row), r_per_filter = 1) and against
batch_run_pf_r on the same expanded rows.  R is allocated at exactly (T, n, zmax) and holds NaN wherever the contract says "never read": the rows
of idle entries and of entries with an unknown kind, and the positions beyond Z of the others.  Both kernel families: lane per filter (kinematic6,
attitude) and lane group (kinematic9, live)."""
import os
import re

import numpy as np
import pytest

from conftest import assert_close
from run_pf_cases import expected_flags_untouched
from run_pf_r_cases import oracle_walk_r
from run_pf_rd_cases import entry_variances, expand
from test_gpu_run_pf import SMALL, _compare, _filter, _fpw, _inputs
from test_gpu_run_pf_r import _walk_r

pytestmark = pytest.mark.gpu

MODELS = ["kinematic6", "attitude", "kinematic9", "live"]


def _block(f):
  """Steps per block of k_run_dpf (lane-per-filter models: the title line of the generated kernel states it); 4 for the lane-group models."""
  if f.name not in SMALL:
    return 4
  from examples import GENERATED_DIR
  with open(os.path.join(GENERATED_DIR, f"{f.name}.hip"), encoding="utf-8") as fh:
    return int(re.search(r"diagonal R per entry \(gR \(T, n, \d+\)\): blocks of (\d+) steps", fh.read()).group(1))


def _variances(seed, kd, f, Rs, zmax):
  return entry_variances(np.random.default_rng(seed + 17), kd, {k: f.zdims[k] for k in Rs}, Rs, zmax)


def _run(f, sym, x0, Ps, kd, dts, zs, R, G=2):
  """One launch of `sym` (batch_run_pf_rd: R (T, n, zmax); batch_run_pf_r: (T, n, zmax^2)) with guard rows around z, the flags and both traces; R at
  exactly its size.  -> (got, guards_ok)"""
  import torch
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  T, n = kd.shape
  D, E, zmax = x0.shape[1], Ps.shape[1], zs.shape[2]
  w = zmax if sym == "batch_run_pf_rd" else zmax * zmax
  zg = torch.full((T + 2 * G, n, zmax), 777.0, dtype=torch.float64, device=dev)
  txg = torch.full((T + 2 * G, n, D), 5.0, dtype=torch.float64, device=dev)
  tPg = torch.full((T + 2 * G, n, E, E), 5.0, dtype=torch.float64, device=dev)
  fg = torch.full((T + 2 * G, n), 99, dtype=torch.uint8, device=dev)
  zg[G:G + T] = t(zs)
  f.init_state(x0, Ps, 0.0)
  # (an empty tensor has no address: T == 0 still wants pointers)
  kdd, dtd, Rd = t(kd if T else np.zeros((1, n)), torch.int32), t(dts if T else np.zeros((1, n))), t(R if T else np.zeros((1, n, w)))
  assert Rd.numel() == max(T, 1) * n * w
  f._call(sym, f._p(f.x), f._p(f.P), f._p(f.Q), f._p(kdd), f._p(dtd), T, f._p(zg[G:]), f._p(Rd), n, f.norm_quats, f._p(fg[G:]),
          f._p(txg[G:]), f._p(tPg[G:]), f._stream())
  torch.cuda.synchronize()
  ok = bool((fg[:G] == 99).all()) and bool((fg[G + T:] == 99).all())
  for a, fill in ((zg, 777.0), (txg, 5.0), (tPg, 5.0)):
    ok = ok and bool((a[:G] == fill).all()) and bool((a[G + T:] == fill).all())
  return (f.state(), f.covs(), zg[G:G + T].cpu().numpy(), fg[G:G + T].cpu().numpy(), txg[G:G + T].cpu().numpy(), tPg[G:G + T].cpu().numpy()), ok


@pytest.mark.parametrize("n_case", ["1", "FPW+1", "203"])
@pytest.mark.parametrize("name", MODELS)
def test_shapes_against_the_step_walk(name, n_case):
  n = {"1": 1, "FPW+1": _fpw(name) + 1, "203": 203}[n_case]
  probe = _filter(name, 1)[0]
  K = _block(probe)
  assert probe._has_batch_run_pf_rd()
  for T in sorted({0, 1, K - 1, K, K + 1, 3 * K + 2}):
    seed = 1000 * n + T
    f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, seed)
    Ps = 0.5 * (P0 + P0.transpose(0, 2, 1))
    Rv = _variances(seed, kd, f, Rs, zmax)
    what = f"{name} n={n} T={T}"
    got, guards = _run(f, "batch_run_pf_rd", x0, Ps, kd, dts, zs, Rv)
    assert guards, what + ": guard rows"
    if T == 0:
      assert np.array_equal(got[0], x0) and np.array_equal(got[1], Ps)
      continue
    assert np.isnan(Rv[~on]).all() and (on.all() or np.isnan(Rv).any())
    want = _walk_r(f, x0, P0, kd, dts, zs, expand(Rv, kd, {k: f.zdims[k] for k in Rs}, zmax))
    for a in got:
      assert not np.isnan(a.astype(np.float64)).any(), what + ": NaN in an output (an unused double of R has reached it)"
    fl = got[3]
    assert np.array_equal(fl[~on], expected_flags_untouched(kd, kinds)[~on]), what + ": 16 at idle entries, 8 at the unknown kind"
    if info["unknown"] is not None:
      assert fl[info["unknown"]] == 8
    nv = info["never"]
    if nv is not None:
      assert np.array_equal(got[0][nv], x0[nv]) and np.array_equal(got[1][nv], Ps[nv]), what + ": the never-stepped filter, bit for bit"
    _compare(name, what, got, want, on, zs, Rs, kd, nv)


@pytest.mark.parametrize("name", MODELS)
def test_against_batch_run_pf_r_on_the_expanded_rows(name):
  """The result contract: batch_run_pf_r on diag(row).  Two fused kernels on the same numbers (they may contract FMAs differently, and the
  lane-group update keeps the noise a vector): the lane-per-filter bounds for both families, equal flags."""
  n = 203
  f0 = _filter(name, 1)[0]
  T = 2 * _block(f0) + 1
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 41)
  Ps = 0.5 * (P0 + P0.transpose(0, 2, 1))
  Rv = _variances(41, kd, f, Rs, zmax)
  got, guards = _run(f, "batch_run_pf_rd", x0, Ps, kd, dts, zs, Rv)
  want, guards_r = _run(f, "batch_run_pf_r", x0, Ps, kd, dts, zs, expand(Rv, kd, {k: f.zdims[k] for k in Rs}, zmax))
  assert guards and guards_r
  assert np.array_equal(got[3], want[3]), "flags"
  _compare("kinematic6", f"{name} variances vs batch_run_pf_r on diag(row)", got, want, on, zs, Rs, kd, info["never"])      # (the lane-per-filter bounds)


@pytest.mark.parametrize("name", ["kinematic6_maha", "live_maha"])
def test_the_gate_reads_the_entry_variances(name):
  """The same observation, far from the prediction, in two filters in the same state whose entries differ in their variances by 10^4: the chi-square
  gate fires for the one with the small variances and not for the other, in the kernel as in the step walk."""
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  from oracle_lib import OracleLib
  gen = ensure_generated([name])
  if name == "kinematic6_maha":
    from examples.kinematic6_kf import Kinematic6Kalman as M
    D, E, quat, kind = 6, 6, [], 1
    x1 = np.asarray(M.initial_x, dtype=np.float64)
  else:
    from examples.live_kf import LiveKalman as M, ObservationKind as LK
    from conftest import golden
    D, E, quat, kind = 23, 22, [3], int(LK.ECEF_POS)
    x1 = golden("live_single_steps.npz")["x_in"][0]
  var = np.diag(np.atleast_2d(M.obs_noise[kind])).copy()
  n, T = 2, 1
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat, per_filter=True,
                 maha_test_kinds=[kind])
  assert f._has_batch_run_pf_rd()
  Z, zmax = f.zdims[kind], max(f.zdims.values())
  P1 = np.diag(M.initial_P_diag) * 1e-6      # a confident filter: the innovation covariance is R's
  hx = np.zeros(Z)
  OracleLib(name).call(f"h_{kind}", x1.copy(), np.zeros(4), hx)
  zs = np.zeros((T, n, zmax))
  zs[0, :, :Z] = hx + 10.0 * np.sqrt(var)    # 10 sigma of the small variances, 0.1 sigma of the large ones
  Rv = np.full((T, n, zmax), np.nan)
  Rv[0, 0, :Z] = var
  Rv[0, 1, :Z] = 1e4 * var
  kd, dts = np.full((T, n), kind, dtype=np.int32), np.zeros((T, n))
  x0, P0 = np.tile(x1, (n, 1)), np.tile(P1, (n, 1, 1))
  got, guards = _run(f, "batch_run_pf_rd", x0, P0, kd, dts, zs, Rv)
  want = _walk_r(f, x0, P0, kd, dts, zs, expand(Rv, kd, {kind: Z}, zmax))
  assert guards
  assert got[3][0, 0] & 1 and not got[3][0, 1] & 1, got[3]
  assert np.array_equal(got[3], want[3])
  assert np.abs(got[0][1] - x0[1]).max() > 0.0, "the accepted observation moves its filter"


def _launches(f):
  """Record the entry points f._call launches."""
  real, seen = f._call, []

  def spy(sym, *args):
    seen.append(sym)
    return real(sym, *args)
  f._call = spy
  return seen


def test_run_logs_plumbing():
  """run_logs with variances per entry: a dict with one kind (T, N, Z) and one shared diagonal (Z, Z), the (T, N, zmax) device tensor (no copy), a
  numpy array, exact=True and a library "without" the kernel agree; a full matrix anywhere in the dict routes to batch_run_pf_r, a (Z, Z)-only
  dict still launches batch_run_pf; filter_times() and the ring state are as documented; wrong shapes are named."""
  import torch
  from rednose_amd.helpers import KalmanError
  name, n, T = "attitude", 131, 9
  f, M, qi, kinds, Rs, x0, P0, kd, info, on, ts, dts, t_last, zs, zmax = _inputs(name, n, T, 5, unknown=False)
  Z = {k: f.zdims[k] for k in kinds}
  k_entry, k_shared = kinds[0], kinds[1]
  Rs = dict(Rs)
  Rs[k_shared] = np.diag(np.diag(Rs[k_shared]))                 # the shared value: exactly diagonal
  Rv = _variances(5, kd, f, Rs, zmax)
  Rv[kd == k_shared, :Z[k_shared]] = np.diag(Rs[k_shared])
  V3 = np.full((T, n, Z[k_entry]), np.nan)                       # read only where that kind occurs
  V3[kd == k_entry] = Rv[kd == k_entry][:, :Z[k_entry]]
  as_dict = {k_entry: V3, k_shared: Rs[k_shared]}
  out, calls = {}, {}
  for mode in ("dict", "tensor", "array", "exact", "no kernel"):
    f = _filter(name, n)[0]
    f.init_state(x0, P0, 0.0)
    assert f._has_batch_run_pf_rd()
    if mode == "no kernel":
      f._has_batch_run_pf_rd = lambda: False
    elif mode != "exact":
      f._run_logs_stepwise = None            # the kernel serves these: the walk must not be entered
    arg = as_dict if mode in ("dict", "exact", "no kernel") else (torch.as_tensor(Rv, device=f.device) if mode == "tensor" else Rv)
    calls[mode] = _launches(f)
    y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), arg, trace=True, flags=True, exact=mode == "exact")
    torch.cuda.synchronize()
    if mode == "tensor":
      assert f._keepalive[2].data_ptr() == arg.data_ptr(), "a device tensor in the kernel's layout is used without a copy"
    assert f.pf_stats == {"fast": 0, "legacy": 0} and f.rewind_stats == {"device": 0, "torch": 0}
    assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
    out[mode] = (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy())
  for mode in ("dict", "tensor", "array"):
    assert calls[mode] == ["batch_run_pf_rd"], (mode, calls[mode])
  assert calls["no kernel"] == ["batch_run_pf_r"], "without the kernel the variances are expanded: today's path"
  assert "batch_run_pf_rd" not in calls["exact"] and "batch_run_pf_r" not in calls["exact"] and len(calls["exact"]) >= T
  for mode in ("tensor", "array"):
    for a, b in zip(out["dict"], out[mode]):
      assert np.array_equal(a, b), f"dict vs {mode}: the same launch on the same numbers"
  walk = _walk_r(f, x0, P0, kd, dts, zs, expand(Rv, kd, Z, zmax))
  _compare(name, "kernel vs walk", out["dict"], walk, on, zs, Rs, kd, info["never"])
  _compare(name, "exact vs walk", out["exact"], walk, on, zs, Rs, kd, info["never"])
  _compare("kinematic6", "kernel vs batch_run_pf_r on the expanded rows", out["dict"], out["no kernel"], on, zs, Rs, kd, info["never"])
  # routing: a full matrix anywhere in the dict takes batch_run_pf_r on the expanded rows
  R4 = np.full((T, n, Z[k_shared], Z[k_shared]), np.nan)
  R4[kd == k_shared] = Rs[k_shared]
  sd = np.sqrt(np.diag(Rs[k_shared]))
  full = Rs[k_shared] + 0.1 * np.outer(sd, sd) * (1.0 - np.eye(Z[k_shared]))      # correlations of 0.1: positive definite, not diagonal
  for label, arg, same in (("(T, N, Z) with (T, N, Z, Z)", {k_entry: V3, k_shared: R4}, True), ("a non-diagonal shared value", {k_entry: V3, k_shared: full}, False)):
    f = _filter(name, n)[0]
    f.init_state(x0, P0, 0.0)
    f._run_logs_stepwise = None
    seen = _launches(f)
    y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), arg, trace=True, flags=True)
    torch.cuda.synchronize()
    assert seen == ["batch_run_pf_r"], (label, seen)
    if same:      # the same expanded rows as the library "without" the kernel: the same launch on the same numbers
      for a, b in zip(out["no kernel"], (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy())):
        assert np.array_equal(a, b), label
  # (Z, Z) values only: batch_run_pf as before
  f = _filter(name, n)[0]
  f.init_state(x0, P0, 0.0)
  f._run_logs_stepwise = None
  seen = _launches(f)
  f.run_logs(ts, kd, zs.copy(), Rs)
  torch.cuda.synchronize()
  assert seen == ["batch_run_pf"], seen
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
  # wrong shapes name the expected one
  f = _filter(name, n)[0]
  f.init_state(x0, P0, 0.0)
  with pytest.raises(KalmanError, match=rf"\(T, N, zmax\) = \({T}, {n}, {zmax}\)"):
    f.run_logs(ts, kd, zs.copy(), Rv[:, :-1])
  with pytest.raises(KalmanError, match=rf"Rs\[{k_entry}\].*\(T, N, Z\) = \({T}, {n}, {Z[k_entry]}\)"):
    f.run_logs(ts, kd, zs.copy(), {k_entry: V3[:, :-1], k_shared: Rs[k_shared]})
  with pytest.raises(KeyError):
    f.run_logs(ts, kd, zs.copy(), {k_entry: V3})


def test_randz10_variances_against_the_oracle():
  """randz10, the model with a 9-dimensional kind: run_logs with variances per entry -- one batch_run_pf_rd launch where its library carries the
  kernel, today's path on the expanded rows where it does not -- against the oracle stepping every filter through its own entries, at the bounds
  of test_gpu_run_pf_r.py::test_masked_walk_with_entry_noise_against_the_oracle."""
  import torch
  from examples import ensure_generated, model_class_of
  from oracle_lib import OracleLib
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  from run_pf_cases import make_schedule, stepped_mask
  from test_gpu_run_pf import _times
  from test_run_pf_rd_abi import WITH
  name, n, T = "randz10", 9, 5
  M = model_class_of(name)
  gen = ensure_generated([name])
  D = M.dim
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, D, batch=n, per_filter=True)
  assert f._has_batch_run_pf_rd() == (name in WITH)
  kinds = tuple(sorted(f.zdims))
  Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
  zmax = max(f.zdims.values())
  assert zmax == 9
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
  Rv = entry_variances(rng, kd, dict(f.zdims), Rs, zmax)
  f.init_state(x0, P0, 0.0)
  seen = _launches(f)
  y, tx, tP, fl = f.run_logs(ts, kd, zs.copy(), Rv, trace=True, flags=True)
  torch.cuda.synchronize()
  if name in WITH:
    assert seen == ["batch_run_pf_rd"], seen
  else:
    assert "batch_run_pf_rd" not in seen and "batch_run_pf_r" not in seen and len(seen) > 1, seen      # the step walk
  xo, Po, zo = x0.copy(), P0.copy(), zs.copy()
  fr, txr, tPr = oracle_walk_r(OracleLib(name), {k: f.zdims[k] for k in kinds}, expand(Rv, kd, dict(f.zdims), zmax), M.Q, kd, dts, xo, Po, zo, trace=True)
  what = f"{name} variances per entry vs oracle"
  for a in (f.state(), f.covs(), y.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy()):
    assert not np.isnan(a).any(), what + ": NaN in an output"
  assert np.array_equal(fl.cpu().numpy(), fr)
  assert np.array_equal(y.cpu().numpy()[~on], zs[~on])
  nv = info["never"]
  assert np.array_equal(f.state()[nv], x0[nv]) and np.array_equal(f.covs()[nv], P0[nv]), what + ": the never-stepped filter"
  # tests/test_gpu_random.py's step-against-oracle bounds for the lane-group models
  assert_close(f.state(), xo, rtol=1e-9, floor=1e-11, what=what + " x")
  assert_close(f.covs().reshape(n, -1), Po.reshape(n, -1), rtol=1e-8, floor=1e-10, what=what + " P")
  assert_close(tP.cpu().numpy().reshape(T * n, -1), tPr.reshape(T * n, -1), rtol=1e-8, floor=1e-10, what=what + " trace P")
  assert np.array_equal(f.filter_times().cpu().numpy(), t_last)
