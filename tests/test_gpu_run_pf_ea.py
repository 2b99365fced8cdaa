"""GPU tests of the fused run with a schedule per filter of MSCKF models ({name}_batch_run_pf_ea, k_run_epf; BatchedEKF.run_logs(extra_args=,
augment=)) and of the masked window shift ({name}_batch_augment_masked).  feature: 8 filters per wavefront, the predicates of the null-space
projected update and of the window shift diverge inside a wavefront; feature36: one filter per wavefront.  Against the step walk
(run_logs(exact=True)) and the oracle on ragged logs, and against the reference's golden stream spread over filters with idle entries of
their own.  The measured maxima go to profiles/run_pf_ea_parity.json under RN_WRITE_PARITY=1 (fractions of the tolerances they are held to)."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import REPO, assert_close, golden
from run_pf_cases import expected_flags_untouched
from run_pf_ea_cases import FEATURE, oracle_walk_ea, spread_stream, window_shift

pytestmark = pytest.mark.gpu

T_LOG, T0_LOG = 12, 0.9
WALK_X, WALK_P, WALK_Y = (1e-9, 1e-11), (1e-8, 1e-10), (1e-8, 1e-10)      # the lane-group fused-vs-step bounds (rtol, floor; y: rtol, atol)
ORACLE_X, ORACLE_P = (1e-8, 1e-10), (1e-7, 1e-9)                          # test_gpu_msckf.test_fused_run_with_landmarks_and_window_shifts'
_PARITY = {}


def _model(name):
  from examples.feature_kf import FeatureKalman, WideFeatureKalman
  return {"feature": FeatureKalman, "feature36": WideFeatureKalman}[name]


def _filter(name, n):
  import torch
  assert torch.cuda.is_available()
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  FK = _model(name)
  return BatchedEKF(ensure_generated([name]), name, FK.Q, FK.initial_x, np.diag(FK.initial_P_diag), 6, 6, batch=n, per_filter=True, **FK.filter_kwargs())


def _dims(FK):
  return (6, 6, FK.dim_augment, FK.dim_augment)


def _record(key, **figures):
  _PARITY[key] = {k: float(v) for k, v in figures.items()}
  if os.environ.get("RN_WRITE_PARITY"):
    fn = os.path.join(REPO, "profiles", "run_pf_ea_parity.json")
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


_LOGS = {}


def _log_inputs(name, n, T=T_LOG, seed=5):
  """One seeded case per (model, n), shared by the tests below (which copy what a call consumes): states with a symmetric P0, the ragged logs of
  rts_pf_cases.schedule, landmarks [2, 1, 8] + N(0, 1) at the feature entries (NaN elsewhere), observations near h(x0, landmark), window shifts at
  about a third of the entries and, ignored, at every idle one."""
  from oracle_lib import OracleLib
  from rts_pf_cases import forward_dts, schedule
  if (name, n, T) not in _LOGS:
    FK = _model(name)
    o = OracleLib(name)
    D = FK.dim_state
    rng = np.random.default_rng(seed + n)
    x0 = np.tile(FK.initial_x, (n, 1)) + rng.normal(size=(n, D)) * 0.1
    A = rng.normal(size=(n, D, D)) * 0.1
    P0 = np.diag(FK.initial_P_diag)[None] + A @ A.transpose(0, 2, 1)
    Rs = {k: np.ascontiguousarray(FK.obs_noise[k], dtype=np.float64) for k in (1, FEATURE)}
    sch = schedule(n, T, [1, FEATURE], seed=seed)
    kd = np.ascontiguousarray(sch["kinds"])
    on = kd > 0
    eas = np.full((T, n, 3), np.nan)
    eas[kd == FEATURE] = np.array([2.0, 1.0, 8.0]) + rng.normal(size=(int((kd == FEATURE).sum()), 3))
    zs = rng.normal(size=(T, n, 6)) * 0.5
    for k, Z in ((1, 3), (FEATURE, 6)):
      for t, i in zip(*np.nonzero(kd == k)):
        hx = np.zeros(Z)
        o.call(f"h_{k}", x0[i].copy(), np.ascontiguousarray(eas[t, i]) if k == FEATURE else np.zeros(4), hx)
        zs[t, i, :Z] = hx + rng.normal(size=Z) * np.sqrt(np.diag(Rs[k]))
    aug = (rng.uniform(size=(T, n)) < 1.0 / 3.0) | ~on
    dts = forward_dts(sch["ts_fwd"], kd, np.full(n, T0_LOG))
    _LOGS[name, n, T] = dict(FK=FK, Rs=Rs, x0=x0, P0=P0, ts=sch["ts_fwd"], kd=kd, zs=zs, dts=dts, on=on, eas=eas, aug=aug)
  return _LOGS[name, n, T]


def _replay(f, c, exact=False, augment=True):
  """run_logs(trace=True, flags=True) from the case's start -> ((x, P, y, flags, trace_x, trace_P) as numpy arrays, the entry points launched)"""
  import torch
  n = c["x0"].shape[0]
  f.init_state(c["x0"], c["P0"], np.full(n, T0_LOG))
  real, seen = f._call, []

  def spy(sym, *args):
    seen.append(sym)
    return real(sym, *args)
  f._call = spy
  y, tx, tP, fl = f.run_logs(c["ts"], c["kd"], c["zs"].copy(), c["Rs"], trace=True, flags=True, exact=exact, extra_args=c["eas"],
                             augment=c["aug"] if augment else None)
  torch.cuda.synchronize()
  del f._call
  return (f.state(), f.covs(), y.cpu().numpy(), fl.cpu().numpy(), tx.cpu().numpy(), tP.cpu().numpy()), seen


@pytest.mark.parametrize("name,n", [("feature", 1), ("feature", 9), ("feature", 19), ("feature36", 1), ("feature36", 3)])
def test_one_launch_against_the_step_walk_and_the_oracle(name, n):
  """run_logs with landmarks and window shifts per filter: ONE batch_run_pf_ea launch, against run_logs(exact=True) on a second object (one
  `_masked` launch per kind and step, one batch_augment_masked per step with a shift) at the lane-group fused-vs-step bounds, and against
  the oracle's walk at the bounds of the shared-schedule MSCKF run.  Flags, idle z rows and never-stepped filters bit for bit."""
  from oracle_lib import OracleLib
  c = _log_inputs(name, n)
  T, kd, on, zs, Rs, FK = T_LOG, c["kd"], c["on"], c["zs"], c["Rs"], c["FK"]
  f, g = _filter(name, n), _filter(name, n)
  assert f._has_batch_run_pf_ea() and not f._has_batch_run_pf()
  got, seen = _replay(f, c)
  assert seen == ["batch_run_pf_ea"], seen
  want, walked = _replay(g, c, exact=True)
  n_shift_steps = int(((c["aug"] != 0) & on).any(axis=1).sum())
  assert "batch_run_pf_ea" not in walked and walked.count("batch_augment_masked") == n_shift_steps and n_shift_steps > 0
  assert sum(s.startswith("batch_predict_update_") for s in walked) >= int(on.any(axis=1).sum())
  what = f"{name} n={n} T={T}"
  for a in got:
    assert np.isfinite(a.astype(np.float64)).all(), what + ": an output is not finite"
  never = ~on.any(axis=0)
  assert np.array_equal(got[0][never], c["x0"][never]) and np.array_equal(got[1][never], c["P0"][never]), what + ": filters without an entry, bit for bit"
  assert np.array_equal(got[3], want[3]) and np.array_equal(got[3][~on], expected_flags_untouched(kd, [1, FEATURE])[~on]), what + ": flags"
  assert np.array_equal(got[2][~on], zs[~on]), what + ": z rows of idle entries pass through bit for bit"
  xo, Po, zo = c["x0"].copy(), c["P0"].copy(), zs.copy()
  fr, txr, tPr = oracle_walk_ea(OracleLib(name), {1: 3, FEATURE: 6}, Rs, np.asarray(FK.Q, dtype=np.float64), kd, c["dts"], xo, Po, zo, c["eas"], c["aug"], _dims(FK))
  r = lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(a.shape[0] * a.shape[1], -1)      # noqa: E731
  fig = dict(x_walk=_of_tol(got[0], want[0], *WALK_X), P_walk=_of_tol(got[1].reshape(n, -1), want[1].reshape(n, -1), *WALK_P),
             trace_x_walk=_of_tol(r(got[4]), r(want[4]), *WALK_X), trace_P_walk=_of_tol(r(got[5]), r(want[5]), *WALK_P),
             x_oracle=_of_tol(got[0], xo, *ORACLE_X), P_oracle=_of_tol(got[1].reshape(n, -1), Po.reshape(n, -1), *ORACLE_P),
             trace_x_oracle=_of_tol(r(got[4]), r(txr), *ORACLE_X), trace_P_oracle=_of_tol(r(got[5]), r(tPr), *ORACLE_P))
  zabs = max(1.0, np.abs(zs).max())
  for k, Zy in ((1, 3), (FEATURE, 3)):      # feature tracks: Z - 3 residual rows in the reference's basis, the rest of the row passes through
    m = kd == k
    fig[f"y{k}_walk"] = _of_tol(got[2][m][:, :Zy], want[2][m][:, :Zy], WALK_Y[0], 0.0, atol=WALK_Y[1] * zabs)
    assert np.array_equal(got[2][m][:, Zy:], zs[m][:, Zy:]), what + f" kind {k}: z columns beyond the residual"
  print(what, {k: f"{v:.3e}" for k, v in fig.items()}, "(fractions of the tolerance)")
  _record(f"parity/{name}/n={n}", **fig)
  assert_close(got[0], want[0], rtol=WALK_X[0], floor=WALK_X[1], what=what + " x vs the step walk")
  assert_close(got[1].reshape(n, -1), want[1].reshape(n, -1), rtol=WALK_P[0], floor=WALK_P[1], what=what + " P vs the step walk")
  assert_close(r(got[4]), r(want[4]), rtol=WALK_X[0], floor=WALK_X[1], what=what + " trace x vs the step walk")
  assert_close(r(got[5]), r(want[5]), rtol=WALK_P[0], floor=WALK_P[1], what=what + " trace P vs the step walk")
  for k, Zy in ((1, 3), (FEATURE, 3)):
    m = kd == k
    assert_close(got[2][m][:, :Zy], want[2][m][:, :Zy], rtol=WALK_Y[0], atol=WALK_Y[1] * zabs, what=what + f" y kind {k} vs the step walk")
  # (bit 4 aside: window entries shifted in without a predict in between are copies of one position, the landmark Jacobian of such a track has rank 2,
  # and the kernels ignore the measurement and say so -- both paths alike, asserted above --, where the oracle's C path has no such flag)
  assert np.array_equal(got[3] & ~np.uint8(4), fr), what + ": flags vs the oracle"
  assert_close(got[0], xo, rtol=ORACLE_X[0], floor=ORACLE_X[1], what=what + " x vs the oracle")
  assert_close(got[1].reshape(n, -1), Po.reshape(n, -1), rtol=ORACLE_P[0], floor=ORACLE_P[1], what=what + " P vs the oracle")
  assert_close(r(got[4]), r(txr), rtol=ORACLE_X[0], floor=ORACLE_X[1], what=what + " trace x vs the oracle (rows BEFORE the shift)")
  assert_close(r(got[5]), r(tPr), rtol=ORACLE_P[0], floor=ORACLE_P[1], what=what + " trace P vs the oracle (rows BEFORE the shift)")
  # every filter's own shift times
  want_times = np.zeros((n, FK.n_window))
  for i in range(n):
    own = [c["ts"][t, i] for t in range(T) if on[t, i] and c["aug"][t, i]]
    row = ([0.0] * FK.n_window + own)[-FK.n_window:]
    want_times[i] = row
  assert np.array_equal(f.filter_augment_times(), want_times) and np.array_equal(g.filter_augment_times(), want_times)


@pytest.mark.parametrize("name,n,T,short", [("feature", 11, 60, 20), ("feature36", 3, 20, 8)])
def test_the_reference_stream_spread_over_filters(name, n, T, short):
  """The reference's golden MSCKF stream, n copies, each with idle entries inserted at its own seeded positions (one log ends early): at every real
  entry the trace row is the reference's filtered estimate, the full logs end in its final state, in one launch."""
  FK = _model(name)
  g = golden("feature_stream.npz" if name == "feature" else "feature36_stream.npz")
  S = len(g["ts"])
  s = spread_stream(g, n, T, seed=7, short=(n - 2, short))
  f = _filter(name, n)
  f.init_state(FK.initial_x, np.diag(FK.initial_P_diag), None)
  Rs = {1: FK.obs_noise[1], 2: FK.obs_noise[2]}
  seen, real = [], f._call

  def spy(sym, *args):
    seen.append(sym)
    return real(sym, *args)
  f._call = spy
  ys, tx, tP, fl = f.run_logs(s["ts"], s["kinds"], s["zs"].copy(), Rs, trace=True, flags=True, extra_args=s["eas"], augment=s["augment"])
  import torch
  torch.cuda.synchronize()
  del f._call
  assert seen == ["batch_run_pf_ea"], seen
  at = s["at"]
  real_e = at >= 0
  assert (real_e.sum(axis=0) == np.where(np.arange(n) == n - 2, short, S)).all() and (~real_e).any(axis=1).sum() >= T // 4
  X, P, F = tx.cpu().numpy(), tP.cpu().numpy(), fl.cpu().numpy()
  assert np.array_equal(F, np.where(real_e, 0, 16))
  assert_close(X[real_e], g["xk_k"][at[real_e]], rtol=1e-8, floor=1e-10, what=f"{name}: filtered states at the real entries")
  assert_close(P[real_e].reshape(int(real_e.sum()), -1), g["Pk_k"][at[real_e]].reshape(int(real_e.sum()), -1), rtol=1e-7, floor=1e-9,
               what=f"{name}: filtered covariances at the real entries")
  full = real_e.sum(axis=0) == S
  assert full.sum() == n - 1
  assert_close(f.state()[full], np.tile(g["x_after"][-1], (n - 1, 1)), rtol=1e-8, floor=1e-10, what=f"{name}: state after the last window shift")
  assert_close(f.covs()[full].reshape(n - 1, -1), np.tile(g["P_after"][-1].reshape(1, -1), (n - 1, 1)), rtol=1e-7, floor=1e-9)
  i = n - 2
  assert_close(f.state()[i], g["x_after"][short - 1], rtol=1e-8, floor=1e-10, what=f"{name}: the short log's final state")
  assert_close(f.covs()[i].reshape(1, -1), g["P_after"][short - 1].reshape(1, -1), rtol=1e-7, floor=1e-9)
  times = f.filter_augment_times()
  for i in range(n):
    m = short if i == n - 2 else S
    own = [float(g["ts"][e]) for e in range(m) if g["augment"][e]]
    assert list(times[i]) == ([0.0] * FK.n_window + own)[-FK.n_window:], i
  assert np.array_equal(f.filter_times().cpu().numpy(), np.where(np.arange(n) == n - 2, g["ts"][short - 1], g["ts"][-1]))


def _lds():
  fn = os.path.join(REPO, "tools", "liblds_poison.so")
  if not os.path.exists(fn):
    return None
  lib = ctypes.CDLL(fn)
  lib.lds_poison.argtypes, lib.lds_poison.restype = [ctypes.c_void_p], None
  lib.lds_fill.argtypes, lib.lds_fill.restype = [ctypes.c_uint64, ctypes.c_void_p], None
  return lib


@pytest.mark.parametrize("name,n", [("feature", 19), ("feature36", 3)])
def test_same_call_same_bits_whatever_lds_held(name, n):
  """Three calls on identical inputs from a re-initialised object: behind the NaN pattern of lds_poison, behind lds_fill(1e30) and behind
  lds_fill(-0.0).  Every output finite and the same bits in all three: the stale slot of a group that is idle, of another kind or not
  shifting reaches nothing.  A comparison of values -- three calls, no loop."""
  import torch
  c = _log_inputs(name, n)
  f = _filter(name, n)
  lds = _lds()
  bits = lambda v: int(np.float64(v).view(np.uint64))      # noqa: E731
  out = []
  for label, refill in (("lds_poison", lambda: lds.lds_poison(None)), ("lds_fill(1e30)", lambda: lds.lds_fill(bits(1e30), None)),
                        ("lds_fill(-0.0)", lambda: lds.lds_fill(bits(-0.0), None))):
    if lds is not None:
      refill()
      torch.cuda.synchronize()
    got, seen = _replay(f, c)
    assert seen == ["batch_run_pf_ea"], (label, seen)
    out.append((label, got))
  names = ("x", "P", "y", "flags", "trace_x", "trace_P")
  for label, got in out:
    for a, nm in zip(got, names):
      assert np.isfinite(a.astype(np.float64)).all(), f"{name} behind {label}: {nm} is not finite"
  for label, got in out[1:]:
    for a, b, nm in zip(out[0][1], got, names):
      diff = (a.view(np.uint64) != b.view(np.uint64)) if a.dtype == np.float64 else (a != b)
      assert not diff.any(), f"{name}: {nm} behind {label} differs from the call behind {out[0][0]} in {int(diff.sum())} of {diff.size} entries"


@pytest.mark.parametrize("name", ["feature", "feature36"])
def test_masked_window_shift(name):
  """batch_augment_masked with half the filters active: batch_augment on those, the others bit for bit; active == NULL: every filter."""
  import torch
  FK = _model(name)
  n, D = 13, FK.dim_state
  rng = np.random.default_rng(77)
  x0 = rng.normal(size=(n, D))
  P0 = rng.normal(size=(n, D, D))
  act = (np.arange(n) % 2 == 0)
  f, g = _filter(name, n), _filter(name, n)
  f.init_state(x0, P0, None)
  g.init_state(x0, P0, None)
  a8 = torch.as_tensor(act.astype(np.uint8), device=f.device)
  f._call("batch_augment_masked", f._p(f.x), f._p(f.P), f._p(a8), n, f._stream())
  g._call("batch_augment", g._p(g.x), g._p(g.P), n, g._stream())
  torch.cuda.synchronize()
  xs, Ps = window_shift(x0, P0, *_dims(FK))
  assert np.array_equal(g.state(), xs) and np.array_equal(g.covs(), Ps), "batch_augment against its numpy restatement"
  assert np.array_equal(f.state()[act], g.state()[act]) and np.array_equal(f.covs()[act], g.covs()[act]), "the active filters shift as batch_augment shifts them"
  assert np.array_equal(f.state()[~act], x0[~act]) and np.array_equal(f.covs()[~act], P0[~act]), "the others are untouched bit for bit"
  f.init_state(x0, P0, None)
  f._call("batch_augment_masked", f._p(f.x), f._p(f.P), None, n, f._stream())
  torch.cuda.synchronize()
  assert np.array_equal(f.state(), xs) and np.array_equal(f.covs(), Ps), "active == NULL: batch_augment"


def test_run_logs_plumbing_errors():
  """What run_logs refuses: a feature kind without extra_args, augment on a model without a window, wrong shapes, an unsorted log."""
  from examples import ensure_generated
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  c = _log_inputs("feature", 9)
  T, n = c["kd"].shape
  f = _filter("feature", n)
  run = lambda **kw: f.run_logs(**{**dict(ts=c["ts"], kinds=c["kd"], zs=c["zs"].copy(), Rs=c["Rs"], extra_args=c["eas"], augment=c["aug"]), **kw})      # noqa: E731
  f.init_state(c["x0"], c["P0"], np.full(n, T0_LOG))
  with pytest.raises(KalmanError, match="extra arguments"):
    run(extra_args=None)
  with pytest.raises(KalmanError, match="extra_args must be"):
    run(extra_args=c["eas"][:, :, :2])
  with pytest.raises(KalmanError, match="extra_args must be"):
    run(extra_args=c["eas"][:-1])
  with pytest.raises(KalmanError, match="augment must be"):
    run(augment=c["aug"][:, :-1])
  ts = c["ts"].copy()
  full = int(np.nonzero(c["on"].all(axis=0))[0][0])
  ts[[3, 4], full] = ts[[4, 3], full] + np.array([0.5, 0.0])      # entry 3 now lies after entry 4
  with pytest.raises(KalmanError, match="sort the log"):
    run(ts=ts)
  assert np.array_equal(f.state(), c["x0"]) and np.array_equal(f.filter_augment_times(), np.zeros((n, 3))), "a refused call changes nothing"
  k = BatchedEKF(ensure_generated(["kinematic9"]), "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=4, per_filter=True)
  kk = np.full((2, 4), k.kinds[0], dtype=np.int32)
  Z = k.zdims[k.kinds[0]]
  with pytest.raises(KalmanError, match="augment"):
    k.run_logs(np.tile(np.array([[0.1], [0.2]]), (1, 4)), kk, np.zeros((2, 4, max(k.zdims.values()))), {k.kinds[0]: np.eye(Z)}, augment=np.ones((2, 4)))
  # a log of an MSCKF model without feature entries needs no extra_args
  kd1 = np.where(c["kd"] > 0, 1, 0).astype(np.int32)
  f.run_logs(c["ts"], kd1, c["zs"].copy(), c["Rs"], augment=c["aug"])
