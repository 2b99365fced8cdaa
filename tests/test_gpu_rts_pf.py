"""The smoother with a schedule per filter ({name}_batch_rts_pf, BatchedEKF.rts_smooth_logs / smooth_logs): N ragged logs smoothed in one
launch.  Yardstick (a): the numpy restatement of the reference's rts_smooth on the oracle's f_fun / F_fun (tests/rts_pf_cases.py), filter by
filter, resynchronised every step on the kernel's own row k + 1, at the bounds tests/test_gpu_random.py::test_smoother_many_shapes grants every
smoother kernel (1e-7 relative on states and on covariances).  Yardstick (b): the reference's own result, tests/golden/live_rts.npz, at the bounds
of tests/test_gpu_rts.py::test_rts_live_vs_reference_and_inplace.  All three kernels: rn::k_rts<.., true> (rand5, kinematic6), k_rts4_pf (rand8,
kinematic9, randaff11, randz10) and rn::k_rts_group<.., true> (live, whose k_rts4_pf does not fit the register file).  The measured maxima go to profiles/rts_pf_parity.json when
RN_WRITE_PARITY=1 (the committed file is such a run's)."""
import json
import os

import numpy as np
import pytest

from conftest import REPO, assert_close, golden
from rts_pf_cases import UNKNOWN_KIND, OracleModel, forward_dts, restate, schedule

pytestmark = pytest.mark.gpu

BOUND = 1e-7
MODELS = ["rand5", "kinematic6", "rand8", "kinematic9", "randaff11", "randz10", "live"]
_PARITY = {}


def _record(key, **figures):
  _PARITY[key] = {k: float(v) for k, v in figures.items()}
  if os.environ.get("RN_WRITE_PARITY"):
    fn = os.path.join(REPO, "profiles", "rts_pf_parity.json")
    old = {}
    if os.path.exists(fn):
      with open(fn, encoding="utf-8") as f:
        old = json.load(f)
    old.update(_PARITY)
    with open(fn, "w", encoding="utf-8") as f:
      json.dump(old, f, indent=1, sort_keys=True)
      f.write("\n")


_CASES = {}


def _case(name):
  """-> (model class, (D, E), quaternion indices, kinds, {kind: R}, states(rng, n) -> x0, P0, hx)"""
  if name in _CASES:
    return _CASES[name]
  if name in ("randaff11", "randz10"):
    import examples.random_kf as R
    M = R.RandomAffine11Kalman if name == "randaff11" else R.RandomWideObs10Kalman
    D = int(M.initial_x.shape[0])

    def states(rng, n):
      x0 = M.initial_x[None] + rng.normal(size=(n, D)) * 0.3
      A = rng.normal(size=(n, D, D)) * 0.2
      return x0, np.diag(M.initial_P_diag)[None] + A @ A.transpose(0, 2, 1), None
    out = M, (D, D), [], tuple(sorted(M.obs_noise)), {k: np.atleast_2d(M.obs_noise[k]) for k in M.obs_noise}, states
  else:
    from test_gpu_run_pf import _case as pf_case
    M, kw, _, kinds, Rs, states = pf_case(name)
    if name == "live":      # (its states() evaluates h over the golden rows: once per module)
      memo = {}

      def live_states(rng, n, states=states):
        if "g" not in memo:
          memo["g"] = states(np.random.default_rng(0), 512)
        x0, P0, hx = memo["g"]
        idx = rng.integers(0, 512, size=n)
        return x0[idx], P0[idx], {k: v[idx] for k, v in hx.items()}
      states = live_states
    out = M, kw["dim"], kw["quat"], tuple(kinds), Rs, states
  _CASES[name] = out
  return out


def _filter(name, n, per_filter=True):
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  M, (D, E), quat, kinds, Rs, states = _case(name)
  gen = ensure_generated([M.name])
  return BatchedEKF(gen, M.name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat, per_filter=per_filter)


def _observations(name, rng, kd, hx):
  """zs (T, n, zmax): near h(x0) where the case provides it (live), small random numbers otherwise"""
  M, _, _, kinds, Rs, _ = _case(name)
  T, n = kd.shape
  zmax = max(r.shape[0] for r in Rs.values())
  zs = rng.normal(size=(T, n, zmax)) * 0.5
  if hx is not None:
    for k in kinds:
      Z = Rs[k].shape[0]
      sel = kd == k
      zs[:, :, :Z] = np.where(sel[:, :, None], hx[k][None] + rng.normal(size=(T, n, Z)) * 1e-3, zs[:, :, :Z])
  return zs


def _norm_pred(name):
  quat = _case(name)[2]
  if not quat:
    return None

  def norm(x):
    x = x.copy()
    for q in quat:
      x[q:q + 4] /= np.linalg.norm(x[q:q + 4])
    return x
  return norm


def _oracle_model(name):
  from oracle_lib import OracleLib
  M, (D, E) = _case(name)[:2]
  return OracleModel(OracleLib(M.name), D, E)


def _trace(name, n, T, seed, t0=0.9):
  """A ragged schedule from the builder, replayed by run_logs(trace=True) -> (filter, schedule, dts, act, trace_x, trace_P)"""
  f = _filter(name, n)
  M, _, _, kinds, Rs, states = _case(name)
  rng = np.random.default_rng(seed)
  x0, P0, hx = states(rng, n)
  sch = schedule(n, T, kinds, seed=seed)
  zs = _observations(name, rng, sch["kinds"], hx)
  f.init_state(x0, P0, np.full(n, t0))
  _, tx, tP, _ = f.run_logs(sch["ts_fwd"], sch["kinds"], zs, Rs, trace=True)
  dts = forward_dts(sch["ts"], sch["kinds_rts"], np.full(n, t0))
  act = np.isin(sch["kinds_rts"], np.array(kinds)).astype(np.uint8)
  assert np.array_equal(dts * act, forward_dts(sch["ts_fwd"], sch["kinds"], np.full(n, t0)) * act)      # the unknown-kind entry moves no dt
  return f, sch, dts, act, tx, tP


@pytest.mark.parametrize("name", MODELS)
def test_shapes_against_the_restatement(name):
  """n in {1, 4, 7, 130} x T in {1, 2, 3, 9}: one full tile plus a ragged one for both kernels (2 resp. 4 filters per wavefront), more than one
  block, and the T at which the recursion has no step (1), only its first (2), and a first plus one other (3).  Every filter and row against (a);
  pass-through rows bit for bit; separate outputs and in place agree bit for bit."""
  import torch
  model, Q, norm = _oracle_model(name), np.asarray(_case(name)[0].Q, dtype=np.float64), _norm_pred(name)
  worst = dict(x=0.0, P=0.0)
  rows = 0
  for n in (1, 4, 7, 130):
    for T in (1, 2, 3, 9):
      f, sch, dts, act, tx, tP = _trace(name, n, T, seed=3)
      X, P = tx.cpu().numpy(), tP.cpu().numpy()
      assert np.isfinite(X).all() and np.isfinite(P).all(), f"{name} n={n} T={T}: the forward trace is not finite; kinds {sch['kinds'].T.tolist()[:4]}"
      xs, Ps = f.rts_smooth_logs(tx, tP, sch["ts"], sch["kinds_rts"], t0=np.full(n, 0.9))
      torch.cuda.synchronize()
      assert torch.equal(tx.cpu(), torch.as_tensor(X)) and torch.equal(tP.cpu(), torch.as_tensor(P)), "separate outputs: the trace is an input"
      xs_, Ps_ = xs.cpu().numpy(), Ps.cpu().numpy()
      bad = sorted(set(zip(*np.nonzero(~np.isfinite(Ps_).all(axis=(2, 3)) | ~np.isfinite(xs_).all(axis=2)))))
      assert not bad, f"{name} n={n} T={T}: non-finite smoothed rows (t, i) {bad[:12]}; act of those filters {[act[:, i].tolist() for i in sorted({b[1] for b in bad})[:4]]}"
      r = restate(model, X, P, dts, act, xs_, Ps_, Q, norm_pred=norm)
      print(f"{name} n={n} T={T}: x {r['worst']['x']:.3e} P {r['worst']['P']:.3e} pass-through rows {len(r['passed'])}")
      assert r["bits"], f"{name} n={n} T={T}: a pass-through row changed"
      assert r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, (name, n, T, r["worst"])
      worst = {k: max(worst[k], r["worst"][k]) for k in worst}
      rows += len(r["passed"])
      xi, Pi = f.rts_smooth_logs(tx, tP, sch["ts"], sch["kinds_rts"], t0=np.full(n, 0.9), inplace=True)
      torch.cuda.synchronize()
      assert xi.data_ptr() == tx.data_ptr() and torch.equal(xi, xs) and torch.equal(Pi, Ps), f"{name} n={n} T={T}: in place differs"
  assert rows > 0
  _record(f"shapes/{name}", x=worst["x"], P=worst["P"])


@pytest.mark.parametrize("name", ["kinematic6", "kinematic9", "randaff11"])
def test_last_predicted_is_taken_where_passed(name):
  """x_last / P_last: row i is filter i's newest smoothed pair, at its own last entry (row 0 included)."""
  import torch
  model, Q, norm = _oracle_model(name), np.asarray(_case(name)[0].Q, dtype=np.float64), _norm_pred(name)
  n, T = 7, 9
  f, sch, dts, act, tx, tP = _trace(name, n, T, seed=5)
  rng = np.random.default_rng(6)
  X, P = tx.cpu().numpy(), tP.cpu().numpy()
  xl = X[-1] + rng.normal(size=X[-1].shape) * 1e-3
  Pl = 1.5 * np.tril(P[-1]) + 1.5 * np.tril(P[-1], -1).transpose(0, 2, 1)
  xs, Ps = f.rts_smooth_logs(tx, tP, sch["ts"], sch["kinds_rts"], t0=np.full(n, 0.9), last_predicted=(xl, Pl))
  torch.cuda.synchronize()
  xs_, Ps_ = xs.cpu().numpy(), Ps.cpu().numpy()
  for i in range(n):
    st = np.nonzero(act[:, i])[0]
    if len(st):
      assert np.array_equal(xs_[st[-1], i], xl[i]) and np.array_equal(Ps_[st[-1], i], Pl[i]), i
  r = restate(model, X, P, dts, act, xs_, Ps_, Q, norm_pred=norm, x_last=xl, P_last=Pl)
  assert r["bits"] and r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, r["worst"]
  _record(f"last_predicted/{name}", x=r["worst"]["x"], P=r["worst"]["P"])


@pytest.mark.parametrize("name,n", [("kinematic6", 5), ("rand8", 7), ("randaff11", 7)])
def test_entry_point_with_guard_rows_in_place_and_not_newest_pair_passed_and_null(name, n):
  """{name}_batch_rts_pf itself, T = 7, one full tile plus a ragged one (2 resp. 4 filters per wavefront), with two guard rows in front of and behind
  both outputs: nothing outside rows 0 .. T - 1 is written, in place and with separate outputs, with x_last / P_last passed and NULL; every case
  against (a), pass-through rows bit for bit.  randaff11 is affine (predict(0) is not the identity): its idle entries must still be identity steps."""
  import itertools
  import torch
  model, Q, norm = _oracle_model(name), np.asarray(_case(name)[0].Q, dtype=np.float64), _norm_pred(name)
  T = 7
  f, sch, dts, act, tx, tP = _trace(name, n, T, seed=13)
  assert act.any(axis=0).sum() >= min(n, 4) and (act == 0).any()
  X, P = tx.cpu().numpy(), tP.cpu().numpy()
  D, E = X.shape[2], P.shape[2]
  rng = np.random.default_rng(14)
  xl = X[-1] + rng.normal(size=X[-1].shape) * 1e-3
  Pl = 1.5 * np.tril(P[-1]) + 1.5 * np.tril(P[-1], -1).transpose(0, 2, 1)
  dev = f.device
  d_dts, d_act = torch.as_tensor(dts, device=dev).contiguous(), torch.as_tensor(act, device=dev).contiguous()
  d_xl, d_Pl = torch.as_tensor(xl, device=dev).contiguous(), torch.as_tensor(Pl, device=dev).contiguous()
  nq = f.norm_quats | (f.norm_quats << 1)
  worst = dict(x=0.0, P=0.0)
  for inplace, last in itertools.product((False, True), (False, True)):
    bx = torch.full((T + 4, n, D), 7.0, dtype=torch.float64, device=dev)
    bP = torch.full((T + 4, n, E, E), 7.0, dtype=torch.float64, device=dev)
    xs, Ps = bx[2:T + 2], bP[2:T + 2]      # (two rows: 16-byte aligned whatever n * D is)
    if inplace:
      xs.copy_(tx); Ps.copy_(tP)
    xf, Pf = (xs, Ps) if inplace else (tx, tP)
    f._call("batch_rts_pf", f._p(xf), f._p(Pf), f._p(d_dts), f._p(d_act), T, f._p(f.Q), n, nq, f._p(xs), f._p(Ps),      # pylint: disable=protected-access
            f._p(d_xl) if last else None, f._p(d_Pl) if last else None, f._stream())
    torch.cuda.synchronize()
    what = f"{name} inplace={inplace} newest pair passed={last}"
    for g in (bx[:2], bx[T + 2:], bP[:2], bP[T + 2:]):
      assert bool((g == 7.0).all()), what + ": a guard row was written"
    assert torch.equal(tx.cpu(), torch.as_tensor(X)) and torch.equal(tP.cpu(), torch.as_tensor(P)), what + ": the trace was written"
    r = restate(model, X, P, dts, act, xs.cpu().numpy(), Ps.cpu().numpy(), Q, norm_pred=norm, x_last=xl if last else None, P_last=Pl if last else None)
    print(f"{what}: x {r['worst']['x']:.3e} P {r['worst']['P']:.3e} pass-through rows {len(r['passed'])}")
    assert r["bits"], what + ": a pass-through row changed"
    assert r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, (what, r["worst"])
    worst = {k: max(worst[k], r["worst"][k]) for k in worst}
  _record(f"entry_point/{name}", x=worst["x"], P=worst["P"])


def test_golden_live_with_idle_rows_inserted():
  """tests/golden/live_rts.npz replicated to 6 filters: 0 as it is, 1 .. 3 with idle rows inserted at different places (duplicated pairs, act = 0), 4 as
  it is, 5 without an entry.  The real rows of filters 0 .. 3 against the reference's xs_smooth / Ps_smooth at the bounds of
  test_rts_live_vs_reference_and_inplace; smoothed quaternions unit-norm as there."""
  import torch
  from examples.live_kf import LiveKalman as L
  g = golden("live_rts.npz")
  T0, n, extra = len(g["t"]), 6, 3
  T = T0 + extra
  f = _filter("live", n)
  idle_at = {1: [1, 2, T - 1], 2: [T0 // 2, T0 // 2 + 1, T0 // 2 + 5], 3: [5, T - 3, T - 2]}      # rows of the padded log that hold no entry
  ts = np.full((T, n), np.nan); kinds = np.zeros((T, n), dtype=np.int32)
  xf = np.zeros((T, n, 23)); Pf = np.zeros((T, n, 22, 22))
  real = {}
  kind = int(f.kinds[0])
  for i in range(n):
    rows = [r for r in range(T) if r not in idle_at.get(i, [])][:T0] if i != 5 else []
    real[i] = rows
    j = -1
    for r in range(T):
      if r in rows:
        j += 1
        ts[r, i] = g["t"][j]; kinds[r, i] = kind
      jj = max(j, 0)      # an idle row holds the pair its filter already had (in front of the first entry: anything the filter started from)
      xf[r, i] = g["xk_k"][jj]; Pf[r, i] = g["Pk_k"][jj]
  t0 = np.full(n, g["t"][0])      # the first entry's dt is 0 whatever it is: the golden recursion does not reach behind it
  xs, Ps = f.rts_smooth_logs(xf, Pf, ts, kinds, t0=t0, norm_quats=True)
  torch.cuda.synchronize()
  X, P = xs.cpu().numpy(), Ps.cpu().numpy()
  idx = g["Ps_smooth_idx"]
  worst = dict(x=0.0, P=0.0)
  for i in range(4):
    rows = np.array(real[i])
    assert_close(X[rows, i], g["xs_smooth"], rtol=1e-8, floor=1e-8, what=f"smoothed live states, filter {i}")
    assert_close(P[rows[idx], i].reshape(len(idx), -1), g["Ps_smooth"].reshape(len(idx), -1), rtol=1e-8, floor=1e-8, what=f"smoothed live covs, filter {i}")
    worst["x"] = max(worst["x"], float(np.max(np.abs(X[rows, i] - g["xs_smooth"]) / np.maximum(np.abs(g["xs_smooth"]).max(axis=1, keepdims=True), 1e-300))))
    worst["P"] = max(worst["P"], float(max(np.abs(P[rows[k], i] - g["Ps_smooth"][a]).max() / np.abs(g["Ps_smooth"][a]).max() for a, k in enumerate(idx))))
    qn = np.linalg.norm(X[rows[1:], i, 3:7], axis=1)
    assert np.abs(qn - 1).max() < 1e-14
  assert np.array_equal(X[:, 5], xf[:, 5]) and np.array_equal(P[:, 5], Pf[:, 5])      # no entry: every row passes through
  for i in (1, 3):      # rows behind the last entry pass through
    last = real[i][-1]
    assert np.array_equal(X[last + 1:, i], xf[last + 1:, i]) and np.array_equal(P[last + 1:, i], Pf[last + 1:, i])
  _record("golden/live", x=worst["x"], P=worst["P"])


@pytest.mark.parametrize("name", ["kinematic6", "rand5", "kinematic9", "rand8"])
def test_shared_schedule_is_a_special_case(name):
  """Every entry real, on common times: batch_rts_pf against batch_rts on the same trace.  The per-filter instantiations walk the same
  statements in the same order as the shared-schedule kernels of the same template (dt is read instead of subtracted: the forward fill
  subtracts the same two doubles), so for rn::k_rts the results are asserted BIT FOR BIT.  The lane-group libraries listed here launch k_rts4 for
  batch_rts and k_rts4_pf for batch_rts_pf: the same phases, but k_rts4 takes a separate path through steps with dt == 0 where k_rts4_pf forces
  Ck = I inside the full path (sums in another order), so they are held to the bounds
  tests/test_gpu_run_pf.py::test_shared_schedule_is_a_special_case grants batch_run_pf against batch_run for lane-group models
  (x: rtol 1e-9, floor 1e-11; P: rtol 1e-8, floor 1e-10)."""
  import torch
  M, _, _, kinds, Rs, states = _case(name)
  n, T = 131, 9
  rng = np.random.default_rng(9)
  x0, P0, hx = states(rng, n)
  dts = rng.uniform(0.005, 0.03, size=T); dts[[2, 5]] = 0.0
  ts = 1.0 + np.cumsum(dts)
  sched = np.array([kinds[t % len(kinds)] for t in range(T)], dtype=np.int32)
  kd = np.tile(sched[:, None], (1, n))
  zs = _observations(name, rng, kd, hx)
  f = _filter(name, n)
  f.init_state(x0, P0, np.full(n, 0.9))
  tsn = np.tile(ts[:, None], (1, n))
  _, tx, tP, _ = f.run_logs(tsn, kd, zs, Rs, trace=True)
  xa, Pa = f.rts_smooth(tx, tP, ts)
  xb, Pb = f.rts_smooth_logs(tx, tP, tsn, kd, t0=np.full(n, 0.9))
  torch.cuda.synchronize()
  dx = float((xa - xb).abs().max()); dP = float((Pa - Pb).abs().max())
  _record(f"shared/{name}", x_abs=dx, P_abs=dP)
  if name in ("kinematic6", "rand5"):
    assert torch.equal(xa, xb) and torch.equal(Pa, Pb), (dx, dP)
  else:
    assert_close(xb.cpu().numpy().reshape(T * n, -1), xa.cpu().numpy().reshape(T * n, -1), rtol=1e-9, floor=1e-11, what=f"{name} x")
    assert_close(Pb.cpu().numpy().reshape(T * n, -1), Pa.cpu().numpy().reshape(T * n, -1), rtol=1e-8, floor=1e-10, what=f"{name} P")


@pytest.mark.parametrize("name", ["kinematic6", "kinematic9", "live"])
def test_wavefront_neighbours_do_not_matter(name):
  """A filter's log smoothed once in a tile of copies of itself and once among different logs: both runs are held to (a); their mutual
  difference goes to the parity file (asserted zero: nothing a filter computes reads another filter's values)."""
  import torch
  model, Q, norm = _oracle_model(name), np.asarray(_case(name)[0].Q, dtype=np.float64), _norm_pred(name)
  n, T = 7, 9
  f, sch, dts, act, tx, tP = _trace(name, n, T, seed=11)
  xs, Ps = f.rts_smooth_logs(tx, tP, sch["ts"], sch["kinds_rts"], t0=np.full(n, 0.9))
  worst = dict(x=0.0, P=0.0, mutual_x=0.0, mutual_P=0.0)
  for i in (0, 1, 3):
    col = lambda a: np.ascontiguousarray(np.repeat(a[:, i:i + 1], n, axis=1))      # noqa: E731
    X1, P1 = col(tx.cpu().numpy()), col(tP.cpu().numpy())
    x1, p1 = f.rts_smooth_logs(X1, P1, col(sch["ts"]), col(sch["kinds_rts"]), t0=np.full(n, 0.9))
    torch.cuda.synchronize()
    r = restate(model, X1, P1, col(dts), col(act), x1.cpu().numpy(), p1.cpu().numpy(), Q, norm_pred=norm)
    assert r["bits"] and r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, (i, r["worst"])
    worst["x"], worst["P"] = max(worst["x"], r["worst"]["x"]), max(worst["P"], r["worst"]["P"])
    worst["mutual_x"] = max(worst["mutual_x"], float((x1[:, 0] - xs[:, i]).abs().max()))
    worst["mutual_P"] = max(worst["mutual_P"], float((p1[:, 0] - Ps[:, i]).abs().max()))
    assert torch.equal(x1[:, 0], xs[:, i]) and torch.equal(p1[:, 0], Ps[:, i]), i
  r = restate(model, tx.cpu().numpy(), tP.cpu().numpy(), dts, act, xs.cpu().numpy(), Ps.cpu().numpy(), Q, norm_pred=norm)
  assert r["bits"] and r["worst"]["x"] < BOUND and r["worst"]["P"] < BOUND, r["worst"]
  _record(f"neighbours/{name}", **worst)


def test_plumbing():
  """smooth_logs == run_logs(trace=True) + rts_smooth_logs(inplace=True) bit for bit; zs untouched; filter_times() as after run_logs; the refusals."""
  import torch
  from rednose_amd.helpers.ekf_sym import KalmanError
  name, n, T = "kinematic9", 7, 9
  M, _, _, kinds, Rs, states = _case(name)
  rng = np.random.default_rng(21)
  x0, P0, hx = states(rng, n)
  sch = schedule(n, T, kinds, seed=21)
  zs = _observations(name, rng, sch["kinds"], hx)
  f, g = _filter(name, n), _filter(name, n)
  f.init_state(x0, P0, np.full(n, 0.9)); g.init_state(x0, P0, np.full(n, 0.9))
  zd = torch.as_tensor(zs, device=f.device)
  keep = zd.clone()
  xs, Ps, ys, fl = f.smooth_logs(sch["ts_fwd"], sch["kinds"], zd, Rs, flags=True)
  assert torch.equal(zd, keep), "smooth_logs consumed zs"
  yb, tx, tP, fb = g.run_logs(sch["ts_fwd"], sch["kinds"], zs.copy(), Rs, trace=True, flags=True)
  xb, Pb = g.rts_smooth_logs(tx, tP, sch["ts_fwd"], sch["kinds"], t0=np.full(n, 0.9), inplace=True)
  torch.cuda.synchronize()
  assert torch.equal(xs, xb) and torch.equal(Ps, Pb) and torch.equal(ys, yb) and torch.equal(fl, fb)
  assert torch.equal(f.filter_times(), g.filter_times()) and torch.equal(f.x, g.x) and torch.equal(f.P, g.P)
  # the refusals
  with pytest.raises(KalmanError, match="per_filter"):
    _filter(name, n, per_filter=False).rts_smooth_logs(tx, tP, sch["ts_fwd"], sch["kinds"])
  with pytest.raises(KalmanError, match="has_batch_rts_pf"):
    from examples import ensure_generated
    from examples.feature_kf import FeatureKalman as FK
    from rednose_amd.helpers.ekf_sym import BatchedEKF
    ff = BatchedEKF(ensure_generated(["feature"]), "feature", FK.Q, FK.initial_x, np.diag(FK.initial_P_diag), 6, 6, batch=2, per_filter=True,
                    **FK.filter_kwargs())
    ff.rts_smooth_logs(np.zeros((2, 2, ff.dim_x)), np.zeros((2, 2, ff.dim_err, ff.dim_err)), np.ones((2, 2)), np.zeros((2, 2), dtype=np.int32))
  bad = sch["ts_fwd"].copy()
  bad[[0, 1], 0] = bad[[1, 0], 0] + np.array([0.5, 0.0])      # filter 0: row 0 later than row 1
  with pytest.raises(KalmanError, match="sort the log"):
    g.rts_smooth_logs(tx, tP, bad, sch["kinds"])
  nan = sch["ts_fwd"].copy(); nan[0, 0] = np.nan
  with pytest.raises(KalmanError, match="without a time"):
    g.rts_smooth_logs(tx, tP, nan, sch["kinds"])
  for args in ((tx.cpu().numpy()[:, :-1].tolist(), tP, sch["ts_fwd"], sch["kinds"]), (tx[:, :-1], tP, sch["ts_fwd"], sch["kinds"]), (tx, tP[:-1], sch["ts_fwd"], sch["kinds"]), (tx, tP, sch["ts_fwd"][:, :-1], sch["kinds"]),
               (tx, tP, sch["ts_fwd"], sch["kinds"][:-1])):
    with pytest.raises(KalmanError):
      g.rts_smooth_logs(*args)
  assert sch["unknown"] is not None and UNKNOWN_KIND not in kinds


def test_smoothing_reduces_the_covariance_trace():
  """A consistent kinematic9 log per filter (observations of the true trajectory plus their noise): the check of
  tests/test_gpu_rts.py::test_forward_trace_then_smooth_reduces_uncertainty, over the real rows of every filter."""
  import torch
  name, n, T = "kinematic9", 64, 40
  M, _, _, kinds, Rs, states = _case(name)
  rng = np.random.default_rng(31)
  sch = schedule(n, T, kinds, seed=31)
  f = _filter(name, n)
  f.init_state(M.initial_x, np.diag(M.initial_P_diag), np.full(n, 0.9))
  zmax = max(r.shape[0] for r in Rs.values())
  zs = np.zeros((T, n, zmax))
  for k in kinds:      # the filters start at initial_x with initial_P: observations of a state at rest there, with their noise
    Z = Rs[k].shape[0]
    zs[:, :, :Z] = np.where((sch["kinds"] == k)[:, :, None], rng.multivariate_normal(np.zeros(Z), Rs[k], size=(T, n)) * 0.1, zs[:, :, :Z])
  xs, Ps, _, _ = f.smooth_logs(sch["ts_fwd"], sch["kinds"], zs, Rs)
  g = _filter(name, n)
  g.init_state(M.initial_x, np.diag(M.initial_P_diag), np.full(n, 0.9))
  _, tx, tP, _ = g.run_logs(sch["ts_fwd"], sch["kinds"], zs.copy(), Rs, trace=True)
  torch.cuda.synchronize()
  assert torch.isfinite(xs).all() and torch.isfinite(Ps).all()
  tr_f = torch.diagonal(tP, dim1=-2, dim2=-1).sum(-1).cpu().numpy()
  tr_s = torch.diagonal(Ps, dim1=-2, dim2=-1).sum(-1).cpu().numpy()
  real = sch["kinds"] > 0
  for i in range(n):      # (a filter's newest smoothed pair is its PREDICTED one: not below the filtered)
    st = np.nonzero(real[:, i])[0]
    if len(st):
      real[st[-1], i] = False
  assert real.sum() > T * n // 3
  assert (tr_s[real] <= tr_f[real] * (1 + 1e-9)).all()
  assert (tr_s[real] < tr_f[real] * (1 - 1e-6)).sum() > real.sum() // 4, "smoothing changed next to nothing"
