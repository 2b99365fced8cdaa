"""Per-filter timelines with the in-order bookkeeping on the device ({name}_batch_timeline_plan / _push, BatchedEKF(device_timeline=...)):
  1. the two kernels against a numpy restatement of their contract (include/rednose_amd_filter.h), bit for bit -- they copy and subtract;
  2. the fast path against the torch bookkeeping (device_timeline=False) on the golden per-filter logs, bit for bit after every call;
  3. an in-order stream never leaves the fast path and ends where the shared timeline ends;
  4. the device_timeline argument, reset_rewind() / init_state() in mid-stream."""
import ctypes

import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

SENT = -777.25          # what untouched memory holds


@pytest.fixture(scope="module")
def gen():
  import torch
  assert torch.cuda.is_available()
  from examples import ensure_generated
  return ensure_generated(["kinematic", "kinematic6", "kinematic9", "live", "feature"])


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernels' contract, restated
# ------------------------------------------------------------------------------------------------------------------
def plan_model(t, active, ft):
  on = np.ones(len(t), dtype=bool) if active is None else active != 0
  late = on & (t < ft)                                   # (False where ft is NaN)
  act = on & ~late
  with np.errstate(invalid="ignore"):
    dt = np.where(act, np.where(np.isnan(ft), 0.0, t - ft), 0.0)
  return dt, act.astype(np.uint8), late.astype(np.uint8), int(late.sum())


def push_model(t, act, ft, x, P, ring, K, kind, nobs, Z, EA, z_obs, R, per, ea):
  """ring: dict of numpy arrays in BatchedEKF._ring_alloc's layout, modified in place like ft.  z_obs (n, nobs, Z), R (nobs, Z, Z) or
  (n, nobs, Z, Z), ea (n, nobs, EA) or None."""
  for i in np.nonzero(act)[0]:
    ft[i] = t[i]
    if K == 0:
      continue
    full = ring["length"][i] >= K
    ring["head"][i] = (ring["head"][i] + 1) % K if full else ring["head"][i]
    ring["length"][i] = ring["length"][i] if full else ring["length"][i] + 1
    s = (ring["head"][i] + ring["length"][i] - 1) % K
    ring["t"][s, i], ring["x"][s, i], ring["P"][s, i], ring["kind"][s, i], ring["nobs"][s, i] = t[i], x[i], P[i], kind, nobs
    for j in range(nobs):
      ring["z"][s, i, j, :Z] = z_obs[i, j]
      ring["R"][s, i, j, :Z, :Z] = R[i, j] if per else R[j]
      if EA:
        ring["ea"][s, i, j, :EA] = ea[i, j]


MODELS = {       # name: (D, E, kinds exercised)
  "kinematic": (2, 2, (1,)),
  "kinematic9": (9, 9, (1, 2, 3)),
  "live": (23, 22, (10, 3)),
  "feature": (15, 15, (1, 2)),           # kind 2: a feature track with 3 extra arguments
}


@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_plan_and_push_against_the_numpy_model(gen, name, n, K):
  import torch
  from rednose_amd.helpers import load_code
  ffi, lib = load_code(gen, name, backend="ctypes")
  D, E, kinds = MODELS[name]
  dims = (ctypes.c_int * 3)()
  getattr(lib, f"{name}_dims")(ctypes.cast(dims, ctypes.c_void_p))
  assert (dims[0], dims[1]) == (D, E)
  nk = getattr(lib, f"{name}_num_kinds")()
  kk = (ctypes.c_int * nk)()
  getattr(lib, f"{name}_kinds")(ctypes.cast(kk, ctypes.c_void_p))
  zd = {int(k): getattr(lib, f"{name}_kind_zdim")(int(k)) for k in kk}
  ed = {int(k): getattr(lib, f"{name}_kind_eadim")(int(k)) for k in kk}
  zmax, eamax, nmax = getattr(lib, f"{name}_zmax")(), max(list(ed.values()) + [1]), 3
  assert zmax == max(zd.values())
  rng = np.random.default_rng(1000 * n + 10 * K + len(name))
  dev = torch.device("cuda:0")
  p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None      # noqa: E731
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)           # noqa: E731
  stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

  def call(sym, *args):
    rc = getattr(lib, f"{name}_batch_timeline_{sym}")(*args)
    assert rc == 0, ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()

  ft = rng.uniform(0.0, 1.0, n)
  ft[rng.random(n) < 0.2] = np.nan                       # not started
  ft[0] = np.nan if n > 1 else 0.5
  ring = dict(t=np.full((K, n), SENT), x=np.full((K, n, D), SENT), P=np.full((K, n, E, E), SENT), kind=np.full((K, n), -5, dtype=np.int32),
              nobs=np.full((K, n), -6, dtype=np.int32), z=np.full((K, n, nmax, zmax), SENT), R=np.full((K, n, nmax, zmax, zmax), SENT),
              ea=np.full((K, n, nmax, eamax), SENT), head=np.zeros(n, dtype=np.int64), length=np.zeros(n, dtype=np.int64))
  ft_d = up(ft)
  ring_d = {k: up(v) for k, v in ring.items()} if K else None
  n_late_d = torch.zeros(1, dtype=torch.int32, device=dev)
  n_late_total = 0
  for it in range(K + 3):                                # more pushes than the ring holds: it wraps
    kind = kinds[it % len(kinds)]
    Z, EA = zd[kind], ed[kind]
    nobs = 1 + it % nmax
    per = it % 2
    with_active = it != 1
    active = (rng.random(n) < 0.7).astype(np.uint8) * np.uint8(1 + it) if with_active else None      # any non-zero byte is "active"
    t = np.where(np.isnan(ft), 0.5, ft) + rng.uniform(-0.3, 0.5, n)      # t < ft, t > ft ...
    eq = rng.random(n) < 0.15
    t[eq] = np.where(np.isnan(ft[eq]), t[eq], ft[eq])                        # ... and t == ft: in order, dt = 0
    x, P = rng.normal(size=(n, D)), rng.normal(size=(n, E, E))
    z_obs = rng.normal(size=(n, nobs, Z))
    R = rng.normal(size=(n, nobs, Z, Z)) if per else rng.normal(size=(nobs, Z, Z))
    ea = rng.normal(size=(n, nobs, EA)) if EA else None
    # -- plan: pure
    t_d, a_d = up(t), (up(active) if with_active else None)
    dt_d = torch.full((n,), SENT, dtype=torch.float64, device=dev)
    act_d, late_d = torch.full((n,), 99, dtype=torch.uint8, device=dev), torch.full((n,), 99, dtype=torch.uint8, device=dev)
    z_src, z_keep = up(z_obs), torch.full((n * nobs * Z + 5,), SENT, dtype=torch.float64, device=dev)
    call("plan", p(t_d), p(a_d), p(ft_d), n, p(dt_d), p(act_d), p(late_d), p(n_late_d), p(z_src), p(z_keep), n * nobs * Z, stream)
    torch.cuda.synchronize()
    dt, act, late, cnt = plan_model(t, active, ft)
    n_late_total += cnt
    what = f"{name} n={n} K={K} call {it}"
    assert np.array_equal(dt_d.cpu().numpy(), dt), what
    assert np.array_equal(act_d.cpu().numpy(), act) and np.array_equal(late_d.cpu().numpy(), late), what
    assert int(n_late_d.cpu().numpy()[0]) == n_late_total, what                  # accumulates
    assert np.array_equal(z_keep.cpu().numpy()[:n * nobs * Z], z_obs.reshape(-1)) and np.all(z_keep.cpu().numpy()[n * nobs * Z:] == SENT), what
    assert np.array_equal(ft_d.cpu().numpy(), ft, equal_nan=True), f"{what}: plan wrote ft"
    if it == 0 and n >= 63:
      assert cnt > 0 and (dt[act != 0] == 0).any() and (dt > 0).any() and np.isnan(ft[act != 0]).any()      # every case of the contract occurs
    # -- push
    x_d, P_d, R_d, ea_d = up(x), up(P), up(R), (up(ea) if EA else None)
    if K:
      r = ring_d
      call("push", p(t_d), p(act_d), p(ft_d), p(x_d), p(P_d), n, K, nmax, p(r["t"]), p(r["x"]), p(r["P"]), p(r["kind"]), p(r["nobs"]), p(r["z"]), p(r["R"]),
           p(r["ea"]), p(r["head"]), p(r["length"]), kind, nobs, p(z_src), nobs * Z, Z, p(R_d), per, nobs * Z * Z, Z * Z, p(ea_d), nobs * EA, EA, stream)
    else:
      call("push", p(t_d), p(act_d), p(ft_d), None, None, n, 0, 0, *([None] * 10), kind, nobs, None, 0, 0, None, 0, 0, 0, None, 0, 0, stream)
    torch.cuda.synchronize()
    push_model(t, act, ft, x, P, ring, K, kind, nobs, Z, EA, z_obs, R, per, ea)
    assert np.array_equal(ft_d.cpu().numpy(), ft, equal_nan=True), f"{what}: ft"      # inactive and late filters keep theirs
    if K:
      for key in ring:
        assert np.array_equal(ring_d[key].cpu().numpy(), ring[key]), f"{what}: ring {key}"      # untouched slots and columns keep the sentinel
  if K and n >= 63:
    assert (ring["length"] == K).any() and ((ring["head"] != 0).any() or K == 1), "some rings are full and have wrapped"


# ------------------------------------------------------------------------------------------------------------------
# 2. fast path == torch bookkeeping, bit for bit
# ------------------------------------------------------------------------------------------------------------------
class Pair:
  """Two BatchedEKF objects fed identical calls: `a` with the torch bookkeeping, `b` the default (device timeline)."""

  def __init__(self, make):
    self.a, self.b = make(device_timeline=False), make()
    assert self.b._device_timeline and not self.a._device_timeline      # pylint: disable=protected-access
    self.calls = self.late_calls = 0

  def call(self, t, kind, z, R, active=None, **kw):
    import torch
    a, b = self.a, self.b
    ft = a.filter_times().cpu().numpy()
    tt = np.broadcast_to(np.asarray(t, dtype=np.float64), ft.shape)
    on = np.ones(len(ft), dtype=bool) if active is None else np.asarray(active, dtype=bool)
    self.late_calls += int((on & (tt < ft)).any())
    self.calls += 1
    cp = lambda v: v.copy() if isinstance(v, np.ndarray) else v      # noqa: E731
    ra = a.predict_and_update_batch(cp(t), kind, cp(z), cp(R), active=cp(active), **kw)
    rb = b.predict_and_update_batch(cp(t), kind, cp(z), cp(R), active=cp(active), **kw)
    what = f"call {self.calls}"

    def flat(r):            # the tensors of a return value: y, or the Estimate tuple with its list of residuals
      out = []
      for v in (r if isinstance(r, tuple) else (r,)):
        out.extend(w for w in (v if isinstance(v, list) else [v]) if isinstance(w, torch.Tensor))
      return out
    fa, fb = flat(ra), flat(rb)
    assert len(fa) == len(fb) and len(fa) >= 1
    for u, v in zip(fa, fb):
      assert np.array_equal(u.cpu().numpy(), v.cpu().numpy(), equal_nan=True), f"{what}: returned tensors"
    self.same(what)
    return rb

  def same(self, what):
    a, b = self.a, self.b
    assert np.array_equal(a.state(), b.state()) and np.array_equal(a.covs(), b.covs()), f"{what}: x / P"
    assert np.array_equal(a.flags.cpu().numpy(), b.flags.cpu().numpy()), f"{what}: flags"
    assert np.array_equal(a.filter_times().cpu().numpy(), b.filter_times().cpu().numpy(), equal_nan=True), f"{what}: filter times"
    ra, rb = a._ring, b._ring      # pylint: disable=protected-access
    assert (ra is None) == (rb is None), what
    if ra is None:
      return
    assert ra["nmax"] == rb["nmax"]
    La, Ha, Lb, Hb = (r_[k].cpu().numpy() for r_ in (ra, rb) for k in ("length", "head"))
    assert np.array_equal(La, Lb) and np.array_equal(Ha, Hb), f"{what}: ring lengths / heads"
    K = ra["t"].shape[0]
    valid = ((np.arange(K)[:, None] - Ha[None, :]) % K) < La[None, :]            # slots that hold an entry
    for key in ("t", "x", "P", "kind", "nobs", "z", "R", "ea"):
      va, vb = ra[key].cpu().numpy(), rb[key].cpu().numpy()
      if key in ("z", "R", "ea"):                           # an entry holds nobs observations
        nobs = ra["nobs"].cpu().numpy()
        m = valid[:, :, None] & (np.arange(va.shape[2])[None, None, :] < nobs[:, :, None])
        assert np.array_equal(va[m], vb[m]), f"{what}: ring {key}"
      else:
        assert np.array_equal(va[valid], vb[valid]), f"{what}: ring {key}"

  def check_stats(self):
    s = self.b.pf_stats
    assert s["fast"] + s["legacy"] == self.calls and s["legacy"] == self.late_calls, (s, self.calls, self.late_calls)
    assert self.a.pf_stats == {"fast": 0, "legacy": self.calls}


@pytest.mark.parametrize("copies", [1, 7])
def test_fast_path_equals_torch_path_on_the_swapped_pair_logs(gen, copies):
  """Part A of perfilter_timelines.npz (test_gpu_timelines.py): a stress log -- 411 of its 700 calls have a late filter -- so both paths
  are used, in alternation, on the same rings.  The default object keeps the golden tolerances."""
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  g = golden("perfilter_timelines.npz")
  NA, T = g["A_t"].shape
  n = NA * copies
  tile = lambda a: np.concatenate([a] * copies, axis=0)      # noqa: E731
  pr = Pair(lambda **kw: BatchedEKF(gen, "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.eye(2), 2, 2, batch=n, rewind_to_keep=512,
                                    per_filter=True, **kw))
  R = np.array([[0.1**2]])
  keep = set(g["A_keep"].tolist())
  f = pr.b
  for j in range(T):
    y = pr.call(tile(g["A_t"][:, j]), 1, tile(g["A_z"][:, j:j + 1]), R)
    assert y is not None
    fl = f.flags.cpu().numpy()
    assert np.array_equal((fl & 32) != 0, tile(g["A_none"][:, j])), f"arrival {j}: which filters ignored their observation"
    assert np.abs(f.filter_times().cpu().numpy() - tile(g["A_ft"][:, j])).max() < 1e-12, f"arrival {j}: filter times"
    if j in keep:
      a = j // 25
      assert_close(f.state(), tile(g["A_x"][:, a]), rtol=1e-9, floor=1e-11, what=f"arrival {j} x")
      assert_close(f.covs().reshape(n, -1), tile(g["A_P"][:, a]).reshape(n, -1), rtol=1e-9, floor=1e-11, what=f"arrival {j} P")
  assert_close(f.state(), tile(g["A_x_final"]), rtol=1e-9, floor=1e-11, what="final x")
  assert_close(f.covs().reshape(n, -1), tile(g["A_P_final"]).reshape(n, -1), rtol=1e-9, floor=1e-11, what="final P")
  pr.check_stats()
  assert f.pf_stats["fast"] > 0 and f.pf_stats["legacy"] > 0, f.pf_stats


def test_fast_path_equals_torch_path_on_the_three_kind_logs(gen):
  """Part B: the 9-state model, masks, three kinds, one late observation per filter."""
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  g = golden("perfilter_timelines.npz")
  NB, TB = g["B_t"].shape
  pr = Pair(lambda **kw: BatchedEKF(gen, "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=NB, rewind_to_keep=64, per_filter=True, **kw))
  f = pr.b
  for j in range(TB):
    for k in (1, 2, 3):
      act = g["B_kind"][:, j] == k
      if not act.any():
        continue
      Z = K9.obs_noise[k].shape[0]
      y = pr.call(np.nan_to_num(g["B_t"][:, j]), k, g["B_z"][:, j, :Z].copy(), K9.obs_noise[k], active=act)
      fl = f.flags.cpu().numpy()
      assert np.array_equal((fl & 16) != 0, ~act) and not (fl & 32).any()
      assert_close(y.cpu().numpy()[act], g["B_y"][act, j, :Z], rtol=1e-7, atol=1e-9, what=f"arrival {j} kind {k} residuals")
    assert_close(f.state(), g["B_x"][:, j], rtol=1e-8, floor=1e-10, what=f"arrival {j} x")
    assert_close(f.covs().reshape(NB, -1), g["B_P"][:, j].reshape(NB, -1), rtol=1e-8, floor=1e-10, what=f"arrival {j} P")
  pr.check_stats()
  assert f.pf_stats["fast"] > 0 and f.pf_stats["legacy"] > 0, f.pf_stats


def test_fast_path_equals_torch_path_on_the_multi_observation_logs(gen):
  """The per-filter part of multi_obs.npz (test_gpu_multi_obs.py): 1-3 observations per call, a noise matrix per filter and observation,
  Estimates every sixth arrival, one late multi-observation call per filter."""
  import torch
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  g = golden("multi_obs.npz")
  NB, TB = g["A_t"].shape
  pr = Pair(lambda **kw: BatchedEKF(gen, "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=NB, rewind_to_keep=64, per_filter=True, **kw))
  f = pr.b
  for j in range(TB):
    est_at = j % 6 == 0
    for k in (1, 2, 3):
      Z = K9.obs_noise[k].shape[0]
      for n in (1, 2, 3):
        act = (g["A_kind"][:, j] == k) & (g["A_n"][:, j] == n)
        if not act.any():
          continue
        z = g["A_z"][:, j, :n, :Z].copy()
        R = g["A_Rscale"][:, j, :n, None, None] * K9.obs_noise[k][None, None]
        ret = pr.call(g["A_t"][:, j].copy(), k, z, R, active=act, keep_estimate=est_at)
        y = torch.stack(ret[6], 1) if est_at else ret
        assert tuple(y.shape) == (NB, n, Z)
        assert_close(y.cpu().numpy()[act].reshape(-1, Z), g["A_y"][act, j, :n, :Z].reshape(-1, Z), rtol=1e-7, atol=1e-9, what=f"arrival {j} kind {k} n {n} residuals")
        if est_at:
          assert_close(ret[7].cpu().numpy()[act].reshape(-1, Z), g["A_z"][act, j, :n, :Z].reshape(-1, Z), rtol=0, atol=0, what="Estimate.z is the observation, not the residual")
    assert_close(f.state(), g["A_x"][:, j], rtol=1e-8, floor=1e-10, what=f"arrival {j} x")
    assert_close(f.covs().reshape(NB, -1), g["A_P"][:, j].reshape(NB, -1), rtol=1e-8, floor=1e-10, what=f"arrival {j} P")
  pr.check_stats()
  assert f.pf_stats["fast"] > 0 and f.pf_stats["legacy"] > 0, f.pf_stats
  assert f._ring["nmax"] == 3      # pylint: disable=protected-access


# ------------------------------------------------------------------------------------------------------------------
# 3. an in-order stream stays on the fast path
# ------------------------------------------------------------------------------------------------------------------
def _k6(gen, n, **kw):
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  return BatchedEKF(gen, "kinematic6", K6.Q, K6.initial_x, np.diag(K6.initial_P_diag), 6, 6, batch=n, **kw)


def test_in_order_stream_never_leaves_the_fast_path(gen):
  """200 in-order calls, 4 096 filters, a ring of 8: all served by the device timeline.  With one common time per call the steps are the
  shared timeline's -- same kernels, same dt = t - ft -- so the final state is its state, bit for bit."""
  import torch
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  n, calls = 4096, 200
  rng = np.random.default_rng(5)
  f = _k6(gen, n, per_filter=True, rewind_to_keep=8)
  s = _k6(gen, n)
  x0 = np.tile(K6.initial_x, (n, 1)) + 0.1 * rng.normal(size=(n, 6))
  f.init_state(x0, np.diag(K6.initial_P_diag), 0.0)
  s.init_state(x0, np.diag(K6.initial_P_diag), 0.0)
  t = 0.0
  for i in range(calls):
    t += float(rng.uniform(0.0, 0.02)) if i % 10 else 0.0            # (t == ft is in order too)
    z = rng.normal(size=(n, 3))
    yf = f.predict_and_update_batch(np.full(n, t), 1, z.copy(), K6.obs_noise[1])
    ys = s.predict_and_update_batch(t, 1, z.copy(), K6.obs_noise[1])
    if i % 50 == 0:
      assert np.array_equal(yf.cpu().numpy(), ys.cpu().numpy())
  torch.cuda.synchronize()
  assert f.pf_stats == {"fast": calls, "legacy": 0}
  assert np.array_equal(f.state(), s.state()) and np.array_equal(f.covs(), s.covs())
  assert np.array_equal(f.filter_times().cpu().numpy(), np.full(n, t))
  r = f._ring      # pylint: disable=protected-access
  assert (r["length"].cpu().numpy() == 8).all() and (r["head"].cpu().numpy() == (calls - 8) % 8).all()
  newest = (r["head"].cpu().numpy() + 7) % 8
  assert np.array_equal(r["x"].cpu().numpy()[newest, np.arange(n)], f.state()) and np.array_equal(r["t"].cpu().numpy()[newest, np.arange(n)], np.full(n, t))


# ------------------------------------------------------------------------------------------------------------------
# 4. the argument; reset_rewind() / init_state() in mid-stream
# ------------------------------------------------------------------------------------------------------------------
def test_device_timeline_true_needs_the_symbols(gen, monkeypatch):
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  f = _k6(gen, 8, per_filter=True, device_timeline=True)
  assert f._device_timeline      # pylint: disable=protected-access
  monkeypatch.setattr(BatchedEKF, "_has_timeline_abi", lambda self: False)      # a library generated before the entry points existed
  with pytest.raises(KalmanError):
    _k6(gen, 8, per_filter=True, device_timeline=True)
  g = _k6(gen, 8, per_filter=True)                   # None: the torch bookkeeping, silently
  assert not g._device_timeline      # pylint: disable=protected-access
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  g.predict_and_update_batch(np.full(8, 0.1), 1, np.zeros((8, 3)), K6.obs_noise[1])
  assert g.pf_stats == {"fast": 0, "legacy": 1}


def test_reset_rewind_and_init_state_in_mid_stream(gen):
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  n = 300
  rng = np.random.default_rng(11)
  pr = Pair(lambda **kw: _k6(gen, n, per_filter=True, rewind_to_keep=4, **kw))
  off = rng.uniform(0.0, 0.005, n)
  t = 0.0

  def some_calls(count, late_at=()):
    nonlocal t
    for i in range(count):
      t += 0.01
      tt = t + off
      if i in late_at:
        tt = tt.copy()
        tt[::7] -= 0.015             # behind the previous call of those filters
      act = rng.random(n) < 0.8
      pr.call(tt, 1, rng.normal(size=(n, 3)), K6.obs_noise[1], active=act)

  some_calls(7, late_at=(5,))
  for f in (pr.a, pr.b):
    f.reset_rewind()
  assert (pr.b._ring["length"].cpu().numpy() == 0).all()      # pylint: disable=protected-access
  some_calls(6, late_at=(4,))
  x0 = np.tile(K6.initial_x, (n, 1)) + 0.1 * rng.normal(size=(n, 6))
  ft0 = rng.uniform(0.0, 0.5, n)
  ft0[::5] = np.nan
  for f in (pr.a, pr.b):
    f.init_state(x0, np.diag(K6.initial_P_diag), ft0)
  t = 1.0
  pr.same("after init_state")
  some_calls(7, late_at=(3,))
  for f in (pr.a, pr.b):
    f.init_state(x0, np.diag(K6.initial_P_diag), 2.0)      # one time for all
  t = 2.0
  some_calls(5)
  pr.check_stats()
  assert pr.b.pf_stats["fast"] >= 20 and pr.b.pf_stats["legacy"] == 3, pr.b.pf_stats
