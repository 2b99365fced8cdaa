"""The late observation of per-filter timelines on the device ({name}_batch_rewind_locate / _fetch, BatchedEKF(device_rewind=True)):
  1. the two kernels against the numpy model of their contract (tests/rewind_model.py), exactly, with guard rows around every output;
  2. an object with device_rewind=True against the torch bookkeeping (device_timeline=False) on the golden per-filter logs, after every
     call: bookkeeping exactly, arithmetic to what the mixed-kind kernel is granted against the per-kind kernels (tests/test_gpu_kinds.py:
     rtol 1e-9, floor 1e-11 of the row maximum -- different kernels with their own FMA contraction; the torch replay uses the per-kind ones);
  3. a ring of three entries: late by one and by two entries on a full ring (the last replay's push evicts), too old for the ring, older
     than max_rewind_age, in order and inactive filters in the same calls;
  4. what stays on the torch path on such an object: several observations per call or per ring entry, keep_estimate."""
import ctypes

import numpy as np
import pytest

from conftest import assert_close, golden
import rewind_model as rm

pytestmark = pytest.mark.gpu

SENT = -777.25          # what untouched memory holds


@pytest.fixture(scope="module")
def gen():
  import torch
  assert torch.cuda.is_available()
  from examples import ensure_generated
  return ensure_generated(["kinematic", "kinematic6", "kinematic9", "live"])


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernels' contract
# ------------------------------------------------------------------------------------------------------------------
class Guarded:
  """A device array of n rows with one guard row in front and one behind; the kernels get the address of row 1."""

  def __init__(self, host, dev):
    import torch
    host = np.ascontiguousarray(host)
    self.full = torch.as_tensor(np.concatenate([np.full_like(host[:1], 99), host, np.full_like(host[:1], 99)], axis=0), device=dev)
    self.t = self.full[1:-1]
    assert self.t.is_contiguous()

  def ptr(self):
    return ctypes.c_void_p(self.t.data_ptr())

  def check(self, want, what):
    got = self.full.cpu().numpy()
    assert (got[0] == 99).all() and (got[-1] == 99).all(), f"{what}: guard rows"
    assert np.array_equal(got[1:-1], want), what


MODELS = {"kinematic": (2, 2), "kinematic9": (9, 9), "live": (23, 22)}      # name: (D, E); kinematic9: D and E * E odd, rows at 8-byte alignment


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_locate_and_fetch_against_the_numpy_model(gen, name, n, K):
  import torch
  from rednose_amd.helpers import load_code
  ffi, lib = load_code(gen, name, backend="ctypes")
  D, E = MODELS[name]
  dims = (ctypes.c_int * 3)()
  getattr(lib, f"{name}_dims")(ctypes.cast(dims, ctypes.c_void_p))
  assert (dims[0], dims[1]) == (D, E)
  nk = getattr(lib, f"{name}_num_kinds")()
  kk = (ctypes.c_int * nk)()
  getattr(lib, f"{name}_kinds")(ctypes.cast(kk, ctypes.c_void_p))
  zd = {int(k): getattr(lib, f"{name}_kind_zdim")(int(k)) for k in kk}
  zmax, nmax, age = getattr(lib, f"{name}_zmax")(), 2, 1.0
  rng = np.random.default_rng(1000 * n + 10 * K + len(name))
  dev = torch.device("cuda:0")
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)           # noqa: E731
  p = lambda a: ctypes.c_void_p(a.data_ptr())                                   # noqa: E731
  stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
  what = f"{name} n={n} K={K}"

  def call(sym, *args):
    rc = getattr(lib, f"{name}_batch_rewind_{sym}")(*args)
    assert rc == 0, ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()

  g = rm.random_rings(rng, n, K, D, E, zmax, list(zd) + [9999], nmax=nmax, age=age)      # 9999: not a kind of the model
  h = dict(x=rng.normal(size=(n, D)), P=rng.normal(size=(n, E, E)), ft=rng.uniform(20.0, 30.0, n), dt=rng.normal(size=n), act=rng.integers(0, 2, n).astype(np.uint8),
           length=g["length"].copy())
  ring_d = {k: up(g[k]) for k in ("ring_t", "ring_x", "ring_P", "ring_kind", "ring_z", "ring_R", "head")}
  d = {k: Guarded(v, dev) for k, v in h.items()}
  d.update(slot=Guarded(np.full(n, -7, dtype=np.int32), dev), rep_n=Guarded(np.full(n, -7, dtype=np.int32), dev), drop=Guarded(np.full(n, 7, dtype=np.uint8), dev),
           counts=Guarded(np.zeros(2, dtype=np.int32), dev))
  late_d, t_d = up(g["late"]), up(g["t"])
  call("locate", p(late_d), p(t_d), n, K, p(ring_d["ring_t"]), p(ring_d["ring_x"]), p(ring_d["ring_P"]), p(ring_d["head"]), d["length"].ptr(), age,
       d["x"].ptr(), d["P"].ptr(), d["ft"].ptr(), d["dt"].ptr(), d["act"].ptr(), d["slot"].ptr(), d["rep_n"].ptr(), d["drop"].ptr(), d["counts"].ptr(), stream)
  torch.cuda.synchronize()
  slot, rep_n, drop, counts = rm.locate_model(g["late"], g["t"], g["ring_t"], g["ring_x"], g["ring_P"], g["head"], h["length"], age, h["x"], h["P"], h["ft"],
                                              h["dt"], h["act"])
  # everything of a filter that is not late comes back bit for bit: the model leaves it alone, the comparison is exact
  for k in ("x", "P", "ft", "dt", "act", "length"):
    d[k].check(h[k], f"{what}: {k}")
  late = g["late"] != 0
  got_slot = d["slot"].t.cpu().numpy()
  ok = late & (drop == 0)
  assert np.array_equal(got_slot[ok], slot[ok]) and (got_slot[~ok] == -7).all(), f"{what}: rep_slot"      # (not written where nothing is replayed)
  slot = np.where(ok, slot, -7).astype(np.int32)
  d["slot"].check(slot, f"{what}: rep_slot")
  d["rep_n"].check(rep_n, f"{what}: rep_n")
  d["drop"].check(drop, f"{what}: drop")
  d["counts"].check(counts, f"{what}: counts")
  for k in ("ring_t", "ring_x", "ring_P", "head"):
    assert np.array_equal(ring_d[k].cpu().numpy(), g[k]), f"{what}: locate wrote {k}"
  if n >= 63:
    assert drop.any() and (K == 1 or (rep_n > 0).any()) and (late & (drop == 0) & (rep_n == 0)).any() and not late.all()

  # fetch: every replay position and one past the last, chained through t_out like the orchestrator chains it
  t_prev_h, t_prev_d = g["t"], t_d
  for q in range(int(counts[0]) + 1):
    o = dict(t=np.full(n, SENT), dt=np.full(n, SENT), kinds=np.full(n, -5, dtype=np.int32), act=np.full(n, 9, dtype=np.uint8), z=np.full((n, zmax), SENT),
             z_keep=np.full((n, zmax), SENT), R=np.full((n, zmax * zmax), SENT))
    od = {k: Guarded(v, dev) for k, v in o.items()}
    call("fetch", d["slot"].ptr(), d["rep_n"].ptr(), q, p(t_prev_d), n, K, nmax, p(ring_d["ring_t"]), p(ring_d["ring_kind"]), p(ring_d["ring_z"]), p(ring_d["ring_R"]),
         od["t"].ptr(), od["dt"].ptr(), od["kinds"].ptr(), od["act"].ptr(), od["z"].ptr(), od["z_keep"].ptr(), od["R"].ptr(), stream)
    torch.cuda.synchronize()
    rm.fetch_model(slot, rep_n, q, t_prev_h, g["ring_t"], g["ring_kind"], g["ring_z"], g["ring_R"], zd, o["t"], o["dt"], o["kinds"], o["act"], o["z"], o["z_keep"], o["R"])
    for k in o:
      od[k].check(o[k], f"{what}: fetch {q} {k}")       # rows of filters without this position keep the sentinel in z / z_keep / R
    if q == int(counts[0]):
      assert (o["act"] == 0).all()
    t_prev_h, t_prev_d, keep = o["t"], od["t"].t, od      # noqa: F841  (the buffer stays alive while the next launch reads it)
  for k in ("ring_t", "ring_kind", "ring_z", "ring_R"):
    assert np.array_equal(ring_d[k].cpu().numpy(), g[k]), f"{what}: fetch wrote {k}"


# ------------------------------------------------------------------------------------------------------------------
# 2. / 3. device rewind == torch bookkeeping
# ------------------------------------------------------------------------------------------------------------------
RTOL, FLOOR = 1e-9, 1e-11       # mixed-kind kernel against the per-kind kernels (tests/test_gpu_kinds.py)


def rows_close(got, want, what):
  assert_close(got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1), rtol=RTOL, floor=FLOOR, what=what)


class Pair:
  """Two BatchedEKF objects fed identical calls: `a` with the torch bookkeeping, `b` with the device timeline and device_rewind=True."""

  def __init__(self, make):
    self.a, self.b = make(device_timeline=False), make(device_rewind=True)
    assert self.b._device_rewind and self.b._device_timeline and not self.a._device_timeline      # pylint: disable=protected-access
    self.calls = self.late_calls = 0

  def count(self, t, on):
    ft = self.a.filter_times().cpu().numpy()
    tt = np.broadcast_to(np.asarray(t, dtype=np.float64), ft.shape)
    self.late_calls += int((on & (tt < ft)).any())
    self.calls += 1

  def call(self, t, kind, z, R, active=None):
    self.count(t, np.ones(self.a.batch, dtype=bool) if active is None else np.asarray(active, dtype=bool))
    cp = lambda v: v.copy() if isinstance(v, np.ndarray) else v      # noqa: E731
    ya = self.a.predict_and_update_batch(cp(t), kind, cp(z), cp(R), active=cp(active))
    yb = self.b.predict_and_update_batch(cp(t), kind, cp(z), cp(R), active=cp(active))
    what = f"call {self.calls}"
    rows_close(yb.cpu().numpy(), ya.cpu().numpy(), f"{what}: residuals")
    self.same(what, self.a.flags.cpu().numpy())
    return yb

  def same(self, what, flags_a):
    a, b = self.a, self.b
    assert np.array_equal(flags_a, b.flags.cpu().numpy()), f"{what}: flags"
    assert np.array_equal(a.filter_times().cpu().numpy(), b.filter_times().cpu().numpy(), equal_nan=True), f"{what}: filter times"
    rows_close(b.state(), a.state(), f"{what}: x")
    rows_close(b.covs(), a.covs(), f"{what}: P")
    ra, rb = a._ring, b._ring      # pylint: disable=protected-access
    assert (ra is None) == (rb is None), what
    if ra is None:
      return
    assert ra["nmax"] == rb["nmax"] == 1
    La, Ha, Lb, Hb = (r_[k].cpu().numpy() for r_ in (ra, rb) for k in ("length", "head"))
    assert np.array_equal(La, Lb) and np.array_equal(Ha, Hb), f"{what}: ring lengths / heads"
    K = ra["t"].shape[0]
    valid = ((np.arange(K)[:, None] - Ha[None, :]) % K) < La[None, :]            # slots that hold an entry
    for key in ("t", "kind", "nobs", "z", "R"):
      assert np.array_equal(ra[key].cpu().numpy()[valid], rb[key].cpu().numpy()[valid]), f"{what}: ring {key}"
    for key in ("x", "P"):
      rows_close(rb[key].cpu().numpy()[valid], ra[key].cpu().numpy()[valid], f"{what}: ring {key}")

  def check_stats(self):
    a, b = self.a, self.b
    assert b.rewind_stats == {"device": self.late_calls, "torch": 0}, (b.rewind_stats, self.late_calls)
    assert a.rewind_stats["device"] == 0 and a.rewind_stats["torch"] >= min(self.late_calls, 1), a.rewind_stats
    assert b.pf_stats == {"fast": self.calls, "legacy": 0}, (b.pf_stats, self.calls)      # a late call served on the device is a fast call


def test_device_rewind_equals_torch_path_on_the_swapped_pair_logs(gen):
  """Part A of perfilter_timelines.npz: 411 of its 700 calls have a late filter, a ring of 512."""
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  g = golden("perfilter_timelines.npz")
  n, T = g["A_t"].shape
  pr = Pair(lambda **kw: BatchedEKF(gen, "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.eye(2), 2, 2, batch=n, rewind_to_keep=512,
                                    per_filter=True, **kw))
  R = np.array([[0.1**2]])
  keep = set(g["A_keep"].tolist())
  f = pr.b
  for j in range(T):
    pr.call(g["A_t"][:, j], 1, g["A_z"][:, j:j + 1], R)
    fl = f.flags.cpu().numpy()
    assert np.array_equal((fl & 32) != 0, g["A_none"][:, j]), f"arrival {j}: which filters ignored their observation"
    assert np.abs(f.filter_times().cpu().numpy() - g["A_ft"][:, j]).max() < 1e-12, f"arrival {j}: filter times"
    if j in keep:
      a = j // 25
      assert_close(f.state(), g["A_x"][:, a], rtol=1e-9, floor=1e-11, what=f"arrival {j} x")
      assert_close(f.covs().reshape(n, -1), g["A_P"][:, a].reshape(n, -1), rtol=1e-9, floor=1e-11, what=f"arrival {j} P")
  assert_close(f.state(), g["A_x_final"], rtol=1e-9, floor=1e-11, what="final x")
  assert_close(f.covs().reshape(n, -1), g["A_P_final"].reshape(n, -1), rtol=1e-9, floor=1e-11, what="final P")
  assert pr.late_calls == 411 and pr.calls == 700
  pr.check_stats()


def test_device_rewind_equals_torch_path_on_the_three_kind_logs(gen):
  """Part B through predict_and_update_kinds: the 9-state model, three kinds, idle ticks, one late observation per filter, a ring of 64.
  The torch object has no mixed-kind call (it needs the device timeline): it gets the per-kind calls that call stands for."""
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  g = golden("perfilter_timelines.npz")
  NB, TB = g["B_t"].shape
  pr = Pair(lambda **kw: BatchedEKF(gen, "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=NB, rewind_to_keep=64, per_filter=True, **kw))
  a, b = pr.a, pr.b
  Rs = {k: K9.obs_noise[k] for k in (1, 2, 3)}
  Zs = {k: Rs[k].shape[0] for k in Rs}
  for j in range(TB):
    kd = g["B_kind"][:, j].astype(np.int32)
    tj = np.nan_to_num(g["B_t"][:, j])
    has = kd > 0
    pr.count(tj, has)
    ya, fa = g["B_z"][:, j].copy(), np.full(NB, 16, dtype=np.uint8)
    for k in (1, 2, 3):
      m = kd == k
      if m.any():
        y = a.predict_and_update_batch(tj.copy(), k, g["B_z"][:, j, :Zs[k]].copy(), Rs[k], active=m).cpu().numpy()
        ya[m, :Zs[k]] = y[m]
        fa = np.where(m, a.flags.cpu().numpy(), fa)
    yb = b.predict_and_update_kinds(tj.copy(), kd, g["B_z"][:, j].copy(), Rs).cpu().numpy()
    rows_close(yb, ya, f"arrival {j}: residuals")
    pr.same(f"arrival {j}", fa)
    fl = b.flags.cpu().numpy()
    assert np.array_equal((fl & 16) != 0, ~has) and not (fl & 32).any()
    for k in (1, 2, 3):
      m = kd == k
      if m.any():
        assert_close(yb[m, :Zs[k]], g["B_y"][m, j, :Zs[k]], rtol=1e-7, atol=1e-9, what=f"arrival {j} kind {k} residuals")
    assert_close(b.state(), g["B_x"][:, j], rtol=1e-8, floor=1e-10, what=f"arrival {j} x")
    assert_close(b.covs().reshape(NB, -1), g["B_P"][:, j].reshape(NB, -1), rtol=1e-8, floor=1e-10, what=f"arrival {j} P")
  assert pr.late_calls >= 1
  pr.check_stats()


def _k6(gen, n, **kw):
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  return BatchedEKF(gen, "kinematic6", K6.Q, K6.initial_x, np.diag(K6.initial_P_diag), 6, 6, batch=n, **kw)


def test_small_ring_with_eviction(gen):
  """A ring of 3.  Every third call is scripted from the rings as they are: by f % 6 a filter is late by one entry, late by two entries
  (on a full ring the last replay's push evicts the oldest entry), below its oldest entry (flag 48, state untouched), inside its ring
  but more than max_rewind_age behind its newest entry (the same), in order, or inactive; the roles rotate from round to round."""
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  n, K, age = 130, 3, 0.015
  rng = np.random.default_rng(3)
  pr = Pair(lambda **kw: _k6(gen, n, per_filter=True, rewind_to_keep=K, max_rewind_age=age, **kw))
  x0 = np.tile(K6.initial_x, (n, 1)) + 0.1 * rng.normal(size=(n, 6))
  for f in (pr.a, pr.b):
    f.init_state(x0, np.diag(K6.initial_P_diag), np.zeros(n))
  seen = dict(one=0, two=0, evict=0, below=0, aged=0, order=0, idle=0)
  for rnd in range(6):
    for _ in range(3 if rnd == 0 else 2):                  # in order, a step of 0.01: a full ring spans 0.02 > max_rewind_age
      ft = pr.a.filter_times().cpu().numpy()
      pr.call(ft + 0.01, 1, rng.normal(size=(n, 3)), K6.obs_noise[1], active=rng.random(n) < 0.9)
    r = pr.a._ring      # pylint: disable=protected-access
    H, L, rt = r["head"].cpu().numpy(), r["length"].cpu().numpy(), r["t"].cpu().numpy()
    ft = pr.a.filter_times().cpu().numpy()
    x_before, ft_before = pr.b.state(), ft.copy()
    t, act, role, dropped = ft + 0.01, np.ones(n, dtype=bool), (np.arange(n) + rnd) % 6, np.zeros(n, dtype=bool)
    for f in range(n):
      T = [rt[(H[f] + j) % K, f] for j in range(L[f])]
      if L[f] == 0:                                        # (never stepped so far)
        seen["order"] += 1
        continue
      assert T == sorted(T) and T[-1] == ft[f]
      if role[f] == 0 and L[f] >= 2 and T[-1] - T[-2] > 0.008:
        t[f] = T[-2] + 0.005
        seen["one"] += 1
        seen["evict"] += int(L[f] == K)
      elif role[f] == 1 and L[f] == K and T[1] - T[0] > 0.008:
        t[f] = T[0] + 0.007                                # (within max_rewind_age of the newest entry: 0.02 - 0.007 < 0.015)
        seen["two"] += 1
      elif role[f] == 2:
        t[f] = T[0] - 0.003
        dropped[f] = True
        seen["below"] += 1
      elif role[f] == 5 and L[f] == K and T[-1] - T[0] > age + 0.003:
        t[f] = T[0] + 0.002
        dropped[f] = True
        seen["aged"] += 1
      elif role[f] == 4:
        act[f] = False
        seen["idle"] += 1
      else:
        seen["order"] += 1
    pr.call(t, 1, rng.normal(size=(n, 3)), K6.obs_noise[1], active=act)
    fl = pr.b.flags.cpu().numpy()
    assert np.array_equal(fl == 48, dropped) and np.array_equal(fl == 16, ~act), f"round {rnd}: flags"
    assert np.array_equal(pr.b.state()[dropped], x_before[dropped]) and np.array_equal(pr.b.filter_times().cpu().numpy()[dropped], ft_before[dropped])
    assert (pr.b._ring["length"].cpu().numpy()[act & (role == 0) & (L == K)] == K).all()      # pylint: disable=protected-access
  assert all(v >= 10 for v in seen.values()), seen
  assert pr.late_calls == 6
  pr.check_stats()


# ------------------------------------------------------------------------------------------------------------------
# 4. what stays on the torch path
# ------------------------------------------------------------------------------------------------------------------
def test_fallbacks_to_the_torch_path(gen):
  import torch
  from examples.kinematic6_kf import Kinematic6Kalman as K6
  n = 70
  rng = np.random.default_rng(8)
  c, d = _k6(gen, n, per_filter=True, rewind_to_keep=4, device_rewind=True), _k6(gen, n, per_filter=True, rewind_to_keep=4)
  assert c._device_rewind and not d._device_rewind and d._device_timeline      # pylint: disable=protected-access
  t = 0.0

  def both(tt, z, **kw):
    out = [f.predict_and_update_batch(tt.copy(), 1, z.copy(), K6.obs_noise[1], **kw) for f in (c, d)]
    flat = [[w for v in (o if isinstance(o, tuple) else (o,)) for w in (v if isinstance(v, list) else [v]) if isinstance(w, torch.Tensor)] for o in out]
    assert len(flat[0]) == len(flat[1]) >= 1 and all(torch.equal(u, v) for u, v in zip(*flat)), "returned tensors"
    assert np.array_equal(c.state(), d.state()) and np.array_equal(c.covs(), d.covs()) and torch.equal(c.flags, d.flags)
    assert torch.equal(c.filter_times(), d.filter_times())
    rc, rd = c._ring, d._ring      # pylint: disable=protected-access
    assert torch.equal(rc["head"], rd["head"]) and torch.equal(rc["length"], rd["length"]) and rc["nmax"] == rd["nmax"]
    H, L = rc["head"].cpu().numpy(), rc["length"].cpu().numpy()
    valid = ((np.arange(4)[:, None] - H[None, :]) % 4) < L[None, :]            # slots that hold an entry (free ones were never written)
    for key in ("t", "x", "P", "kind", "nobs", "z", "R"):
      assert np.array_equal(rc[key].cpu().numpy()[valid], rd[key].cpu().numpy()[valid]), key

  def in_order(count):
    nonlocal t
    for _ in range(count):
      t += 0.01
      both(np.full(n, t), rng.normal(size=(n, 3)))

  def late_times():
    tt = np.full(n, t + 0.01)
    tt[::3] = t - 0.015                                      # behind the last two calls of those filters
    return tt

  in_order(4)
  both(late_times(), rng.normal(size=(n, 3)), keep_estimate=True)
  assert c.rewind_stats == {"device": 0, "torch": 1}
  in_order(2)
  both(late_times(), rng.normal(size=(n, 2, 3)))                 # two observations per filter
  assert c.rewind_stats == {"device": 0, "torch": 2} and c._ring["nmax"] == 2      # pylint: disable=protected-access
  in_order(2)
  both(late_times(), rng.normal(size=(n, 3)))                    # one observation, but the ring holds entries with two
  assert c.rewind_stats == {"device": 0, "torch": 3}
  assert c.pf_stats == d.pf_stats == {"fast": 8, "legacy": 3}
  assert d.rewind_stats == {"device": 0, "torch": 3}


def test_device_rewind_is_opt_in_and_needs_its_parts(gen, monkeypatch):
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  f = _k6(gen, 8, per_filter=True, rewind_to_keep=4)
  assert f.rewind_stats == {"device": 0, "torch": 0} and f.pf_stats == {"fast": 0, "legacy": 0} and not f._device_rewind      # pylint: disable=protected-access
  with pytest.raises(KalmanError):
    _k6(gen, 8, per_filter=True, rewind_to_keep=4, device_timeline=False, device_rewind=True)
  for part in ("_has_rewind_abi", "_has_step_kinds"):      # a library generated before the entry points existed / without the mixed-kind kernel
    with monkeypatch.context() as mp:
      mp.setattr(BatchedEKF, part, lambda self: False)
      with pytest.raises(KalmanError):
        _k6(gen, 8, per_filter=True, rewind_to_keep=4, device_rewind=True)
  assert _k6(gen, 8, per_filter=True, rewind_to_keep=4, device_rewind=True)._device_rewind      # pylint: disable=protected-access
