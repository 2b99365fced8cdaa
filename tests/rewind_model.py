"""A numpy model of rn::k_rewind_locate and rn::k_rewind_fetch, written from their contract (include/rednose_amd_filter.h,
RN_DECLARE_BATCH_REWIND), plus the random rings the CPU and the GPU test put them through.  A helper module, not a test."""
from bisect import bisect_right

import numpy as np


def clamp_ring(head, length, K):
  """A ring position is never trusted as an address: 0 <= head < K, 0 <= length <= K."""
  H = np.where((head < 0) | (head >= K), 0, head)
  return H, np.clip(length, 0, K)


def locate_model(late, t, ring_t, ring_x, ring_P, head, length, max_rewind_age, x, P, ft, dt, act):
  """ring_t (K, n), ring_x (K, n, D), ring_P (K, n, E, E), head / length (n).  x, P, ft, dt, act and `length` are modified in place like the
  kernel modifies them; -> rep_slot, rep_n (int32), drop (uint8), counts (2 x int32)."""
  K, n = ring_t.shape
  rep_slot, rep_n, drop = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
  counts = np.zeros(2, dtype=np.int32)
  Hc, Lc = clamp_ring(head, length, K)
  j = np.arange(K)
  for f in np.nonzero(late)[0]:
    H, L = int(Hc[f]), int(Lc[f])
    T = ring_t[(H + j[:L]) % K, f]
    if L == 0 or t[f] < T[0] or t[f] < T[L - 1] - max_rewind_age:
      drop[f] = 1
      counts[1] += 1
      continue
    ix = max(int(np.sum(T <= t[f])), 1)
    src = (H + ix - 1) % K
    x[f], P[f] = ring_x[src, f], ring_P[src, f]
    ft[f] = T[ix - 1]
    dt[f] = t[f] - T[ix - 1]
    act[f] = 1
    rep_slot[f], rep_n[f] = (H + ix) % K, L - ix
    length[f] = ix
    counts[0] = max(counts[0], L - ix)
  return rep_slot, rep_n, drop, counts


def locate_restated(t, times, max_rewind_age):
  """One filter, the way the reference's orchestrator decides (its too-old test in front of the rewind, then bisect_right on the list of
  checkpoint times, oldest first): None = too old, else (index of the checkpoint restored, number of entries to replay)."""
  times = list(times)
  if len(times) == 0 or t < times[0] or t < times[-1] - max_rewind_age:
    return None
  ix = bisect_right(times, t)
  return ix - 1, len(times) - ix


def fetch_model(rep_slot, rep_n, q, t_prev, ring_t, ring_kind, ring_z, ring_R, zdims, t_out, dt_out, kinds_out, act_out, z_out, z_keep, R_out):
  """ring_kind (K, n), ring_z (K, n, nmax, zmax), ring_R (K, n, nmax, zmax, zmax); zdims {kind: Z}, the model's table.  The outputs --
  t_out, dt_out (n), kinds_out (n) int32, act_out (n) uint8, z_out / z_keep (n, zmax), R_out (n, zmax * zmax) -- are modified in place."""
  K, n = ring_t.shape
  for f in range(n):
    if rep_n[f] <= q or rep_slot[f] < 0:
      t_out[f], dt_out[f], kinds_out[f], act_out[f] = t_prev[f], 0.0, 0, 0
      continue
    s = (int(rep_slot[f]) + q) % K
    kind = int(ring_kind[s, f])
    Z = zdims.get(kind, 0)
    t_out[f] = ring_t[s, f]
    dt_out[f] = ring_t[s, f] - t_prev[f]
    kinds_out[f] = kind
    act_out[f] = 1 if Z > 0 else 0
    z_out[f] = ring_z[s, f, 0]
    z_keep[f] = ring_z[s, f, 0]
    R_out[f, :Z * Z] = ring_R[s, f, 0, :Z, :Z].reshape(-1)


def random_rings(rng, n, K, D, E, zmax, kinds, nmax=1, age=1.0):
  """n rings of K entries in BatchedEKF._ring_alloc's layout, and a call's t / late for them, covering what a rewind meets: every length
  from 0 to K, wrapped heads, equal times, t equal to an entry's time, t below the oldest entry, t older than `age` behind the newest
  entry, t at or above the newest.  Entry times are sorted in ring order; slots outside the ring hold noise that must not be looked at.
  -> dict(t, late, ring_t, ring_x, ring_P, ring_kind, ring_z, ring_R, head, length, case)."""
  kinds = list(kinds)
  ring_t = rng.uniform(-50.0, 50.0, (K, n))                    # what free slots hold
  ring_x, ring_P = rng.normal(size=(K, n, D)), rng.normal(size=(K, n, E, E))
  ring_kind = rng.choice(np.asarray(kinds, dtype=np.int32), size=(K, n)).astype(np.int32)
  ring_z, ring_R = rng.normal(size=(K, n, nmax, zmax)), rng.normal(size=(K, n, nmax, zmax, zmax))
  head = rng.integers(0, K, n).astype(np.int64)
  length = (np.arange(n) % (K + 1)).astype(np.int64)            # every L from 0 to K
  rng.shuffle(length)
  t, case = np.zeros(n), np.zeros(n, dtype=np.int64)
  for f in range(n):
    L, H = int(length[f]), int(head[f])
    steps = rng.uniform(0.01, 0.2, L) * (rng.random(L) > 0.3)   # zero steps: equal times
    T = 10.0 + np.cumsum(steps)
    if L > 1 and rng.random() < 0.3:
      T[0] = T[-1] - age - rng.uniform(0.0, 1.0)                # a ring that spans more than max_rewind_age
    ring_t[(H + np.arange(L)) % K, f] = T
    c = int(rng.integers(0, 6))
    case[f] = c
    if L == 0:
      t[f] = rng.uniform(0.0, 20.0)
    elif c == 0:
      t[f] = T[int(rng.integers(0, L))]                          # equal to an entry's time
    elif c == 1:
      t[f] = T[0] - rng.uniform(1e-9, 0.5)                       # below the oldest entry
    elif c == 2:
      t[f] = T[-1] - age - rng.uniform(1e-9, 0.5)                # older than max_rewind_age
    elif c == 3:
      t[f] = T[-1] + rng.uniform(0.0, 0.1) * int(rng.integers(0, 2))      # at or above the newest
    elif c == 4:
      t[f] = T[-1] - age                                         # exactly at the age limit: not too old
    else:
      t[f] = rng.uniform(T[0], T[-1]) if L > 1 else T[0]         # somewhere inside
  late = (rng.random(n) < 0.7).astype(np.uint8) * np.uint8(3)   # any non-zero byte is "late"
  return dict(t=t, late=late, ring_t=ring_t, ring_x=ring_x, ring_P=ring_P, ring_kind=ring_kind, ring_z=ring_z, ring_R=ring_R, head=head,
              length=length, case=case)
