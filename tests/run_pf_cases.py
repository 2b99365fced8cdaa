"""Shared by the tests of the fused run with a schedule per filter (batch_run_pf, BatchedEKF.run_logs): seeded per-filter schedules and
the oracle's walk through them, filter by filter.  Not a test module."""
import numpy as np

UNKNOWN = 4242      # a kind no model has


def make_schedule(rng, T, n, kinds, FT, idle=0.3):
  """-> (kinds (T, n) int32, info).  Every filter draws its kinds over all kinds of the model and sits out round(idle * T) of its T entries
  (kind 0 or -1).  Where n allows it: the first tile of FT filters carries one kind only, one filter (info["never"]) is idle throughout,
  one entry (info["unknown"] = (t, i)) has a kind the model does not have, and every kind of the model appears in the second, mixed tile."""
  kinds = [int(k) for k in kinds]
  kd = rng.choice(np.array(kinds, dtype=np.int32), size=(T, n)).astype(np.int32)
  if n > FT:
    kd[:, :FT] = kinds[-1]
    for j, k in enumerate(kinds):
      if T > 0 and FT + 2 + j < n:
        kd[j % T, FT + 2 + j] = k
  n_idle = int(round(idle * T))
  for i in range(n):
    at = rng.permutation(T)[:n_idle]
    kd[at, i] = rng.choice(np.array([0, -1], dtype=np.int32), size=n_idle)
  info = {"never": None, "unknown": None}
  if n > 1 and T > 0:
    info["never"] = n - 1
    kd[:, info["never"]] = 0
  if n > 2 and T > 0:
    info["unknown"] = (T // 2, 1 if n <= FT + 1 else FT + 1)
    kd[info["unknown"]] = UNKNOWN
  if n > FT:                               # the mixed tile keeps every kind after the idle draw
    for j, k in enumerate(kinds):
      if T > 0 and FT + 2 + j < n and FT + 2 + j != info["never"]:
        kd[j % T, FT + 2 + j] = k
  return np.ascontiguousarray(kd), info


def stepped_mask(kd, kinds):
  return np.isin(kd, np.array([int(k) for k in kinds]))


def expected_flags_untouched(kd, kinds):
  """16 at idle entries, 8 at entries whose kind the model does not have, 0 elsewhere (the stepped entries: compare those with the oracle's)."""
  return np.where(kd <= 0, 16, np.where(stepped_mask(kd, kinds), 0, 8)).astype(np.uint8)


def oracle_walk(o, zdim, Rs, Q, kd, dts, x, P, zs, quat_idx=-1, trace=False):
  """Every filter stepped through its own entries with OracleLib.batch_step (predict(dt) + update of its kind), in place on x, P, zs.
  -> (flags (T, n), trace_x, trace_P)."""
  T, n = kd.shape
  fl = expected_flags_untouched(kd, list(zdim))
  tx = np.zeros((T,) + x.shape) if trace else None
  tP = np.zeros((T,) + P.shape) if trace else None
  for t in range(T):
    for k, Z in zdim.items():
      sel = np.nonzero(kd[t] == k)[0]
      if sel.size == 0:
        continue
      xr, Pr, zr = x[sel].copy(), P[sel].copy(), np.ascontiguousarray(zs[t, sel, :Z])
      fr = np.zeros(sel.size, dtype=np.uint8)
      o.batch_step(k, xr, Pr, zr, np.ascontiguousarray(Rs[k], dtype=np.float64), Q, np.ascontiguousarray(dts[t, sel]), quat_idx=quat_idx, flags=fr)
      x[sel], P[sel], zs[t, sel, :Z], fl[t, sel] = xr, Pr, zr, fr
    if trace:
      tx[t], tP[t] = x, P
  return fl, tx, tP


def r_table(kinds_zdim, Rs, zmax):
  """(num_kinds, zmax * zmax): one row per kind in the model's order, the leading Z * Z entries are that kind's row-major R."""
  tab = np.zeros((len(kinds_zdim), zmax * zmax))
  for i, (k, Z) in enumerate(kinds_zdim):
    if k not in Rs:      # (a kind of the library the schedule does not use)
      continue
    tab[i, :Z * Z] = np.asarray(Rs[k], dtype=np.float64).reshape(-1)
  return tab
