"""Shared by the tests of the fused run with a schedule per filter and a noise matrix per entry (batch_run_pf_r, BatchedEKF.run_logs with
per-entry Rs): the entries' noise in the kernel's layout, the oracle's walk with every entry's own R, and the clearance of its gate decisions.
Beside tests/run_pf_cases.py, which holds the schedules.  Not a test module."""
import numpy as np

from run_pf_cases import expected_flags_untouched, stepped_mask


def entry_noise(rng, kd, zdim, Rs, zmax, c=0.5):
  """-> R (T, n, zmax * zmax) in the layout of batch_run_pf_r.  Entry (t, i) of kind k (Z x Z) gets s (R_k + c v v^T), v ~ N(0, diag R_k) and s
  log-uniform in [0.25, 4]: symmetric positive definite with off-diagonal entries.  NaN everywhere else: the rows of idle entries and of entries
  with an unknown kind, and the positions beyond Z * Z of every row -- what the kernel must never use."""
  T, n = kd.shape
  R = np.full((T, n, zmax * zmax), np.nan)
  for k, Z in zdim.items():
    Rk = np.asarray(Rs[k], dtype=np.float64).reshape(Z, Z)
    for t, i in zip(*np.nonzero(kd == k)):
      v = rng.normal(size=Z) * np.sqrt(np.diag(Rk))
      s = np.exp(rng.uniform(np.log(0.25), np.log(4.0)))
      R[t, i, :Z * Z] = (s * (Rk + c * np.outer(v, v))).reshape(-1)
  return R


def entry_matrix(R, t, i, Z):
  return R[t, i, :Z * Z].reshape(Z, Z)


def table_rows(kd, kinds_zdim, Rs, zmax):
  """The degenerate per-entry noise: every entry's row filled from the per-kind table (idle and unknown entries: NaN)."""
  T, n = kd.shape
  R = np.full((T, n, zmax * zmax), np.nan)
  for k, Z in kinds_zdim:
    R[kd == k, :Z * Z] = np.asarray(Rs[k], dtype=np.float64).reshape(-1)
  return R


def oracle_walk_r(o, zdim, R, Q, kd, dts, x, P, zs, quat_idx=-1, trace=False):
  """run_pf_cases.oracle_walk with every entry's own R: each filter stepped through its own entries with OracleLib.batch_step, R (n_sel, Z, Z) per
  filter, in place on x, P, zs.  -> (flags (T, n), trace_x, trace_P)."""
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
      Rr = np.ascontiguousarray(R[t, sel, :Z * Z].reshape(sel.size, Z, Z))
      assert np.isfinite(Rr).all()
      fr = np.zeros(sel.size, dtype=np.uint8)
      o.batch_step(k, xr, Pr, zr, Rr, Q, np.ascontiguousarray(dts[t, sel]), quat_idx=quat_idx, flags=fr)
      x[sel], P[sel], zs[t, sel, :Z], fl[t, sel] = xr, Pr, zr, fr
    if trace:
      tx[t], tP[t] = x, P
  return fl, tx, tP


def gates_clear(o, zdim, R, Q, kd, dts, x0, P0, zs, quat_idx=-1, margin=1e-6):
  """Are the oracle's gate decisions clear of the threshold by `margin` (relative, on the squared distance)?  P0, Q and every R scaled by one
  factor a leave every gain and so every state as they are and scale every innovation covariance by a: the squared Mahalanobis distance of
  every gate test moves by 1 / a and nothing else does.  The flags of the walks at a = 1 +- margin equal those at a = 1 exactly when no decision
  lies within the margin."""
  ref = None
  for a in (1.0, 1.0 + margin, 1.0 - margin):
    fl, _, _ = oracle_walk_r(o, zdim, a * R, a * Q, kd, dts, x0.copy(), a * P0, zs.copy(), quat_idx=quat_idx)
    if ref is None:
      ref = fl
    elif not np.array_equal(fl, ref):
      return False
  return True


__all__ = ["entry_noise", "entry_matrix", "table_rows", "oracle_walk_r", "gates_clear", "stepped_mask"]
