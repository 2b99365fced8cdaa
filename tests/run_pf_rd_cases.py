"""Shared by the tests of the fused run with a schedule per filter and a DIAGONAL noise per entry (batch_run_pf_rd, BatchedEKF.run_logs with
variances per entry): the entries' variances in the kernel's layout and their expansion into the full rows of batch_run_pf_r, on which
run_pf_r_cases.oracle_walk_r gives the reference.  Not a test module."""
import numpy as np


def entry_variances(rng, kd, zdim, Rs, zmax):
  """-> R (T, n, zmax) in the layout of batch_run_pf_rd.  Entry (t, i) of kind k gets s diag(R_k), s log-uniform in [0.25, 4] per entry.  NaN
  everywhere else: the rows of idle entries and of entries with an unknown kind, and the positions beyond Z of every row -- what the kernel must
  never use."""
  T, n = kd.shape
  R = np.full((T, n, zmax), np.nan)
  for k, Z in zdim.items():
    m = kd == k
    d = np.diag(np.asarray(Rs[k], dtype=np.float64).reshape(Z, Z))
    R[m, :Z] = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=int(m.sum())))[:, None] * d[None]
  return R


def expand(Rv, kd, zdim, zmax):
  """Variances (T, n, zmax) -> the rows (T, n, zmax^2) of batch_run_pf_r: row-major diag(v) in the leading Z * Z doubles of the entries of a kind,
  NaN everywhere else."""
  T, n = kd.shape
  R = np.full((T, n, zmax * zmax), np.nan)
  for k, Z in zdim.items():
    m = kd == k
    full = np.zeros((int(m.sum()), Z, Z))
    full[:, np.arange(Z), np.arange(Z)] = Rv[m, :Z]
    R[m, :Z * Z] = full.reshape(-1, Z * Z)
  return R
