"""Shared by the tests of the fused run with a schedule per filter of MSCKF models (batch_run_pf_ea, BatchedEKF.run_logs(extra_args=, augment=)):
the window shift restated in numpy, the oracle's walk through per-filter logs with landmarks and shifts, and the golden stream spread over
filters with idle entries of their own.  Not a test module."""
import numpy as np

from run_pf_cases import expected_flags_untouched

FEATURE = 2      # the feature-track kind of examples/feature_kf.py (3 extra arguments: the landmark)


def window_shift(x, P, d1, d2, d3, d4):
  """EKF_sym.augment (rednose_amd/helpers/ekf_sym.py, the reference's ekf_sym.py:365-391) on a batch: x (m, D), P (m, E, E) -> shifted copies.
  The oldest window entry drops out, the first d3 main states become the newest; P loses rows / columns [d2, d2 + d4) and gets the first d4 again."""
  x, P = x.copy(), P.copy()
  E = P.shape[-1]
  x[:, d1:-d3] = x[:, d1 + d3:].copy()
  x[:, -d3:] = x[:, :d3]
  keep = [i for i in range(E) if not d2 <= i < d2 + d4]
  src = np.array(keep + keep[:d4])
  return x, P[:, src][:, :, src]


def oracle_walk_ea(o, zdim, Rs, Q, kd, dts, x, P, zs, ea, aug, dims):
  """Every filter stepped through its own entries with OracleLib.batch_step(..., ea=) and shifted where a stepped entry has aug != 0, in place on
  x, P, zs -> (flags (T, n), trace_x, trace_P); the trace rows are the estimates BEFORE the shift."""
  T, n = kd.shape
  fl = expected_flags_untouched(kd, list(zdim))
  tx, tP = np.zeros((T,) + x.shape), np.zeros((T,) + P.shape)
  for t in range(T):
    on = np.zeros(n, dtype=bool)
    for k, Z in zdim.items():
      sel = np.nonzero(kd[t] == k)[0]
      if sel.size == 0:
        continue
      on[sel] = True
      xr, Pr, zr = x[sel].copy(), P[sel].copy(), np.ascontiguousarray(zs[t, sel, :Z])
      fr = np.zeros(sel.size, dtype=np.uint8)
      o.batch_step(k, xr, Pr, zr, np.ascontiguousarray(Rs[k], dtype=np.float64), Q, np.ascontiguousarray(dts[t, sel]), flags=fr,
                   ea=np.ascontiguousarray(ea[t, sel]) if k == FEATURE else None)
      x[sel], P[sel], zs[t, sel, :Z], fl[t, sel] = xr, Pr, zr, fr
    tx[t], tP[t] = x, P
    sh = on & (aug[t] != 0)
    if sh.any():
      x[sh], P[sh] = window_shift(x[sh], P[sh], *dims)
  return fl, tx, tP


def spread_stream(g, n, T, seed, short=None):
  """The golden stream (feature_stream.npz / feature36_stream.npz) as n logs of T rows: filter i carries the stream's entries in order with idle
  entries inserted at its own seeded positions; `short` = (filter, count): that filter's log ends after `count` entries.
  -> dict(ts, kinds, zs, eas, augment: (T, n, ...) arrays; at (T, n): the stream index of a real entry, -1 at idle ones)."""
  S = len(g["ts"])
  rng = np.random.default_rng(seed)
  at = np.full((T, n), -1, dtype=np.int64)
  for i in range(n):
    m = S if short is None or short[0] != i else short[1]
    assert m <= T
    rows = np.sort(rng.permutation(T)[:m])
    at[rows, i] = np.arange(m)
  real = at >= 0
  ix = np.where(real, at, 0)
  zmax = g["zs"].shape[1]
  out = dict(at=at,
             ts=np.where(real, g["ts"][ix], np.nan),
             kinds=np.where(real, g["kinds"][ix], 0).astype(np.int32),
             zs=np.where(real[:, :, None], g["zs"][ix], 777.0).reshape(T, n, zmax),
             eas=np.where(real[:, :, None], g["eas"][ix], np.nan),
             augment=np.where(real, g["augment"][ix] != 0, rng.uniform(size=(T, n)) < 0.5))      # set at random at idle entries: ignored there
  return out
