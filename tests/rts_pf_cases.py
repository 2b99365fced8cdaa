"""Shared by the tests of the smoother with a schedule per filter (batch_rts_pf; not a test module): a seeded builder of ragged logs and the
numpy restatement of the reference's rts_smooth (rednose/helpers/ekf_sym.py:651-690) applied filter by filter to the contract of
include/rednose_amd_filter.h RN_DECLARE_BATCH_RTS_PF."""
import numpy as np

UNKNOWN_KIND = 9999      # a kind no model has: such an entry does not step its filter (the rule of batch_run_pf)


def schedule(n, T, kset, seed=0):
  """-> dict(ts (T, n) with NaN where a filter has no entry, kinds (T, n) for the forward run (<= 0: idle), kinds_rts (T, n): the same with one
  idle entry turned into an unknown-kind entry at the time of the entry before it).  Filter i gets log i % 7:
    0 a full log on the common times            1 that log with idle entries inserted (its last entries fall off the end)
    2 a log that ends >= 2 rows early           3 one that starts >= 2 rows late        (>= 2 where T >= 4, else what fits)
    4 no entry at all                           5 the only entry is row 0               6 the only entry is mid-log
  About a third of the common time differences are exactly 0.  Row 1's is 0 and filters 1 .. 3 are arranged around it so that, for T >= 5, backward
  step k = 0 finds all four filters of the first tile at an identity step (0: dt == 0; 1: dt == 0; 2: dt == 0, behind it its last entry; 3: idle,
  its entries start later) while the steps behind it find them at different ones."""
  rng = np.random.default_rng(1000 * seed + 10 * T + n)
  kset = sorted(kset)
  dts = rng.uniform(0.005, 0.03, size=T)
  dts[rng.random(T) < 0.35] = 0.0
  if T >= 2:
    dts[1] = 0.0
  if T >= 3:
    dts[T - 1] = 0.02      # (the newest step of the full logs is a real predict)
  common = 1.0 + np.cumsum(dts)
  ckinds = rng.choice(kset, size=T).astype(np.int32)
  ts = np.full((T, n), np.nan)
  kinds = np.zeros((T, n), dtype=np.int32)
  unknown = None
  for i in range(n):
    log = i % 7
    if log == 0:
      rows = list(range(T)); src = rows
    elif log == 1:
      idle = sorted(rng.choice(np.arange(2, T), size=min(2, max(0, T - 2)), replace=False).tolist()) if T > 2 else []
      rows = [r for r in range(T) if r not in idle]; src = list(range(len(rows)))
    elif log == 2:
      rows = list(range(max(1, T - 2))); src = rows
    elif log == 3:
      rows = list(range(min(2, T - 1), T)); src = rows
    elif log == 4:
      rows = []; src = []
    elif log == 5:
      rows = [0]; src = [0]
    else:
      rows = [T // 2]; src = rows
    for r, s_ in zip(rows, src):
      ts[r, i] = common[s_] + 0.001 * (i // 7)      # (later copies of a log are shifted: no two filters need the same numbers)
      kinds[r, i] = ckinds[s_]
    if log == 1 and unknown is None and T > 2 and idle:
      unknown = (idle[0], i)
  ts_fwd = ts.copy()
  kinds_rts = kinds.copy()
  if unknown is not None:
    u, i = unknown
    kinds_rts[u, i] = UNKNOWN_KIND
    ts[u, i] = ts[max(r for r in range(u) if kinds[r, i] > 0), i]      # (an entry's time must not lie before its filter's: the time of the real entry before it)
  return dict(ts=ts, ts_fwd=ts_fwd, kinds=kinds, kinds_rts=kinds_rts, unknown=unknown)


def forward_dts(ts, kinds, t0=None):
  """The forward fill of run_logs in numpy -> dts (T, n): every entry's (kind > 0) time minus its filter's previous entry's (t0, default NaN = not
  started: dt 0, in front of the first one)."""
  T, n = kinds.shape
  prev = np.full(n, np.nan) if t0 is None else np.array(t0, dtype=np.float64)
  dts = np.zeros((T, n))
  for t in range(T):
    has = kinds[t] > 0
    d = np.where(np.isnan(prev), 0.0, ts[t] - prev)
    dts[t] = np.where(has, d, 0.0)
    prev = np.where(has, ts[t], prev)
  return dts


def restate(model, X, P, dts, act, xs, Ps, Q, norm_pred=None, x_last=None, P_last=None):
  """The contract, filter by filter, resynchronised every step on the kernel's own row k + 1 (xs, Ps) -> dict of the worst relative deviations
  (`x`: of max(1, |xk_n|_max); `P`: of the matrix maximum) and `passed`: (t, i) of the rows that must have come through bit for bit, with
  `bits`: whether they all did.

  model: f(x, dt) -> x1, F(x, dt) -> (E, E), err(x, d) -> x, inv_err(x, y) -> d (the oracle's functions); norm_pred(x) renormalises a recomputed
  predicted state as the forward pass did (None: nothing to renormalise)."""
  T, n = act.shape
  E = P.shape[-1]
  sym = lambda a: np.tril(a) + np.tril(a, -1).T      # noqa: E731  (the contract of batch_rts: lower triangles are read)
  worst = dict(x=0.0, P=0.0)
  passed, bits = [], True

  def relx(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())

  def relP(got, want):
    return np.abs(got - want).max() / np.abs(want).max()

  for i in range(n):
    steps = np.nonzero(act[:, i])[0]
    m = int(steps[-1]) if len(steps) else -1
    for t in range(m + 1, T):      # rows behind m: every row of a filter without an entry
      passed.append((t, i))
      bits = bits and np.array_equal(xs[t, i].view(np.int64), X[t, i].view(np.int64)) and np.array_equal(Ps[t, i].view(np.int64), P[t, i].view(np.int64))
    if m == 0:
      if x_last is None:
        passed.append((0, i))
        bits = bits and np.array_equal(xs[0, i].view(np.int64), X[0, i].view(np.int64)) and np.array_equal(Ps[0, i].view(np.int64), P[0, i].view(np.int64))
      else:
        worst["x"] = max(worst["x"], relx(xs[0, i], x_last[i])); worst["P"] = max(worst["P"], relP(Ps[0, i], P_last[i]))
    for k in range(m - 1, -1, -1):
      xk, Pkk = X[k, i], sym(P[k, i])
      if act[k + 1, i]:
        dt = float(dts[k + 1, i])
        x1k = model.f(xk, dt)
        if norm_pred is not None:
          x1k = norm_pred(x1k)
        Fk = model.F(xk, dt)
        P1k = Fk @ Pkk @ Fk.T + dt * Q
        Ck = np.linalg.solve(P1k, Fk @ Pkk.T).T
      else:      # no predict happened between the two rows
        x1k, P1k, Ck = xk.copy(), Pkk, np.eye(E)
      if k + 1 == m:      # the start: smoothed(m) := predicted(m)
        want_x, want_P = (x1k, P1k) if x_last is None else (x_last[i], P_last[i])
        worst["P"] = max(worst["P"], relP(Ps[m, i], want_P))
        # (the state of row m leaves renormalised where the caller asked for it: compared through the step below, which starts from the kernel's own)
        if x_last is None and norm_pred is None:
          worst["x"] = max(worst["x"], relx(xs[m, i], want_x))
      x1n = xs[k + 1, i]
      xkn = model.err(xk, Ck @ model.inv_err(x1k, x1n))
      worst["x"] = max(worst["x"], relx(xs[k, i], xkn))
      Pkn = P[k, i] + Ck @ (sym(Ps[k + 1, i]) - P1k) @ Ck.T
      worst["P"] = max(worst["P"], relP(Ps[k, i], Pkn))
  return dict(worst=worst, passed=passed, bits=bits)


class OracleModel:
  """f / F / err / inv_err of a model from its oracle library (oracle_lib.OracleLib)."""

  def __init__(self, o, D, E):
    self.o, self.D, self.E = o, D, E

  def f(self, x, dt):
    out = np.zeros(self.D)
    self.o.call("f_fun", np.ascontiguousarray(x).copy(), float(dt), out)
    return out

  def F(self, x, dt):
    out = np.zeros(self.E * self.E)
    self.o.call("F_fun", np.ascontiguousarray(x).copy(), float(dt), out)
    return out.reshape(self.E, self.E)

  def err(self, x, d):
    out = np.zeros(self.D)
    self.o.call("err_fun", np.ascontiguousarray(x).copy(), np.ascontiguousarray(d).copy(), out)
    return out

  def inv_err(self, x, y):
    out = np.zeros(self.E)
    self.o.call("inv_err_fun", np.ascontiguousarray(x).copy(), np.ascontiguousarray(y).copy(), out)
    return out
