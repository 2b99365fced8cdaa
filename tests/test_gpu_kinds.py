"""A different observation kind per filter in one launch ({name}_batch_predict_update_kinds, BatchedEKF.predict_and_update_kinds):
against the path it replaces -- one `_masked` launch per kind on a copy of the state --, against the oracle, against the golden logs of the
reference class (tests/golden/perfilter_timelines.npz part B, one call per arrival index), and ring for ring against the per-kind calls."""
import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

LIVE_KINDS = (3, 4, 9, 10, 12, 13, 14, 19)


def _case(name):
  """-> (model class, constructor keywords, quaternion index of the oracle, kinds, {kind: R}, states(rng, n) -> x0, P0, hx {kind: (n, Z)} or None)"""
  if name == "live":
    from examples.live_kf import LiveKalman as L
    from oracle_lib import OracleLib
    g = golden("live_single_steps.npz")
    o = OracleLib("live")
    Rs = {k: np.atleast_2d(L.obs_noise.get(k, np.eye(1 if k == 3 else 3) * 0.1)) for k in LIVE_KINDS}

    def states(rng, n):
      idx = rng.integers(0, g["x_in"].shape[0], size=n)
      x0 = g["x_in"][idx] + rng.normal(size=(n, 23)) * 1e-3
      P0 = g["P_in"][idx] * rng.uniform(0.5, 2.0, size=(n, 1, 1))
      hx = {}
      for k in LIVE_KINDS:          # observations near h(x): the golden states, one evaluation per golden row
        Z = Rs[k].shape[0]
        rows = np.zeros((g["x_in"].shape[0], Z))
        for i in range(rows.shape[0]):
          out = np.zeros(Z)
          o.call(f"h_{k}", g["x_in"][i].copy(), np.zeros(1), out)
          rows[i] = out
        hx[k] = rows[idx]
      return x0, P0, hx
    return L, dict(dim=(23, 22), quat=[3]), 3, LIVE_KINDS, Rs, states
  if name == "attitude":
    from examples.attitude_kf import AttitudeKalman as AK

    def states(rng, n):
      q = rng.normal(size=(n, 4))
      q /= np.linalg.norm(q, axis=1, keepdims=True)
      x0 = np.concatenate([q, rng.normal(size=(n, 3)) * 0.5], axis=1)
      A = rng.normal(size=(n, 6, 6)) * 0.2
      return x0, np.diag(AK.initial_P_diag)[None] + A @ A.transpose(0, 2, 1), None
    return AK, dict(dim=(7, 6), quat=[0]), 0, (1, 2), {k: AK.obs_noise[k] for k in (1, 2)}, states
  if name == "kinematic9":
    from examples.kinematic9_kf import Kinematic9Kalman as M
    D = 9
  else:
    import examples.random_kf as R
    M = getattr(R, f"Random{name[4:]}Kalman")
    D = M.dim

  def states(rng, n):
    x0 = M.initial_x[None] + rng.normal(size=(n, D)) * 0.3
    A = rng.normal(size=(n, D, D)) * 0.2
    return x0, np.diag(M.initial_P_diag)[None] + A @ A.transpose(0, 2, 1), None
  return M, dict(dim=(D, D), quat=[]), -1, (1, 2, 3), {k: np.atleast_2d(M.obs_noise[k]) for k in (1, 2, 3)}, states


def _filter(gen, name, M, kw, n, **more):
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  D, E = kw["dim"]
  return BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=kw["quat"], **more)


def _inputs(name, n, seed):
  """Seeded kinds over all kinds of the model (every tile and pass mixed) with the first 64 filters uniform, a ragged last tile, per-filter
  dt, ~40 % inactive filters, one unknown kind."""
  M, kw, qi, kinds, Rs, states = _case(name)
  rng = np.random.default_rng(seed)
  x0, P0, hx = states(rng, n)
  zmax = max(R.shape[0] for R in Rs.values())
  kd = rng.choice(np.array(kinds, dtype=np.int32), size=n).astype(np.int32)
  kd[:64] = kinds[-1]
  act = rng.random(n) >= 0.4
  act[:3] = (True, False, True)
  unknown = 70
  kd[unknown], act[unknown] = 12345, True
  z = rng.normal(size=(n, zmax))
  for k in kinds:
    Z = Rs[k].shape[0]
    m = kd == k
    if hx is not None:
      z[m, :Z] = hx[k][m] + rng.normal(size=(int(m.sum()), Z)) * np.sqrt(np.diag(Rs[k]))
  dt = rng.uniform(0.0, 0.05, size=n)
  Rrow = {k: np.concatenate([Rs[k].reshape(-1), np.zeros(zmax * zmax - Rs[k].size)]) for k in kinds}
  Rtab = lambda lib_kinds: np.stack([Rrow.get(k, np.zeros(zmax * zmax)) for k in lib_kinds])      # noqa: E731  (one row per kind of the library, in its order)
  Rtab.row = Rrow
  return M, kw, qi, kinds, Rs, x0, P0, kd, act, unknown, z, dt, Rtab, zmax


def _rowmax_close(got, want, tol, what):
  got, want = np.asarray(got).reshape(len(got), -1), np.asarray(want).reshape(len(want), -1)
  scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)
  err = np.abs(got - want) / scale
  print(f"{what}: worst error {err.max():.3e} of the row maximum (bound {tol:.0e})")
  assert err.max() <= tol, f"{what}: {err.max():.3e} of the row maximum at {np.unravel_index(err.argmax(), err.shape)}"


@pytest.mark.parametrize("n", [203, 4099])
@pytest.mark.parametrize("name", ["kinematic9", "attitude", "live", "rand5", "rand11"])
@pytest.mark.parametrize("per_filter_R", [False, True])
def test_raw_abi_against_the_masked_launches_and_the_oracle(name, n, per_filter_R):
  import torch
  from examples import ensure_generated
  from oracle_lib import OracleLib
  gen = ensure_generated([name])
  M, kw, qi, kinds, Rs, x0, P0, kd, act, unknown, z, dt, Rtab, zmax = _inputs(name, n, 11 * n + len(name))
  f = _filter(gen, name, M, kw, n)
  assert f._has_step_kinds()
  dev = f.device
  t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
  rng = np.random.default_rng(5)
  if per_filter_R:          # every filter its own noise: the shared matrix of its kind, scaled
    scale = rng.uniform(0.5, 2.0, size=n)
    Rpf = np.zeros((n, zmax * zmax))
    for i, k in enumerate(kinds):
      m = kd == k
      Rpf[m] = Rtab.row[k][None] * scale[m, None]
    Rpf[unknown] = 1.0
    Rdev = t(Rpf)
  else:
    Rdev = t(Rtab(f.kinds))
  # ---- the path this replaces: one `_masked` launch per kind on a copy of the state ----
  xr, Pr, zr = t(x0), t(P0), z.copy()
  flr = np.full(n, 16, dtype=np.uint8)
  dtd = t(dt)
  for i, k in enumerate(kinds):
    Z = Rs[k].shape[0]
    m = act & (kd == k)
    zk, fk, a8 = t(z[:, :Z]), torch.zeros(n, dtype=torch.uint8, device=dev), t(m, torch.uint8)
    Rk = t(Rpf[:, :Z * Z]) if per_filter_R else t(Rs[k])
    f._call(f"batch_predict_update_{k}_masked", f._p(xr), f._p(Pr), f._p(f.Q), f._p(dtd), 0.0, f._p(zk), f._p(Rk), int(per_filter_R), None, n,
            f.norm_quats, f._p(fk), f._p(a8), f._stream())
    torch.cuda.synchronize()
    zr[m, :Z] = zk.cpu().numpy()[m]
    flr[m] = fk.cpu().numpy()[m]
  flr[unknown] = 8
  # ---- one launch, with guard rows around every output ----
  G = 4
  guard = lambda a, fill: np.concatenate([np.full((G,) + a.shape[1:], fill, a.dtype), a, np.full((G,) + a.shape[1:], fill, a.dtype)])      # noqa: E731
  xg, Pg, zg = t(guard(x0, 7.25)), t(guard(P0, 7.25)), t(guard(z, 7.25))
  fg = torch.full((n + 2 * G,), 0xAA, dtype=torch.uint8, device=dev)
  kdd, a8 = t(kd, torch.int32), t(act, torch.uint8)
  assert (G * kw["dim"][0]) % 2 == 0 and (G * zmax) % 2 == 0      # (the guarded views stay 16-byte aligned)
  xv, Pv, zv, fv = xg[G:G + n], Pg[G:G + n], zg[G:G + n], fg[G:G + n]
  f._call("batch_predict_update_kinds", f._p(xv), f._p(Pv), f._p(f.Q), f._p(dtd), 0.0, f._p(kdd), f._p(zv), f._p(Rdev), int(per_filter_R), n,
          f.norm_quats, f._p(fv), f._p(a8), f._stream())
  torch.cuda.synchronize()
  X, P, Y, FL = xv.cpu().numpy(), Pv.cpu().numpy(), zv.cpu().numpy(), fv.cpu().numpy()
  for arr, fill in ((xg, 7.25), (Pg, 7.25), (zg, 7.25), (fg, 0xAA)):
    a = arr.cpu().numpy()
    assert (a[:G] == fill).all() and (a[-G:] == fill).all(), "guard rows"
  on = act & np.isin(kd, kinds)
  assert on.sum() >= n // 2, "at most half of a batch may be untouched"
  assert np.array_equal(FL, flr), (FL[FL != flr][:8], flr[FL != flr][:8])
  assert FL[unknown] == 8 and (FL[~act] == 16).all()
  assert np.array_equal(X[~on], x0[~on]) and np.array_equal(P[~on], P0[~on]) and np.array_equal(Y[~on], z[~on]), "untouched filters, bit for bit"
  for k in kinds:             # the z columns beyond Z pass through
    Z, m = Rs[k].shape[0], kd == k
    assert np.array_equal(Y[m, Z:], z[m, Z:])
  what = f"{name} n={n} per_filter_R={per_filter_R}"
  _rowmax_close(X[on], xr.cpu().numpy()[on], 1e-13, what + " x vs masked launches")
  _rowmax_close(P[on], Pr.cpu().numpy()[on], 1e-13, what + " P vs masked launches")
  for k in kinds:
    Z, m = Rs[k].shape[0], on & (kd == k)
    if m.any():
      _rowmax_close(Y[m, :Z], zr[m, :Z], 1e-13, f"{what} y kind {k} vs masked launches")
  # ---- the oracle on a 256-filter subset (all of a small batch) ----
  o = OracleLib(name)
  sub = np.arange(min(n, 256))
  live = name == "live"
  for k in kinds:
    Z = Rs[k].shape[0]
    sel = sub[on[sub] & (kd[sub] == k)]
    if sel.size == 0:
      continue
    xo, Po, zo = x0[sel].copy(), P0[sel].copy(), np.ascontiguousarray(z[sel, :Z])
    Ro = np.ascontiguousarray(Rpf[sel, :Z * Z].reshape(-1, Z, Z)) if per_filter_R else Rs[k]
    o.batch_step(k, xo, Po, zo, Ro, M.Q, dt[sel], quat_idx=qi)
    assert_close(X[sel], xo, rtol=1e-11, floor=1e-13, what=f"{what} kind {k} x vs oracle")
    assert_close(P[sel].reshape(sel.size, -1), Po.reshape(sel.size, -1), rtol=1e-10 if live else 1e-11, floor=1e-12 if live else 1e-13, what=f"{what} kind {k} P vs oracle")
    if live:
      assert_close(Y[sel, :Z], zo, rtol=1e-9, atol=1e-9, what=f"{what} kind {k} y vs oracle")
    else:
      assert_close(Y[sel, :Z], zo, rtol=1e-11, atol=1e-13 * max(1.0, np.abs(z).max()), what=f"{what} kind {k} y vs oracle")


def test_update_only_entry_point_and_uniform_zero_dt():
  """batch_update_kinds (no predict) equals the per-kind update launches; a mixed step with the shared dt = 0 takes the models' dt = 0 shortcut."""
  import torch
  from examples import ensure_generated
  for name in ("kinematic9", "attitude"):
    gen = ensure_generated([name])
    n = 203
    M, kw, qi, kinds, Rs, x0, P0, kd, act, unknown, z, dt, Rtab, zmax = _inputs(name, n, 3)
    f = _filter(gen, name, M, kw, n)
    dev = f.device
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    xr, Pr, zr = t(x0), t(P0), z.copy()
    kdd, a8, Rt = t(kd, torch.int32), t(act, torch.uint8), t(Rtab(f.kinds))       # (held: a temporary's memory is reused by the next allocation)
    for k in kinds:
      Z, m = Rs[k].shape[0], act & (kd == k)
      zk, Rk, m8 = t(z[:, :Z]), t(Rs[k]), t(m, torch.uint8)
      f._call(f"batch_update_{k}_masked", f._p(xr), f._p(Pr), f._p(zk), f._p(Rk), 0, None, n, f.norm_quats, None, f._p(m8), f._stream())
      torch.cuda.synchronize()
      zr[m, :Z] = zk.cpu().numpy()[m]
    on = act & np.isin(kd, kinds)
    for entry in ("update", "predict_update_dt0"):
      xv, Pv, zv, fl = t(x0), t(P0), t(z), torch.zeros(n, dtype=torch.uint8, device=dev)
      if entry == "update":
        f._call("batch_update_kinds", f._p(xv), f._p(Pv), f._p(kdd), f._p(zv), f._p(Rt), 0, n, f.norm_quats, f._p(fl), f._p(a8), f._stream())
      elif name == "kinematic9":      # predict(dt = 0) is the identity for this model
        f._call("batch_predict_update_kinds", f._p(xv), f._p(Pv), f._p(f.Q), None, 0.0, f._p(kdd), f._p(zv), f._p(Rt), 0, n, f.norm_quats, f._p(fl), f._p(a8), f._stream())
      else:
        continue
      torch.cuda.synchronize()
      _rowmax_close(xv.cpu().numpy()[on], xr.cpu().numpy()[on], 1e-13, f"{name} {entry} x")
      _rowmax_close(Pv.cpu().numpy()[on], Pr.cpu().numpy()[on], 1e-13, f"{name} {entry} P")
      assert np.array_equal(xv.cpu().numpy()[~on], x0[~on]) and np.array_equal(Pv.cpu().numpy()[~on], P0[~on]) and np.array_equal(zv.cpu().numpy()[~on], z[~on])


def _k9(gen, n, **kw):
  from examples.kinematic9_kf import Kinematic9Kalman as K9
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  return K9, BatchedEKF(gen, "kinematic9", K9.Q, K9.initial_x, np.diag(K9.initial_P_diag), 9, 9, batch=n, per_filter=True, device_timeline=True, **kw)


def test_golden_logs_one_call_per_arrival_index():
  """Part B of the golden (10 reference-class logs of the 9-state model: own kind order, idle ticks, one late observation each) with ONE
  call per arrival index where the per-kind path needs one masked launch per kind present (140 for these 48 indices)."""
  from examples import ensure_generated
  gen = ensure_generated(["kinematic9"])
  g = golden("perfilter_timelines.npz")
  NB, TB = g["B_t"].shape
  K9, f = _k9(gen, NB, rewind_to_keep=64)
  assert f._has_step_kinds()
  Rs = {k: K9.obs_noise[k] for k in (1, 2, 3)}
  Zs = {k: Rs[k].shape[0] for k in Rs}
  ft = np.full(NB, -np.inf)
  late_idx, calls = 0, 0
  for j in range(TB):
    kd = g["B_kind"][:, j].astype(np.int32)
    tj = np.nan_to_num(g["B_t"][:, j])
    has = kd > 0
    late_idx += int((has & (tj < ft)).any())
    ft = np.where(has, np.maximum(ft, tj), ft)
    y = f.predict_and_update_kinds(tj, kd, g["B_z"][:, j].copy(), Rs).cpu().numpy()
    calls += 1
    fl = f.flags.cpu().numpy()
    assert np.array_equal((fl & 16) != 0, ~has) and not (fl & 32).any()
    for k in (1, 2, 3):
      m = kd == k
      if m.any():
        assert_close(y[m, :Zs[k]], g["B_y"][m, j, :Zs[k]], rtol=1e-7, atol=1e-9, what=f"arrival {j} kind {k} residuals")
    assert_close(f.state(), g["B_x"][:, j], rtol=1e-8, floor=1e-10, what=f"arrival {j} x")
    assert_close(f.covs().reshape(NB, -1), g["B_P"][:, j].reshape(NB, -1), rtol=1e-8, floor=1e-10, what=f"arrival {j} P")
  assert calls == TB
  print(f"arrival indices with a late observation: {late_idx}; calls on the device path: {f.pf_stats['fast']}, per-kind path: {f.pf_stats['legacy']}")
  assert f.pf_stats["fast"] >= TB - late_idx and f.pf_stats["fast"] + f.pf_stats["legacy"] == TB
  assert f.pf_stats["fast"] >= 40


def _drive(gen, mixed, n, T, seed=9):
  rng = np.random.default_rng(seed)
  K9, f = _k9(gen, n, rewind_to_keep=8)
  Rs = {k: K9.obs_noise[k] for k in (1, 2, 3)}
  x0 = K9.initial_x[None] + rng.normal(size=(n, 9)) * 0.1
  f.init_state(x0, np.diag(K9.initial_P_diag), np.zeros(n))
  tcur = np.zeros(n)
  log = []
  for _ in range(T):
    kd = rng.integers(0, 4, size=n).astype(np.int32)       # 0: idle
    tcur = tcur + rng.uniform(0.005, 0.02, size=n)
    z = rng.normal(size=(n, 3))
    log.append((tcur.copy(), kd, z))
    if mixed:
      f.predict_and_update_kinds(tcur, kd, z.copy(), Rs)
    else:
      for k in (1, 2, 3):
        if (kd == k).any():
          f.predict_and_update_batch(tcur, k, z[:, :Rs[k].shape[0]].copy(), Rs[k], active=kd == k)
  return K9, f, Rs, log


def test_ring_entries_are_those_of_the_per_kind_calls():
  import torch
  from examples import ensure_generated
  gen = ensure_generated(["kinematic9"])
  n, T = 130, 20
  K9, a, Rs, log = _drive(gen, True, n, T)
  _, b, _, _ = _drive(gen, False, n, T)
  assert a.pf_stats["fast"] == T and a.pf_stats["legacy"] == 0
  ra, rb = a._ring, b._ring
  for key in ("t", "kind", "nobs", "head", "length"):
    assert torch.equal(ra[key], rb[key]), key
  kind = ra["kind"].cpu().numpy()
  za, Ra, zb, Rb = ra["z"].cpu().numpy(), ra["R"].cpu().numpy(), rb["z"].cpu().numpy(), rb["R"].cpu().numpy()
  assert (kind > 0).sum() >= 8 * n // 2
  for k in (1, 2, 3):
    Z, m = Rs[k].shape[0], kind == k
    assert np.array_equal(za[m][:, 0, :Z], zb[m][:, 0, :Z]) and np.array_equal(Ra[m][:, 0, :Z, :Z], Rb[m][:, 0, :Z, :Z]), k
  filled = kind > 0
  _rowmax_close(ra["x"].cpu().numpy()[filled], rb["x"].cpu().numpy()[filled], 1e-13, "ring x")
  _rowmax_close(ra["P"].cpu().numpy()[filled], rb["P"].cpu().numpy()[filled], 1e-13, "ring P")
  # one late observation of a single kind into both: the rewind and the replay run through the entries of either ring
  ft = a.filter_times().cpu().numpy()
  t_late = ft - 0.012
  act = np.zeros(n, dtype=bool)
  act[::3] = True
  z = np.random.default_rng(1).normal(size=(n, 3))
  for f in (a, b):
    f.predict_and_update_batch(t_late, 2, z[:, :Rs[2].shape[0]].copy(), Rs[2], active=act)
    assert not (f.flags.cpu().numpy() & 32).any()
  assert_close(a.state(), b.state(), rtol=1e-9, floor=1e-11, what="states after a late observation")
  assert_close(a.covs().reshape(n, -1), b.covs().reshape(n, -1), rtol=1e-9, floor=1e-11, what="covariances after a late observation")


def test_a_library_without_the_kernel_is_served_by_the_per_kind_path():
  from examples import ensure_generated
  gen = ensure_generated(["kinematic9"])
  n = 77
  rng = np.random.default_rng(4)
  out = []
  for has in (True, False):
    K9, f = _k9(gen, n, rewind_to_keep=8)
    if not has:
      f._has_step_kinds = lambda: False
    Rs = {k: K9.obs_noise[k] for k in (1, 2, 3)}
    kd = np.random.default_rng(2).integers(0, 4, size=n).astype(np.int32)
    z = np.random.default_rng(3).normal(size=(n, 3))
    y = f.predict_and_update_kinds(np.full(n, 0.02), kd, z.copy(), Rs).cpu().numpy()
    assert f.pf_stats == ({"fast": 1, "legacy": 0} if has else {"fast": 0, "legacy": 1})
    out.append((f.state(), f.covs(), y, f.flags.cpu().numpy(), f.filter_times().cpu().numpy()))
    with pytest.raises(KeyError):
      f.predict_and_update_kinds(np.full(n, 0.03), np.full(n, 99, dtype=np.int32), z.copy(), Rs)
  (xa, Pa, ya, fa, ta), (xb, Pb, yb, fb, tb) = out
  _rowmax_close(xa, xb, 1e-13, "x, kernel vs per-kind path")
  _rowmax_close(Pa, Pb, 1e-13, "P, kernel vs per-kind path")
  assert np.abs(ya - yb).max() <= 1e-13 * np.abs(z).max() and np.array_equal(fa, fb) and np.array_equal(ta, tb, equal_nan=True)
