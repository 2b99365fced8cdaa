"""The prologue of the lane-per-filter step kernels (the first tile requested before anything else, Q by LDS-DMA with it,
the tile loop rotated) through the C ABI, every entry that launches k_step_* / k_stepc_* / k_kinds / k_predict, against the oracle:
ragged first, only and last tiles, a batch large enough that a workgroup takes a second tile, shared / per-filter R, scalar / per-filter dt,
mask and flags absent / present, dt = 0 (no Q request), Q on an address that is 8- but not 16-byte aligned, guard rows behind every array.
Tolerances: those of tests/test_gpu_parity.py for kinematic and kinematic6 (one call from identical inputs), of tests/test_gpu_random.py
for the random model."""
import ctypes
import os

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

BIG = 64 * 4096 + 64 + 5      # rn::MAX_GRID = 4096 workgroups: the first 69 filters' workgroups go round the tile loop a second time
SIZES = (1, 63, 64, 65, 64 * 8 + 1, BIG)
MODELS = ("kinematic", "kinematic6", "rand5")      # E * E = 4, 36, 25 (odd: the last Q word pair and the P tile end inside a transfer)
TOL = {"kinematic": dict(rtol=1e-12, floor=1e-14, y=1e-14), "kinematic6": dict(rtol=1e-12, floor=1e-14, y=1e-14), "rand5": dict(rtol=1e-11, floor=1e-13, y=1e-13)}
GUARD = 777.0


def _model(name):
  if name == "kinematic":
    from examples.kinematic_kf import KinematicKalman as M
    return M, 2, np.diag([0.1**2, 2.0**2]), np.eye(1) * 0.1**2
  if name == "kinematic6":
    from examples.kinematic6_kf import Kinematic6Kalman as M
    return M, 6, np.asarray(M.Q, dtype=np.float64), np.atleast_2d(M.obs_noise[1])
  from examples.random_kf import Random5Kalman as M
  return M, 5, np.asarray(M.Q, dtype=np.float64), np.atleast_2d(M.obs_noise[1])


@pytest.fixture(scope="module")
def env():
  import torch
  from examples import ensure_generated
  from oracle_lib import OracleLib
  assert torch.cuda.is_available(), "these tests need the MI355X"
  gen = ensure_generated(list(MODELS))
  return torch, {m: ctypes.CDLL(os.path.join(gen, f"lib{m}.so")) for m in MODELS}, {m: OracleLib(m) for m in MODELS}, gen


_INPUTS = {}


def _inputs(name, n):
  """Seeded inputs of a model, made once for the largest batch: a smaller batch is its first n filters."""
  if name not in _INPUTS:
    M, E, Q, R = _model(name)
    Z = R.shape[0]
    rng = np.random.default_rng(len(name))
    m = BIG
    x0 = np.asarray(getattr(M, "initial_x", np.zeros(E)), dtype=np.float64)[None] + rng.normal(size=(m, E)) * 0.3
    A = rng.normal(size=(m, E, E)) * 0.2
    P0 = np.eye(E)[None] + A @ A.transpose(0, 2, 1)
    W = rng.normal(size=(m, E, E))      # asymmetric: the step kernels use both halves of P like the reference
    P0 = P0 + 1e-3 * (W - W.transpose(0, 2, 1))
    z = rng.normal(size=(m, Z))
    B = rng.normal(size=(m, Z, Z)) * 0.05
    Rn = R[None] * rng.uniform(0.5, 2.0, size=(m, 1, 1)) + B @ B.transpose(0, 2, 1)
    dts = rng.uniform(0.0, 0.05, size=m)
    act = (rng.uniform(size=m) < 0.6).astype(np.uint8)
    act[:3] = (1, 0, 1)
    _INPUTS[name] = (x0, P0, z, Rn, dts, act, Q, R)
  return tuple(np.ascontiguousarray(a[:n]) for a in _INPUTS[name][:6]) + _INPUTS[name][6:]


class _Dev:
  """Device copies with a guard row behind each array, and the pointers the C ABI takes."""

  def __init__(self, torch):
    self.torch, self.keep = torch, []

  def arr(self, a, dtype=None, guard=GUARD, shift=0):
    torch = self.torch
    a = np.ascontiguousarray(a)
    row = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    flat = np.concatenate([np.full(shift, guard, dtype=a.dtype), a.reshape(-1), np.full(row, guard, dtype=a.dtype)])
    t = torch.as_tensor(flat, device="cuda:0")
    self.keep.append(t)
    return t[shift:shift + a.size].view(a.shape if a.size else (0,)), t[shift + a.size:]

  @staticmethod
  def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _step(torch, lib, name, n, *, per_R, per_dt, masked, with_flags, odd_Q=False, do_predict=True, ckpt=False):
  """One call of the per-kind step entry the options select -> (x, P, y, flags or None, checkpoint or None) as numpy, guards checked."""
  x0, P0, z, Rn, dts, act, Q, R = _inputs(name, n)
  d = _Dev(torch)
  x, gx = d.arr(x0)
  P, gP = d.arr(P0)
  y, gy = d.arr(z)
  Rd, _ = d.arr(Rn if per_R else R)
  Qd, _ = d.arr(Q, shift=1 if odd_Q else 2)      # (the allocation is 16-byte aligned: one double in is 8- but not 16-byte aligned)
  assert Qd.data_ptr() % 16 == (8 if odd_Q else 0)
  dv = d.arr(dts)[0] if per_dt else None
  fl, gfl = d.arr(np.full(n, 99, dtype=np.uint8), guard=99) if with_flags else (None, None)
  ac = d.arr(act, guard=1)[0] if masked else None
  c = [d.arr(np.full(a.shape, 5.0)) for a in (x0, P0, z)] if ckpt else None
  p, i64, ci = d.p, ctypes.c_int64(n), ctypes.c_int
  dt = ctypes.c_double(0.0 if per_dt else 0.0125)
  if ckpt:
    rc = getattr(lib, f"{name}_batch_predict_update_1_ckpt")(p(x), p(P), p(Qd), p(dv), dt, p(y), p(Rd), ci(per_R), None, i64, ci(0), p(fl),
                                                           p(c[0][0]), p(c[1][0]), p(c[2][0]), None)
  elif do_predict:
    rc = getattr(lib, f"{name}_batch_predict_update_1_masked")(p(x), p(P), p(Qd), p(dv), dt, p(y), p(Rd), ci(per_R), None, i64, ci(0), p(fl), p(ac), None)
  else:
    rc = getattr(lib, f"{name}_batch_update_1_masked")(p(x), p(P), p(y), p(Rd), ci(per_R), None, i64, ci(0), p(fl), p(ac), None)
  assert rc == 0
  torch.cuda.synchronize()
  for g in (gx, gP, gy):
    assert bool((g == GUARD).all()), "a store went behind the batch"
  if with_flags:
    assert bool((gfl == 99).all())
  ck = None
  if ckpt:
    for _, g in c:
      assert bool((g == GUARD).all())
    ck = tuple(t.cpu().numpy() for t, _ in c)
  return x.cpu().numpy(), P.cpu().numpy(), y.cpu().numpy(), (fl.cpu().numpy() if with_flags else None), ck


def _oracle(o, name, n, *, per_R, per_dt, do_predict=True):
  x0, P0, z, Rn, dts, act, Q, R = _inputs(name, n)
  xr, Pr, zr = x0.copy(), P0.copy(), z.copy()
  o.batch_step(1, xr, Pr, zr, Rn if per_R else R, Q, dts if per_dt else 0.0125, do_predict=do_predict)
  return xr, Pr, zr


def _check(name, got, want, on, what, inputs):
  x0, P0, z = inputs
  tol = TOL[name]
  x, P, y = got[:3]
  xr, Pr, zr = want
  n = len(x0)
  assert_close(x[on], xr[on], rtol=tol["rtol"], floor=tol["floor"], what=what + " x")
  assert_close(P[on].reshape(int(on.sum()), -1), Pr[on].reshape(int(on.sum()), -1), rtol=tol["rtol"], floor=tol["floor"], what=what + " P")
  assert_close(y[on], zr[on], rtol=tol["rtol"], atol=tol["y"] * max(1.0, np.abs(z).max()), what=what + " y")
  off = ~on
  assert np.array_equal(x[off], x0[off]) and np.array_equal(P[off], P0[off]) and np.array_equal(y[off], z[off]), what + ": a masked-out filter changed"
  if got[3] is not None:
    assert np.array_equal(got[3], np.where(on, 0, 16).astype(np.uint8)), what + " flags"
  assert n == len(x)


# the options, each against its opposite; every variant is one launch
VARIANTS = {
  "plain": dict(per_R=False, per_dt=False, masked=False, with_flags=False),
  "per-filter": dict(per_R=True, per_dt=True, masked=True, with_flags=True, odd_Q=True),
  "flags": dict(per_R=False, per_dt=True, masked=False, with_flags=True),
  "mask": dict(per_R=True, per_dt=False, masked=True, with_flags=False, odd_Q=True),
  "dt0": dict(per_R=False, per_dt=False, masked=False, with_flags=True, do_predict=False),
  "dt0 per-filter": dict(per_R=True, per_dt=False, masked=True, with_flags=False, do_predict=False),
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_step_entries_against_the_oracle(env, name, n):
  """k_step_1<true> / <false> under every option, and k_stepc_1<true>: the oracle's step, masked-out filters bit for bit, flags, guard rows;
  the checkpointing entry gives the plain step's bits and keeps the observations and the filtered pair."""
  torch, libs, oracles, _ = env
  x0, P0, z, Rn, dts, act, Q, R = _inputs(name, n)
  want = {}
  plain = None
  for vname, v in VARIANTS.items():
    if n == BIG and vname not in ("plain", "per-filter"):      # (the second trip of the loop does not depend on more than these two cover)
      continue
    key = (v["per_R"], v["per_dt"], v.get("do_predict", True))
    if key not in want:
      want[key] = _oracle(oracles[name], name, n, per_R=key[0], per_dt=key[1], do_predict=key[2])
    got = _step(torch, libs[name], name, n, **v)
    on = act != 0 if v["masked"] else np.ones(n, dtype=bool)
    _check(name, got, want[key], on, f"{name} n={n} {vname}", (x0, P0, z))
    if vname == "flags":
      plain = got
  if plain is not None:
    v = VARIANTS["flags"]
    ck = _step(torch, libs[name], name, n, ckpt=True, **v)
    for a, b in zip(ck[:4], plain[:4]):
      assert np.array_equal(a, b), f"{name} n={n}: checkpointing step vs plain step"
    assert np.array_equal(ck[4][0], ck[0]) and np.array_equal(ck[4][1], ck[1]) and np.array_equal(ck[4][2], z), f"{name} n={n}: checkpoint"


@pytest.mark.parametrize("name", MODELS)
def test_a_filter_does_not_depend_on_its_tile_or_the_loop_trip(env, name):
  """Bit for bit: the first 65 filters of the large batch (tiles 0 and 1 of workgroups that go on to a second tile) equal the same filters run
  as a batch of 65 (a full tile and a ragged one)."""
  torch, libs, _, _ = env
  for vname in ("plain", "per-filter"):
    big = _step(torch, libs[name], name, BIG, **VARIANTS[vname])
    small = _step(torch, libs[name], name, 65, **VARIANTS[vname])
    for a, b, what in zip(big[:3], small[:3], "xPy"):
      assert np.array_equal(a[:65], b), f"{name} {vname}: {what} of the first 65 filters depends on the batch"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_predict_alone_against_the_oracle(env, name, n):
  """k_predict, scalar dt unmasked and per-filter dt masked with Q on an odd double: masked-out filters bit for bit, and predict alone followed
  by the update entry against the oracle's fused step (as tests/test_gpu_parity.py::test_per_filter_R_and_dt does)."""
  torch, libs, oracles, _ = env
  lib = libs[name]
  x0, P0, z, Rn, dts, act, Q, R = _inputs(name, n)
  for per_dt, masked, odd_Q in ((False, False, False), (True, True, True)):
    d = _Dev(torch)
    x, gx = d.arr(x0)
    P, gP = d.arr(P0)
    y, gy = d.arr(z)
    Rd, _ = d.arr(R)
    Qd, _ = d.arr(Q, shift=1 if odd_Q else 2)
    dv = d.arr(dts)[0] if per_dt else None
    ac = d.arr(act, guard=1)[0] if masked else None
    p, i64, ci = d.p, ctypes.c_int64(n), ctypes.c_int
    assert getattr(lib, f"{name}_batch_predict_masked")(p(x), p(P), p(Qd), p(dv), ctypes.c_double(0.0 if per_dt else 0.0125), i64, ci(0), p(ac), None) == 0
    torch.cuda.synchronize()
    assert bool((gx == GUARD).all()) and bool((gP == GUARD).all())
    on = act != 0 if masked else np.ones(n, dtype=bool)
    xp, Pp = x.cpu().numpy(), P.cpu().numpy()
    assert np.array_equal(xp[~on], x0[~on]) and np.array_equal(Pp[~on], P0[~on]), f"{name} n={n}: predict changed a masked-out filter"
    assert getattr(lib, f"{name}_batch_update_1_masked")(p(x), p(P), p(y), p(Rd), ci(0), None, i64, ci(0), None, p(ac), None) == 0
    torch.cuda.synchronize()
    want = _oracle(oracles[name], name, n, per_R=False, per_dt=per_dt)
    _check(name, (x.cpu().numpy(), P.cpu().numpy(), y.cpu().numpy(), None), want, on, f"{name} n={n} predict alone, then update (per_dt={per_dt})", (x0, P0, z))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["kinematic6", "rand5"])
def test_kind_per_filter_entry_against_the_oracle(env, name, n):
  """k_kinds<true> / <false>: every filter its own kind (per-filter R in the fused run's layout, then the shared table), per-filter dt, a mask,
  one unknown kind (flag 8, untouched), against the oracle's step of each filter's kind."""
  torch, libs, oracles, gen = env
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  lib, o = libs[name], oracles[name]
  M, E, Q, _ = _model(name)
  assert getattr(lib, f"{name}_has_step_kinds")() == 1
  kinds = (1,) if name == "kinematic6" else (1, 2, 3)
  Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
  zmax = max(r.shape[0] for r in Rs.values())
  order = [int(k) for k in BatchedEKF(gen, name, Q, np.zeros(E), np.eye(E), E, E, batch=1).kinds]
  x0, P0, _, _, dts, act, _, _ = _inputs(name, n)
  rng = np.random.default_rng(n)
  kd = rng.choice(np.array(kinds, dtype=np.int32), size=n).astype(np.int32)
  act = act.copy()
  unknown = 4 if n > 4 else -1
  if unknown >= 0:
    kd[unknown], act[unknown] = 12345, 1
  z = rng.normal(size=(n, zmax))
  scale = rng.uniform(0.5, 2.0, size=n)
  Rpf = np.ones((n, zmax * zmax))
  for k in kinds:
    Rpf[kd == k, :Rs[k].size] = Rs[k].reshape(1, -1) * scale[kd == k, None]
  Rtab = np.zeros((len(order), zmax * zmax))
  for i, k in enumerate(order):
    if k in Rs:
      Rtab[i, :Rs[k].size] = Rs[k].reshape(-1)
  tol = TOL[name]
  for per_R, do_predict, masked in ((True, True, True), (False, True, False), (False, False, True)):
    d = _Dev(torch)
    x, gx = d.arr(x0)
    P, gP = d.arr(P0)
    y, gy = d.arr(z)
    Rd, _ = d.arr(Rpf if per_R else Rtab)
    Qd, _ = d.arr(Q, shift=1)
    dv, _ = d.arr(dts)
    kdv, _ = d.arr(kd, guard=0)
    fl, gfl = d.arr(np.full(n, 99, dtype=np.uint8), guard=99)
    ac = d.arr(act, guard=1)[0] if masked else None
    p, i64, ci = d.p, ctypes.c_int64(n), ctypes.c_int
    if do_predict:
      rc = getattr(lib, f"{name}_batch_predict_update_kinds")(p(x), p(P), p(Qd), p(dv), ctypes.c_double(0.0), p(kdv), p(y), p(Rd), ci(per_R), i64, ci(0), p(fl), p(ac), None)
    else:
      rc = getattr(lib, f"{name}_batch_update_kinds")(p(x), p(P), p(kdv), p(y), p(Rd), ci(per_R), i64, ci(0), p(fl), p(ac), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((gx == GUARD).all()) and bool((gP == GUARD).all()) and bool((gy == GUARD).all()) and bool((gfl == 99).all())
    X, Pn, Y, F = x.cpu().numpy(), P.cpu().numpy(), y.cpu().numpy(), fl.cpu().numpy()
    live = (act != 0) if masked else np.ones(n, dtype=bool)
    what = f"{name} n={n} kinds per_R={per_R} predict={do_predict}"
    want_flags = np.where(live, 0, 16).astype(np.uint8)
    if unknown >= 0:
      want_flags[unknown] = 8
    assert np.array_equal(F, want_flags), what + " flags"
    same = ~live
    if unknown >= 0:
      same[unknown] = True
    assert np.array_equal(X[same], x0[same]) and np.array_equal(Pn[same], P0[same]) and np.array_equal(Y[same], z[same]), what + ": an untouched filter changed"
    for k in kinds:
      sel = np.flatnonzero(live & (kd == k))
      if sel.size == 0:
        continue
      Z = Rs[k].shape[0]
      xo, Po, zo = x0[sel].copy(), P0[sel].copy(), np.ascontiguousarray(z[sel, :Z])
      Rk = (Rpf[sel, :Z * Z].reshape(-1, Z, Z) if per_R else Rs[k])
      o.batch_step(k, xo, Po, zo, np.ascontiguousarray(Rk), Q, dts[sel], do_predict=do_predict)
      assert_close(X[sel], xo, rtol=tol["rtol"], floor=tol["floor"], what=f"{what} kind {k} x")
      assert_close(Pn[sel].reshape(sel.size, -1), Po.reshape(sel.size, -1), rtol=tol["rtol"], floor=tol["floor"], what=f"{what} kind {k} P")
      assert_close(Y[sel, :Z], zo, rtol=tol["rtol"], atol=tol["y"] * max(1.0, np.abs(z).max()), what=f"{what} kind {k} y")
      assert np.array_equal(Y[sel, Z:], z[sel, Z:]), what + " padding columns"
