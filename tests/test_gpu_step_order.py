"""The lane-per-filter step kernels (k_step_{kind}, k_stepc_{kind}) keep part of their input in flight while they compute and send x and the
residual off before the covariance is finished.  What leaves must not depend on any of that: full and ragged tiles, one and many tiles per
workgroup, with and without an `active` mask, a shared and a per-filter R, a scalar and a per-filter dt, always with flags.

  * the checkpointing step against the plain one: the same bits in x, P, y and the flags, the checkpoint holds the observations as they came
    and the filtered pair, nothing is written past it;
  * the fused step against predict + update-only (the same device functions in two launches): hipcc contracts multiplies and adds into
    FMAs per kernel, so the two agree to the last bits, not bit for bit (tests/test_gpu_parity.py::test_split_predict_then_update_equals_fused,
    whose tolerance this is); a masked-out filter comes back bit for bit as it went in, with flag 16;
  * the fused step against the CPU oracle, at the single-call tolerance of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

MODELS = ("kinematic6", "kinematic", "attitude")


@pytest.fixture(scope="module")
def env():
  import torch
  assert torch.cuda.is_available()
  from examples import ensure_generated
  return torch, ensure_generated(list(MODELS))


def model(name):
  from examples import model_class_of
  M = model_class_of(name)
  return M, int(M.initial_x.shape[0]), int(M.initial_P_diag.shape[0]), list(getattr(M, "quaternion_idxs", []))


def step_outputs(torch, gen, name, n, masked, rpf, seed=0):
  """One step of every filter of a batch through the three routes.  -> dict of device tensors."""
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  M, D, E, quat = model(name)
  f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat)
  dev, p = f.device, f._p      # pylint: disable=protected-access
  kind = sorted(f.zdims)[0]
  Z = f.zdims[kind]
  g = torch.Generator(device=dev).manual_seed(1000 * seed + n + 7 * masked + 13 * rpf)
  rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float64)      # noqa: E731
  x0 = torch.as_tensor(np.asarray(M.initial_x, dtype=np.float64), device=dev)[None] + 0.05 * rnd(n, D)
  for q in quat:
    x0[:, q:q + 4] /= x0[:, q:q + 4].norm(dim=1, keepdim=True)
  sd = torch.sqrt(torch.as_tensor(np.asarray(M.initial_P_diag, dtype=np.float64), device=dev))
  A = 0.1 * rnd(n, E, E) * sd[None, :, None]
  P0 = torch.diag(sd * sd)[None] + A @ A.transpose(1, 2)
  z0 = rnd(n, Z)
  R1 = torch.as_tensor(np.atleast_2d(np.asarray(M.obs_noise[kind], dtype=np.float64)), device=dev)
  if rpf:
    B = 0.3 * rnd(n, Z, Z) * torch.sqrt(torch.diagonal(R1))[None, :, None]
    R = (R1[None] + B @ B.transpose(1, 2)).contiguous()
  else:
    R = R1.contiguous()
  # a mask goes with a per-filter dt (filters on their own timelines); without one every filter advances by the same scalar
  act = (torch.rand((n,), generator=g, device=dev) < 0.7).to(torch.uint8) if masked else None
  dtv = (0.005 + 0.01 * torch.rand((n,), generator=g, device=dev, dtype=torch.float64)) if masked else None
  dts = 0.01
  sfx = "_masked" if masked else ""
  tail = ((p(act),) if masked else ()) + (f._stream(),)      # pylint: disable=protected-access
  per = int(rpf)
  out = dict(x0=x0, P0=P0, z0=z0, act=act, dt=dtv if masked else dts, R=R, kind=kind)

  def fresh():
    return x0.clone(), P0.clone(), z0.clone(), torch.full((n,), 99, dtype=torch.uint8, device=dev)
  call = f._call      # pylint: disable=protected-access
  x, P, z, fl = fresh()
  call(f"batch_predict_update_{kind}{sfx}", p(x), p(P), p(f.Q), p(dtv), dts, p(z), p(R), per, None, n, f.norm_quats, p(fl), *tail)
  out["fused"] = (x, P, z, fl)
  x, P, z, fl = fresh()
  call(f"batch_predict{sfx}", p(x), p(P), p(f.Q), p(dtv), dts, n, f.norm_quats, *tail)
  call(f"batch_update_{kind}{sfx}", p(x), p(P), p(z), p(R), per, None, n, f.norm_quats, p(fl), *tail)
  out["split"] = (x, P, z, fl)
  # the checkpointing step takes no mask
  x, P, z, fl = fresh()
  cx = torch.full((n + 1, D), 7.0, dtype=torch.float64, device=dev)
  cP = torch.full((n + 1, E, E), 7.0, dtype=torch.float64, device=dev)
  cz = torch.full((n + 1, Z), 7.0, dtype=torch.float64, device=dev)
  call(f"batch_predict_update_{kind}_ckpt", p(x), p(P), p(f.Q), p(dtv), dts, p(z), p(R), per, None, n, f.norm_quats, p(fl), p(cx), p(cP), p(cz), f._stream())      # pylint: disable=protected-access
  out["ckpt"] = (x, P, z, fl, cx, cP, cz)
  if masked:      # ... so its plain twin for this case is the fused step with every filter active
    x, P, z, fl = fresh()
    call(f"batch_predict_update_{kind}", p(x), p(P), p(f.Q), p(dtv), dts, p(z), p(R), per, None, n, f.norm_quats, p(fl), f._stream())      # pylint: disable=protected-access
    out["fused_all"] = (x, P, z, fl)
  else:
    out["fused_all"] = out["fused"]
  torch.cuda.synchronize()
  return out


def close(torch, a, b, rtol, floor, what, atol=0.0):
  """conftest.assert_close (|a - b| <= rtol |b| + floor x the record's largest entry + atol) on device tensors; prints the largest difference."""
  a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
  assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), what + ": non-finite"
  print(f"{what}: max |a - b| {float((a - b).abs().max()):.3e}, bit-identical {torch.equal(a, b)}")
  assert_close(a.cpu().numpy(), b.cpu().numpy(), rtol=rtol, floor=floor, what=what, atol=atol)


@pytest.mark.parametrize("rpf", [False, True], ids=["sharedR", "perfilterR"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("n", [64, 65, 1000, 65536])
@pytest.mark.parametrize("name", MODELS)
def test_step_kernels_agree(env, name, n, masked, rpf):
  torch, gen = env
  o = step_outputs(torch, gen, name, n, masked, rpf)
  what = f"{name} n {n} {'masked' if masked else 'all'} {'per-filter' if rpf else 'shared'} R"
  x0, P0, z0, act = o["x0"], o["P0"], o["z0"], o["act"]
  # checkpointing step == plain step, bit for bit
  xa, Pa, ya, fa = o["fused_all"]
  xc, Pc, yc, fc, cx, cP, cz = o["ckpt"]
  assert torch.equal(xc, xa) and torch.equal(Pc, Pa) and torch.equal(yc, ya) and torch.equal(fc, fa), what + ": checkpointing step vs plain step"
  assert torch.equal(cx[:n], xa) and torch.equal(cP[:n], Pa) and torch.equal(cz[:n], z0), what + ": checkpoint"
  assert bool((cx[n] == 7.0).all()) and bool((cP[n] == 7.0).all()) and bool((cz[n] == 7.0).all()), what + ": guard rows"
  # fused step vs predict + update-only
  xf, Pf, yf, ff = o["fused"]
  xs, Ps, ys, fs = o["split"]
  close(torch, xf, xs, 1e-13, 1e-14, what + ": fused vs split x")
  close(torch, Pf, Ps, 1e-13, 1e-14, what + ": fused vs split P")
  close(torch, yf, ys, 1e-13, 0.0, what + ": fused vs split y", atol=1e-14)
  assert torch.equal(ff, fs), what + ": flags"
  if masked:
    off = act == 0
    assert int(off.sum()) > 0 and int((~off).sum()) > 0
    assert torch.equal(xf[off], x0[off]) and torch.equal(Pf[off], P0[off]) and torch.equal(yf[off], z0[off]), what + ": masked-out filters pass through"
    assert bool((ff[off] == 16).all()) and bool((ff[~off] == 0).all()), what + ": flags of a masked call"
    # an active filter does not see its neighbours' mask
    assert torch.equal(xf[~off], xa[~off]) and torch.equal(Pf[~off], Pa[~off]) and torch.equal(yf[~off], ya[~off]), what + ": active filters"
  else:
    assert bool((ff == 0).all()), what + ": flags"


@pytest.mark.parametrize("rpf", [False, True], ids=["sharedR", "perfilterR"])
@pytest.mark.parametrize("n", [64, 65, 1000])
@pytest.mark.parametrize("name", ("kinematic6", "kinematic"))
def test_fused_step_against_oracle(env, name, n, rpf):
  """Single-call tolerance of tests/test_gpu_parity.py: rtol 1e-12, floor 1e-14 x the record's largest entry."""
  torch, gen = env
  from oracle_lib import OracleLib
  M, D, E, _ = model(name)
  o = step_outputs(torch, gen, name, n, False, rpf, seed=1)
  xr, Pr, zr = o["x0"].cpu().numpy().copy(), o["P0"].cpu().numpy().copy(), o["z0"].cpu().numpy().copy()
  R = o["R"].cpu().numpy()
  lib = OracleLib(name)
  if rpf:
    for i in range(n):
      lib.batch_step(o["kind"], xr[i:i + 1], Pr[i:i + 1], zr[i:i + 1], R[i], M.Q, 0.01)
  else:
    lib.batch_step(o["kind"], xr, Pr, zr, R, M.Q, 0.01)
  xf, Pf, yf, _ = o["fused"]
  what = f"{name} n {n} {'per-filter' if rpf else 'shared'} R vs oracle"
  close(torch, xf, torch.as_tensor(xr, device=xf.device), 1e-12, 1e-14, what + " x")
  close(torch, Pf, torch.as_tensor(Pr, device=xf.device), 1e-12, 1e-14, what + " P")
  close(torch, yf, torch.as_tensor(zr, device=xf.device), 1e-12, 1e-14, what + " y", atol=1e-14 * float(o["z0"].abs().max()))
