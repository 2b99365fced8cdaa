"""CPU test of the device rewind's entry points ({name}_batch_rewind_locate / _fetch, include/rednose_amd_filter.h RN_DECLARE_BATCH_REWIND):
every generated library exports them, the generic header declares them, they fail loudly -- non-zero status, last_error_string set -- on
NULL required pointers, bad sizes and without a device, their kernels use no scratch memory, and the numpy model the GPU test holds the
kernels to (tests/rewind_model.py) is the reference's per-filter decision: the too-old test, then bisect_right."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import rewind_model as rm

NULL = None
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def test_every_library_exports_locate_and_fetch(gen_dir):
  names = _names()
  assert len(names) >= 6
  for name in names:
    dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
    with open(os.path.join(gen_dir, f"{name}.h"), encoding="utf-8") as f:
      text = f.read()
    for s in ("locate", "fetch"):
      assert hasattr(dll, f"{name}_batch_rewind_{s}"), f"lib{name}.so does not export {name}_batch_rewind_{s}"
      assert f"int {name}_batch_rewind_{s}(" in text


def test_generic_header_declares_them():
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_REWIND(name)" in text
  body = text[text.index("#define RN_DECLARE_BATCH_REWIND(name)"):]
  body = body[:body.index("#define", 10)]
  from rednose_amd.helpers import parse_prototypes
  with open(os.path.join(REPO, "include", "kinematic6.h"), encoding="utf-8") as f:
    protos = parse_prototypes(f.read())
  flat = re.sub(r"\\\n", " ", body)
  for s, count in (("locate", 20), ("fetch", 19)):
    m = re.search(r"RN_FN\(name, batch_rewind_%s\)\((.*?)\);" % s, flat, re.S)
    assert m, s
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(protos[f"kinematic6_batch_rewind_{s}"][1]) == count


def _load(gen_dir, name="kinematic6"):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


#            late  t     n  K  ring: t x P head length             age  x     P     ft    dt    act   slot  n     drop  counts stream
LOCATE_OK = [FAKE, FAKE, 8, 4, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL]
#           slot  n     q  t_prev n  K  nmax ring: t kind z R           t_out dt    kinds act   z     z_keep R     stream
FETCH_OK = [FAKE, FAKE, 0, FAKE, 8, 4, 1, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL]


@pytest.mark.parametrize("name", ["kinematic6", "live", "feature"])
def test_bad_arguments_fail_loudly(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  locate, fetch = getattr(lib, f"{name}_batch_rewind_locate"), getattr(lib, f"{name}_batch_rewind_fetch")
  for fn, ok_args, ptrs, bad in ((locate, LOCATE_OK, [0, 1, 4, 5, 6, 7, 8] + list(range(10, 19)), ((2, -1), (3, 0), (3, -2))),
                                 (fetch, FETCH_OK, [0, 1, 3] + list(range(7, 18)), ((4, -1), (5, 0), (6, 0), (2, -1)))):
    assert all(ok_args[i] is FAKE for i in ptrs) and len(ptrs) == sum(a is FAKE for a in ok_args)      # every pointer is required
    for i in ptrs:
      args = list(ok_args)
      args[i] = NULL
      ok, why = _failed(ffi, lib, name, fn(*args))
      assert ok and why[0] == 2, (i, why)
    for i, v in bad:                    # n < 0, K < 1, nmax < 1, q < 0
      args = list(ok_args)
      args[i] = v
      ok, why = _failed(ffi, lib, name, fn(*args))
      assert ok and why[0] == 2, (i, v, why)
  # n == 0 with valid arguments is a no-op, not an error
  assert locate(*(LOCATE_OK[:2] + [0] + LOCATE_OK[3:])) == 0
  assert fetch(*(FETCH_OK[:4] + [0] + FETCH_OK[5:])) == 0


def test_without_a_device_they_fail_loudly(gen_dir):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  name = "kinematic6"
  ffi, lib = _load(gen_dir, name)
  for sym, args in (("locate", LOCATE_OK), ("fetch", FETCH_OK)):
    ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_rewind_{sym}")(*args))
    assert ok and why[0] == 1, (sym, why)
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  with pytest.raises(KalmanError):
    BatchedEKF(gen_dir, name, np.eye(6), np.zeros(6), np.eye(6), 6, 6, batch=8, per_filter=True, rewind_to_keep=4, device_rewind=True)


def test_rewind_kernels_use_no_scratch_memory(gen_dir):
  for name in _names():
    rows = {}
    with open(os.path.join(gen_dir, f"{name}.kernels.txt"), encoding="utf-8") as f:
      for line in f:
        parts = line.split()
        if parts and parts[0].startswith("k_rewind_"):
          rows[parts[0]] = int(parts[3])
    assert rows == {"k_rewind_locate": 0, "k_rewind_fetch": 0}, (name, rows)


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_numpy_model_is_the_reference_decision_per_filter(K):
  """locate_model on a few thousand random rings against bisect_right and the reference's too-old test, one filter at a time; the
  fetch model against a gather written per filter."""
  n, D, E, zmax, age = 900, 3, 2, 3, 1.0
  zdims = {1: 1, 2: 3, 5: 2}
  rng = np.random.default_rng(40 + K)
  g = rm.random_rings(rng, n, K, D, E, zmax, list(zdims) + [77], age=age)          # 77: not a kind of the table
  x, P = rng.normal(size=(n, D)), rng.normal(size=(n, E, E))
  ft, dt, act = rng.uniform(20.0, 30.0, n), np.zeros(n), np.zeros(n, dtype=np.uint8)
  x0, P0, ft0, len0 = x.copy(), P.copy(), ft.copy(), g["length"].copy()
  length = g["length"].copy()
  slot, rep_n, drop, counts = rm.locate_model(g["late"], g["t"], g["ring_t"], g["ring_x"], g["ring_P"], g["head"], length, age, x, P, ft, dt, act)
  seen = set()
  for f in range(n):
    H, L = int(g["head"][f]), int(len0[f])
    times = [g["ring_t"][(H + j) % K, f] for j in range(L)]
    assert times == sorted(times)
    if not g["late"][f]:
      same = (drop[f], rep_n[f], act[f], dt[f], ft[f], length[f]) == (0, 0, 0, 0.0, ft0[f], L)
      assert same and np.array_equal(x[f], x0[f]) and np.array_equal(P[f], P0[f]), f
      continue
    want = rm.locate_restated(g["t"][f], times, age)
    if want is None:
      seen.add("old" if L else "empty")
      assert (drop[f], rep_n[f], act[f], dt[f], ft[f], length[f]) == (1, 0, 0, 0.0, ft0[f], L) and np.array_equal(x[f], x0[f]), f
      continue
    at, todo = want
    seen.add("newest" if todo == 0 else ("replay1" if todo == 1 else "replay"))
    if g["t"][f] == times[at]:
      seen.add("equal")
    src = (H + at) % K
    assert np.array_equal(x[f], g["ring_x"][src, f]) and np.array_equal(P[f], g["ring_P"][src, f]), f
    assert (drop[f], rep_n[f], act[f], dt[f], ft[f], length[f]) == (0, todo, 1, g["t"][f] - times[at], times[at], at + 1), f
    assert slot[f] == (H + at + 1) % K
  late = g["late"] != 0
  assert counts[0] == rep_n.max() and counts[1] == drop.sum() and not drop[~late].any()
  assert {"old", "empty", "newest", "equal"} <= seen and (K < 2 or "replay1" in seen) and (K < 3 or "replay" in seen), seen
  assert (g["head"][late] + len0[late] > K).any() or K == 1, "wrapped rings among the late filters"
  # fetch: every replay position, chained through t_out like the orchestrator chains it
  t_prev = g["t"].copy()
  for q in range(int(counts[0]) + 1):
    t_out, dt_out = np.full(n, -1.0), np.full(n, -1.0)
    kinds_out, act_out = np.full(n, -1, dtype=np.int32), np.full(n, 9, dtype=np.uint8)
    z_out, z_keep, R_out = np.full((n, zmax), -2.0), np.full((n, zmax), -3.0), np.full((n, zmax * zmax), -4.0)
    rm.fetch_model(slot, rep_n, q, t_prev, g["ring_t"], g["ring_kind"], g["ring_z"], g["ring_R"], zdims, t_out, dt_out, kinds_out, act_out, z_out, z_keep, R_out)
    for f in range(n):
      if rep_n[f] <= q:
        assert (t_out[f], dt_out[f], kinds_out[f], act_out[f]) == (t_prev[f], 0.0, 0, 0) and (z_out[f] == -2.0).all() and (R_out[f] == -4.0).all(), (q, f)
        continue
      s = (int(g["head"][f]) + int(length[f]) + q) % K             # the entry behind the ones the rewind kept
      kind = int(g["ring_kind"][s, f])
      Z = zdims.get(kind, 0)
      assert (t_out[f], dt_out[f], kinds_out[f], act_out[f]) == (g["ring_t"][s, f], g["ring_t"][s, f] - t_prev[f], kind, int(Z > 0)), (q, f)
      assert np.array_equal(z_out[f], g["ring_z"][s, f, 0]) and np.array_equal(z_keep[f], z_out[f])
      assert np.array_equal(R_out[f, :Z * Z].reshape(Z, Z), g["ring_R"][s, f, 0, :Z, :Z]) and (R_out[f, Z * Z:] == -4.0).all()
    t_prev = t_out
  assert (act_out == 0).all()                # one position past the longest replay: nothing left
