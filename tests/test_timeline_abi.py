"""CPU test of the device-timeline entry points ({name}_batch_timeline_plan / _push, include/rednose_amd_filter.h RN_DECLARE_BATCH_TIMELINE):
every generated library exports them, the generic header declares them, they fail loudly -- non-zero status, last_error_string set --
on NULL required pointers and without a device, and neither they nor anything else in the generated sources stores through the scalar unit."""
import ctypes
import glob
import os
import re

import pytest

from conftest import REPO

NULL = None


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def test_every_library_exports_plan_and_push(gen_dir):
  names = _names()
  assert len(names) >= 6
  for name in names:
    dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
    for s in ("plan", "push"):
      assert hasattr(dll, f"{name}_batch_timeline_{s}"), f"lib{name}.so does not export {name}_batch_timeline_{s}"
    with open(os.path.join(gen_dir, f"{name}.h"), encoding="utf-8") as f:
      text = f.read()
    assert f"int {name}_batch_timeline_plan(" in text and f"int {name}_batch_timeline_push(" in text


def test_generic_header_declares_them():
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_TIMELINE(name)" in text
  body = text[text.index("#define RN_DECLARE_BATCH_TIMELINE(name)"):]
  body = body[:body.index("#define", 10)]
  assert "RN_FN(name, batch_timeline_plan)" in body and "RN_FN(name, batch_timeline_push)" in body
  # the macro's parameter lists are the generated header's, name by name
  from rednose_amd.helpers import parse_prototypes
  with open(os.path.join(REPO, "include", "kinematic6.h"), encoding="utf-8") as f:
    protos = parse_prototypes(f.read())
  flat = re.sub(r"\\\n", " ", body)
  for s in ("plan", "push"):
    m = re.search(r"RN_FN\(name, batch_timeline_%s\)\((.*?)\);" % s, flat, re.S)
    assert m, s
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(protos[f"kinematic6_batch_timeline_{s}"][1])


def _load(gen_dir, name="kinematic6"):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device


@pytest.mark.parametrize("name", ["kinematic6", "live", "feature"])
def test_null_required_pointers_fail_loudly(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  plan, push = getattr(lib, f"{name}_batch_timeline_plan"), getattr(lib, f"{name}_batch_timeline_push")
  kind = {"kinematic6": 1, "live": 10, "feature": 1}[name]
  plan_ok = [FAKE, NULL, FAKE, 8, FAKE, FAKE, FAKE, FAKE, NULL, NULL, 0, NULL]
  for i in (0, 2, 4, 5, 6, 7):          # t, ft, dt_out, act_out, late_out, n_late
    args = list(plan_ok)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, plan(*args))
    assert ok and why[0] == 2, (i, why)
  ok, why = _failed(ffi, lib, name, plan(*(plan_ok[:3] + [-1] + plan_ok[4:])))
  assert ok and why[0] == 2, why
  ok, why = _failed(ffi, lib, name, plan(*(plan_ok[:8] + [NULL, FAKE, 24, NULL])))      # z_keep without z_src
  assert ok and why[0] == 2, why
  #          t     act   ft    x     P     n  K  nmax ring: t x P kind nobs z R ea head length                       kind nobs z_obs + strides  R per + strides     ea + strides
  push_ok = [FAKE, FAKE, FAKE, FAKE, FAKE, 8, 4, 1] + [FAKE] * 10 + [kind, 1, FAKE, 3, 0, FAKE, 0, 9, 0, FAKE, 0, 0, NULL]
  for i in [0, 1, 2, 3, 4] + list(range(8, 18)) + [20, 23]:      # every required pointer (ea: NULL is fine for kinds without extra arguments)
    args = list(push_ok)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, push(*args))
    assert ok and why[0] == 2, (i, why)
  for i, bad in ((5, -1), (6, -1), (7, 0), (18, 12345), (19, 0), (19, 2), (21, -1)):      # n, K, nmax, unknown kind, nobs < 1, nobs > nmax, a negative stride
    args = list(push_ok)
    args[i] = bad
    ok, why = _failed(ffi, lib, name, push(*args))
    assert ok and why[0] == 2, (i, why)
  if name == "feature":                  # the feature-track kind takes extra arguments: its ea pointer is required
    args = list(push_ok)
    args[18], args[27] = 2, NULL
    ok, why = _failed(ffi, lib, name, push(*args))
    assert ok and why[0] == 2, why
  # n == 0 with valid arguments is a no-op, not an error
  assert plan(*(plan_ok[:3] + [0] + plan_ok[4:])) == 0
  assert push(*(push_ok[:5] + [0] + push_ok[6:])) == 0


def test_without_a_device_they_fail_loudly(gen_dir):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  name = "kinematic6"
  ffi, lib = _load(gen_dir, name)
  rc = getattr(lib, f"{name}_batch_timeline_plan")(FAKE, NULL, FAKE, 8, FAKE, FAKE, FAKE, FAKE, NULL, NULL, 0, NULL)
  ok, why = _failed(ffi, lib, name, rc)
  assert ok and why[0] == 1, why
  rc = getattr(lib, f"{name}_batch_timeline_push")(FAKE, FAKE, FAKE, NULL, NULL, 8, 0, 0, *([NULL] * 10), 1, 1, NULL, 0, 0, NULL, 0, 0, 0, NULL, 0, 0, NULL)
  ok, why = _failed(ffi, lib, name, rc)
  assert ok and why[0] == 1, why
  from rednose_amd.helpers import KalmanError
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  import numpy as np
  with pytest.raises(KalmanError):
    BatchedEKF(gen_dir, name, np.eye(6), np.zeros(6), np.eye(6), 6, 6, batch=8, per_filter=True, device_timeline=True)


def test_no_store_through_the_scalar_unit_in_any_source(gen_dir):
  """The timeline kernels are plain C++ with vector stores, and no generated or hand-written source names a scalar store, a scalar
  atomic or a scalar data cache write-back / discard, in code, inline assembly or a comment.  (The mnemonics are assembled here from
  pieces, so this file does not name them either.)"""
  s = "s" + "_"
  words = [s + "store", s + "buffer" + "_store", s + "scratch" + "_store", s + "atomic", s + "buffer" + "_atomic", s + "dcache" + "_wb", s + "dcache" + "_discard"]
  pat = re.compile("|".join(r"(?<![a-z])" + re.escape(w) for w in words), re.I)
  files = sorted(glob.glob(os.path.join(gen_dir, "*.hip")) + glob.glob(os.path.join(REPO, "rednose_amd", "templates", "*.h")) +
                 glob.glob(os.path.join(REPO, "rednose_amd", "codegen", "*.py")) + glob.glob(os.path.join(REPO, "tools", "*.hip")))
  assert len([f for f in files if f.endswith(".hip")]) >= len(_names()), files
  for fn in files:
    with open(fn, encoding="utf-8", errors="replace") as f:
      m = pat.search(f.read())
    assert m is None, f"{os.path.relpath(fn, REPO)} names {m.group(0)}"


def test_timeline_kernels_use_no_scratch_memory(gen_dir):
  for name in _names():
    rows = {}
    with open(os.path.join(gen_dir, f"{name}.kernels.txt"), encoding="utf-8") as f:
      for line in f:
        parts = line.split()
        if parts and parts[0].startswith("k_timeline_"):
          rows[parts[0]] = int(parts[3])
    assert set(rows) == {"k_timeline_plan", "k_timeline_push"} and not any(rows.values()), (name, rows)
