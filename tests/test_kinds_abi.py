"""CPU test of the mixed-kind step entry points ({name}_has_step_kinds, _batch_predict_update_kinds, _batch_update_kinds,
_batch_timeline_push_kinds; include/rednose_amd_filter.h RN_DECLARE_BATCH_KINDS): every generated library exports them, the libraries
that carry the kernel say so and their k_kinds rows use no scratch memory, the others answer status 4, and bad arguments fail loudly
before anything is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NULL = None
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device
ODD = ctypes.c_void_p(0x1008)       # 8-byte but not 16-byte aligned
SYMS = ("has_step_kinds", "batch_predict_update_kinds", "batch_update_kinds", "batch_timeline_push_kinds")
WITH = ["kinematic", "kinematic6", "kinematic9", "attitude", "live", "live_maha"]
WITHOUT = ["feature", "feature36"]


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def _wide_kind_models():
  from examples import _wide_obs
  return [f"randz{n}" for n, _ in _wide_obs()]


def _random_models():
  return [n for n in _names() if re.fullmatch(r"rand(aff)?\d+(_maha)?", n)]


def _has(gen_dir, name):
  dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
  fn = getattr(dll, f"{name}_has_step_kinds")
  fn.restype = ctypes.c_int
  return fn()


def test_every_library_exports_the_four_symbols(gen_dir):
  names = _names()
  assert len(names) >= 20
  for name in names:
    dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
    with open(os.path.join(gen_dir, f"{name}.h"), encoding="utf-8") as f:
      text = f.read()
    for s in SYMS:
      assert hasattr(dll, f"{name}_{s}"), f"lib{name}.so does not export {name}_{s}"
      assert f"int {name}_{s}(" in text, f"{name}.h does not declare {name}_{s}"
      assert not s[-1].isdigit()


def test_which_libraries_carry_the_kernel(gen_dir):
  for name in WITH + _random_models():
    assert _has(gen_dir, name) == 1, f"{name}: expected the mixed-kind step kernel"
  for name in WITHOUT + _wide_kind_models():
    assert _has(gen_dir, name) == 0, f"{name}: MSCKF models and models with a wide kind ship without the mixed-kind step kernel"
  assert _wide_kind_models()


def test_kernel_rows_use_no_scratch_memory(gen_dir):
  for name in _names():
    rows = {}
    with open(os.path.join(gen_dir, f"{name}.kernels.txt"), encoding="utf-8") as f:
      for line in f:
        parts = line.split()
        if parts and parts[0].startswith("k_kinds"):
          rows[parts[0]] = dict(scratch=int(parts[3]), lds=int(parts[4]), spills=int(parts[5]))
    if _has(gen_dir, name):
      assert set(rows) == {"k_kinds<true>", "k_kinds<false>"}, (name, rows)
      for k, v in rows.items():
        assert v["scratch"] == 0 and v["spills"] == 0 and v["lds"] <= 65536, (name, k, v)
    else:
      assert not rows, (name, rows)


def test_generic_header_declares_them(gen_dir):
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_KINDS(name)" in text
  body = text[text.index("#define RN_DECLARE_BATCH_KINDS(name)"):]
  body = re.sub(r"\\\n", " ", body[:body.index("#define", 10)])
  from rednose_amd.helpers import parse_prototypes
  with open(os.path.join(REPO, "include", "kinematic6.h"), encoding="utf-8") as f:
    protos = parse_prototypes(f.read())
  for s in SYMS:
    m = re.search(r"RN_FN\(name, %s\)\((.*?)\);" % s, body, re.S)
    assert m, s
    args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
    assert len(args) == len(protos[f"kinematic6_{s}"][1]), s


def _load(gen_dir, name):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


#           x     P     Q     dt_vec dt   kinds z     R     per n  norm flags active stream
PU_OK = [FAKE, FAKE, FAKE, NULL, 0.01, FAKE, FAKE, FAKE, 0, 8, 0, NULL, NULL, NULL]
#          x     P     kinds z     R     per n  norm flags active stream
U_OK = [FAKE, FAKE, FAKE, FAKE, FAKE, 0, 8, 0, NULL, NULL, NULL]
#             t     act   ft    x     P     n  K  nmax  ring: t x P kind nobs z R ea head length  kinds z_obs R     per stream
PUSH_OK = [FAKE, FAKE, FAKE, FAKE, FAKE, 8, 4, 1] + [FAKE] * 10 + [FAKE, FAKE, FAKE, 0, NULL]


@pytest.mark.parametrize("name", ["kinematic6", "kinematic9", "live"])
def test_bad_arguments_fail_loudly(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  pu, up, push = (getattr(lib, f"{name}_{s}") for s in SYMS[1:])
  for fn, ok_args, required, n_at, z_at, r_at, per_at in ((pu, PU_OK, (0, 1, 2, 5, 6, 7), 9, 6, 7, 8), (up, U_OK, (0, 1, 2, 3, 4), 6, 3, 4, 5)):
    for i in required:                   # NULL x / P / (Q) / kinds / z / R
      args = list(ok_args)
      args[i] = NULL
      ok, why = _failed(ffi, lib, name, fn(*args))
      assert ok and why[0] == 2, (i, why)
    args = list(ok_args)
    args[n_at] = -1
    ok, why = _failed(ffi, lib, name, fn(*args))
    assert ok and why[0] == 2, why
    for i in (0, 1, z_at):               # misaligned x / P / z
      args = list(ok_args)
      args[i] = ODD
      ok, why = _failed(ffi, lib, name, fn(*args))
      assert ok and why[0] == 3, (i, why)
    args = list(ok_args)                 # R per filter must be aligned, a shared table need not be
    args[r_at], args[per_at] = ODD, 1
    ok, why = _failed(ffi, lib, name, fn(*args))
    assert ok and why[0] == 3, why
    args = list(ok_args)
    args[n_at] = 0
    assert fn(*args) == 0                # n == 0 with valid arguments is a no-op
  for i in [0, 1, 2, 3, 4] + list(range(8, 21)):      # every required pointer of the checkpoint
    args = list(PUSH_OK)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, push(*args))
    assert ok and why[0] == 2, (i, why)
  for i, bad in ((5, -1), (6, -1), (7, 0)):           # n, K, nmax
    args = list(PUSH_OK)
    args[i] = bad
    ok, why = _failed(ffi, lib, name, push(*args))
    assert ok and why[0] == 2, (i, why)
  assert push(*(PUSH_OK[:5] + [0] + PUSH_OK[6:])) == 0


@pytest.mark.parametrize("name", WITHOUT)
def test_libraries_without_the_kernel_answer_unsupported(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  for s, args in zip(SYMS[1:], (PU_OK, U_OK, PUSH_OK)):
    ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_{s}")(*args))
    assert ok and why[0] == 4, (s, why)


def test_without_a_device_they_fail_loudly(gen_dir):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  name = "kinematic6"
  ffi, lib = _load(gen_dir, name)
  for s, args in zip(SYMS[1:], (PU_OK, U_OK, PUSH_OK)):
    ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_{s}")(*args))
    assert ok and why[0] == 1, (s, why)
