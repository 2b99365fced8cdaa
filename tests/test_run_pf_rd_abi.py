"""CPU test of the fused run with a schedule per filter and a diagonal noise per entry ({name}_has_batch_run_pf_rd, {name}_batch_run_pf_rd;
include/rednose_amd_filter.h RN_DECLARE_BATCH_RUN_PF_RD): every generated library exports both symbols, the libraries that carry the kernel are
pinned and their k_run_dpf rows use neither scratch memory nor spilled registers, the others answer status 4, and bad arguments fail loudly
before anything is launched.  The twin of tests/test_run_pf_r_abi.py."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from test_run_pf_abi import SMALL, WIDE, WITHOUT as WITHOUT_PF

NULL = None
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device
ODD = ctypes.c_void_p(0x1008)       # 8-byte but not 16-byte aligned
SYMS = ("has_batch_run_pf_rd", "batch_run_pf_rd")
# every library with k_run_pf, randz10 included: a row of its 9-dimensional kind is 9 doubles where batch_run_pf_r's 81 made that kernel spill
# (the rows that decided it are in DESIGN.md section 12)
DROPPED = set()
WITH = (SMALL | WIDE) - DROPPED
WITHOUT = WITHOUT_PF | DROPPED
#         x     P     Q     kinds dts   T  z     R     n  norm flags tx    tP    stream
RUN_OK = [FAKE, FAKE, FAKE, FAKE, FAKE, 5, FAKE, FAKE, 8, 0, NULL, NULL, NULL, NULL]


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def _has(gen_dir, name):
  dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
  fn = getattr(dll, f"{name}_has_batch_run_pf_rd")
  fn.restype = ctypes.c_int
  return fn()


def test_every_library_exports_both_symbols(gen_dir):
  names = _names()
  assert len(names) >= 20
  for name in names:
    dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
    with open(os.path.join(gen_dir, f"{name}.h"), encoding="utf-8") as f:
      text = f.read()
    for s in SYMS:
      assert hasattr(dll, f"{name}_{s}"), f"lib{name}.so does not export {name}_{s}"
      assert f"int {name}_{s}(" in text, f"{name}.h does not declare {name}_{s}"


def test_which_libraries_carry_the_kernel(gen_dir):
  assert {name for name in _names() if _has(gen_dir, name) == 1} == WITH
  assert set(_names()) == WITH | WITHOUT


def test_kernel_rows_use_no_scratch_memory_and_no_spilled_registers(gen_dir):
  for name in _names():
    rows = {}
    with open(os.path.join(gen_dir, f"{name}.kernels.txt"), encoding="utf-8") as f:
      for line in f:
        parts = line.split()
        if parts and parts[0].startswith("k_run_dpf"):
          rows[parts[0]] = dict(scratch=int(parts[3]), lds=int(parts[4]), spills=int(parts[5]))
    if _has(gen_dir, name):
      assert set(rows) == ({"k_run_dpf", "k_run_dpf_tr"} if name in SMALL else {"k_run_dpf"}), (name, rows)
      for k, v in rows.items():
        assert v["scratch"] == 0 and v["spills"] == 0 and v["lds"] <= 65536, (name, k, v)
    else:
      assert not rows, (name, rows)


def test_generic_header_declares_them(gen_dir):
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_RUN_PF_RD(name)" in text
  body = text[text.index("#define RN_DECLARE_BATCH_RUN_PF_RD(name)"):]
  body = re.sub(r"\\\n", " ", body[:body.index("#define", 10)])
  from rednose_amd.helpers import parse_prototypes
  for hdr_dir in (os.path.join(REPO, "include"), gen_dir):          # the committed copy of the generated header, and the generated one
    with open(os.path.join(hdr_dir, "kinematic6.h"), encoding="utf-8") as f:
      protos = parse_prototypes(f.read())
    for s in SYMS:
      m = re.search(r"RN_FN\(name, %s\)\((.*?)\);" % s, body, re.S)
      assert m, s
      args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
      assert len(args) == len(protos[f"kinematic6_{s}"][1]), s
    assert len(protos["kinematic6_batch_run_pf_rd"][1]) == len(RUN_OK)
    assert protos["kinematic6_batch_run_pf_rd"][1] == protos["kinematic6_batch_run_pf"][1], "batch_run_pf's arguments"


def _load(gen_dir, name):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9", "live"])
def test_bad_arguments_fail_loudly(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  run = getattr(lib, f"{name}_batch_run_pf_rd")
  for i in (0, 1, 2, 3, 4, 6, 7):          # NULL x / P / Q / kinds / dts / z / R
    args = list(RUN_OK)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (5, 8):                         # T < 0, n < 0
    args = list(RUN_OK)
    args[i] = -1
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (0, 1, 6, 7, 11, 12):           # misaligned x / P / z / R (rows of variances per entry: read by the lanes) / trace_x / trace_P
    args = list(RUN_OK)
    args[i] = ODD
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 3, (i, why)
  for i in (5, 8):                         # T == 0 or n == 0 with valid arguments is a no-op
    args = list(RUN_OK)
    args[i] = 0
    assert run(*args) == 0


@pytest.mark.parametrize("name", sorted(WITHOUT))
def test_libraries_without_the_kernel_answer_unsupported(gen_dir, name):
  assert name in _names()
  ffi, lib = _load(gen_dir, name)
  ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_run_pf_rd")(*RUN_OK))
  assert ok and why[0] == 4, why


def test_without_a_device_it_fails_loudly(gen_dir):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  name = "kinematic6"
  ffi, lib = _load(gen_dir, name)
  ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_run_pf_rd")(*RUN_OK))
  assert ok and why[0] == 1, why
