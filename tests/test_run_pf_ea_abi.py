"""CPU test of the fused run with a schedule per filter of MSCKF models ({name}_has_batch_run_pf_ea, {name}_batch_run_pf_ea;
include/rednose_amd_filter.h RN_DECLARE_BATCH_RUN_PF_EA) and of the masked window shift ({name}_batch_augment_masked): every generated library
exports the first two symbols, the libraries that carry the kernel are pinned and their k_run_epf rows use neither scratch memory nor spilled
registers, the others answer status 4, and bad arguments fail loudly before anything is launched.  Modelled on tests/test_run_pf_rd_abi.py."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NULL = None
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device
ODD = ctypes.c_void_p(0x1008)       # 8-byte but not 16-byte aligned
SYMS = ("has_batch_run_pf_ea", "batch_run_pf_ea")
# the MSCKF models.  feature36 (36 error states, one filter per wavefront) fits as well: 256 + 12 registers, no scratch memory
DROPPED = set()
WITH = {"feature", "feature36"} - DROPPED
#         x     P     Q     kinds dts   T  z     R     n  norm flags tx    tP    ea    augment stream
RUN_OK = [FAKE, FAKE, FAKE, FAKE, FAKE, 5, FAKE, FAKE, 8, 0, NULL, NULL, NULL, FAKE, FAKE, NULL]


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def _has(gen_dir, name):
  dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
  fn = getattr(dll, f"{name}_has_batch_run_pf_ea")
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
  for name in WITH:      # batch_run_pf's own answer stays 0 for MSCKF models
    fn = getattr(ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so")), f"{name}_has_batch_run_pf")
    fn.restype = ctypes.c_int
    assert fn() == 0


def test_kernel_rows_use_no_scratch_memory_and_no_spilled_registers(gen_dir):
  for name in _names():
    rows = {}
    with open(os.path.join(gen_dir, f"{name}.kernels.txt"), encoding="utf-8") as f:
      for line in f:
        parts = line.split()
        if parts and parts[0].startswith("k_run_epf"):
          rows[parts[0]] = dict(scratch=int(parts[3]), lds=int(parts[4]), spills=int(parts[5]))
    if _has(gen_dir, name):
      assert set(rows) == {"k_run_epf"}, (name, rows)
      for k, v in rows.items():
        assert v["scratch"] == 0 and v["spills"] == 0 and v["lds"] <= 65536, (name, k, v)
    else:
      assert not rows, (name, rows)


def test_masked_window_shift_is_exported_by_the_msckf_libraries_only(gen_dir):
  for name in _names():
    dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
    with open(os.path.join(gen_dir, f"{name}.h"), encoding="utf-8") as f:
      text = f.read()
    msckf = name in ("feature", "feature36")
    assert hasattr(dll, f"{name}_batch_augment_masked") == msckf == hasattr(dll, f"{name}_batch_augment"), name
    assert (f"int {name}_batch_augment_masked(double *x, double *P, const uint8_t *active, int64_t n, void *stream);" in text) == msckf, name


def test_generic_header_declares_them(gen_dir):
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_RUN_PF_EA(name)" in text
  assert "int {name}_batch_augment_masked(double *x, double *P, const uint8_t *active, int64_t n, void *stream);" in text
  body = text[text.index("#define RN_DECLARE_BATCH_RUN_PF_EA(name)"):]
  body = re.sub(r"\\\n", " ", body[:body.index("#define", 10)])
  from rednose_amd.helpers import parse_prototypes
  for hdr_dir in (os.path.join(REPO, "include"), gen_dir):          # the committed copy of the generated header, and the generated one
    with open(os.path.join(hdr_dir, "feature.h"), encoding="utf-8") as f:
      protos = parse_prototypes(f.read())
    for s in SYMS:
      m = re.search(r"RN_FN\(name, %s\)\((.*?)\);" % s, body, re.S)
      assert m, s
      args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
      assert len(args) == len(protos[f"feature_{s}"][1]), s
    assert len(protos["feature_batch_run_pf_ea"][1]) == len(RUN_OK)
    assert protos["feature_batch_run_pf_ea"][1][:13] == protos["feature_batch_run_pf"][1][:13], "batch_run_pf's arguments, then ea and augment"
    assert protos["feature_batch_run_pf_ea"][1] == protos["feature_batch_run"][1], "the argument list of batch_run (kinds and dts are (T, n) here)"
    assert len(protos["feature_batch_augment_masked"][1]) == 5
    with open(os.path.join(hdr_dir, "kinematic6.h"), encoding="utf-8") as f:
      assert "kinematic6_batch_run_pf_ea" in parse_prototypes(f.read())


def _load(gen_dir, name):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


@pytest.mark.parametrize("name", sorted(WITH))
def test_bad_arguments_fail_loudly(gen_dir, name):
  import torch
  ffi, lib = _load(gen_dir, name)
  run = getattr(lib, f"{name}_batch_run_pf_ea")
  for i in (0, 1, 2, 3, 4, 6, 7, 13):      # NULL x / P / Q / kinds / dts / z / R / ea
    args = list(RUN_OK)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (5, 8):                         # T < 0, n < 0
    args = list(RUN_OK)
    args[i] = -1
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (0, 1, 6, 11, 12):              # misaligned x / P / z / trace_x / trace_P
    args = list(RUN_OK)
    args[i] = ODD
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 3, (i, why)
  for i in (5, 8):                         # T == 0 or n == 0 with valid arguments is a no-op
    args = list(RUN_OK)
    args[i] = 0
    assert run(*args) == 0
  if not torch.cuda.is_available():        # augment may be NULL (no shifts): past the checks, the launch finds no device -- 1, not 2
    args = list(RUN_OK)
    args[14] = NULL
    ok, why = _failed(ffi, lib, name, run(*args))
    assert ok and why[0] == 1, why
    aug = getattr(lib, f"{name}_batch_augment_masked")
    ok, why = _failed(ffi, lib, name, aug(FAKE, FAKE, NULL, 4, NULL))      # active may be NULL as well
    assert ok and why[0] == 1, why
  aug = getattr(lib, f"{name}_batch_augment_masked")
  for args in ([NULL, FAKE, FAKE, 4, NULL], [FAKE, NULL, FAKE, 4, NULL], [FAKE, FAKE, FAKE, -1, NULL]):
    ok, why = _failed(ffi, lib, name, aug(*args))
    assert ok and why[0] == 2, (args, why)
  assert aug(FAKE, FAKE, FAKE, 0, NULL) == 0


def test_libraries_without_the_kernel_answer_unsupported(gen_dir):
  without = [n for n in _names() if n not in WITH]
  assert len(without) >= 18
  for name in without:
    ffi, lib = _load(gen_dir, name)
    ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_run_pf_ea")(*RUN_OK))
    assert ok and why[0] == 4, (name, why)
