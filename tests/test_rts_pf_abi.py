"""CPU test of the smoother with a schedule per filter ({name}_has_batch_rts_pf, {name}_batch_rts_pf; include/rednose_amd_filter.h
RN_DECLARE_BATCH_RTS_PF): every generated library exports both symbols, the libraries that carry the kernel are pinned and their kernel rows
use no scratch memory and spill nothing, the fallback no_rts_pf drops this kernel alone, the others answer status 4, and bad arguments fail
loudly before anything is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NULL = None
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced on the host: the argument checks come first, and no kernel runs without a device
ODD = ctypes.c_void_p(0x1008)       # 8-byte but not 16-byte aligned
SYMS = ("has_batch_rts_pf", "batch_rts_pf")
# rn::k_rts<RtsModel, true>: the lane-per-filter models
SMALL = {"kinematic", "kinematic6", "kinematic6_maha", "attitude", "rand3", "rand5", "randaff5"}
# k_rts4_pf (codegen/emit_rts4.py): the libraries whose batch_rts launches k_rts4 and whose k_rts4_pf met the shipping conditions
RTS4 = {"kinematic9", "rand8", "rand11", "randaff11", "rand13", "rand13_maha", "randz10"}
# rn::k_rts_group<RtsModel, true>: live and live_maha, whose k_rts4_pf spills registers (fallback no_rts4_pf, as no_rts4 hands batch_rts to
# rn::k_rts_group), and of the libraries whose batch_rts launches rn::k_rts_group, rand24 and rand32
GROUP = {"live", "live_maha", "rand24", "rand32"}
WITH = SMALL | RTS4 | GROUP
# the MSCKF models, and the three in which no per-filter smoother fits the register file (fallback no_rts_pf).  The rows that decided every
# fallback are in DESIGN.md section 12.
WITHOUT = {"feature", "feature36", "rand17", "rand40", "rand56"}
#         xf    Pf    dts   act   T  Q     n  nq xs    Ps    xl    Pl    stream
RTS_OK = [FAKE, FAKE, FAKE, FAKE, 5, FAKE, 8, 0, FAKE, FAKE, NULL, NULL, NULL]


@pytest.fixture(scope="module")
def gen_dir():
  from examples import ensure_generated
  return ensure_generated()            # every model of examples.model_table(); hipcc cross-compiles gfx950 without a GPU


def _names():
  from examples import model_table
  return sorted(model_table().keys())


def _has(gen_dir, name):
  dll = ctypes.CDLL(os.path.join(gen_dir, f"lib{name}.so"))
  fn = getattr(dll, f"{name}_has_batch_rts_pf")
  fn.restype = ctypes.c_int
  return fn()


def _rows(folder, name):
  rows = {}
  with open(os.path.join(folder, f"{name}.kernels.txt"), encoding="utf-8") as f:
    for line in f:
      parts = line.split()
      if parts and parts[0].startswith("k_"):
        rows[parts[0]] = dict(vgprs=int(parts[1]), scratch=int(parts[3]), lds=int(parts[4]), spills=int(parts[5]), occ=int(parts[6]))
  return rows


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


def test_kernel_rows_use_no_scratch_memory_and_spill_nothing(gen_dir):
  for name in _names():
    rows = {k: v for k, v in _rows(gen_dir, name).items() if k.endswith("<pf>") or k == "k_rts4_pf"}
    if _has(gen_dir, name):
      assert set(rows) == ({"k_rts<pf>"} if name in SMALL else {"k_rts4_pf"} if name in RTS4 else {"k_rts_group<pf>"}), (name, rows)
      for k, v in rows.items():
        assert v["scratch"] == 0 and v["spills"] == 0 and v["lds"] <= 65536, (name, k, v)
    else:
      assert not rows, (name, rows)


def test_kernel_rows_keep_two_wavefronts_per_simd(gen_dir):
  """The occupancy column of the per-filter rows.  k_rts4_pf keeps two wavefronts per SIMD within the 20 KB of LDS per wavefront (the budget of
  k_rts4); so does rn::k_rts_group<.., true> where it stands in for it (live: RtsModel::WAVES = 2 up to 22 error states), and so do the
  lane-per-filter kernels.  rand24 and rand32 have rn::k_rts_group's one-wavefront budget in batch_rts too."""
  for name in sorted(WITH):
    (k, v), = [(k, v) for k, v in _rows(gen_dir, name).items() if k.endswith("<pf>") or k == "k_rts4_pf"]
    if name in ("rand24", "rand32"):
      assert v["occ"] >= 1, (name, k, v)
    else:
      assert v["occ"] >= 2, (name, k, v)
      assert name in SMALL or v["lds"] <= 20480, (name, k, v)


def test_register_broadcast_kernel_passes_the_dpp_hazard_check(gen_dir):
  """rednose_amd.build.compile_filter runs dpp_hazards over every kernel whose name contains k_rts4 -- k_rts4_pf among them -- and gen_code falls
  back (no_rts4_pf) on any finding: a shipped k_rts4_pf has none."""
  from rednose_amd import build as rn_build
  for name in ("kinematic9", "rand13"):      # odd and even records
    dis = rn_build.disassemble(os.path.join(gen_dir, f"lib{name}.so"))
    if dis is None:
      pytest.skip("no LLVM tools")
    assert "k_rts4_pf" in dis
    assert rn_build.dpp_hazards(dis, kernel="9k_rts4_pfE") == [], name


def test_fallback_of_the_register_broadcast_kernel_is_the_lane_group_smoother():
  """emit(fallbacks=("no_rts4_pf",)): batch_rts_pf launches rn::k_rts_group<RtsModel, true>, k_rts4_pf is gone, k_rts4 and batch_rts stay."""
  import sys
  sys.path.insert(0, os.path.join(REPO, "tools"))
  from emit_digest import example_spec, without
  from rednose_amd.codegen import emit
  spec = example_spec("kinematic9")
  hdr0, src0 = emit.emit(spec)
  hdr1, src1 = emit.emit(spec, fallbacks=("no_rts4_pf",))
  assert hdr0 == hdr1 and "int kinematic9_has_batch_rts_pf(void) { return 1; }" in src1
  assert "void k_rts4_pf(" in src0 and "k_rts4_pf" not in src1 and "rn::k_rts_group<RtsModel, true>" in src1 and "void k_rts4(" in src1
  assert without("kinematic9", hdr0, src0, SYMS + ("k_rts4_pf",)) == without("kinematic9", hdr1, src1, SYMS)


@pytest.mark.parametrize("name", ["kinematic6", "kinematic9"])
def test_fallback_drops_this_kernel_alone(tmp_path, name):
  """emit(fallbacks=("no_rts_pf",)): has_batch_rts_pf answers 0, batch_rts_pf is the unsupported stub, the per-filter launch is gone -- and every
  other line of the library's text is the default build's."""
  import sys
  sys.path.insert(0, os.path.join(REPO, "tools"))
  from emit_digest import example_spec
  from rednose_amd.codegen import emit
  spec = example_spec(name)
  assert "no_rts_pf" in emit.FALLBACKS
  hdr0, src0 = emit.emit(spec)
  hdr1, src1 = emit.emit(spec, fallbacks=("no_rts_pf",))
  assert hdr0 == hdr1
  assert f"int {name}_has_batch_rts_pf(void) {{ return 1; }}" in src0 and f"int {name}_has_batch_rts_pf(void) {{ return 0; }}" in src1
  launch = "hipLaunchKernelGGL(k_rts4_pf," if name == "kinematic9" else "<RtsModel, true>"
  assert launch in src0 and launch not in src1
  assert ("void k_rts4_pf(" in src0) == (name == "kinematic9") and "void k_rts4_pf(" not in src1

  # the library's text minus the two functions of this ABI block, taken out as tools/emit_digest.py --without takes them out for the digest
  # record (profiles/emit_digests_rts_pf.txt): exactly two prototypes and two definitions go, one of each form _Abi.fn prints
  from emit_digest import without
  h0, s0 = without(name, hdr0, src0, SYMS + ("k_rts4_pf",))
  h1, s1 = without(name, hdr1, src1, SYMS + ("k_rts4_pf",))
  assert "k_rts4_pf" not in s0 and ("void k_rts4(" in s0) == (name == "kinematic9")
  assert s0 == s1 and h0 == h1 and "batch_rts_pf" not in s0 and "batch_rts_pf" not in h0
  assert hdr0.count("\n") - h0.count("\n") == 2
  gone = [ln for ln in src0.split("\n") if ln not in set(s0.split("\n"))]
  assert any(ln.startswith(f"int {name}_has_batch_rts_pf(void)") for ln in gone) and any(ln.startswith(f"int {name}_batch_rts_pf(") for ln in gone), gone[:3]
  assert f"int {name}_batch_rts(" in s0 and f"int {name}_batch_run_pf(" in s0 and s0.count("{") == s0.count("}")
  # a stub (the braces on lines of their own around one statement) goes whole as well
  stub = without(name, hdr1, src1, ("batch_rts_pf",))[1]
  assert "batch_rts_pf: not generated" not in stub and f"{name}_has_batch_rts_pf" in stub
  assert emit.rts_pf(spec, ()) and not emit.rts_pf(spec, ("no_rts_pf",)) and not emit.rts_pf(spec, ("no_rts",))


def test_generic_header_declares_them(gen_dir):
  with open(os.path.join(REPO, "include", "rednose_amd_filter.h"), encoding="utf-8") as f:
    text = f.read()
  assert "#define RN_DECLARE_BATCH_RTS_PF(name)" in text
  body = text[text.index("#define RN_DECLARE_BATCH_RTS_PF(name)"):]
  body = re.sub(r"\\\n", " ", body[:body.index("#define", 10)])
  from rednose_amd.helpers import parse_prototypes
  for hdr in ("kinematic", "kinematic6", "kinematic9", "live", "feature"):      # the committed per-model headers
    with open(os.path.join(REPO, "include", f"{hdr}.h"), encoding="utf-8") as f:
      protos = parse_prototypes(f.read())
    for s in SYMS:
      m = re.search(r"RN_FN\(name, %s\)\((.*?)\);" % s, body, re.S)
      assert m, s
      args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
      assert len(args) == len(protos[f"{hdr}_{s}"][1]), (hdr, s)
    assert len(protos[f"{hdr}_batch_rts_pf"][1]) == len(RTS_OK)


def _load(gen_dir, name):
  from rednose_amd.helpers import load_code
  return load_code(gen_dir, name, backend="ctypes")


def _failed(ffi, lib, name, rc):
  msg = ffi.string(getattr(lib, f"{name}_last_error_string")()).decode()
  code = getattr(lib, f"{name}_last_error")()
  getattr(lib, f"{name}_clear_error")()
  return rc != 0 and code == rc and len(msg) > 0, (rc, code, msg)


@pytest.mark.parametrize("name", ["kinematic6", "attitude", "kinematic9", "live", "rand24"])
def test_bad_arguments_fail_loudly(gen_dir, name):
  ffi, lib = _load(gen_dir, name)
  rts = getattr(lib, f"{name}_batch_rts_pf")
  for i in (0, 1, 2, 3, 5, 8, 9):          # NULL xf / Pf / dts / act / Q / xs / Ps
    args = list(RTS_OK)
    args[i] = NULL
    ok, why = _failed(ffi, lib, name, rts(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (4, 6):                         # T < 0, n < 0
    args = list(RTS_OK)
    args[i] = -1
    ok, why = _failed(ffi, lib, name, rts(*args))
    assert ok and why[0] == 2, (i, why)
  for i in (0, 1, 8, 9, 10, 11):           # misaligned xf / Pf / xs / Ps / x_last / P_last
    args = list(RTS_OK)
    args[i] = ODD
    ok, why = _failed(ffi, lib, name, rts(*args))
    assert ok and why[0] == 3, (i, why)
  for i in (4, 6):                         # T == 0 or n == 0 with valid arguments is a no-op
    args = list(RTS_OK)
    args[i] = 0
    assert rts(*args) == 0


@pytest.mark.parametrize("name", sorted(WITHOUT))
def test_libraries_without_the_kernel_answer_unsupported(gen_dir, name):
  assert name in _names()
  ffi, lib = _load(gen_dir, name)
  ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_rts_pf")(*RTS_OK))
  assert ok and why[0] == 4, why


def test_without_a_device_it_fails_loudly(gen_dir):
  import torch
  if torch.cuda.is_available():
    pytest.skip("a GPU is present")
  name = "kinematic6"
  ffi, lib = _load(gen_dir, name)
  ok, why = _failed(ffi, lib, name, getattr(lib, f"{name}_batch_rts_pf")(*RTS_OK))
  assert ok and why[0] == 1, why
