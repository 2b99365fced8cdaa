#!/usr/bin/env python3
"""sha256 of `{name}.h` / `{name}.hip` as emitted (nothing compiled: no GPU, no hipcc) over models x fallbacks x tuning knobs, a line each.
A change to the emitters that must leave every generated text as it is: run it with --tree on the parent checkout and on the branch, compare.

  python tools/emit_digest.py OUT.txt [--tree OTHER_CHECKOUT] [--jobs N] [--with KNOB=V,..] [--without SUFFIX,..]

--with appends knob settings to every configuration's RN_TUNE and leaves the labels as they are: a new knob whose value V is meant to reproduce a
parent that does not know the knob is checked by comparing that file with the parent's own.  Configurations come and go with the knobs, so two
digest files are compared by label: every line they share a label for must be the same line (`grep -Fxvf PARENT.txt BRANCH.txt` prints what is not).
--without takes the named functions of the C ABI ({name}_SUFFIX: prototype and definition) and the named kernels (k_...) out of the texts before
they are hashed: a change that adds entry points or kernels and must leave everything else as it is gives, with what it adds named, the parent's own lines.
A name behind `dev:` is a `__device__` function of the generated text (dev:update_2_rows_epf), taken out the same way."""
import argparse
import hashlib
import os
import re
import sys
import tempfile
from concurrent.futures import ProcessPoolExecutor

KNOBS = ("small_timeline=1", "run_block=-1")      # of the lane-per-filter family: the stamped step kernels, the fused run without its blocked kernels
FALLBACK_MODELS = {"force_wide": ("kinematic6", "attitude"), "no_run_blk": ("kinematic", "kinematic6"), "no_kinds": ("kinematic6", "kinematic9", "live"),
                   "no_model_defaults": ("live", "feature36"), "no_run2": ("live",), "no_tri": ("live",), "no_rts4": ("live",), "rts_one_wave": ("live",),
                   "no_rts": ("live",), "no_run": ("rand40", "feature36"),
                   "no_run_pf": ("kinematic6", "kinematic9", "live", "rand17"),
                   "no_run_pf_r": ("kinematic6", "kinematic9", "live"),
                   "no_run_pf_rd": ("kinematic6", "kinematic9", "live", "randz10"),
                   "no_rts4_pf": ("kinematic9", "live"),
                   "no_rts_pf": ("kinematic6", "kinematic9", "live", "rand24"),
                   "no_run_pf_ea": ("feature", "feature36")}      # models on which the fallback changes the text
GV_MODELS = ("gv_runtime", "gv_runtime10", "gv_extra")
LANE_GROUP_KNOBS = {      # of the lane-group family: the branches of its step kernels, the fused runs and the smoother that no default model takes
  "live": ("wide_timeline=1", "wide_lean_q=0", "wide_inline=0", "wide_db=1,wide_ft=16", "wide_lean=0,wide_lb=0,wide_db=-1,wide_ft=0", "run2_prio=3",
           "nt_trace=0", "rts_dt0=0", "tri_trace=0", "run2=0", "rts4=0"),
  "kinematic9": ("wide_fpw=2", "wide_db=1", "wide_lean=1", "wide_lean=1,wide_lean_q=1", "wide_ft=8,wide_lb=2"),
  "rand13": ("wide_timeline=1",), "rand17": ("wide_timeline=1",), "rand24": ("wide_timeline=1",),
  "feature": ("wide_lean=1",), "feature36": ("wide_ft=8",), "randz10": ("wide_lean=1",)}
# of the smoother k_rts4: with those above, full and packed x odd and even records x with and without the identity-gain step (appended at the end)
RTS4_KNOBS = {"rand17": ("rts_dt0=0", "tri_trace=0"), "kinematic9": ("rts_dt0=0",), "rand8": ("rts_dt0=0",)}


def configurations():
  """-> [(model, RN_TUNE, fallback or None)]"""
  import examples
  from rednose_amd.codegen import emit
  assert set(FALLBACK_MODELS) == set(emit.FALLBACKS), "a fallback without models in this matrix"
  cfg = [(n, "", None) for n in examples.model_table()] + [(n, "exact_math=1", None) for n in examples.EXACT_NAMES]
  cfg += [(n, "", fb) for fb in emit.FALLBACKS for n in FALLBACK_MODELS[fb]]
  cfg += [(n, kn, None) for n in ("kinematic6", "attitude") for kn in KNOBS] + [("kinematic9", "wide_timeline=1", None)]
  cfg += [(n, "", None) for n in GV_MODELS]
  cfg += [(n, kn, None) for n, knobs in LANE_GROUP_KNOBS.items() for kn in knobs]
  return cfg + [(n, kn, None) for n, knobs in RTS4_KNOBS.items() for kn in knobs]


def gv_spec(name):
  """The models of tests/test_global_vars.py: a run-time scalar (`set_gain`) in either kernel family, and an extra routine."""
  import sympy as sp
  from rednose_amd.codegen.spec import build_spec
  n, gain = (10 if name.endswith("10") else 2), (sp.Float(1.0) if name == "gv_extra" else sp.Symbol("gain"))
  state_sym, dt, other = sp.MatrixSymbol("state", n, 1), sp.Symbol("dt"), sp.MatrixSymbol("other", 2, 1)
  state = sp.Matrix(state_sym)
  rate = sp.Matrix([gain * state[i + 1, 0] if i < n - 1 else 0 for i in range(n)])
  obs = [[sp.Matrix([state[0, 0] + (gain * state[n - 1, 0] if n > 2 else 0)]), 1, None]]
  energy = sp.Matrix([[0.5 * state[1, 0]**2 + 9.81 * state[0, 0] + other[0, 0] * other[1, 0]]])
  extra = dict(extra_routines=[("energy", energy, [state_sym, other])]) if name == "gv_extra" else dict(global_vars=[gain])
  return build_spec(name, state + dt * rate, dt, state_sym, obs, n, n, **extra)


class _Spec(Exception):
  pass


def example_spec(name):
  """The FilterSpec the example's own generate_code() hands to the emitter (whatever it passes to gen_code): gen_code stops there."""
  import examples
  from rednose_amd.helpers import ekf_sym

  def grab(spec, fallbacks=()):
    raise _Spec(spec)
  real, ekf_sym.emit = ekf_sym.emit, grab
  try:
    with tempfile.TemporaryDirectory() as d:
      examples.model_table()[name](d)
    raise RuntimeError(f"{name}: generate_code did not reach the emitter")
  except _Spec as e:
    return e.args[0]
  finally:
    ekf_sym.emit = real


def without(name, hdr, src, suffixes):
  """(hdr, src) minus the C ABI functions {name}_SUFFIX: their prototypes in the header, their definitions in the source (one-line bodies
  `sig { ... }` and bodies between the braces' own lines, the two forms emit._Abi.fn prints).  A suffix that starts with `k_` names a kernel
  instead: its `__global__` definition goes, up to the closing brace in the first column, with the `// ----` title line in front of it; one
  that starts with `dev:` a `__device__` function."""
  for sfx in suffixes:
    if sfx.startswith("dev:"):      # a device function: from its `__device__` line to the closing brace in the first column
      src = re.sub(r"^__device__[^\n]*\bvoid %s\(.*?^\}\n" % re.escape(sfx[4:]), "", src, flags=re.M | re.S)
      continue
    if sfx.startswith("k_"):
      src = re.sub(r"(?:^// ----[^\n]*\n\n?)?^__global__[^\n]*\bvoid %s\(.*?^\}\n" % sfx, "", src, flags=re.M | re.S)
      continue
    hdr = re.sub(r"^\w[\w ]*?\*?%s_%s\(.*?\);\n" % (name, sfx), "", hdr, flags=re.M)
    src = re.sub(r"^\w[\w ]*?\*?%s_%s\([^\n]*\) \{(?: [^\n]* \}\n|\n.*?\n\}\n)" % (name, sfx), "", src, flags=re.M | re.S)
  return hdr, src


def digest(cfg):
  from rednose_amd.codegen import emit
  name, tune, fb = cfg
  os.environ["RN_TUNE"] = ",".join(t for t in (tune, os.environ.get("RN_DIGEST_WITH", "")) if t)
  hdr, src = emit.emit(gv_spec(name) if name in GV_MODELS else example_spec(name), (fb,) if fb else ())
  hdr, src = without(name, hdr, src, [sfx for sfx in os.environ.get("RN_DIGEST_WITHOUT", "").split(",") if sfx])
  label = name + (f" RN_TUNE={tune}" if tune else "") + (f" fallback={fb}" if fb else "")
  return f"{label}: h {hashlib.sha256(hdr.encode()).hexdigest()} hip {hashlib.sha256(src.encode()).hexdigest()}"


if __name__ == "__main__":
  ap = argparse.ArgumentParser(description=__doc__.split("\n", 1)[0])
  ap.add_argument("out")
  ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), help="checkout to take rednose_amd and examples from")
  ap.add_argument("--jobs", type=int, default=4)
  ap.add_argument("--with", dest="extra", default="", help="knob settings appended to every configuration's RN_TUNE (labels unchanged)")
  ap.add_argument("--without", dest="without", default="", help="suffixes of C ABI functions taken out of the texts before hashing")
  args = ap.parse_args()
  os.environ["RN_DIGEST_WITH"] = args.extra
  os.environ["RN_DIGEST_WITHOUT"] = args.without
  tree = os.path.abspath(args.tree)
  sys.path.insert(0, tree)
  with ProcessPoolExecutor(args.jobs, initializer=sys.path.insert, initargs=(0, tree)) as ex:
    lines = list(ex.map(digest, configurations()))
  with open(args.out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
  print(f"{len(lines)} configurations -> {args.out}")
