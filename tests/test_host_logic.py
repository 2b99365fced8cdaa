"""CPU tests of the host-side orchestrator (rednose_amd.helpers.ekf_sym.EKF_sym): time bookkeeping, rewind /
fast-forward ring, Estimate tuples, rts_smooth, maha_test.

The class binds whatever library exports the reference's scalar C ABI.  Here -- and only here, as the
checker -- it is pointed at the ORACLE build of that ABI (oracle/_ref or oracle/_port) so the host logic can
be exercised without a GPU and compared with trajectories produced by the reference's own Python class
(tests/golden/, oracle/make_golden.py).  The product path (generated HIP library) is covered by -m gpu tests.
"""
import os
import re

import numpy as np
import pytest

from conftest import assert_close, golden
from oracle_lib import OracleLib
from rednose_amd.helpers.ekf_sym import EKF_sym


def oracle_folder(name):
  lib = OracleLib(name)
  return os.path.dirname(lib.path)


def test_known_answer_through_orchestrator():
  """/root/reference/examples/test_kinematic_kf.py:11-55 driven through EKF_sym.predict_and_update_batch."""
  g = golden("kinematic_stream.npz")
  f = EKF_sym(oracle_folder("kinematic"), "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
  R = np.array([[[0.1**2]]])
  for t, meas in zip(g["ts"], g["zs"]):
    est = f.predict_and_update_batch(t, 1, np.array([[meas]]), R)
    assert len(est) == 9 and est[4] == t and est[5] == 1
  lit = g["literals"]
  x, std = f.state(), np.sqrt(np.diag(f.covs()))
  for got, want in zip((x[0], std[0], x[1], std[1]), lit):
    assert round(abs(got - want), 7) == 0          # the reference's assertAlmostEqual
  assert_close(x, g["xs"][-1], rtol=1e-11, floor=1e-13)


def test_rewind_and_fast_forward_matches_reference_class():
  """/root/reference/examples/test_compare.py:103-120: samples 20 and 40 arrive swapped."""
  g = golden("compare_rewind.npz")
  f = EKF_sym(oracle_folder("compare"), "compare", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
  R = np.array([[[0.1**2]]])
  for i, (t, meas) in enumerate(zip(g["ts"], g["zs"])):
    f.predict_and_update_batch(t, 1, np.array([[meas]]), R)
    assert abs(f.get_filter_time() - g["filter_times"][i]) < 1e-12
    assert_close(f.state(), g["xs"][i], rtol=1e-10, floor=1e-12, what=f"state step {i}")
    assert_close(f.covs().reshape(-1), g["Ps"][i].reshape(-1), rtol=1e-10, floor=1e-12, what=f"cov step {i}")


def test_too_old_observation_is_dropped():
  f = EKF_sym(oracle_folder("kinematic"), "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
  R = np.array([[[0.01]]])
  for i in range(300):
    assert f.predict_and_update_batch(0.01 * i, 1, np.array([[0.1]]), R) is not None
  x_before = f.state().copy()
  assert f.predict_and_update_batch(0.5, 1, np.array([[0.1]]), R) is None     # > max_rewind_age (1 s) behind
  assert np.array_equal(x_before, f.state())
  with pytest.raises(KeyError):
    f.predict_and_update_batch(3.1, 7, np.array([[0.1]]), R)                   # unknown kind (ekf_sym.py:343)
  with pytest.raises(AssertionError):
    f.predict(1.0)                                                            # dt < 0 (ekf_sym.py:459)


def test_rewind_ring_is_bounded():
  f = EKF_sym(oracle_folder("kinematic"), "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
  R = np.array([[[0.01]]])
  for i in range(600):
    f.predict_and_update_batch(0.001 * i, 1, np.array([[0.1]]), R)
  assert len(f.rewind_t) == len(f.rewind_states) == len(f.rewind_obscache) == 512
  f.init_state(np.array([0.5, 0.0]), np.eye(2), None)
  assert len(f.rewind_t) == 0 and f.get_filter_time() is None


def _estimates(g, with_pk=True):
  n = len(g["t"])
  return [(g["xk_km1"][i], g["xk_k"][i], g["Pk_km1"][i], g["Pk_k"][i], g["t"][i], 0, None, None, None) for i in range(n)]


def test_rts_smooth_kinematic_matches_reference():
  g = golden("kinematic_rts.npz")
  f = EKF_sym(oracle_folder("kinematic"), "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
  xs, Ps = f.rts_smooth(_estimates(g), norm_quats=False)
  assert_close(xs, g["xs_smooth"], rtol=1e-10, floor=1e-12, what="smoothed states")
  assert_close(Ps.reshape(len(Ps), -1), g["Ps_smooth"].reshape(len(Ps), -1), rtol=1e-9, floor=1e-11, what="smoothed covs")


def test_rts_smooth_live_matches_reference():
  from examples.live_kf import LiveKalman as L
  g = golden("live_rts.npz")
  f = EKF_sym(oracle_folder("live"), "live", L.Q, L.initial_x, np.diag(L.initial_P_diag), 23, 22, quaternion_idxs=[3])
  est_in = _estimates(g)
  keep_copy = [e[1].copy() for e in est_in]
  xs, Ps = f.rts_smooth(est_in, norm_quats=True)
  assert all(np.array_equal(a, e[1]) for a, e in zip(keep_copy, est_in)), "rts_smooth must not modify its input"
  assert_close(xs, g["xs_smooth"], rtol=1e-7, floor=1e-9, what="smoothed states")
  idx = g["Ps_smooth_idx"]
  assert_close(Ps[idx].reshape(len(idx), -1), g["Ps_smooth"].reshape(len(idx), -1), rtol=1e-6, floor=1e-8, what="smoothed covs")


def test_maha_test_matches_reference_decisions():
  from examples.live_kf import LiveKalman as L
  g = golden("live_maha.npz")
  f = EKF_sym(oracle_folder("live"), "live", L.Q, L.initial_x, np.diag(L.initial_P_diag), 23, 22)
  got = np.array([f.maha_test(g["x"][i], g["P"][i], 12, g["z"][i], g["R"]) for i in range(len(g["x"]))])
  assert np.array_equal(got, g["accepted"])


def test_kernel_resource_report_parser():
  """rednose_amd.build.kernel_resources: hipcc remarks -> per-kernel numbers written next to every library."""
  from rednose_amd.build import kernel_resources
  remarks = """x.hip:1:1: remark: Function Name: _ZN12_GLOBAL__N_112k_fn_err_funEPKdS1_Pd [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: 13 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
x.hip:2:1: remark: Function Name: _ZN12_GLOBAL__N_18k_step_1ILb1EEEvPdS1_S1_PKdiS3_S3_S3_dliPh [-Rpass-analysis=kernel-resource-usage]
x.hip:2:1: remark:     VGPRs: 242 [-Rpass-analysis=kernel-resource-usage]
x.hip:2:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
x.hip:2:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]
x.hip:2:1: remark:     LDS Size [bytes/block]: 28960 [-Rpass-analysis=kernel-resource-usage]
x.hip:3:1: remark: Function Name: _ZN2rn10k_rts_wideIN12_GLOBAL__N_18RtsModelEEEvPKdS4_S4_lS4_liPdS5_ [-Rpass-analysis=kernel-resource-usage]
x.hip:3:1: remark:     ScratchSize [bytes/lane]: 464 [-Rpass-analysis=kernel-resource-usage]
x.hip:3:1: remark:     VGPRs Spill: 129 [-Rpass-analysis=kernel-resource-usage]
"""
  u = kernel_resources(remarks)
  assert list(u) == ["k_fn_err_fun", "k_step_1<true>", "k_rts_wide"]
  assert u["k_step_1<true>"] == dict(vgprs=242, agprs=0, scratch=0, lds=28960, vgpr_spill=0, occupancy=2)
  assert u["k_rts_wide"]["scratch"] == 464 and u["k_rts_wide"]["vgpr_spill"] == 129


def test_gen_code_falls_back_instead_of_failing(tmp_path, monkeypatch):
  """gen_code must not leave a model unbuildable because an OPTIONAL kernel does not fit the register file: a smoother that
  still touches scratch after the one-wavefront fallback is dropped (library without batch_rts, RuntimeWarning), the
  forward filter ships.  No process-global state survives the call (round 2 kept model names in module-level sets).
  hipcc is replaced by a stub that reports scratch for k_rts_group on every build."""
  import warnings
  import examples.random_kf as R
  from rednose_amd import build as rb
  from rednose_amd.codegen import emit as rn_emit
  seen = []

  def fake_compile(folder, name, **kw):
    src = open(f"{folder}/{name}.hip", encoding="utf-8").read()
    has_rts = "_batch_rts(" in src
    seen.append(has_rts)
    usage = {"k_step_1<true>": dict(vgprs=200, agprs=0, scratch=0, lds=0, vgpr_spill=0, occupancy=2)}
    if has_rts:
      usage["k_rts_group"] = dict(vgprs=256, agprs=256, scratch=64, lds=0, vgpr_spill=8, occupancy=1)
    fake_compile.last_usage = usage
    rb.compile_filter.last_usage = usage
    return f"{folder}/lib{name}.so"
  monkeypatch.setattr(rb, "compile_filter", fake_compile)
  M = R.Random11Kalman
  with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    M.generate_code(str(tmp_path))
  assert seen == [True, True, False], seen            # default, one wavefront per SIMD, without the smoother
  assert any("WITHOUT batch_rts" in str(x.message) for x in w)
  assert "_batch_rts(" not in open(tmp_path / f"{M.name}.h", encoding="utf-8").read()
  assert (tmp_path / f"{M.name}.digest").exists()
  assert rn_emit._active == frozenset() and not hasattr(rn_emit, "FORCE_WIDE")      # pylint: disable=protected-access


def test_fused_run_generates_for_wide_observations():
  """8 filters x 9 observation entries > 64 lanes: the fused run carries two entries per lane instead of asserting."""
  import examples.random_kf as R
  from rednose_amd.codegen.spec import build_spec
  from rednose_amd.codegen.emit import emit
  mdl = R.RandomWideObs10Kalman.model()
  hdr, src = emit(build_spec(**mdl))
  assert "randz10_batch_run(" in hdr and "zn[2]" in src and "ERR_UNSUPPORTED" not in src.split("randz10_batch_run(")[1].split("}")[0]


def test_blocked_fused_run_is_emitted_and_falls_back(tmp_path, monkeypatch):
  """Lane-per-filter models run their fused schedules in blocks of steps (k_run_blk without the trace, k_run_blk_tr with it,
  emit_small.run_kernel_blk): {name}_run_unroll reports the block size, multi-kind models get a shorter block, and a build in which
  ONLY those kernels spill is re-emitted with the step-at-a-time k_run instead (fallback no_run_blk), not moved to the lane-group
  family."""
  import examples.random_kf as R
  from examples.kinematic_kf import KinematicKalman
  from rednose_amd import build as rb
  from rednose_amd.codegen import emit_small
  from rednose_amd.codegen.emit import emit, family
  from rednose_amd.codegen.spec import build_spec
  spec = build_spec(**KinematicKalman.model())
  assert family(spec) == "small" and emit_small.run_block(spec) == 16
  _, src = emit(spec)
  launch = src.split("kinematic_batch_run(")[1]
  assert "void k_run_blk(" in src and "void k_run_blk_tr(" in src and "void k_run(" not in src
  assert "if (trace_x == nullptr && trace_P == nullptr) {" in launch and "k_run_blk," in launch and "k_run_blk_tr," in launch
  assert "kinematic_run_unroll(void) { return 16; }" in src
  spec3 = build_spec(**R.Random3Kalman.model())           # three kinds: 16 / 3 -> blocks of 4 steps (code size)
  assert emit_small.run_block(spec3) == 4
  _, src = emit(spec, fallbacks=("no_run_blk",))
  assert "k_run_blk" not in src and "void k_run(" in src and "kinematic_run_unroll(void) { return 8; }" in src      # the step-at-a-time kernel's prefetch depth
  monkeypatch.setenv("RN_TUNE", "run_block=-1")
  assert emit_small.run_block(spec) == 0
  monkeypatch.delenv("RN_TUNE")

  seen = []

  def fake_compile(folder, name, **kw):
    src_ = open(f"{folder}/{name}.hip", encoding="utf-8").read()
    blk = "void k_run_blk(" in src_
    seen.append((blk, "family=small" in src_))
    usage = {"k_run": dict(vgprs=200, agprs=0, scratch=0, lds=0, vgpr_spill=0, occupancy=2)}
    if blk:           # the traced twin is the one that does not fit
      usage["k_run_blk"] = dict(vgprs=256, agprs=100, scratch=0, lds=0, vgpr_spill=0, occupancy=1)
      usage["k_run_blk_tr"] = dict(vgprs=256, agprs=256, scratch=32, lds=0, vgpr_spill=4, occupancy=1)
    rb.compile_filter.last_usage = usage
    return f"{folder}/lib{name}.so"
  monkeypatch.setattr(rb, "compile_filter", fake_compile)
  KinematicKalman.generate_code(str(tmp_path))
  assert seen == [(True, True), (False, True)], seen       # second build: same family, without the blocked kernel


def _lane_per_filter_model(name):
  import examples.random_kf as R
  from examples.attitude_kf import AttitudeKalman
  from examples.kinematic_kf import KinematicKalman
  from examples.kinematic6_kf import Kinematic6Kalman
  return {"kinematic": KinematicKalman, "kinematic6": Kinematic6Kalman, "attitude": AttitudeKalman, "rand5": R.Random5Kalman}[name].model()


@pytest.mark.parametrize("name", ["kinematic", "kinematic6", "attitude", "rand5"])      # Z = 1, Z > 1, odd E^2: the smallest that separate the cases
def test_step_kernels_leave_exactly_the_observation_tile_in_flight(name):
  """Every lane-per-filter step kernel (k_step_*, k_stepc_*, k_kinds) has ONE counted wait, wait_but_loads<N>, and N is the number of 16-byte
  LDS-DMA requests of its observation tile alone -- (32 Z + 63) // 64 for 64 rows of Z doubles, worked out here from Z, not taken from the emitter:
  exactly that tile may stay in flight under the predict."""
  from rednose_amd.codegen import emit, emit_small
  from rednose_amd.codegen.spec import build_spec
  spec = build_spec(**_lane_per_filter_model(name))
  assert emit.family(spec, ()) == "small"
  text = emit_small.kernels(spec)
  zdim = {f"{pre}{k.kind}": k.zdim for k in spec.kinds for pre in ("k_step_", "k_stepc_")}
  if emit.step_kinds(spec, ()):
    zdim["k_kinds"] = max(k.zdim for k in spec.kinds)
  heads = list(re.finditer(r"^__global__ __launch_bounds__\(64\) void (k_stepc?_\d+|k_kinds)\(", text, flags=re.M))
  assert sorted(m.group(1) for m in heads) == sorted(zdim), "one kernel per name"
  for m in heads:
    body = text[m.start():text.index("\n}\n", m.start())]
    waits = re.findall(r"wait_but_loads<(\d+)>\(", body)
    Z = zdim[m.group(1)]
    assert waits == [str((32 * Z + 63) // 64)], f"{name} {m.group(1)} (Z = {Z}): counted waits {waits}"


@pytest.mark.parametrize("knob", ["head", "zwait", "split", "waves"])
def test_retired_step_kernel_knobs_are_unknown(monkeypatch, knob):
  """The measured-and-lost alternatives of the lane-per-filter step kernels are gone: naming one in RN_TUNE is an error, not a silent default."""
  from rednose_amd.codegen import tuning
  monkeypatch.setenv("RN_TUNE", f"small_{knob}=0")
  with pytest.raises(ValueError, match="unknown knob"):
    tuning.current()


def test_cffi_branch_of_load_code_runs_the_known_answers(monkeypatch):
  """`load_code` prefers cffi where it is importable -- which is every real rednose environment (rednose/helpers/__init__.py:3,18-31)
  -- and this image has none, so that branch (header lines -> ffi.cdef -> ffi.dlopen, ffi.cast marshalling in EKF_sym) never ran.
  Here it runs against the ctypes-backed stand-in the oracle tooling uses to import the reference (oracle/cffi_shim: cdef / dlopen /
  cast, the three cffi features the reference's orchestrator uses): the known-answer stream of test_kinematic_kf.py through
  EKF_sym over the cffi-loaded library, and the loader's refusal logic.  It is a stand-in, not cffi: what this pins is OUR side of
  the branch."""
  import sys
  from conftest import REPO
  import rednose_amd.helpers as H
  monkeypatch.syspath_prepend(os.path.join(REPO, "oracle", "cffi_shim"))
  monkeypatch.delenv("RN_LOADER", raising=False)
  sys.modules.pop("cffi", None)
  try:
    ffi, lib = H.load_code(oracle_folder("kinematic"), "kinematic", backend="cffi")
    assert type(ffi).__module__ == "cffi" and not isinstance(ffi, H.CtypesFFI)
    assert "kinematic_predict" in dir(lib) and "kinematic_h_1" in dir(lib)
    g = golden("kinematic_stream.npz")
    f = EKF_sym(oracle_folder("kinematic"), "kinematic", np.diag([0.1**2, 2.0**2]), np.array([0.5, 0.0]), np.diag([1.0, 1.0]), 2, 2)
    assert type(f._ffi).__module__ == "cffi"           # pylint: disable=protected-access
    R = np.array([[[0.1**2]]])
    for t, meas in zip(g["ts"], g["zs"]):
      f.predict_and_update_batch(t, 1, np.array([[meas]]), R)
    x, std = f.state(), np.sqrt(np.diag(f.covs()))
    for got, want in zip((x[0], std[0], x[1], std[1]), g["literals"]):
      assert round(abs(got - want), 7) == 0
  finally:
    sys.modules.pop("cffi", None)


@pytest.mark.skipif(not os.path.exists("/root/reference/rednose/helpers/ekf_sym.py"), reason="needs the reference tree (this container only)")
def test_reference_class_binds_the_hip_libraries():
  """The drop-in claim of the boundary, as far as it can be taken on ONE machine: the reference's OWN, unmodified Python loader and
  orchestrator (/root/reference/rednose/helpers/__init__.py:18-31 load_code, ekf_sym.py:258-349 EKF_sym.__init__) pointed at the HIP
  builds generated/libkinematic.so and generated/liblive.so -- header parsed by its `void ` filter, library dlopen'ed, observation kinds
  discovered by scanning dir(lib) for {name}_h_<int> / {name}_He_<int>, every function pointer bound.  Its compute calls then reach the
  HIP entry points: with no device here they record an error in the library instead of touching x / P (checked), on the GPU box the same
  symbols run the kernels (rednose_amd's twin of the class drives them there: the Python reference may not travel to the GPU box in any
  form, and this container has no GPU).  Runs in a subprocess: `rednose` and the cffi stand-in stay out of this process."""
  import subprocess
  import sys
  from conftest import REPO
  from examples import ensure_generated
  gen = ensure_generated(["kinematic", "live"])
  code = r"""
import ctypes, sys
import numpy as np
sys.path[:0] = [sys.argv[2], "/root/reference"]
from rednose.helpers.ekf_sym import EKF_sym            # the reference's class, unmodified
from rednose.helpers import load_code                   # ... and its loader
gen = sys.argv[1]
f = EKF_sym(gen, "kinematic", np.diag([0.01, 4.0]), np.array([0.5, 0.0]), np.eye(2), 2, 2)
assert sorted(f.hs.keys()) == [1] and sorted(f.Hs.keys()) == [1] and f.feature_track_kinds == [], (f.hs.keys(), f.feature_track_kinds)
x0, P0 = f.state().copy(), f.covs().copy()
f.predict_and_update_batch(0.0, 1, np.array([[0.3]]), np.array([[[0.01]]]))       # reaches kinematic_predict / kinematic_update_1 of the HIP build
dll = ctypes.CDLL(gen + "/libkinematic.so")
dll.kinematic_last_error_string.restype = ctypes.c_char_p
print("kinematic last_error", dll.kinematic_last_error(), dll.kinematic_last_error_string().decode())
print("kinematic untouched", int(np.array_equal(f.state(), x0) and np.array_equal(f.covs(), P0)))
Q = np.eye(22) * 1e-3
x = np.zeros(23); x[3] = 1.0
g = EKF_sym(gen, "live", Q, x, np.eye(22), 23, 22)
print("live kinds", sorted(g.hs.keys()), "updates", sorted(g._updates.keys()) if hasattr(g, "_updates") else "-")
ffi, lib = load_code(gen, "live")
names = [n for n in dir(lib) if n.startswith("live_")]
print("live symbols", len(names), int("live_predict" in names and "live_update_12" in names and "live_H_mod_fun" in names and "live_err_fun" in names))
"""
  res = subprocess.run([sys.executable, "-c", code, gen, os.path.join(REPO, "oracle", "cffi_shim")], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
  assert res.returncode == 0, res.stderr[-3000:]
  lines = res.stdout.strip().split("\n")
  err = [ln for ln in lines if ln.startswith("kinematic last_error")][0].split(" ", 3)
  assert int(err[2]) != 0, "a compute call without a device must leave an error in the library"
  assert "kinematic untouched 1" in lines, "a failed call must not touch x / P"
  assert [ln for ln in lines if ln.startswith("live kinds")][0].startswith("live kinds [3, 4, 9, 10, 12, 13, 14, 19]")
  sym = [ln for ln in lines if ln.startswith("live symbols")][0].split()
  assert int(sym[2]) >= 8 * 3 + 6 and sym[3] == "1"


def test_nullspace_residual_follows_eigens_pivot_order_and_rank_decision(tmp_path):
  """rn::nullspace_residual (codegen/lower.py: the MSCKF residual in the reference's basis, A = Hea^T.fullPivLu().kernel(), ekf_c.c:71-73)
  compiled for the host against the numpy restatement of Eigen's FullPivLU (tests/conftest.py): random Jacobians, Jacobians with TIED
  entries (equal magnitudes in different rows and columns -- which one becomes the pivot decides the basis: Eigen's visitor walks the
  corner column by column and keeps the first maximum), a Jacobian whose LATER pivot exceeds the first (the rank threshold scales with the
  largest pivot met, not the first), and rank-deficient ones (returns false, residual zeroed)."""
  import ctypes
  import subprocess
  from conftest import fullpiv_kernel
  from rednose_amd.codegen.lower import NULLSPACE_RESIDUAL
  src = tmp_path / "ns.cpp"
  src.write_text("#include <cmath>\n#define __device__\n#define __forceinline__ inline\nusing std::fabs;\n" + NULLSPACE_RESIDUAL + """
extern "C" int ns63(const double* Hea, const double* y, double* out) {
  double H[18], yy[6], o[3];
  for (int i = 0; i < 18; i++) H[i] = Hea[i];
  for (int i = 0; i < 6; i++) yy[i] = y[i];
  const bool ok = rn::nullspace_residual<6, 3>(H, yy, o);
  for (int i = 0; i < 3; i++) out[i] = o[i];
  return ok ? 1 : 0;
}
""", encoding="utf-8")
  lib = tmp_path / "libns.so"
  subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", str(src), "-o", str(lib)], check=True)
  fn = ctypes.CDLL(str(lib)).ns63
  dp = ctypes.POINTER(ctypes.c_double)
  fn.argtypes = [dp, dp, dp]
  rng = np.random.default_rng(11)
  cases = [rng.normal(size=(6, 3)) for _ in range(40)]
  tied = np.array([[2.0, -2.0, 1.0], [2.0, 1.0, -2.0], [-2.0, 2.0, 2.0], [1.0, 2.0, 0.5], [0.5, -1.0, 2.0], [2.0, 2.0, 2.0]])
  cases += [tied, tied[::-1].copy(), tied[:, ::-1].copy(), np.sign(rng.normal(size=(6, 3))) * 3.0]
  grow = np.array([[1.0, 1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 0.0, 1e-3], [0.3, 0.2, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]])      # second pivot (2) > first (1)
  cases.append(grow)
  for Hea in cases:
    y = rng.normal(size=6)
    Aref = fullpiv_kernel(Hea.T)
    out = np.zeros(3)
    ok = fn(np.ascontiguousarray(Hea).ctypes.data_as(dp), y.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert ok == 1 and Aref.shape == (6, 3)
    assert_close(out, Aref.T @ y, rtol=1e-12, floor=1e-14, what="residual in Eigen's kernel basis")
  deficient = [np.tile(rng.normal(size=(2, 3)), (3, 1)), np.zeros((6, 3)), np.outer(rng.normal(size=6), rng.normal(size=3))]
  for Hea in deficient:
    out = np.ones(3)
    assert fn(np.ascontiguousarray(Hea).ctypes.data_as(dp), rng.normal(size=6).ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    assert not out.any() and fullpiv_kernel(Hea.T).shape[1] > 3


def test_lowered_sin_cos_pairs_and_their_accuracy(tmp_path):
  """rednose_amd/codegen/lower.py prints sin(a) / cos(a) through ONE rn::sincos_fast per distinct argument; the function itself (pure
  IEEE arithmetic: the host build computes what the device computes) against libm's long double routines over 2e6 arguments up to
  2^45, the quadrant boundaries, and NaN beyond 2^45 and for NaN / inf."""
  import ctypes
  import subprocess
  import sympy as sp
  from rednose_amd.codegen.lower import Block
  a, b = sp.symbols("a b")
  blk = Block()
  blk.add("o0", sp.sin(a) * sp.cos(a) + sp.sin(2 * a * b))
  blk.add("o1", sp.cos(a) * b + sp.cos(2 * a * b) * sp.sin(b))
  stmts, _ = blk.lower()
  text = "\n".join(stmts)
  assert text.count("rn::sincos_fast(") == 3      # arguments a, 2 a b, b: one pair each
  assert " sin(" not in text and " cos(" not in text and "(sin(" not in text and "(cos(" not in text
  # the compound argument 2 a b became a temporary: its pair is computed after that temporary, the two plain arguments' pairs first, together
  tmp = [i for i, ln in enumerate(stmts) if ln.startswith("const double t1 = 2.0*a*b")][0]
  assert [i for i, ln in enumerate(stmts) if "rn::sincos_fast(t1," in ln][0] == tmp + 1
  assert "rn::sincos_fast(a," in stmts[0] and "rn::sincos_fast(b," in stmts[1]
  from rednose_amd.codegen.lower import SINCOS_FAST
  src = "\n".join(["#include <cmath>", "#define __device__", "#define __forceinline__ inline", SINCOS_FAST,
                   'extern "C" void sc(const double* a, double* s, double* c, double* rs, double* rc, long n) {',
                   "  for (long i = 0; i < n; i++) { rn::sincos_fast(a[i], s[i], c[i]); rs[i] = (double)sinl((long double)a[i]); rc[i] = (double)cosl((long double)a[i]); } }"])
  cpp, lib = tmp_path / "sc.cpp", tmp_path / "libsc.so"
  cpp.write_text(src, encoding="utf-8")
  res = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  fn = ctypes.CDLL(str(lib)).sc
  rng = np.random.default_rng(5)
  k = np.arange(-40000, 40001) * (np.pi / 2)
  big = np.ldexp(rng.uniform(1.0, 2.0, 400000), rng.integers(16, 45, 400000)) * rng.choice([-1.0, 1.0], 400000)
  args = np.concatenate([rng.uniform(-4, 4, 500000), rng.uniform(-100, 100, 500000), rng.uniform(-65536, 65536, 500000), rng.uniform(-1e-3, 1e-3, 250000),
                         big, k, np.nextafter(k, 1e9), np.nextafter(k, -1e9), k + np.pi / 4,
                         [0.0, -0.0, 65536.0, -65536.0, 1e6, -3e9, 2.0**31, 2.0**31 + 1, -2.0**40, 2.0**45, -2.0**45]])
  out = [np.empty_like(args) for _ in range(4)]
  dp = ctypes.POINTER(ctypes.c_double)
  fn(args.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in out], ctypes.c_long(args.size))
  s, c, rs, rc = out
  assert float(np.abs(s - rs).max()) < 2.5e-16 and float(np.abs(c - rc).max()) < 2.5e-16
  bad = np.array([np.nan, np.inf, -np.inf, 2.0**45 + 1, -1e300])
  ob = [np.zeros(5) for _ in range(4)]
  fn(bad.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in ob], ctypes.c_long(5))
  assert np.isnan(ob[0]).all() and np.isnan(ob[1]).all()


def test_nested_trigonometric_arguments_are_declared_before_use(tmp_path):
  """A sin / cos whose argument contains another one that CSE leaves in place (single use: sin(x + cos(y))): the inner pair has to be
  computed before the call that reads it.  The lowered block is compiled for the host and compared with libm."""
  import ctypes
  import subprocess
  import sympy as sp
  from rednose_amd.codegen.lower import Block, SINCOS_FAST
  x, y = sp.symbols("x y")
  blk = Block(names={x: "v[0]", y: "v[1]"})
  blk.add("o[0]", sp.sin(x + sp.cos(y)))
  blk.add("o[1]", sp.cos(sp.sin(y * sp.cos(x)) + x))
  stmts, _ = blk.lower(decl="")
  declared = set()
  for ln in stmts:
    for name in __import__("re").findall(r"\b(tsc\d+)_[sc]\b", ln.split("rn::sincos_fast(")[-1] if "rn::sincos_fast(" in ln else ln):
      assert name in declared or ln.startswith(f"double {name}_s"), ln
    if ln.startswith("double tsc"):
      arg = ln.split("rn::sincos_fast(")[1].split(",")[0]
      for name in __import__("re").findall(r"\b(tsc\d+)_[sc]\b", arg):
        assert name in declared, f"{name} used before its declaration: {ln}"
      declared.add(ln.split()[1].split("_")[0])
  src = "\n".join(["#include <cmath>", "#define __device__", "#define __forceinline__ inline", SINCOS_FAST,
                   'extern "C" void blk(const double* v, double* o) {'] + ["  " + s_ for s_ in stmts] + ["}"])
  cpp, lib = tmp_path / "nt.cpp", tmp_path / "libnt.so"
  cpp.write_text(src, encoding="utf-8")
  res = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", str(cpp), "-o", str(lib)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  fn = ctypes.CDLL(str(lib)).blk
  dp = ctypes.POINTER(ctypes.c_double)
  for vx, vy in ((0.3, -1.2), (2.5, 0.7), (-4.0, 3.1)):
    v, o = np.array([vx, vy]), np.zeros(2)
    fn(v.ctypes.data_as(dp), o.ctypes.data_as(dp))
    want = [np.sin(vx + np.cos(vy)), np.cos(np.sin(vy * np.cos(vx)) + vx)]
    assert np.allclose(o, want, rtol=0, atol=1e-15), (o, want)


def test_bench_prints_counter_traffic_only_for_the_build_it_was_taken_on(tmp_path, monkeypatch):
  """bench.measured_traffic: a record of profiles/pmc_traffic.json applies to the library whose digest it names, or to a later build the
  record lists under `carried_to` (then the JSON line says so); any other build gets None -- never a number measured on different code.
  The mechanism is checked on a synthetic record file; the committed file is then checked against the libraries in generated/."""
  import json
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
  import bench
  repo = tmp_path / "repo"
  (repo / "profiles").mkdir(parents=True)
  rec = {"lib": "demo", "lib_digest": "a" * 64, "hbm_bytes_per_launch": 12345.0, "carried_to": ["b" * 64], "carried_note": "arithmetic only"}
  (repo / "profiles" / "pmc_traffic.json").write_text(json.dumps({"demo_section": rec, "plain_section": {"lib": "demo", "lib_digest": "c" * 64, "hbm_bytes_per_launch": 7.0}}), encoding="utf-8")
  monkeypatch.setattr(bench, "REPO", str(repo))
  label, lib = "demo_section", "demo"
  bench.TRAFFIC_CARRIED.clear()
  (tmp_path / f"{lib}.digest").write_text(rec["lib_digest"], encoding="utf-8")
  assert bench.measured_traffic(label, lib, str(tmp_path)) == rec["hbm_bytes_per_launch"] and not bench.TRAFFIC_CARRIED
  (tmp_path / f"{lib}.digest").write_text(rec["carried_to"][0], encoding="utf-8")
  assert bench.measured_traffic(label, lib, str(tmp_path)) == rec["hbm_bytes_per_launch"]
  assert label in bench.TRAFFIC_CARRIED and rec["lib_digest"][:12] in bench.TRAFFIC_CARRIED[label]
  assert bench.measured_traffic("plain_section", lib, str(tmp_path)) is None      # no carried_to list: another build gets nothing
  bench.TRAFFIC_CARRIED.clear()
  (tmp_path / f"{lib}.digest").write_text("0" * 64, encoding="utf-8")
  assert bench.measured_traffic(label, lib, str(tmp_path)) is None and not bench.TRAFFIC_CARRIED
  assert bench.measured_traffic("no_such_section", lib, str(tmp_path)) is None
  monkeypatch.undo()
  # the committed records: every one applies to the build in generated/ directly -- profiles/collect_and_bench.sh is the last GPU call of a round,
  # on the shipped libraries, so nothing is carried
  real = os.path.join(os.path.dirname(__file__), "..", "profiles", "pmc_traffic.json")
  gen = os.path.join(os.path.dirname(__file__), "..", "generated")
  recs = json.load(open(real, encoding="utf-8"))
  if os.path.exists(os.path.join(gen, "kinematic6.digest")):
    bench.TRAFFIC_CARRIED.clear()
    for k, v in recs.items():
      if isinstance(v, dict) and "lib" in v:
        assert bench.measured_traffic(k, v["lib"], gen) is not None, k
    assert not bench.TRAFFIC_CARRIED, bench.TRAFFIC_CARRIED


def test_register_broadcast_smoother_is_chosen_where_it_applies_and_falls_back():
  """Which smoother kernel a model's batch_rts launches -- the whole map: lane-per-filter models (<= 7 error states) rn::k_rts; ordinary
  lane-group models whose four images fit 20 KB of LDS (8 .. 22 error states, odd counts included) k_rts4 (emit_rts4); MSCKF models, larger
  models and dense models whose F does not fit the slot rn::k_rts_group, which is also the fallback `no_rts4` (gen_code takes it when k_rts4
  does not fit 256 registers without scratch, or when one of its DPP reads follows the write of its source too closely); libraries that contain
  k_rts4 ask for the exact register-pressure trackers (build.model_flags).  (k_rts3, the smoother in the fused run's layout, is gone.)"""
  import examples.random_kf as R
  from examples.kinematic9_kf import Kinematic9Kalman
  from examples.kinematic6_kf import Kinematic6Kalman
  from examples.live_kf import LiveKalman
  from examples.feature_kf import FeatureKalman, WideFeatureKalman
  from rednose_amd import build as rb
  from rednose_amd.codegen import emit, emit_rts4
  from rednose_amd.codegen.spec import build_spec

  def kernel_of(model):
    spec = build_spec(**model.model())
    if model is LiveKalman:      # (emitting live takes 23 s of sympy; the text the build generated for it IS what this emitter printed -- the build's digest check)
      from examples import ensure_generated
      text = open(os.path.join(ensure_generated(["live"]), "live.hip"), encoding="utf-8").read()
    else:
      _, text = emit.emit(spec)
    m = re.search(r"int \w+_batch_rts\(.*?\n}", text, flags=re.S)
    assert m, model
    launched = re.search(r"hipLaunchKernelGGL\((?:rn::)?(k_rts\w*)", m.group(0)).group(1)
    assert ("void k_rts4(" in text) == (launched == "k_rts4") and "k_rts3" not in text
    assert rb.model_flags(text) == (rb.RTS4_FLAGS if launched == "k_rts4" else [])
    return launched, spec
  # (one model per size class and structure; the classes in between -- 5, 11, 13, 32, 40 states -- are routed by the same conditions and run on
  # the GPU in tests/test_gpu_random.py::test_smoother_many_shapes: building their specs here costs half a minute of sympy)
  expected = {R.Random3Kalman: "k_rts", Kinematic6Kalman: "k_rts",
              R.Random8Kalman: "k_rts4", Kinematic9Kalman: "k_rts4", R.RandomWideObs10Kalman: "k_rts4", R.Random17Kalman: "k_rts4", LiveKalman: "k_rts4",
              R.Random24Kalman: "k_rts_group", R.Random56Kalman: "k_rts_group", FeatureKalman: "k_rts_group", WideFeatureKalman: "k_rts_group"}
  for model, want in expected.items():
    got, spec = kernel_of(model)
    assert got == want, (model.__name__, spec.dim_err, got, want)
    assert emit_rts4.applicable(spec) == (want == "k_rts4")
  s8 = build_spec(**R.Random8Kalman.model())
  assert emit_rts4.rows_per_lane(s8) == 1 and emit_rts4.rows_per_lane(build_spec(**R.Random17Kalman.model())) == 2
  _, text = emit.emit(s8)
  assert "v_fmac_f64_dpp" in text and "row_newbcast" in text and "RN4_SETTLE();" in text
  assert "if (dt == 0.0 && !first)" in text and "static constexpr bool ID0 = true;" in text      # the identity-gain path of dt = 0 steps
  _, textg = emit.emit(s8, fallbacks=("no_rts4",))
  assert "k_rts_group<RtsModel>" in textg and "void k_rts4(" not in textg and rb.model_flags(textg) == []
  os.environ["RN_TUNE"] = "rts_dt0=0"
  try:
    _, text0 = emit.emit(s8)
  finally:
    del os.environ["RN_TUNE"]
  assert "if (dt == 0.0 && !first)" not in text0 and "static constexpr bool ID0 = false;" in text0       # the knob keeps the full solve on every step
  _, texta = emit.emit(build_spec(**R.RandomAffine11Kalman.model()))
  assert "void k_rts4(" in texta and "if (dt == 0.0 && !first)" not in texta and "static constexpr bool ID0 = false;" in texta      # predict(0) is not the identity for this model


def test_two_wavefront_fused_run_is_chosen_where_it_applies_and_falls_back():
  """emit_run2.applicable: lane-group models of the 8-lanes-per-filter layout with 13 .. 22 error states (below, k_run is the faster one) without feature-track kinds, extra arguments
  or a window shift; the library then carries k_run2 INSTEAD of k_run (same batch_run entry point), the fallback `no_run2` (gen_code takes it
  when k_run2 does not fit 256 registers without scratch) and the knob run2=0 emit k_run again."""
  import examples.random_kf as R
  from examples.kinematic9_kf import Kinematic9Kalman
  from rednose_amd.codegen import emit, emit_run2, tuning
  from rednose_amd.codegen.spec import build_spec
  s9 = build_spec(**R.Random13Kalman.model())
  assert emit_run2.applicable(s9) and emit_run2.layout2(s9) == (8, 2, 8, 1) and emit_run2.lds_bytes(s9) <= emit_run2.LDS_BUDGET
  _, text = emit.emit(s9)
  assert "void k_run2(" in text and "void k_run(" not in text and "hipLaunchKernelGGL(k_run2," in text and "dim3(R2_THREADS)" in text
  assert text.count("rn::wg_barrier();") >= 4 and "rn::flag_set(" in text and "rn::flag_wait(" in text
  assert "__syncthreads" not in text      # (its release fence would wait for the trace stores in flight)
  # one update body for all kinds: the per-kind parts are switches inside it
  assert text.count("void update_rows_r2(") == 1 and text.count("void predict_rows_r2(") == 1
  _, text1 = emit.emit(s9, fallbacks=("no_run2",))
  assert "void k_run(" in text1 and "void k_run2(" not in text1 and "hipLaunchKernelGGL(k_run," in text1
  os.environ["RN_TUNE"] = "run2=0"
  try:
    _, text0 = emit.emit(s9)
  finally:
    del os.environ["RN_TUNE"]
  assert "void k_run(" in text0 and "void k_run2(" not in text0
  assert not emit_run2.applicable(build_spec(**R.Random24Kalman.model()))        # 16 lanes per filter
  assert not emit_run2.applicable(build_spec(**Kinematic9Kalman.model()))        # 9 error states: k_run measured faster
  from examples.feature_kf import FeatureKalman
  assert not emit_run2.applicable(build_spec(**FeatureKalman.model()))           # feature-track kinds, window shift


def test_up_to_date_stamp_follows_everything_a_library_depends_on(tmp_path, monkeypatch):
  """examples.ensure_generated skips a model whose `{name}.inputs` stamp equals examples.inputs_digest() -- the digest of the emitters, runtime headers,
  helpers, model definitions, sympy's version and the tuning environment -- and regenerates it otherwise; a missing library or digest file voids the stamp."""
  import examples
  calls = []
  monkeypatch.setattr(examples, "model_table", lambda: {"toy": lambda d: calls.append(d)})
  monkeypatch.setattr(examples, "_ENSURED", set())
  d = str(tmp_path)
  examples.ensure_generated(["toy"], folder=d)
  assert calls == [d] and open(os.path.join(d, "toy.inputs"), encoding="utf-8").read() == examples.inputs_digest()
  examples._ENSURED.clear()      # pylint: disable=protected-access
  examples.ensure_generated(["toy"], folder=d)
  assert len(calls) == 2, "no library next to the stamp: the model is generated again"
  for fn in ("libtoy.so", "toy.digest"):
    open(os.path.join(d, fn), "w", encoding="utf-8").close()
  examples._ENSURED.clear()      # pylint: disable=protected-access
  examples.ensure_generated(["toy"], folder=d)
  assert len(calls) == 2, "stamped, library and digest present: skipped"
  base = examples.inputs_digest()
  monkeypatch.setenv("RN_TUNE", "rts_dt0=0")
  assert examples.inputs_digest() != base, "the tuning environment is part of the digest"
  examples._ENSURED.clear()      # pylint: disable=protected-access
  examples.ensure_generated(["toy"], folder=d)
  assert len(calls) == 3, "another tuning: generated again"
  monkeypatch.delenv("RN_TUNE")
  assert examples.inputs_digest() == base
