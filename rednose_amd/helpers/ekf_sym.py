"""gen_code + filter orchestrators for the MI355X-native engine.  (orchestrators appended below)"""
import ctypes
import logging
import os
from bisect import bisect_right
from collections import OrderedDict, deque

import numpy as np

from rednose_amd import build as rn_build
from rednose_amd.codegen.spec import build_spec
from rednose_amd.codegen.emit import emit
from rednose_amd.codegen.emit_common import NOISE_MODES, TABLE, ENTRY, DIAG
from rednose_amd.helpers import KalmanError, load_code
from rednose_amd.helpers.chi2_lookup import chi2_ppf


def gen_code(folder, name, f_sym, dt_sym, x_sym, obs_eqs, dim_x, dim_err, eskf_params=None, msckf_params=None,  # pylint: disable=dangerous-default-value
             maha_test_kinds=[], quaternion_idxs=[], global_vars=None, extra_routines=[], compile=True, verbose=False):  # pylint: disable=redefined-builtin
  """Same signature as the reference's gen_code (/root/reference/rednose/helpers/ekf_sym.py:29-30).

  Writes `{folder}/{name}.h` (prototype per line) and `{folder}/{name}.hip`, and -- unless
  compile=False -- builds `{folder}/lib{name}.so` for gfx950.  Differences from the reference:
  `quaternion_idxs` is honoured (baked into the kernels, enabled per call by `norm_quats`), and the
  build is skipped when sources and an up-to-date library are already there.
  """
  obs_eqs = [list(eq[:3]) for eq in obs_eqs]
  spec = build_spec(name, f_sym, dt_sym, x_sym, obs_eqs, dim_x, dim_err, eskf_params=eskf_params,
                    msckf_params=msckf_params, maha_test_kinds=maha_test_kinds, quaternion_idxs=quaternion_idxs,
                    global_vars=global_vars, extra_routines=extra_routines)
  header, source = emit(spec)
  os.makedirs(folder, exist_ok=True)
  digest = rn_build.source_digest(header, source)
  stamp_fn = os.path.join(folder, f"{name}.digest")
  lib_fn = os.path.join(folder, f"lib{name}.so")
  fresh = False
  if os.path.exists(stamp_fn) and os.path.exists(lib_fn):
    with open(stamp_fn, encoding="utf-8") as f:
      fresh = f.read().strip() == digest
  if fresh:
    return spec            # sources and library are up to date: nothing is rewritten (safe for concurrent ranks)
  with open(os.path.join(folder, f"{name}.h"), "w", encoding="utf-8") as f:
    f.write(header)
  with open(os.path.join(folder, f"{name}.hip"), "w", encoding="utf-8") as f:
    f.write(source)
  if compile and not fresh:
    # Register spills are not tolerated where they were seen to matter: a lane-per-filter build that spilled (8 error states
    # in round 1) also produced a wrong fused-run trace on some runs, and whether hipcc spills depends on the user's f / h
    # expressions, not only on the state count.  The model is then re-emitted in a fallback structure (emit.FALLBACKS) and
    # rebuilt; the stamp keeps the digest of the FIRST emission, so a later gen_code call of this model emits the default text
    # again, finds it stamped and reuses the library.  RN_ALLOW_SPILLS=1 keeps the first build (experiments).
    from rednose_amd.codegen import emit as rn_emit
    from rednose_amd.codegen import tuning as rn_tuning
    fallbacks = []

    def build():
      if fallbacks:
        hdr_, src_ = emit(spec, fallbacks=tuple(fallbacks))
        with open(os.path.join(folder, f"{name}.h"), "w", encoding="utf-8") as f_:
          f_.write(hdr_)
        with open(os.path.join(folder, f"{name}.hip"), "w", encoding="utf-8") as f_:
          f_.write(src_)
      rn_build.compile_filter(folder, name, verbose=verbose)
      usage = rn_build.compile_filter.last_usage
      return usage, rn_build.spilled_kernels(usage)

    def fall_back(which, why):
      msg = f"{name}: {why} -> {which}"
      (print if verbose else logging.getLogger(__name__).info)(msg)
      fallbacks.append(which)
      return build()

    usage, bad = build()
    if not os.environ.get("RN_ALLOW_SPILLS"):
      def drop(noise):
        # a fused run with a schedule per filter that does not fit: this kernel alone is dropped, the other noise flavours and every other structure
        # of the model stay as they are ({name}_has_batch_run_pf{sfx}() == 0): checked on the first build and again behind no_run_blk, which re-emits
        # these kernels with another block size -- never left to force_wide or no_run below
        pf_bad = [k for k in bad if k.startswith(noise.kernel)]
        return fall_back(noise.fallback, f"the fused run with a schedule per filter{noise.what} {pf_bad} does not fit the register file: library "
                                         "without it") if pf_bad else (usage, bad)
      for noise in reversed(NOISE_MODES):
        usage, bad = drop(noise)
      if "k_run_epf" in bad:
        # an MSCKF model's fused run with a schedule per filter: this kernel alone is dropped ({name}_has_batch_run_pf_ea() == 0), batch_run stays
        usage, bad = fall_back("no_run_pf_ea", "the fused run with a schedule per filter, extra arguments and window shifts per entry does not fit the register "
                                               "file: library without it")
      if "k_rts4_pf" in bad:
        # like no_rts4 for batch_rts: the lane-group smoother's per-filter instantiation serves batch_rts_pf instead
        usage, bad = fall_back("no_rts4_pf", "the register-broadcast smoother with a schedule per filter spills under its two-wavefronts-per-SIMD budget (or a DPP "
                                             "read follows the write of its source too closely): lane-group smoother instead")
      rts_pf_bad = [k for k in bad if k in ("k_rts<pf>", "k_rts_group<pf>")]
      if rts_pf_bad:
        # batch_rts is intact: the smoother with a schedule per filter alone is dropped ({name}_has_batch_rts_pf() == 0), before anything
        # below could answer for it with a fallback of the whole smoother
        usage, bad = fall_back("no_rts_pf", f"the smoother with a schedule per filter {rts_pf_bad} does not fit the register file: library without it")
      if "k_run_blk" in bad or "k_run_blk_tr" in bad:
        usage, bad = fall_back("no_run_blk", "a blocked fused run spills registers: the step-at-a-time k_run serves fused runs instead")
        for noise in reversed(NOISE_MODES):
          usage, bad = drop(noise)
      if bad and rn_emit.family(spec, ()) == "small":
        usage, bad = fall_back("force_wide", f"lane-per-filter kernels {bad} spill registers: regenerating in the lane-group family")
      if "k_rts4" in bad:
        usage, bad = fall_back("no_rts4", "the register-broadcast smoother spills under its two-wavefronts-per-SIMD budget (or a DPP read follows the write of its "
                                          "source too closely): lane-group smoother instead")
      if "k_run2_tri" in bad or "k_rts4_tri" in bad:
        usage, bad = fall_back("no_tri", "a packed-triangle trace kernel spills registers: library without batch_run_tri / batch_rts_tri")
      if "k_run2" in bad:
        usage, bad = fall_back("no_run2", "the two-wavefront fused run spills under its 256-register budget: the single-wavefront k_run instead")
      if "k_run" in bad and usage["k_run"]["scratch"] > 0 and rn_emit.family(spec, tuple(fallbacks)) == "wide":
        # whatever the state count: a lone wavefront pays about a microsecond per scratch access, and the rows of P live in registers
        # for the whole schedule.  BatchedEKF.run() then walks the schedule with the step-granular entry points.
        usage, bad = fall_back("no_run", "the fused run touches scratch memory: library without batch_run (step-granular entry points only)")
      heavy = [k for k in bad if usage[k]["vgpr_spill"] > 8 and not k.startswith(("k_rts", "k_run"))]
      if heavy and rn_tuning.model_defaults(spec):
        # the two-wavefronts-per-SIMD structure chosen for this model size does not fit 256 registers with this model's expressions
        usage, bad = fall_back("no_model_defaults", f"{heavy} spill under the per-model tuning defaults: regenerating with the general structure")
      rts_scratch = lambda: [k for k in bad if k.startswith("k_rts") and usage[k]["scratch"] > 0]      # noqa: E731
      if rts_scratch():
        usage, bad = fall_back("rts_one_wave", "the smoother spills under the two-wavefronts-per-SIMD register budget: one wavefront per SIMD")
      if rts_scratch():
        # the forward filter is intact: ship it without the smoother rather than no library at all (batch_rts is then absent and
        # BatchedEKF.rts_smooth raises KalmanError, as for any model without one)
        import warnings
        warnings.warn(f"{name}: smoother kernel {rts_scratch()} does not fit the register file (see {folder}/{name}.kernels.txt); "
                      f"lib{name}.so is built WITHOUT batch_rts", RuntimeWarning)
        usage, bad = fall_back("no_rts", "the smoother still touches scratch memory: library without batch_rts")
      kinds_bad = [k for k, u in usage.items() if k.startswith("k_kinds") and (u["scratch"] > 0 or u["vgpr_spill"] > 0)]
      if kinds_bad:
        # the per-kind step kernels are intact: a call that mixes kinds is then one `_masked` launch per kind ({name}_has_step_kinds() == 0)
        usage, bad = fall_back("no_kinds", f"the mixed-kind step kernel {kinds_bad} does not fit the register file: library without it")
    with open(stamp_fn, "w", encoding="utf-8") as f:
      f.write(digest)
  return spec


# =====================================================================================================
# single-filter orchestrator (host pointers; every numeric call is a batch-of-one launch on the GPU)
# =====================================================================================================
REWIND_TO_KEEP = 512   # /root/reference/rednose/helpers/ekf_sym.h:18, ekf_sym.py:446


def _solve(a, b):
  return b / a[0][0] if a.shape == (1, 1) else np.linalg.solve(a, b)


class EKF_sym:
  """One filter instance behind the reference's scalar C ABI.

  API and semantics follow the reference's pure-Python orchestrator
  (/root/reference/rednose/helpers/ekf_sym.py:220-690): `init_state`, `state`, `covs`,
  `get/set_filter_time`, `predict`, `predict_and_update_batch` (late observations are handled by rewind +
  fast-forward over a ring of 512 checkpoints, observations older than `max_rewind_age` are dropped
  and None is returned -- :464-482), `rewind` :418-438, `checkpoint` :440-450, `maha_test` :626-649,
  `rts_smooth` :651-690, `augment` :365-391.  Quaternion slices are renormalised after predict AND
  after every update, like the C++ orchestrator (ekf_sym.cc:207,213); the reference's Python class
  skips the post-predict one inside the batch path.

  The library it loads is whatever `{folder}/lib{name}.so` exports with that ABI.  A library generated by
  rednose_amd runs each call on the GPU and reports failures through `{name}_last_error`, which is
  checked after every call (KalmanError).  There is no CPU implementation in this package.
  """

  def __init__(self, folder, name, Q, x_initial, P_initial, dim_main, dim_main_err,  # pylint: disable=dangerous-default-value
               N=0, dim_augment=0, dim_augment_err=0, maha_test_kinds=[], quaternion_idxs=[], global_vars=None,
               max_rewind_age=1.0, logger=logging):
    self.name = name
    self.msckf = N > 0
    self.N = N
    self.dim_augment, self.dim_augment_err = dim_augment, dim_augment_err
    self.dim_main, self.dim_main_err = dim_main, dim_main_err
    self.logger = logger

    x_initial = np.asarray(x_initial, dtype=np.float64).reshape((-1, 1))
    self.dim_x = x_initial.shape[0]
    self.dim_err = P_initial.shape[0]
    assert dim_main + dim_augment * N == self.dim_x
    assert dim_main_err + dim_augment_err * N == self.dim_err
    assert Q.shape == P_initial.shape

    self.maha_test_kinds = list(maha_test_kinds)
    self.quaternion_idxs = list(quaternion_idxs)
    self.Q = np.ascontiguousarray(Q, dtype=np.float64)
    self.max_rewind_age = max_rewind_age
    self.init_state(x_initial, P_initial, None)

    self._ffi, self._lib = load_code(folder, name)
    self._check = getattr(self._lib, f"{name}_last_error", None)
    self._errstr = getattr(self._lib, f"{name}_last_error_string", None)
    self._clear = getattr(self._lib, f"{name}_clear_error", None)
    kinds, self.feature_track_kinds = [], []
    for sym in dir(self._lib):
      if sym.startswith(f"{name}_h_"):
        kinds.append(int(sym[len(name) + 3:]))
      if sym.startswith(f"{name}_He_"):
        self.feature_track_kinds.append(int(sym[len(name) + 4:]))
    self.kinds = sorted(kinds)

    self.f = self._wrap("f_fun", "vsv")
    self.F = self._wrap("F_fun", "vsv")
    self.err_function = self._wrap("err_fun", "vvv")
    self.inv_err_function = self._wrap("inv_err_fun", "vvv")
    self.H_mod = self._wrap("H_mod_fun", "vv")
    self.hs = {k: self._wrap(f"h_{k}", "vvv") for k in self.kinds}
    self.Hs = {k: self._wrap(f"H_{k}", "vvv") for k in self.kinds}
    self.Hes = {k: self._wrap(f"He_{k}", "vvv") for k in self.feature_track_kinds}
    self._predict_c = self._wrap("predict", "vvvs")
    self._updates = {k: self._wrap(f"update_{k}", "vvvvv") for k in self.kinds}
    self.set_globals = {}
    if global_vars is not None:
      for g in global_vars:
        self.set_globals[g] = getattr(self._lib, f"{name}_set_{g}")

  # -- library plumbing ---------------------------------------------------------------------------
  def _raise_if_failed(self, sym):
    if self._check is not None and self._check() != 0:
      msg = self._ffi.string(self._errstr()).decode() if self._errstr is not None else "library error"
      if self._clear is not None:
        self._clear()
      raise KalmanError(f"{self.name}_{sym}: {msg}")

  def _wrap(self, sym, sig):
    fn = getattr(self._lib, f"{self.name}_{sym}")
    ffi = self._ffi

    def call(*args):
      cargs = []
      for kind, a in zip(sig, args):
        if kind == "v":
          assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous, "float64 C-contiguous arrays only"
          cargs.append(ffi.cast("double *", a.ctypes.data))
        else:
          cargs.append(ffi.cast("double", a))
      fn(*cargs)
      self._raise_if_failed(sym)
    return call

  # -- state accessors ------------------------------------------------------------------------------
  def init_state(self, state, covs, filter_time):
    self.x = np.array(np.asarray(state).reshape((-1, 1)), dtype=np.float64)
    self.P = np.array(covs, dtype=np.float64)
    self.filter_time = filter_time
    self.augment_times = [0] * self.N
    self.reset_rewind()

  def reset_rewind(self):
    self.rewind_obscache = deque(maxlen=REWIND_TO_KEEP)
    self.rewind_t = deque(maxlen=REWIND_TO_KEEP)
    self.rewind_states = deque(maxlen=REWIND_TO_KEEP)

  def state(self):
    return np.array(self.x).flatten()

  def covs(self):
    return self.P

  def set_filter_time(self, t):
    self.filter_time = t

  def get_filter_time(self):
    return self.filter_time

  def get_augment_times(self):
    return self.augment_times

  def set_global(self, global_var, val):
    self.set_globals[global_var](val)

  def normalize_quaternions(self):
    for idx in self.quaternion_idxs:
      self.normalize_slice(idx, idx + 4)

  def normalize_slice(self, slice_start, slice_end_ex):
    self.x[slice_start:slice_end_ex] /= np.linalg.norm(self.x[slice_start:slice_end_ex])

  # -- MSCKF window shift (host-side bookkeeping only, ekf_sym.py:365-391) ----------------------------
  def augment(self):
    assert self.msckf
    d1, d2, d3, d4 = self.dim_main, self.dim_main_err, self.dim_augment, self.dim_augment_err
    self.x[d1:-d3] = self.x[d1 + d3:]
    self.x[-d3:] = self.x[:d3]
    keep = [i for i in range(self.dim_err) if not d2 <= i < d2 + d4]
    reduced = self.P[np.ix_(keep, keep)]
    lift = np.zeros((self.dim_err, self.dim_err - d4))
    lift[:-d4, :] = np.eye(self.dim_err - d4)
    lift[-d4:, :d4] = np.eye(d4)
    self.P = lift @ reduced @ lift.T
    self.augment_times = self.augment_times[1:] + [self.filter_time]

  # -- time bookkeeping, rewind ring -------------------------------------------------------------------
  def rewind(self, t):
    times = list(self.rewind_t)
    idx = bisect_right(times, t)
    assert times[idx - 1] <= t < times[idx]
    self.filter_time = times[idx - 1]
    self.x[:] = self.rewind_states[idx - 1][0]
    self.P[:] = self.rewind_states[idx - 1][1]
    replay = list(self.rewind_obscache)[idx:]
    for ring in (self.rewind_t, self.rewind_states, self.rewind_obscache):
      while len(ring) > idx:
        ring.pop()
    return replay

  def checkpoint(self, obs):
    self.rewind_t.append(self.filter_time)
    self.rewind_states.append((np.copy(self.x), np.copy(self.P)))
    self.rewind_obscache.append(obs)

  def _predict(self, x, P, dt):
    self._predict_c(x, P, self.Q, float(dt))
    return x, P

  def _update(self, x, P, kind, z, R, extra_args):
    if kind not in self._updates:
      raise KeyError(kind)
    self._updates[kind](x, P, z, R, extra_args)
    if self.msckf and kind in self.feature_track_kinds:
      return x, P, z[:-len(extra_args)]
    return x, P, z

  def predict(self, t):
    if self.filter_time is None:
      self.filter_time = t
    dt = t - self.filter_time
    assert dt >= 0
    self.x, self.P = self._predict(self.x, self.P, dt)
    self.normalize_quaternions()
    self.filter_time = t

  def predict_and_update_batch(self, t, kind, z, R, extra_args=[[]], augment=False):  # pylint: disable=dangerous-default-value
    replay = []
    if self.filter_time is not None and t < self.filter_time:
      if len(self.rewind_t) == 0 or t < self.rewind_t[0] or t < self.rewind_t[-1] - self.max_rewind_age:
        self.logger.error(f"observation too old at {t:.3f} with filter at {self.filter_time:.3f}, ignoring")
        return None
      replay = self.rewind(t)
    ret = self._predict_and_update_batch(t, kind, z, R, extra_args, augment)
    for obs in replay:
      self._predict_and_update_batch(*obs)
    return ret

  def _predict_and_update_batch(self, t, kind, z, R, extra_args, augment=False):
    """predict to t, then apply the n observations z[i] (n, dim_z) with noise R[i] sequentially (:484-531)."""
    z = np.asarray(z)
    R = np.asarray(R)
    assert z.shape[0] == R.shape[0] and z.shape[1] == R.shape[1] == R.shape[2]
    if len(extra_args) != len(z):
      extra_args = [[] for _ in range(len(z))] if len(extra_args) == 1 and len(extra_args[0]) == 0 else extra_args

    if self.filter_time is None:
      self.filter_time = t
    dt = t - self.filter_time
    assert dt >= 0
    self.x, self.P = self._predict(self.x, self.P, dt)
    self.normalize_quaternions()
    self.filter_time = t
    xk_km1, Pk_km1 = np.copy(self.x).flatten(), np.copy(self.P)

    y = []
    for i in range(len(z)):
      z_i = np.array(z[i], dtype=np.float64, order='C')
      R_i = np.array(R[i], dtype=np.float64, order='C')
      ea_i = np.array(extra_args[i], dtype=np.float64, order='C')
      if ea_i.size == 0:
        ea_i = np.zeros(1)
      self.x, self.P, y_i = self._update(self.x, self.P, kind, z_i, R_i, ea_i)
      self.normalize_quaternions()
      y.append(y_i)
    xk_k, Pk_k = np.copy(self.x).flatten(), np.copy(self.P)

    if augment:
      self.augment()
    self.checkpoint((t, kind, z, R, extra_args))
    return xk_km1, xk_k, Pk_km1, Pk_k, t, kind, y, z, extra_args

  # -- analysis tools -------------------------------------------------------------------------------
  def maha_test(self, x, P, kind, z, R, extra_args=[], maha_thresh=0.95):  # pylint: disable=dangerous-default-value
    """True when the observation passes the chi-square gate at `maha_thresh` (ekf_sym.py:626-649)."""
    z = np.asarray(z, dtype=np.float64).reshape((-1, 1))
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).flatten())
    ea = np.ascontiguousarray(extra_args, dtype=np.float64) if len(extra_args) else np.zeros(1)
    h = np.zeros(z.shape[0])
    H = np.zeros((z.shape[0], self.dim_x))
    self.hs[kind](x, ea, h)
    self.Hs[kind](x, ea, H)
    H_mod = np.zeros((self.dim_x, self.dim_err))
    self.H_mod(x, H_mod)
    y = z - h.reshape((-1, 1))
    He = H @ H_mod
    d2 = (y.T @ np.linalg.solve(He @ P @ He.T + R, y)).item()
    return not d2 > chi2_ppf(maha_thresh, y.shape[0])

  def rts_smooth(self, estimates, norm_quats=False):
    """Rauch-Tung-Striebel backward pass over the 9-tuples returned by predict_and_update_batch.

    Follows ekf_sym.py:651-690 step for step -- smoother gain on the main block
    Ck = (Pk1_k^-1 (F Pk_k^T))^T, error-state difference through inv_err_fun / err_fun -- but works
    on copies (the reference aliases and overwrites the caller's estimates).
    Returns (states (n, D), covs (n, E, E)) oldest first.
    """
    d1, d2 = self.dim_main, self.dim_main_err
    xk_n = np.array(estimates[-1][0], dtype=np.float64)
    Pk_n = np.array(estimates[-1][2], dtype=np.float64)
    Fk = np.zeros((self.dim_err, self.dim_err))
    out_x, out_P = [xk_n], [Pk_n]
    for k in range(len(estimates) - 2, -1, -1):
      xk1_n = xk_n
      if norm_quats:
        xk1_n[3:7] /= np.linalg.norm(xk1_n[3:7])
      Pk1_n = Pk_n
      xk1_k, Pk1_k, t2 = estimates[k + 1][0], estimates[k + 1][2], estimates[k + 1][4]
      xk_k, Pk_k, t1 = np.array(estimates[k][1], dtype=np.float64), np.array(estimates[k][3], dtype=np.float64), estimates[k][4]
      self.F(np.ascontiguousarray(xk_k), float(t2 - t1), Fk)
      Ck = np.linalg.solve(Pk1_k[:d2, :d2], Fk[:d2, :d2] @ Pk_k[:d2, :d2].T).T
      delta = np.zeros(self.dim_err)
      self.inv_err_function(np.ascontiguousarray(xk1_k, dtype=np.float64), np.ascontiguousarray(xk1_n), delta)
      delta[:d2] = Ck @ delta[:d2]
      x_new = np.zeros(self.dim_x)
      self.err_function(np.ascontiguousarray(xk_k), delta, x_new)
      xk_n = xk_k
      xk_n[:d1] = x_new[:d1]
      Pk_n = Pk_k
      Pk_n[:d2, :d2] = Pk_k[:d2, :d2] + Ck @ (Pk1_n[:d2, :d2] - Pk1_k[:d2, :d2]) @ Ck.T
      out_x.append(xk_n)
      out_P.append(Pk_n)
    return np.flipud(np.vstack(out_x)), np.stack(out_P, 0)[::-1]


# =====================================================================================================
# batched orchestrator: N independent filters resident in HBM
# =====================================================================================================
class BatchedEKF:
  """N independent filter instances of one model, state resident on one MI355X.

  The batch axis does not exist in the reference (its `predict_and_update_batch` applies n observations
  to ONE filter, ekf_sym.py:484-531); this class adds it behind the same vocabulary.  Layout is the
  natural batch of the reference's per-filter buffers: x (N, D), P (N, E, E) row-major fp64, contiguous.
  A call carries ONE observation kind; z is (N, Z) -- one observation per filter, R one shared (Z, Z) matrix or (N, Z, Z) -- or
  (N, n, Z): the reference's n observations per call (ekf_sym.py:512-524, ekf_sym.cc:172-180: ONE predict, n sequential updates,
  ONE checkpoint), R then (Z, Z), (n, Z, Z) or (N, n, Z, Z) and extra_args (n, EA) or (N, n, EA).  Two time models:
    * shared timeline (default): every call advances all filters to one time t;
    * per-filter timelines (per_filter=True, or the first call that passes a time vector / an `active` mask): every filter
      keeps its own filter_time, a call advances exactly the filters named by `active` to their own t[i], and -- with
      rewind_to_keep > 0 -- a late observation rewinds, applies and fast-forwards ONLY the filters it is late for, each
      through its own ring of checkpoints: N independent instances of the reference's orchestrator
      (/root/reference/rednose/helpers/ekf_sym.cc:83-156, ekf_sym.py:418-482), fed from N independent logs.
      A call in which no active filter is late -- the common one -- does its bookkeeping on the device (device_timeline: None = where
      the library exports {name}_batch_timeline_plan / _push, False = never, True = required, KalmanError otherwise): filter times
      and rings stay in HBM, the host reads one integer per call; `filter_time` is then the (N,) tensor the checkpoint kernel writes
      in place.  A call with a late filter takes the torch path on the same rings.  pf_stats counts the calls of either path.
      device_rewind=True (opt-in; needs the device timeline, {name}_batch_rewind_locate / _fetch and {name}_has_step_kinds() == 1,
      KalmanError otherwise) serves the late call on the device too: the rewind of every late filter in one launch, two integers read
      back, then per overtaken ring position one fetch, one mixed-kind step and one push.  Still on the torch path: ring entries or calls
      with several observations per filter, keep_estimate, libraries without the mixed-kind kernel (and the C++ orchestrator
      EKFSymBatch has no device rewind).  rewind_stats counts the late calls by the path that served them; one served on the device
      also counts as pf_stats["fast"].

  Compute goes through the generated library's `{name}_batch_*` entry points on the current torch HIP
  stream; torch is used only for device memory and streams.  No GPU / no library => KalmanError.
  """
  R_CACHE_ENTRIES = 16

  def __init__(self, folder, name, Q, x_initial, P_initial, dim_main, dim_main_err,  # pylint: disable=dangerous-default-value
               N=0, dim_augment=0, dim_augment_err=0, maha_test_kinds=[], quaternion_idxs=[], global_vars=None,
               max_rewind_age=1.0, logger=logging, batch=1, device=None, rewind_to_keep=0, per_filter=False, device_timeline=None,
               device_rewind=False):
    import torch  # pylint: disable=import-outside-toplevel
    if not torch.cuda.is_available():
      raise KalmanError("BatchedEKF needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
    self._torch = torch
    self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    self.name = name
    self.folder = folder
    self.batch = int(batch)
    self.logger = logger
    self.maha_test_kinds = list(maha_test_kinds)
    self.quaternion_idxs = list(quaternion_idxs)
    self.norm_quats = int(len(self.quaternion_idxs) > 0)
    self.max_rewind_age = max_rewind_age
    # Late-observation handling: the ring of (t, x, P, observation) checkpoints of the reference
    # (REWIND_TO_KEEP = 512, ekf_sym.h:18) held in HBM.  Off by default -- each checkpoint is a full copy of the
    # batch state (N * (D + E*E) * 8 bytes) -- enable with rewind_to_keep=512 for reference behaviour.
    self.rewind_to_keep = int(rewind_to_keep)
    self.per_filter = bool(per_filter)
    self._ring = None                  # per-filter checkpoint rings (allocated by the first per-filter step)
    self.msckf = N > 0
    self.N = N
    self.dim_main, self.dim_augment, self.dim_augment_err = dim_main, dim_augment, dim_augment_err
    self.augment_times = [0] * N
    self._augment_times_pf = None      # (N, n_window) per-filter shift times of run_logs (filter_augment_times())

    # always the ctypes binding: every argument below is a ctypes value (device pointers, stream handles, None), which a
    # cffi-dlopen'ed library would reject; EKF_sym keeps the reference's cffi-first loader for its host-pointer calls
    self._ffi, self._lib = load_code(folder, name, backend="ctypes")
    dims = (ctypes.c_int * 3)()
    getattr(self._lib, f"{name}_dims")(ctypes.cast(dims, ctypes.c_void_p))
    self.dim_x, self.dim_err, self.dim_main_err = int(dims[0]), int(dims[1]), int(dims[2])
    x_initial = np.asarray(x_initial, dtype=np.float64).reshape(-1)
    assert x_initial.shape[0] == self.dim_x and P_initial.shape == (self.dim_err, self.dim_err)
    assert np.asarray(Q).shape == (self.dim_err, self.dim_err)
    nk = getattr(self._lib, f"{name}_num_kinds")()
    kk = (ctypes.c_int * nk)()
    getattr(self._lib, f"{name}_kinds")(ctypes.cast(kk, ctypes.c_void_p))
    self.kinds = [int(k) for k in kk]
    self.zdims = {k: getattr(self._lib, f"{name}_kind_zdim")(k) for k in self.kinds}
    self.eadims = {k: getattr(self._lib, f"{name}_kind_eadim")(k) for k in self.kinds}
    md = (ctypes.c_int * 5)()
    getattr(self._lib, f"{name}_msckf_dims")(ctypes.cast(md, ctypes.c_void_p))
    if self.msckf and (dim_main, dim_main_err, dim_augment, dim_augment_err, N) != tuple(int(v) for v in md):
      raise KalmanError(f"library {name} was generated with msckf dims {tuple(md)}, constructor got "
                        f"{(dim_main, dim_main_err, dim_augment, dim_augment_err, N)}")
    lib_maha = [k for k in self.kinds if getattr(self._lib, f"{name}_kind_maha")(k) == 1]
    if sorted(lib_maha) != sorted(self.maha_test_kinds):
      raise KalmanError(f"library {name} was generated with maha_test_kinds={lib_maha}, constructor got {self.maha_test_kinds}")

    # Per-filter timelines: the in-order bookkeeping of a call (dt = t[i] - ft[i], the late test, the checkpoint) on the device, through
    # {name}_batch_timeline_plan / _push.  None: where the library has them; False: the torch bookkeeping always; True: required.
    self._device_timeline = self._has_timeline_abi() if device_timeline is None else bool(device_timeline)
    if self._device_timeline and not self._has_timeline_abi():
      raise KalmanError(f"device_timeline=True: lib{name}.so has no {name}_batch_timeline_plan / _push: regenerate it (gen_code) with this version of rednose_amd")
    self.pf_stats = {"fast": 0, "legacy": 0}      # per-filter calls served by the device timeline / by the torch bookkeeping (late observations: rewind)
    self._ft_dev = None                # the (N,) tensor of filter times k_timeline_push writes in place (== self.filter_time while it is current)
    self._tl = None                    # buffers of the device timeline (_timeline_buffers)
    # The late call on the device as well (opt-in): {name}_batch_rewind_locate / _fetch and the mixed-kind step replay the overtaken entries.
    self._device_rewind = bool(device_rewind)
    if self._device_rewind and not (self._device_timeline and self._has_rewind_abi() and self._has_step_kinds()):
      raise KalmanError(f"device_rewind=True needs the device timeline, {name}_batch_rewind_locate / _fetch and the mixed-kind step kernel "
                        f"({name}_has_step_kinds() == 1): lib{name}.so lacks one of them")
    self.rewind_stats = {"device": 0, "torch": 0}      # calls with a late filter, by the path that served them
    self._rw = None                    # buffers of the device rewind (_rewind_buffers)

    self.Q = torch.as_tensor(np.ascontiguousarray(Q, dtype=np.float64), device=self.device)
    self._R_cache = OrderedDict()          # small LRU of shared (Z, Z) noise matrices already on the device
    self.flags = torch.zeros(self.batch, dtype=torch.uint8, device=self.device)
    self.init_state(x_initial, P_initial, None)

  # -- plumbing -----------------------------------------------------------------------------------
  def _stream(self):
    return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

  def _call(self, sym, *args):
    rc = getattr(self._lib, f"{self.name}_{sym}")(*args)
    if rc != 0:
      msg = self._ffi.string(getattr(self._lib, f"{self.name}_last_error_string")()).decode()
      getattr(self._lib, f"{self.name}_clear_error")()
      raise KalmanError(f"{self.name}_{sym} -> {rc}: {msg}")

  @staticmethod
  def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None

  def _has_timeline_abi(self):
    return all(hasattr(self._lib, f"{self.name}_batch_timeline_{s}") for s in ("plan", "push"))

  def _has_rewind_abi(self):
    return all(hasattr(self._lib, f"{self.name}_batch_rewind_{s}") for s in ("locate", "fetch"))

  def _dev(self, a, shape=None):
    torch = self._torch
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
    t = t.to(device=self.device, dtype=torch.float64)
    if shape is not None:
      t = t.expand(shape)
    return t.contiguous()

  # -- state --------------------------------------------------------------------------------------
  def init_state(self, state, covs, filter_time):
    """state: (D,) or (N, D); covs: (E, E) or (N, E, E) -- broadcast over the batch."""
    self.x = self._dev(state, (self.batch, self.dim_x)).clone()
    self.P = self._dev(covs, (self.batch, self.dim_err, self.dim_err)).clone()
    if filter_time is not None and not np.isscalar(filter_time):
      filter_time = self._dev(filter_time, (self.batch,)).clone()     # (N,) per-filter times until the first step
    self.filter_time = filter_time
    self._ft_dev = None                # (the device timeline re-seeds its times from filter_time)
    self.reset_rewind()

  def reset_rewind(self):
    keep = self.rewind_to_keep if self.rewind_to_keep > 0 else 1
    self.rewind_t = deque(maxlen=keep)
    self.rewind_states = deque(maxlen=keep)
    self.rewind_obscache = deque(maxlen=keep)
    if getattr(self, "_ring", None) is not None:
      self._ring["length"].zero_()
      self._ring["head"].zero_()

  def state(self):
    return self.x.cpu().numpy()

  def covs(self):
    return self.P.cpu().numpy()

  def get_filter_time(self):
    return self.filter_time

  def set_filter_time(self, t):
    self.filter_time = t

  def set_global(self, global_var, val):
    """Run-time model scalar (gen_code's global_vars); like the reference it is per LIBRARY, shared by every filter."""
    getattr(self._lib, f"{self.name}_set_{global_var}")(float(val))
    if getattr(self._lib, f"{self.name}_last_error")() != 0:
      raise KalmanError(self._ffi.string(getattr(self._lib, f"{self.name}_last_error_string")()).decode())

  # -- hot path -------------------------------------------------------------------------------------
  def _dt(self, t):
    """Time step to `t`: a float when all filters share the filter time, an (N,) device tensor when the batch was
    initialised with per-filter times (init_state(..., filter_time=array)); after the step every filter is at t."""
    torch = self._torch
    if self.filter_time is None:
      self.filter_time = t
    if isinstance(self.filter_time, torch.Tensor):
      dt = torch.nan_to_num(float(t) - self.filter_time, nan=0.0)      # NaN: a filter that has not stepped yet adopts t (dt = 0)
      assert bool((dt >= 0).all()), "observation older than a filter's time"
      return dt
    dt = t - self.filter_time
    assert dt >= 0, "observation older than the filter time (enable rewind_to_keep to reorder late observations)"
    return float(dt)

  def _dt_args(self, dt):
    """-> (dt_vec pointer or None, scalar dt) for the C ABI."""
    if isinstance(dt, self._torch.Tensor):
      self._keepalive_dt = dt.contiguous()
      return self._p(self._keepalive_dt), 0.0
    return None, dt

  def predict(self, t, active=None):
    """Propagate to time t.  Per-filter timelines: t may be (N,) and `active` names the filters to propagate."""
    if self.per_filter or active is not None or not np.isscalar(t):
      torch = self._torch
      N = self.batch
      self.per_filter = True
      tt = (torch.full((N,), float(t), dtype=torch.float64, device=self.device) if np.isscalar(t) else self._dev(t, (N,)))
      act = (torch.ones(N, dtype=torch.bool, device=self.device) if active is None
             else torch.as_tensor(active, device=self.device).to(torch.bool).expand(N).clone())
      ft = self.filter_times()
      dt = torch.where(act, torch.nan_to_num(tt - ft, nan=0.0), torch.zeros_like(tt)).contiguous()
      assert bool((dt >= 0).all()), "predict: dt < 0 for a filter (ekf_sym.py:459)"
      au8 = act.to(torch.uint8)
      self._keepalive_masked = (dt, au8)
      self._call("batch_predict_masked", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt), 0.0, N, self.norm_quats,
                 self._p(au8), self._stream())
      self.filter_time = torch.where(act, tt, ft)
      return
    dt = self._dt(t)
    self.predict_dt(dt)
    self.filter_time = t

  def predict_dt(self, dt):
    """dt: python float (shared) or (N,) tensor / array (per filter)."""
    dt_vec, dt_s = (None, float(dt)) if np.isscalar(dt) else (self._dev(dt, (self.batch,)), 0.0)
    self._keepalive_dt = dt_vec
    self._call("batch_predict", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt_vec), dt_s,
               self.batch, self.norm_quats, self._stream())

  def _obs_args(self, kind, z, R):
    if kind not in self.zdims:
      raise KeyError(kind)
    Z = self.zdims[kind]
    z = self._dev(z, (self.batch, Z))
    if not isinstance(R, self._torch.Tensor):
      R = np.asarray(R, dtype=np.float64)
    if R.ndim == 3 and R.shape[0] == 1 and self.batch != 1:
      R = R[0]
    if R.ndim == 2:
      key = (kind, R.tobytes()) if isinstance(R, np.ndarray) else None
      Rd = self._R_cache.get(key) if key is not None else None
      if Rd is None:
        Rd = self._dev(R, (Z, Z))
        if key is not None:
          self._R_cache[key] = Rd
          while len(self._R_cache) > self.R_CACHE_ENTRIES:       # time-varying noise: bounded, oldest entry goes
            self._R_cache.popitem(last=False)
      elif key is not None:
        self._R_cache.move_to_end(key)
      return z, Rd, 0
    return z, self._dev(R, (self.batch, Z, Z)), 1

  def _ea(self, kind, extra_args):
    """Extra arguments of the observations (one row per filter, e.g. the landmark of a feature track) as an (N, EA)
    device tensor; None for kinds that take none."""
    EA = self.eadims.get(kind, 0)
    if EA == 0:
      return None
    if extra_args is None:
      raise KalmanError(f"kind {kind} takes {EA} extra arguments per observation")
    if not isinstance(extra_args, self._torch.Tensor):
      extra_args = np.asarray(extra_args, dtype=np.float64)
      if extra_args.ndim == 1:
        extra_args = np.tile(extra_args, (self.batch, 1))
    return self._dev(extra_args, (self.batch, EA))

  def update(self, kind, z, R, extra_args=None):
    """Update only (no time propagation).  Returns the residual y (N, Z) as a device tensor (feature-track kinds: the
    first Z - 3 columns hold the null-space projected residual, ekf_c.c:120)."""
    z, R, per = self._obs_args(kind, z, R)
    ea = self._ea(kind, extra_args)
    self._call(f"batch_update_{kind}", self._p(self.x), self._p(self.P), self._p(z), self._p(R), per, self._p(ea),
               self.batch, self.norm_quats, self._p(self.flags), self._stream())
    self._keepalive_ea = ea
    return z

  def augment(self):
    """Batched MSCKF window shift (EKF_sym.augment, ekf_sym.py:365-391) on every filter, in place on the GPU."""
    assert self.msckf
    self._call("batch_augment", self._p(self.x), self._p(self.P), self.batch, self._stream())
    self.augment_times = self.augment_times[1:] + [self.filter_time]

  def get_augment_times(self):
    return self.augment_times

  def predict_and_update_batch(self, t, kind, z, R, extra_args=None, augment=False, keep_estimate=False, active=None):
    """One fused predict(t - filter_time) + update(kind) launch over the whole batch.

    z: (N, Z) (numpy or device tensor; it is consumed -- the kernel overwrites it with the residual y, as the
    reference's update overwrites in_z, ekf_c.c:120).  keep_estimate=True splits the launch in two and
    returns the reference's 9-tuple (xk_km1, xk_k, Pk_km1, Pk_k, t, kind, y, z, extra_args) of device tensors.
    t: one time for all filters, or (N,) times; active: (N,) mask of the filters that have an observation in this call
    (default: all) -- either one switches the orchestrator to per-filter timelines (class docstring): filters that are not
    active pass through untouched (flag bit 4), late ones are rewound individually (rewind_to_keep > 0) or, when too old
    for their ring / max_rewind_age, ignored (flag bit 5, the reference's `return None`, ekf_sym.py:464-471).
    """
    if self.per_filter or active is not None or not np.isscalar(t):
      if not self.per_filter:
        if len(self.rewind_t) > 0 and self.rewind_to_keep > 0:
          raise KalmanError("this orchestrator already holds shared-timeline checkpoints: construct it with per_filter=True "
                            "(or reset_rewind()) before feeding per-filter times / masks")
        self.per_filter = True
      assert not augment, "augment on per-filter timelines is not supported (the reference asserts !augment with its ring, ekf_sym.cc:186)"
      return self._predict_and_update_per_filter(t, kind, z, R, extra_args, active, keep_estimate)
    if self.rewind_to_keep > 0:
      assert not augment, "augment with the rewind ring is not supported (the reference asserts the same, ekf_sym.cc:186)"
      return self._predict_and_update_with_rewind(t, kind, z, R, extra_args, keep_estimate)
    ret = self._apply(t, kind, z, R, extra_args, keep_estimate)
    if augment:
      self.augment()
    return ret

  def _apply(self, t, kind, z, R, extra_args, keep_estimate):
    """predict to t + the observation(s) of one call on the shared timeline: z (N, Z) one per filter, z (N, n, Z) n per filter."""
    if getattr(z, "ndim", None) == 3 or (not hasattr(z, "ndim") and np.ndim(z) == 3):
      return self._predict_and_update_multi(t, kind, z, R, extra_args, keep_estimate)
    return self._predict_and_update(t, kind, z, R, extra_args, keep_estimate)

  # -- n observations per call (the reference's predict_and_update_batch proper) ---------------------
  multi_obs_fused = None      # None: one batch_run launch where the library allows it (see _predict_and_update_multi); False: step-granular launches

  def _multi_obs(self, kind, z, R, extra_args):
    """The n observations of one call in canonical form: zl = n device tensors (N, Z), each in its own allocation (the kernels want
    16-byte aligned rows and overwrite them with the residuals), Rl = n device noise matrices ((Z, Z) shared by the filters or
    (N, Z, Z)), per = 1 for per-filter noise, eal = n (N, EA) tensors or Nones.  Shapes accepted: z (N, n, Z) [or (1, n, Z): the same
    observations for every filter]; R (Z, Z) | (n, Z, Z) | (N, n, Z, Z) -- the reference passes (n, Z, Z), KalmanFilter.get_R(kind, n);
    extra_args (n, EA) | (N, n, EA)."""
    torch = self._torch
    if kind not in self.zdims:
      raise KeyError(kind)
    N, Z, EA = self.batch, self.zdims[kind], self.eadims.get(kind, 0)
    zt = z if isinstance(z, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64))
    if zt.ndim != 3 or zt.shape[0] not in (1, N) or zt.shape[2] != Z:
      raise KalmanError(f"n observations per call: z must be (N, n, {Z}) for kind {kind}, got {tuple(zt.shape)}")
    n = int(zt.shape[1])
    if n == 0:
      return [], [], 0, []
    zt = zt.to(device=self.device, dtype=torch.float64).expand(N, n, Z)
    Rt = R if isinstance(R, torch.Tensor) else np.asarray(R, dtype=np.float64)
    if Rt.ndim == 2:
      Rj = [Rt] * n
    elif Rt.ndim == 3:
      if Rt.shape[0] != n:
        raise KalmanError(f"n observations per call: a 3-D R is (n, Z, Z) -- one matrix per observation, like the reference's -- got {tuple(Rt.shape)} for n = {n}")
      Rj = [Rt[j] for j in range(n)]
    elif Rt.ndim == 4:
      if tuple(Rt.shape[:2]) != (N, n):
        raise KalmanError(f"n observations per call: a 4-D R is (N, n, Z, Z), got {tuple(Rt.shape)}")
      Rj = [Rt[:, j] for j in range(n)]
    else:
      raise KalmanError(f"R: unexpected shape {tuple(Rt.shape)}")
    zl, Rl, pers = [], [], set()
    for j in range(n):
      zj = zt[:, j].contiguous()
      if zj.data_ptr() == zt.data_ptr() and n > 1:      # (cannot happen for n > 1; for n == 1 the caller's tensor is consumed like a 2-D z)
        zj = zj.clone()
      zj, Rd, per = self._obs_args(kind, zj, Rj[j])
      zl.append(zj)
      Rl.append(Rd)
      pers.add(per)
    assert len(pers) == 1
    if EA == 0:
      eal = [None] * n
    else:
      if extra_args is None:
        raise KalmanError(f"kind {kind} takes {EA} extra arguments per observation")
      ea = extra_args if isinstance(extra_args, torch.Tensor) else np.asarray(extra_args, dtype=np.float64)
      if ea.ndim == 2 and tuple(ea.shape) == (n, EA):
        eal = [self._ea(kind, ea[j]) for j in range(n)]
      elif ea.ndim == 3 and tuple(ea.shape) == (N, n, EA):
        eal = [self._ea(kind, ea[:, j]) for j in range(n)]
      else:
        raise KalmanError(f"n observations per call: extra_args must be ({n}, {EA}) or ({N}, {n}, {EA}), got {tuple(ea.shape)}")
    return zl, Rl, pers.pop(), eal

  def _identity_dt0(self):
    fn = getattr(self._lib, f"{self.name}_predict_identity_at_dt0", None)
    return bool(fn()) if fn is not None else False

  def _predict_and_update_multi(self, t, kind, z, R, extra_args, keep_estimate):
    """EKFSym::predict_and_update_batch with n observations (ekf_sym.cc:158-194, ekf_sym.py:484-531) for every filter of the batch: ONE
    predict to t, then the n observations z[:, i] applied in order (quaternions renormalised after each, :521), one Estimate.

    Served by ONE batch_run launch -- a schedule of n steps of this kind with dts = (dt, 0, ..., 0), x and P on chip between the
    updates -- when the noise is shared by the filters, the library has the fused run and its predict(dt = 0) is the identity
    ({name}_predict_identity_at_dt0: the fused run predicts on every step, the reference only once); otherwise by one fused
    predict + update launch and n - 1 batch_update launches.  (batch_run reads (P + P^T) / 2: include/rednose_amd_filter.h;
    multi_obs_fused = False keeps the step-granular launches, the reference's arithmetic on any P.)
    Returns y (N, n, Z), or with keep_estimate the reference's 9-tuple with y a list of n (N, Z) tensors and z (N, n, Z)."""
    torch = self._torch
    zl, Rl, per, eal = self._multi_obs(kind, z, R, extra_args)
    n, N, Z = len(zl), self.batch, self.zdims[kind]
    dt = self._dt(t)
    if n == 0:              # no observations: the reference's loop body never runs -- a predict and a checkpoint
      self.predict_dt(dt)
      self.filter_time = t
      y = torch.empty((N, 0, Z), dtype=torch.float64, device=self.device)
      return (self.x.clone(), self.x.clone(), self.P.clone(), self.P.clone(), t, kind, [], y, extra_args) if keep_estimate else y
    z_orig = torch.stack(zl, 1) if keep_estimate else None
    fl = torch.zeros((n, N), dtype=torch.uint8, device=self.device)
    xk_km1 = Pk_km1 = None
    if keep_estimate:
      self.predict_dt(dt)
      xk_km1, Pk_km1 = self.x.clone(), self.P.clone()
    can_fuse = (per == 0 and not isinstance(dt, torch.Tensor) and n > 1 and self._has_batch_run() and self._identity_dt0())
    fused = can_fuse if self.multi_obs_fused is None else (bool(self.multi_obs_fused) and can_fuse)
    if fused:
      zmax = getattr(self._lib, f"{self.name}_zmax")()
      zs = torch.zeros((n, N, zmax), dtype=torch.float64, device=self.device)
      zs[:, :, :Z] = torch.stack(zl, 0)
      table = torch.zeros((n, zmax * zmax), dtype=torch.float64, device=self.device)
      table[:, :Z * Z] = torch.stack([r_.reshape(-1) for r_ in Rl], 0)
      kd = torch.full((n,), int(kind), dtype=torch.int32, device=self.device)
      dd = torch.zeros(n, dtype=torch.float64, device=self.device)
      if not keep_estimate:
        dd[0] = float(dt)
      ead = max(list(self.eadims.values()) + [0])
      ea = None
      if eal[0] is not None:
        ea = torch.zeros((n, N, ead), dtype=torch.float64, device=self.device)
        ea[:, :, :eal[0].shape[1]] = torch.stack(eal, 0)
      self._call("batch_run", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(kd), self._p(dd), n, self._p(zs), self._p(table), N,
                 self.norm_quats, self._p(fl), None, None, self._p(ea), None, self._stream())
      self._keepalive_multi = (kd, dd, table, ea, zs)
      y = zs[:, :, :Z].permute(1, 0, 2).contiguous()
    else:
      dt_ptr, dt_s = self._dt_args(dt)
      for j in range(n):
        if j == 0 and not keep_estimate:
          self._call(f"batch_predict_update_{kind}", self._p(self.x), self._p(self.P), self._p(self.Q), dt_ptr, dt_s, self._p(zl[0]), self._p(Rl[0]), per,
                     self._p(eal[0]), N, self.norm_quats, self._p(fl[0]), self._stream())
        else:
          self._call(f"batch_update_{kind}", self._p(self.x), self._p(self.P), self._p(zl[j]), self._p(Rl[j]), per, self._p(eal[j]), N, self.norm_quats,
                     self._p(fl[j]), self._stream())
      self._keepalive_multi = (zl, Rl, eal)
      y = torch.stack(zl, 1)
    self.filter_time = t
    self.flags.copy_(fl[n - 1])      # flags: the last observation's, as after n single-observation calls; flags_obs: all of them
    self.flags_obs = fl.t()
    if keep_estimate:
      return xk_km1, self.x.clone(), Pk_km1, self.P.clone(), t, kind, list(y.unbind(1)), z_orig, extra_args
    return y

  # -- per-filter timelines -------------------------------------------------------------------
  def filter_times(self):
    """(N,) device tensor of the filters' times (NaN: not started), whichever time model is in use."""
    torch = self._torch
    ft = self.filter_time
    if isinstance(ft, torch.Tensor):
      return ft
    return torch.full((self.batch,), float("nan") if ft is None else float(ft), dtype=torch.float64, device=self.device)

  def _masked_step(self, kind, zl, Rl, per, eal, dt, act_u8, keep_estimate=False, nobs=None):
    """The observation(s) of one call for the filters with act_u8 != 0 only; dt: (N,) device tensor.  zl / Rl / eal: lists of n (one
    entry per observation of the call: _multi_obs; a single observation is n = 1).  ONE predict -- fused with the first update unless
    the Estimate's predicted pair is wanted -- then the remaining updates as update-only launches (never a predict(0): it is not the
    identity for every model).  nobs (N,) int tensor: filter i has only its first nobs[i] observations (replayed ring entries of
    different calls); None: all n."""
    torch = self._torch
    dt = dt.contiguous()
    keep = [dt, act_u8]
    est = None

    def obs_args(j, a8):
      keep.extend((zl[j], Rl[j], eal[j], a8))
      return (self._p(zl[j]), self._p(Rl[j]), per, self._p(eal[j]), self.batch, self.norm_quats, self._p(self.flags), self._p(a8), self._stream())
    if keep_estimate:
      self._call("batch_predict_masked", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt), 0.0, self.batch, self.norm_quats,
                 self._p(act_u8), self._stream())
      est = (self.x.clone(), self.P.clone())
    for j in range(len(zl)):
      a8 = act_u8 if nobs is None else (act_u8 * (nobs > j).to(torch.uint8))
      if j > 0 and nobs is not None:
        fl_old = self.flags.clone()
      if j == 0 and not keep_estimate:
        self._call(f"batch_predict_update_{kind}_masked", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt), 0.0, *obs_args(j, a8))
      else:
        self._call(f"batch_update_{kind}_masked", self._p(self.x), self._p(self.P), *obs_args(j, a8))
      if j > 0 and nobs is not None:      # a filter with fewer observations keeps the flags of its last one (the launch wrote "not active" for it)
        self.flags.copy_(torch.where(a8 != 0, self.flags, fl_old))
    self._keepalive_masked = keep
    return est

  def _predict_and_update_per_filter(self, t, kind, z, R, extra_args, active, keep_estimate=False):
    torch = self._torch
    N = self.batch
    if kind not in self.zdims:
      raise KeyError(kind)
    if not hasattr(self._lib, f"{self.name}_batch_predict_update_{kind}_masked"):
      raise KalmanError(f"lib{self.name}.so has no masked entry points: regenerate it (gen_code) with this version of rednose_amd")
    multi = (z.ndim if hasattr(z, "ndim") else np.ndim(z)) == 3      # (N, n, Z): n observations per filter in this call
    if multi:
      zl, Rl, per, eal = self._multi_obs(kind, z, R, extra_args)
      if not zl:
        raise KalmanError("per-filter timelines: a call needs at least one observation per filter (use predict(t, active) to propagate only)")
    else:
      zin, Rd, per = self._obs_args(kind, z, R)
      if isinstance(z, torch.Tensor) and zin.data_ptr() == z.data_ptr() and keep_estimate:
        zin = zin.clone()
      zl, Rl, eal = [zin], [Rd], [self._ea(kind, extra_args)]
    if self._device_timeline:
      ret = self._timeline_call(t, active, kind, zl, Rl, per, eal, multi, keep_estimate, extra_args)
      if ret is not None:
        self.pf_stats["fast"] += 1
        return ret[0]
      t, active = self._keepalive_timeline[0], (None if active is None else self._keepalive_timeline[1])      # (on the device already)
    self.pf_stats["legacy"] += 1
    tt = (torch.full((N,), float(t), dtype=torch.float64, device=self.device) if np.isscalar(t) else self._dev(t, (N,)))
    act = (torch.ones(N, dtype=torch.bool, device=self.device) if active is None
           else torch.as_tensor(active, device=self.device).to(torch.bool).expand(N).clone())
    z_obs = [zj.clone() for zj in zl] if (self.rewind_to_keep > 0 or keep_estimate) else None       # the kernels overwrite z with the residuals
    ft = self.filter_times()
    self.filter_time = ft
    late = act & ~torch.isnan(ft) & (tt < ft)
    dropped, any_dropped = None, False
    replay = None
    if bool(late.any()):                   # (the one host round trip of an in-order call: whether any filter has to rewind decides what is launched)
      if self.rewind_to_keep <= 0:
        raise AssertionError("observation older than a filter's time (enable rewind_to_keep to reorder late observations)")
      self.rewind_stats["torch"] += 1
      dropped, replay = self._ring_rewind(late, tt)
      any_dropped = bool(dropped.any())
      if any_dropped:
        self.logger.error(f"observation too old for {int(dropped.sum())} filter(s) of the batch, ignoring it for them")
        act = act & ~dropped
      ft = self.filter_time
    dt = torch.where(act, torch.nan_to_num(tt - ft, nan=0.0), torch.zeros_like(tt))
    est = self._masked_step(kind, zl, Rl, per, eal, dt, act.to(torch.uint8), keep_estimate)
    self.filter_time = torch.where(act, tt, ft)
    if self.rewind_to_keep > 0:
      self._ring_push(act, self.filter_time, kind, z_obs, Rl, per, eal)
    # The Estimate is the state right after THIS call's observations -- the reference captures `ret` before it fast-forwards over the
    # observations the rewind overtook (ekf_sym.py:473-479) -- and the flags the caller reads are this call's too: the
    # replay launches write the replayed (older) observations' flags into the same buffer.
    xk_k, Pk_k = (self.x.clone(), self.P.clone()) if keep_estimate else (None, None)
    if replay is not None:
      fl_new = self.flags.clone()
      self._ring_replay(replay)
      self.flags.copy_(fl_new)        # (into the SAME buffer: bind_step() captured its address)
    if any_dropped:
      self.flags |= dropped.to(torch.uint8) * 32
    if multi:
      y = torch.stack(zl, 1)
      if keep_estimate:
        return est[0], xk_k, est[1], Pk_k, tt, kind, list(y.unbind(1)), torch.stack(z_obs, 1), extra_args
      return y
    if keep_estimate:
      return est[0], xk_k, est[1], Pk_k, tt, kind, zl[0], z_obs[0], extra_args
    return zl[0]

  # -- a kind per filter in one call ---------------------------------------------------------------------------------
  def _has_step_kinds(self):
    fn = getattr(self._lib, f"{self.name}_has_step_kinds", None)
    return fn is not None and int(fn()) == 1

  def predict_and_update_kinds(self, t, kinds, z, R, active=None):
    """One call on per-filter timelines in which every filter brings its OWN observation kind (what N independent EKFSym instances do at a tick:
    `updates.at(kind)`, ekf_sym.cc:196-219).  kinds: (N,) ints, an entry <= 0 = no observation for that filter in this call; z: (N, zmax), the
    first Z of a row are that filter's observation (consumed: overwritten by the residual, the rest of the row passes through); R: a dict
    {kind: (Z, Z)} shared by the filters of a kind, or (N, zmax, zmax) per filter (leading Z x Z block); t / active as predict_and_update_batch.
    Returns the (N, zmax) residuals.

    In order, with the library's mixed-kind kernel: batch_timeline_plan -> one integer read back -> batch_predict_update_kinds (ONE launch,
    the state crosses HBM once whatever the mix) -> batch_timeline_push_kinds; the ring entries are those the per-kind calls write.  With a late
    filter in the call, or a library without the kernel ({name}_has_step_kinds() == 0): one predict_and_update_batch(active = kinds == k) per
    kind present, late observations rewinding as ever."""
    torch = self._torch
    N, zmax = self.batch, max(self.zdims.values())
    if not self.per_filter:
      if len(self.rewind_t) > 0 and self.rewind_to_keep > 0:
        raise KalmanError("this orchestrator already holds shared-timeline checkpoints: construct it with per_filter=True")
      self.per_filter = True
    if not self._device_timeline:
      raise KalmanError("predict_and_update_kinds needs the device timeline (device_timeline=True and a library with batch_timeline_plan / _push)")
    if isinstance(kinds, torch.Tensor) and kinds.is_cuda:
      # kinds that live on the device already: which are present is one more read back (a sort + a wait) in front of the plan -- hand in
      # a numpy array or a list to keep the call at one integer
      kd = kinds.to(device=self.device, dtype=torch.int32).expand(N).contiguous()
      present = [int(k) for k in torch.unique(kd).tolist() if int(k) > 0]
    else:
      kh = np.broadcast_to(np.asarray(kinds.numpy() if isinstance(kinds, torch.Tensor) else kinds).astype(np.int32), (N,))
      present = [int(k) for k in np.unique(kh) if int(k) > 0]       # (on the host, before the upload: the kinds decide what is launched)
      kd = torch.as_tensor(np.ascontiguousarray(kh)).to(self.device)
    for k in present:
      if k not in self.zdims:
        raise KeyError(k)
    zt = z if isinstance(z, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64))
    zt = zt.to(device=self.device, dtype=torch.float64)
    if tuple(zt.shape) != (N, zmax):
      raise KalmanError(f"predict_and_update_kinds: z must be (N, zmax) = ({N}, {zmax}), got {tuple(zt.shape)}")
    zt = zt.contiguous()
    if isinstance(R, dict):
      key = ("kinds",) + tuple((k, np.asarray(R[k], dtype=np.float64).tobytes()) for k in sorted(R))
      Rd = self._R_cache.get(key)
      if Rd is None:
        tab = np.zeros((len(self.kinds), zmax * zmax))
        for i, k in enumerate(self.kinds):
          if k in R:
            Z = self.zdims[k]
            tab[i, :Z * Z] = np.asarray(R[k], dtype=np.float64).reshape(Z * Z)
        Rd = self._R_cache[key] = self._dev(tab)
        while len(self._R_cache) > self.R_CACHE_ENTRIES:
          self._R_cache.popitem(last=False)
      for k in present:
        if k not in R:
          raise KeyError(k)
      per = 0
    else:
      Rfull = self._dev(R, (N, zmax, zmax))
      Zf = torch.zeros(N, dtype=torch.int64, device=self.device)
      for k in present:
        Zf[kd == k] = self.zdims[k]
      # leading Z x Z block of every filter, compact and row-major in front of its row (the convention of batch_run)
      Rd = torch.zeros((N, zmax * zmax), dtype=torch.float64, device=self.device)
      for k in present:
        Z, m = self.zdims[k], kd == k
        Rd[m, :Z * Z] = Rfull[m][:, :Z, :Z].reshape(-1, Z * Z)
      per = 1
    has = kd > 0
    if active is not None:
      has = has & torch.as_tensor(active, device=self.device).to(torch.bool).expand(N)
    if self._has_step_kinds():
      ret = self._timeline_call_kinds(t, has, kd, zt, Rd, per)
      if ret is not None:
        self.pf_stats["fast"] += 1
        return ret
      t = self._keepalive_timeline[0]
    # the per-kind path: a filter is late, or the library has no mixed-kind kernel
    self.pf_stats["legacy"] += 1
    fl = torch.full((N,), 16, dtype=torch.uint8, device=self.device)
    stats, rw_stats = dict(self.pf_stats), dict(self.rewind_stats)
    for k in present:
      Z, m = self.zdims[k], has & (kd == k)
      zk = zt[:, :Z].contiguous()
      Rk = (Rd[self.kinds.index(k), :Z * Z].reshape(Z, Z) if not per else Rd[:, :Z * Z].reshape(N, Z, Z).contiguous())
      if per:
        Rk = torch.where(m[:, None, None], Rk, torch.eye(Z, dtype=torch.float64, device=self.device))      # (filters of other kinds: any regular matrix)
      y = self.predict_and_update_batch(t, k, zk, Rk, active=m)
      zt[:, :Z] = torch.where(m[:, None], y, zt[:, :Z])
      fl = torch.where(m, self.flags, fl)
    self.pf_stats = stats
    if sum(self.rewind_stats.values()) > sum(rw_stats.values()):      # one late call, however many per-kind calls served it
      rw_stats["torch"] += 1
    self.rewind_stats = rw_stats
    self.flags.copy_(fl)
    return zt

  def _timeline_call_kinds(self, t, has, kd, zt, Rd, per):
    """_timeline_call for a kind per filter: plan, the count of late filters read back, ONE mixed-kind step, the checkpoint.  None (nothing
    modified) when a filter is late."""
    torch = self._torch
    N, K, zmax = self.batch, max(self.rewind_to_keep, 0), max(self.zdims.values())
    if isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float64 and tuple(t.shape) == (N,) and t.is_contiguous():
      tt = t
    else:
      tt = torch.full((N,), float(t), dtype=torch.float64, device=self.device) if np.isscalar(t) else self._dev(t, (N,))
    a8 = has.view(torch.uint8).contiguous()
    ft = self.filter_time
    if ft is None or ft is not self._ft_dev:
      ft = self.filter_times()
      ft = ft.contiguous().clone() if ft is self.filter_time else ft
      self._ft_dev = self.filter_time = ft
    copy_z = K > 0
    b = self._timeline_buffers(N * zmax if copy_z else 0)
    self._call("batch_timeline_plan", self._p(tt), self._p(a8), self._p(ft), N, self._p(b["dt"]), self._p(b["act"]), self._p(b["late"]),
               self._p(b["n_late"]), self._p(zt) if copy_z else None, self._p(b["z_keep"]) if copy_z else None, N * zmax if copy_z else 0, self._stream())
    b["host"].copy_(b["n_late"], non_blocking=True)
    torch.cuda.current_stream(self.device).synchronize()
    count = int(b["host_np"][0])
    late, b["seen"] = count != b["seen"], count
    self._keepalive_timeline = (tt, a8, kd, zt, Rd)
    rewound = None
    if late:
      if not self._rewind_on_device(True, False):
        return None
      rewound = self._rewind_locate(tt, ft, b)
    self._call("batch_predict_update_kinds", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(b["dt"]), 0.0, self._p(kd), self._p(zt), self._p(Rd), per,
               N, self.norm_quats, self._p(self.flags), self._p(b["act"]), self._stream())
    if K > 0:
      if self._ring is None:
        self._ring_alloc(1)
      r = self._ring
      self._call("batch_timeline_push_kinds", self._p(tt), self._p(b["act"]), self._p(ft), self._p(self.x), self._p(self.P), N, K, r["nmax"],
                 self._p(r["t"]), self._p(r["x"]), self._p(r["P"]), self._p(r["kind"]), self._p(r["nobs"]), self._p(r["z"]), self._p(r["R"]), self._p(r["ea"]),
                 self._p(r["head"]), self._p(r["length"]), self._p(kd), self._p(b["z_keep"]), self._p(Rd), per, self._stream())
    else:
      self._call("batch_timeline_push_kinds", self._p(tt), self._p(b["act"]), self._p(ft), None, None, N, 0, 0, None, None, None, None, None, None, None, None,
                 None, None, self._p(kd), None, None, 0, self._stream())
    if rewound is not None:
      self._rewind_replay(*rewound)
    return zt

  # -- the in-order call with its bookkeeping on the device ----------------------------------------------------------
  # The checkpoint wants the observation as it came and the step overwrites it: True = k_timeline_plan copies it aside (no launch of its
  # own, a buffer kept from call to call), False = a clone() in front of the step.  Timed by tools/pf_device_timeline_time.py
  # (profiles/pf_device_timeline_call_times.txt).
  timeline_plan_copies_z = True

  def _timeline_buffers(self, zdoubles):
    """What k_timeline_plan writes, kept from call to call (every launch that reads them is on this stream, in front of the next plan):
    dt (N,), act / late (N,) bytes, the count of late filters -- on the device, and the pinned word it is copied to -- and z_keep, the
    observation of a single-observation call as it came."""
    torch = self._torch
    N, stream = self.batch, self._torch.cuda.current_stream(self.device).cuda_stream
    b = self._tl
    if b is None or b["stream"] != stream:
      b = self._tl = dict(stream=stream, dt=torch.empty(N, dtype=torch.float64, device=self.device),
                          act=torch.empty(N, dtype=torch.uint8, device=self.device), late=torch.empty(N, dtype=torch.uint8, device=self.device),
                          n_late=torch.zeros(1, dtype=torch.int32, device=self.device), host=torch.zeros(1, dtype=torch.int32).pin_memory(),
                          seen=0, z_keep=None)
      b["host_np"] = b["host"].numpy()
    if zdoubles and (b["z_keep"] is None or b["z_keep"].numel() < zdoubles):
      b["z_keep"] = torch.empty(zdoubles, dtype=torch.float64, device=self.device)
    return b

  def _timeline_call(self, t, active, kind, zl, Rl, per, eal, multi, keep_estimate, extra_args):
    """One call on per-filter timelines with no late observation, the bookkeeping in two launches around the step: batch_timeline_plan
    (dt, who steps, who is late; include/rednose_amd_filter.h), the count of late filters read back -- the call's one host round trip
    -- the `_masked` step with the plan's outputs, batch_timeline_push (ft and the checkpoint).  -> (result,), or None with NOTHING
    modified when a filter is late: the caller then takes the torch path, whose rewind works on the same rings."""
    torch = self._torch
    N, K, n, Z = self.batch, max(self.rewind_to_keep, 0), len(zl), self.zdims[kind]
    f64 = dict(dtype=torch.float64, device=self.device)
    if isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == torch.float64 and tuple(t.shape) == (N,) and t.is_contiguous():
      tt = t
    else:
      tt = torch.full((N,), float(t), **f64) if np.isscalar(t) else self._dev(t, (N,))
    a8 = None
    if active is not None:
      a8 = torch.as_tensor(active, device=self.device)
      a8 = (a8.view(torch.uint8) if a8.dtype == torch.bool else a8.to(torch.bool).view(torch.uint8)).expand(N).contiguous()
    ft = self.filter_time
    if ft is None or ft is not self._ft_dev:        # (re-)seeded: init_state, set_filter_time, a call the torch path served
      ft = self.filter_times()
      ft = ft.contiguous().clone() if ft is self.filter_time else ft
      self._ft_dev = self.filter_time = ft
    copy_z = self.timeline_plan_copies_z and K > 0 and not multi and not keep_estimate
    b = self._timeline_buffers(N * Z if copy_z else 0)
    self._call("batch_timeline_plan", self._p(tt), self._p(a8), self._p(ft), N, self._p(b["dt"]), self._p(b["act"]), self._p(b["late"]),
               self._p(b["n_late"]), self._p(zl[0]) if copy_z else None, self._p(b["z_keep"]) if copy_z else None, N * Z if copy_z else 0, self._stream())
    b["host"].copy_(b["n_late"], non_blocking=True)
    torch.cuda.current_stream(self.device).synchronize()
    count = int(b["host_np"][0])
    late, b["seen"] = count != b["seen"], count        # (the counter accumulates)
    rewound = None
    if late:
      if not self._rewind_on_device(not multi, keep_estimate):
        self._keepalive_timeline = (tt, a8)
        return None
      rewound = self._rewind_locate(tt, ft, b)
    z_obs = None
    if copy_z:
      z_keep, z_sf, z_so = b["z_keep"], Z, 0
    elif K > 0 or keep_estimate:
      z_obs = [zj.clone() for zj in zl]                # the kernels overwrite z with the residuals
      z_keep, z_sf, z_so = (torch.stack(z_obs, 1), n * Z, Z) if n > 1 else (z_obs[0], Z, 0)
    est = self._masked_step(kind, zl, Rl, per, eal, b["dt"], b["act"], keep_estimate)
    if K > 0:
      if self._ring is None or self._ring["nmax"] < n:
        self._ring_alloc(n)
      r = self._ring
      Rk, r_so = (torch.stack(Rl, 0), (N * Z * Z if per else Z * Z)) if n > 1 else (Rl[0], 0)
      EA = self.eadims.get(kind, 0)
      eak, ea_so = (None, 0) if EA == 0 else ((torch.stack(eal, 0), N * EA) if n > 1 else (eal[0], 0))
      self._call("batch_timeline_push", self._p(tt), self._p(b["act"]), self._p(ft), self._p(self.x), self._p(self.P), N, K, r["nmax"],
                 self._p(r["t"]), self._p(r["x"]), self._p(r["P"]), self._p(r["kind"]), self._p(r["nobs"]), self._p(r["z"]), self._p(r["R"]), self._p(r["ea"]),
                 self._p(r["head"]), self._p(r["length"]), int(kind), n, self._p(z_keep), z_sf, z_so, self._p(Rk), per, Z * Z, r_so,
                 self._p(eak), EA, ea_so, self._stream())
      self._keepalive_timeline = (tt, a8, z_keep, Rk, eak)
      if rewound is not None:
        self._rewind_replay(*rewound)
    else:
      self._call("batch_timeline_push", self._p(tt), self._p(b["act"]), self._p(ft), None, None, N, 0, 0, None, None, None, None, None, None, None, None,
                 None, None, int(kind), n, None, 0, 0, None, 0, 0, 0, None, 0, 0, self._stream())
      self._keepalive_timeline = (tt, a8)
    if not keep_estimate:
      return (torch.stack(zl, 1) if multi else zl[0],)
    xk_k, Pk_k = self.x.clone(), self.P.clone()
    if multi:
      return ((est[0], xk_k, est[1], Pk_k, tt, kind, list(torch.stack(zl, 1).unbind(1)), torch.stack(z_obs, 1), extra_args),)
    return ((est[0], xk_k, est[1], Pk_k, tt, kind, zl[0], z_obs[0], extra_args),)

  # -- the late call on the device (device_rewind=True) ----------------------------------------------------------------
  def _rewind_on_device(self, single, keep_estimate):
    """Does the device serve this late call?  One observation per filter in the call and in every ring entry (the replay is one mixed-kind
    step per position), no Estimate wanted.  Anything else: the torch path, on the same rings."""
    return (self._device_rewind and self.rewind_to_keep > 0 and single and not keep_estimate and
            (self._ring is None or self._ring["nmax"] == 1))

  def _rewind_buffers(self):
    """What batch_rewind_locate writes and the two buffer sets batch_rewind_fetch fills in turn, allocated once per object (and stream): every
    launch that reads them is on this stream, in front of the next call's."""
    torch = self._torch
    N, zmax, stream = self.batch, max(self.zdims.values()), self._torch.cuda.current_stream(self.device).cuda_stream
    w = self._rw
    if w is None or w["stream"] != stream:
      f64, dev = dict(dtype=torch.float64, device=self.device), self.device

      def bufset():
        return dict(t=torch.zeros(N, **f64), dt=torch.zeros(N, **f64), kinds=torch.zeros(N, dtype=torch.int32, device=dev),
                    act=torch.zeros(N, dtype=torch.uint8, device=dev), z=torch.zeros((N, zmax), **f64), z_keep=torch.zeros((N, zmax), **f64),
                    R=torch.zeros((N, zmax * zmax), **f64))
      w = self._rw = dict(stream=stream, slot=torch.zeros(N, dtype=torch.int32, device=dev), n=torch.zeros(N, dtype=torch.int32, device=dev),
                          drop=torch.zeros(N, dtype=torch.uint8, device=dev), counts=torch.zeros(2, dtype=torch.int32, device=dev),
                          host=torch.zeros(2, dtype=torch.int32).pin_memory(), flags=torch.zeros(N, dtype=torch.uint8, device=dev),
                          sets=(bufset(), bufset()))
      w["host_np"] = w["host"].numpy()
    return w

  def _rewind_fetch(self, q, t_prev, dst):
    r, w = self._ring, self._rw
    self._call("batch_rewind_fetch", self._p(w["slot"]), self._p(w["n"]), q, self._p(t_prev), self.batch, self.rewind_to_keep, r["nmax"],
               self._p(r["t"]), self._p(r["kind"]), self._p(r["z"]), self._p(r["R"]), self._p(dst["t"]), self._p(dst["dt"]), self._p(dst["kinds"]),
               self._p(dst["act"]), self._p(dst["z"]), self._p(dst["z_keep"]), self._p(dst["R"]), self._stream())

  def _rewind_locate(self, tt, ft, b):
    """The rewind of the filters the plan found late (batch_rewind_locate on the plan's buffers `b`: a rewound filter steps in this call
    after all, from its checkpoint), the call's second and last host round trip -- how many positions to replay, how many filters
    were too old -- and the fetch of replay position 0, which the call's own push is about to overwrite.  -> (positions, dropped)."""
    torch = self._torch
    if self._ring is None:
      self._ring_alloc(1)
    r, w = self._ring, self._rewind_buffers()
    w["counts"].zero_()
    self._call("batch_rewind_locate", self._p(b["late"]), self._p(tt), self.batch, self.rewind_to_keep, self._p(r["t"]), self._p(r["x"]), self._p(r["P"]),
               self._p(r["head"]), self._p(r["length"]), float(self.max_rewind_age), self._p(self.x), self._p(self.P), self._p(ft), self._p(b["dt"]),
               self._p(b["act"]), self._p(w["slot"]), self._p(w["n"]), self._p(w["drop"]), self._p(w["counts"]), self._stream())
    w["host"].copy_(w["counts"], non_blocking=True)
    torch.cuda.current_stream(self.device).synchronize()
    positions, dropped = int(w["host_np"][0]), int(w["host_np"][1])
    if dropped > 0:
      self.logger.error(f"observation too old for {dropped} filter(s) of the batch, ignoring it for them")
    if positions > 0:
      self._rewind_fetch(0, tt, w["sets"][0])
    self.rewind_stats["device"] += 1
    return positions, dropped

  def _rewind_replay(self, positions, dropped):
    """Behind the call's own step and push: flag 48 for the filters that were too old, then the fast-forward -- per replay position one
    fetch (of the NEXT position), one mixed-kind step and one push, whatever kinds the overtaken entries hold.  The step's flags go to a
    scratch buffer: the flags the caller reads are this call's."""
    N, K, r, w = self.batch, self.rewind_to_keep, self._ring, self._rw
    ft = self._ft_dev
    if dropped > 0:
      self._call("batch_flags_set", self._p(self.flags), self._p(w["drop"]), 48, N, self._stream())
    # Every entry is fetched before a launch overwrites its slot: the call's own push wrote the slot of replay position 0 (fetched by
    # _rewind_locate), the push behind position q writes the slot of position q + 1 (fetched in front of step q).  A push evicts only on a
    # full ring -- the last replay's push at most -- and takes the filter's oldest entry, never a replay entry (the rewind keeps >= 1).
    for q in range(positions):
      cur, nxt = w["sets"][q & 1], w["sets"][(q + 1) & 1]
      if q + 1 < positions:
        self._rewind_fetch(q + 1, cur["t"], nxt)      # (t_prev: this position's times, not ft -- its push has not run yet)
      self._call("batch_predict_update_kinds", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(cur["dt"]), 0.0, self._p(cur["kinds"]),
                 self._p(cur["z"]), self._p(cur["R"]), 1, N, self.norm_quats, self._p(w["flags"]), self._p(cur["act"]), self._stream())
      self._call("batch_timeline_push_kinds", self._p(cur["t"]), self._p(cur["act"]), self._p(ft), self._p(self.x), self._p(self.P), N, K, r["nmax"],
                 self._p(r["t"]), self._p(r["x"]), self._p(r["P"]), self._p(r["kind"]), self._p(r["nobs"]), self._p(r["z"]), self._p(r["R"]), self._p(r["ea"]),
                 self._p(r["head"]), self._p(r["length"]), self._p(cur["kinds"]), self._p(cur["z_keep"]), self._p(cur["R"]), 1, self._stream())

  def _ring_alloc(self, nmax=1):
    """Per-filter checkpoint rings in HBM: K entries per filter, an entry = time, state after the call, and the call's observation(s) --
    up to `nmax` of them (grown on demand by the first call that carries more: _ring_push)."""
    torch = self._torch
    K, N, D, E = self.rewind_to_keep, self.batch, self.dim_x, self.dim_err
    zmax = max(self.zdims.values())
    eam = max(list(self.eadims.values()) + [0])
    f64 = dict(dtype=torch.float64, device=self.device)
    old = self._ring
    self._ring = dict(
      t=torch.full((K, N), float("nan"), **f64), x=torch.empty((K, N, D), **f64), P=torch.empty((K, N, E, E), **f64),
      kind=torch.zeros((K, N), dtype=torch.int32, device=self.device), nobs=torch.ones((K, N), dtype=torch.int32, device=self.device),
      z=torch.zeros((K, N, nmax, zmax), **f64), R=torch.zeros((K, N, nmax, zmax, zmax), **f64), ea=torch.zeros((K, N, nmax, max(eam, 1)), **f64),
      head=torch.zeros(N, dtype=torch.int64, device=self.device), length=torch.zeros(N, dtype=torch.int64, device=self.device), nmax=nmax)
    if old is not None:         # grown: everything kept, the observation arrays copied into the wider ones
      for key in ("t", "x", "P", "kind", "nobs", "head", "length"):
        self._ring[key] = old[key]
      for key in ("z", "R", "ea"):
        self._ring[key][:, :, :old["nmax"]] = old[key]

  def _ring_push(self, mask, times, kind, z_obs, Rl, per, eal, nobs=None):
    """checkpoint (ekf_sym.py:440-450) of the filters in `mask`: state AFTER the call, its time, and the call's observations (lists of n,
    _masked_step; nobs (N,) int tensor when filters carry different counts); each filter has its own circular ring of rewind_to_keep
    entries in HBM."""
    torch = self._torch
    n = len(z_obs)
    if self._ring is None or self._ring["nmax"] < n:
      self._ring_alloc(n)
    r, K = self._ring, self.rewind_to_keep
    idx = torch.nonzero(mask).flatten()
    if idx.numel() == 0:
      return
    full = r["length"][idx] >= K
    r["head"][idx] = torch.where(full, (r["head"][idx] + 1) % K, r["head"][idx])
    r["length"][idx] = torch.where(full, r["length"][idx], r["length"][idx] + 1)
    slot = (r["head"][idx] + r["length"][idx] - 1) % K
    Z = self.zdims[kind]
    r["t"][slot, idx] = times[idx]
    r["x"][slot, idx] = self.x[idx]
    r["P"][slot, idx] = self.P[idx]
    r["kind"][slot, idx] = int(kind)
    r["nobs"][slot, idx] = n if nobs is None else nobs[idx].to(torch.int32)
    for j in range(n):
      r["z"][slot, idx, j, :Z] = z_obs[j][idx]
      r["R"][slot, idx, j, :Z, :Z] = Rl[j][idx] if per else Rl[j]
      if eal[j] is not None:
        r["ea"][slot, idx, j, :eal[j].shape[1]] = eal[j][idx]

  def _ring_rewind(self, late, tt):
    """rewind (ekf_sym.py:418-438) of the filters in `late`, each in its own ring: back to its last checkpoint at or before its
    observation time; -> (mask of filters whose observation is too old and is ignored, what to replay afterwards)."""
    torch = self._torch
    if self._ring is None:
      self._ring_alloc()
    r, K = self._ring, self.rewind_to_keep
    idx = torch.nonzero(late).flatten()
    L, H, ta = r["length"][idx], r["head"][idx], tt[idx]
    j = torch.arange(K, device=self.device)[:, None]
    phys = (H[None, :] + j) % K                                  # (K, m): logical position -> slot
    Tm = r["t"][phys, idx[None, :]]
    valid = j < L[None, :]
    newest = Tm.gather(0, (L - 1).clamp(min=0)[None, :])[0]
    too_old = (L == 0) | (ta < Tm[0]) | (ta < newest - self.max_rewind_age)            # ekf_sym.py:464-471
    ix = (valid & (Tm <= ta[None, :])).sum(0)                     # bisect_right(times, t)
    ok = ~too_old
    dropped = torch.zeros(self.batch, dtype=torch.bool, device=self.device)
    dropped[idx[too_old]] = True
    gi, gix, gL, gH = idx[ok], ix[ok], L[ok], H[ok]
    if gi.numel() == 0:
      return dropped, None
    src = (gH + gix - 1) % K
    self.x[gi] = r["x"][src, gi]
    self.P[gi] = r["P"][src, gi]
    ft = self.filter_time.clone()
    ft[gi] = r["t"][src, gi]
    self.filter_time = ft
    nrep = gL - gix
    maxrep = int(nrep.max())
    rep = dict(idx=gi, n=nrep, t=[], kind=[], nobs=[], z=[], R=[], ea=[])
    for q in range(maxrep):                                      # copies: the pushes below reuse these slots
      p_ = (gH + gix + q) % K
      for key in ("t", "kind", "nobs", "z", "R", "ea"):
        rep[key].append(r[key][p_, gi])
    r["length"][gi] = gix
    return dropped, rep

  def _ring_replay(self, rep):
    """fast-forward (ekf_sym.py:477-479): the overtaken calls of every rewound filter are applied again, oldest first; position q of
    all rewound filters is one group of launches per observation kind present at that position (a call's n observations: one
    predict + update launch and n - 1 update launches, masked to the filters that have that many)."""
    torch = self._torch
    N, gi = self.batch, rep["idx"]
    for q in range(len(rep["t"])):
      has = rep["n"] > q
      for kind in torch.unique(rep["kind"][q][has]).tolist():
        sel = has & (rep["kind"][q] == kind)
        fi = gi[sel]
        Z = self.zdims[kind]
        act = torch.zeros(N, dtype=torch.bool, device=self.device)
        act[fi] = True
        tt = self.filter_time.clone()
        tt[fi] = rep["t"][q][sel]
        nobs = torch.zeros(N, dtype=torch.int32, device=self.device)
        nobs[fi] = rep["nobs"][q][sel]
        nq = int(nobs.max())
        EA = self.eadims.get(kind, 0)
        zl, Rl, eal = [], [], []
        for j in range(nq):
          zin = torch.zeros((N, Z), dtype=torch.float64, device=self.device)
          zin[fi] = rep["z"][q][sel][:, j, :Z]
          Rd = torch.zeros((N, Z, Z), dtype=torch.float64, device=self.device)
          Rd[fi] = rep["R"][q][sel][:, j, :Z, :Z]
          Rd[nobs <= j] = torch.eye(Z, dtype=torch.float64, device=self.device)      # (filters masked out of launch j: any regular matrix)
          ea = None
          if EA:
            ea = torch.zeros((N, EA), dtype=torch.float64, device=self.device)
            ea[fi] = rep["ea"][q][sel][:, j, :EA]
          zl.append(zin)
          Rl.append(Rd)
          eal.append(ea)
        z_obs = [zj.clone() for zj in zl]
        dt = torch.where(act, tt - self.filter_time, torch.zeros_like(tt))
        fl = self.flags.clone()
        self._masked_step(kind, zl, Rl, 1, eal, dt, act.to(torch.uint8), nobs=nobs)
        self.flags.copy_(torch.where(act, self.flags, fl))         # flags of the filters this replay did not touch stay (same buffer: bind_step() holds its address)
        self.filter_time = torch.where(act, tt, self.filter_time)
        self._ring_push(act, self.filter_time, kind, z_obs, Rl, 1, eal, nobs=nobs)

  def _predict_and_update_with_rewind(self, t, kind, z, R, extra_args, keep_estimate):
    """Reference semantics of EKFSym::predict_and_update_batch (ekf_sym.cc:83-117) for the whole batch: an
    observation older than the filter time rewinds every filter to the last checkpoint at or before t, is applied,
    and the overtaken observations are replayed; anything older than max_rewind_age (or than the ring) is dropped."""
    replay = []
    if isinstance(self.filter_time, self._torch.Tensor):
      # per-filter times exist only between init_state and the first step, when the ring is still empty: an observation
      # older than ANY filter's time cannot be reordered and is dropped for the whole batch (ekf_sym.cc:87-94)
      if bool((t < self.filter_time).any()):
        self.logger.error(f"observation too old at {t:.3f} for a filter of the batch, ignoring")
        return None
    elif self.filter_time is not None and t < self.filter_time:
      if len(self.rewind_t) == 0 or t < self.rewind_t[0] or t < self.rewind_t[-1] - self.max_rewind_age:
        self.logger.error(f"observation too old at {t:.3f} with filter at {self.filter_time:.3f}, ignoring")
        return None
      times = list(self.rewind_t)
      idx = bisect_right(times, t)
      assert times[idx - 1] <= t < times[idx]
      self.filter_time = times[idx - 1]
      self.x.copy_(self.rewind_states[idx - 1][0])
      self.P.copy_(self.rewind_states[idx - 1][1])
      replay = list(self.rewind_obscache)[idx:]
      for ring in (self.rewind_t, self.rewind_states, self.rewind_obscache):
        while len(ring) > idx:
          ring.pop()
    ret = self._checkpointed_step(t, kind, z, R, extra_args, keep_estimate)
    for (rt, rkind, rz, rR, rea) in replay:
      self._checkpointed_step(rt, rkind, rz, rR, rea, False)
    return ret

  def _checkpointed_step(self, t, kind, z, R, extra_args, keep_estimate):
    if np.ndim(z) == 3 if not hasattr(z, "ndim") else z.ndim == 3:      # n observations per filter: ONE checkpoint for the call (ekf_sym.cc:191)
      torch = self._torch
      zt = (z if isinstance(z, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64))).to(device=self.device, dtype=torch.float64)
      z_keep = zt.clone()
      ret = self._predict_and_update_multi(t, kind, zt, R, extra_args, keep_estimate)
      self.rewind_t.append(self.filter_time)
      self.rewind_states.append((self.x.clone(), self.P.clone()))
      self.rewind_obscache.append((t, kind, z_keep, R, extra_args))
      return ret
    zin, Rd, per = self._obs_args(kind, z, R)
    ea = self._ea(kind, extra_args)
    ck = f"batch_predict_update_{kind}_ckpt"
    if not keep_estimate and ea is None and hasattr(self._lib, f"{self.name}_{ck}"):
      # one launch: the step writes its own checkpoint -- the observation as it came, the filtered pair -- next to its results
      # (k_stepc_{kind}: 1.5 x the bytes of the plain step instead of the step plus three copies)
      torch = self._torch
      dt = self._dt(t)
      cx, cP, cz = torch.empty_like(self.x), torch.empty_like(self.P), torch.empty_like(zin)
      dt_ptr, dt_s = self._dt_args(dt)
      self._call(ck, self._p(self.x), self._p(self.P), self._p(self.Q), dt_ptr, dt_s, self._p(zin), self._p(Rd), per, None, self.batch,
                 self.norm_quats, self._p(self.flags), self._p(cx), self._p(cP), self._p(cz), self._stream())
      self.filter_time = t
      self.rewind_t.append(self.filter_time)
      self.rewind_states.append((cx, cP))
      self.rewind_obscache.append((t, kind, cz, Rd, None))
      return zin
    z_keep = zin.clone()                     # the kernel overwrites z with the residual; the ring needs the observation
    ret = self._predict_and_update(t, kind, zin, Rd, extra_args, keep_estimate)
    self.rewind_t.append(self.filter_time)
    self.rewind_states.append((self.x.clone(), self.P.clone()))
    self.rewind_obscache.append((t, kind, z_keep, Rd, self._ea(kind, extra_args)))
    return ret

  def _predict_and_update(self, t, kind, z, R, extra_args, keep_estimate):
    dt = self._dt(t)
    zin, R, per = self._obs_args(kind, z, R)
    ea = self._ea(kind, extra_args)
    self._keepalive_ea = ea
    if isinstance(z, self._torch.Tensor) and zin.data_ptr() == z.data_ptr() and keep_estimate:
      zin = zin.clone()
    if keep_estimate:
      z_orig = zin.clone()
      self.predict_dt(dt)
      xk_km1, Pk_km1 = self.x.clone(), self.P.clone()
      self._call(f"batch_update_{kind}", self._p(self.x), self._p(self.P), self._p(zin), self._p(R), per, self._p(ea),
                 self.batch, self.norm_quats, self._p(self.flags), self._stream())
      self.filter_time = t
      return xk_km1, self.x.clone(), Pk_km1, self.P.clone(), t, kind, zin, z_orig, extra_args
    dt_ptr, dt_s = self._dt_args(dt)
    self._call(f"batch_predict_update_{kind}", self._p(self.x), self._p(self.P), self._p(self.Q), dt_ptr, dt_s,
               self._p(zin), self._p(R), per, self._p(ea), self.batch, self.norm_quats, self._p(self.flags), self._stream())
    self.filter_time = t
    return zin

  def bind_step(self, kind, R):
    """Pre-bound fused predict+update for tight loops: returns step(z, dt) that calls the C ABI with everything except the
    observation pointer and dt already marshalled (the generic predict_and_update_batch spends several microseconds per
    call in argument handling, comparable to a small model's kernel time).  z: (N, Z) float64 contiguous device tensor,
    consumed (overwritten with the residual); dt: float.  Time bookkeeping is the caller's."""
    if kind not in self.zdims:
      raise KeyError(kind)
    _, Rd, per = self._obs_args(kind, self._torch.zeros((self.batch, self.zdims[kind]), dtype=self._torch.float64, device=self.device), R)
    fn = getattr(self._lib, f"{self.name}_batch_predict_update_{kind}")
    px, pP, pQ, pR, pfl = self._p(self.x), self._p(self.P), self._p(self.Q), self._p(Rd), self._p(self.flags)
    n, nq, stream = self.batch, self.norm_quats, self._stream()
    void_p = ctypes.c_void_p
    self._keepalive_bind = Rd

    def step(z, dt):
      rc = fn(px, pP, pQ, None, dt, void_p(z.data_ptr()), pR, per, None, n, nq, pfl, stream)
      if rc != 0:
        msg = self._ffi.string(getattr(self._lib, f"{self.name}_last_error_string")()).decode()
        getattr(self._lib, f"{self.name}_clear_error")()
        raise KalmanError(f"{self.name}_batch_predict_update_{kind} -> {rc}: {msg}")
    return step

  # -- analysis: Mahalanobis test without touching the state -----------------------------------------
  def maha_dist(self, kind, z, R, extra_args=None):
    """d2 = y^T (He P He^T + R)^-1 y per filter (N,) device tensor; x, P and z are left untouched.  Like the reference's
    maha_test, no null-space projection is applied to feature-track kinds."""
    zin, Rd, per = self._obs_args(kind, z, R)
    ea = self._ea(kind, extra_args)
    d2 = self._torch.empty(self.batch, dtype=self._torch.float64, device=self.device)
    self._call(f"batch_maha_{kind}", self._p(self.x), self._p(self.P), self._p(zin), self._p(Rd), per, self._p(ea), self.batch, self._p(d2),
               self._stream())
    self._keepalive_maha = (zin, Rd, ea)
    return d2

  def maha_test(self, kind, z, R, maha_thresh=0.95, extra_args=None):
    """Batched EKF_sym.maha_test (/root/reference/rednose/helpers/ekf_sym.py:626-649): True where the observation
    passes the chi-square gate at `maha_thresh`."""
    return ~(self.maha_dist(kind, z, R, extra_args) > chi2_ppf(maha_thresh, self.zdims[kind]))

  # -- fused multi-step run -------------------------------------------------------------------------
  # -- packed-triangle covariance records (libraries with {name}_has_tri_trace()) ---------------------------------------------
  def has_tri_trace(self):
    fn = getattr(self._lib, f"{self.name}_has_tri_trace", None)
    return bool(fn()) if fn is not None else False

  @property
  def dim_tri(self):
    return self.dim_err * (self.dim_err + 1) // 2

  def unpack_tri(self, tri, out=None):
    """(..., E (E + 1) / 2) packed lower triangles (row-major: entry (i, j <= i) at i (i + 1) / 2 + j) -> (..., E, E) symmetric matrices."""
    torch = self._torch
    tri = tri.contiguous()
    lead = tuple(tri.shape[:-1])
    full = out if out is not None else torch.empty(lead + (self.dim_err, self.dim_err), dtype=torch.float64, device=self.device)
    self._call("batch_tri_unpack", self._p(tri), self._p(full), int(np.prod(lead)) if lead else 1, self._stream())
    return full

  def pack_tri(self, full):
    """(..., E, E) -> (..., E (E + 1) / 2): the LOWER triangles (what batch_rts reads of a covariance)."""
    torch = self._torch
    full = self._dev(full).contiguous()
    lead = tuple(full.shape[:-2])
    tri = torch.empty(lead + (self.dim_tri,), dtype=torch.float64, device=self.device)
    self._call("batch_tri_pack", self._p(full), self._p(tri), int(np.prod(lead)) if lead else 1, self._stream())
    return tri

  def run(self, ts, kinds, zs, Rs=None, trace=False, flags=False, out=None, filters=None, extra_args=None, augment=None, exact=False, packed=False):
    """T predict+update steps in ONE launch; x and P stay on chip between steps.

    ts (T,) observation times, kinds (T,) observation kinds -- the schedule is shared by all filters;
    zs (T, N, zmax) observations (rows of kinds with Z < zmax are padded), consumed: overwritten with the
    residuals y.  Rs: {kind: (Z, Z)} (default: none -> KeyError) or a (T, zmax, zmax) array whose leading
    Z*Z entries per step are the row-major R of that step.  trace=True also returns the filtered states
    (T, N, D) and covariances (T, N, E, E) -- what the RTS smoother consumes.
    out = (trace_x, trace_P): preallocated contiguous float64 device tensors for the trace (implies trace=True; a 16 384 x
    210-step live trace is 14 GB -- callers that repeat a run reuse one allocation instead of paying a fresh one each time).
    filters = (lo, hi): run only filters lo .. hi-1 of the batch (their x / P records are contiguous); N above is then
    hi - lo.  extra_args (T, N, EA): per filter and step extra arguments for the kinds that take them (MSCKF feature tracks:
    the landmark; rows of other kinds are ignored); augment (T,) bool: MSCKF window shift after that step.
    exact=True: the REFERENCE'S result for this schedule on any input covariance, symmetric or not -- the schedule is walked with the
    step-granular kernels, which multiply with both halves of P and solve with S as a general matrix like ekf_c.c:24,100-101,115
    (one launch per step: the state crosses HBM every step).  The default (fused launch) computes on (P + P^T) / 2, which is the
    same thing for the covariances a filter produces itself and differs at first order in a caller-supplied skew part
    (include/rednose_amd_filter.h).
    packed=True (libraries with has_tri_trace(): lane-group models of 13 .. 22 error states): the covariance trace is written as packed
    lower triangles, trace_P (T, N, E (E + 1) / 2) -- half the bytes; rts_smooth(..., packed=True) consumes it (unpack_tri() gives matrices).
    Returns (ys, trace_x, trace_P, flags) with None for outputs not requested.
    """
    torch = self._torch
    ts = np.asarray(ts, dtype=np.float64)
    kinds = np.asarray(kinds, dtype=np.int32)
    T = len(ts)
    assert kinds.shape == (T,)
    zmax = getattr(self._lib, f"{self.name}_zmax")()
    if T == 0:         # empty schedule: a no-op, like the C ABI
      return self._dev(zs, (0, self.batch, zmax)), None, None, None
    for k in set(kinds.tolist()):
      if k not in self.zdims:
        raise KeyError(k)
      if self.eadims.get(k, 0) and extra_args is None:
        raise KalmanError(f"kind {k} takes per-observation extra arguments: pass extra_args (T, N, {self.eadims[k]})")
    assert not isinstance(self.filter_time, torch.Tensor), "bring the filters to a common time first (predict(t))"
    t0 = self.filter_time if self.filter_time is not None else ts[0]
    dts = np.diff(np.concatenate([[t0], ts]))
    assert (dts >= 0).all(), "batched filters do not rewind: the schedule must be in time order"
    lo, hi = (0, self.batch) if filters is None else (int(filters[0]), int(filters[1]))
    assert 0 <= lo <= hi <= self.batch
    nb = hi - lo
    zs = self._dev(zs, (T, nb, zmax))
    if isinstance(Rs, dict) or Rs is None:
      table = np.zeros((T, zmax * zmax))
      for k in set(kinds.tolist()):          # one masked assignment per kind (a Python loop over T steps costs a millisecond per 2 000)
        Rk = np.atleast_2d(np.asarray((Rs or {})[k], dtype=np.float64))
        table[kinds == k, :Rk.size] = Rk.reshape(-1)
    else:
      table = np.asarray(Rs, dtype=np.float64).reshape(T, zmax * zmax)
    Rd = self._dev(table)
    kd = torch.as_tensor(kinds, device=self.device)
    dd = self._dev(dts)
    if packed and (exact or not self.has_tri_trace()):
      raise KalmanError(f"run(packed=True): lib{self.name}.so has no packed-triangle trace kernels ({self.name}_has_tri_trace), or exact=True was asked for")
    pshape = (T, nb, self.dim_tri) if packed else (T, nb, self.dim_err, self.dim_err)
    tx, tP, fl = self._trace_buffers(T, nb, pshape, trace, flags, out)
    if nb == 0:
      return zs, tx, tP, fl
    # contiguous views of the filters' records; the C ABI moves them with 16-byte transfers, so record `lo` has to start on an
    # even double: always true for even record sizes, for odd ones (live: 23 states) only at even `lo`
    if (lo * self.dim_x) % 2 or (lo * self.dim_err * self.dim_err) % 2:
      raise KalmanError(f"run(filters=({lo}, {hi})): with {self.dim_x} states / {self.dim_err} error states per filter a sub-batch must "
                        "start at an even filter index (16-byte alignment of its first record)")
    xv, Pv = self.x[lo:hi], self.P[lo:hi]
    ead = max(list(self.eadims.values()) + [0])
    ea = None if extra_args is None else self._dev(extra_args, (T, nb, ead))
    ag = None
    if augment is not None:
      assert self.msckf, "augment: MSCKF models only"
      ag = torch.as_tensor(np.asarray(augment, dtype=np.int32).reshape(T), device=self.device)
    if self._has_batch_run() and not exact:
      self._call("batch_run_tri" if packed else "batch_run", self._p(xv), self._p(Pv), self._p(self.Q), self._p(kd), self._p(dd), T, self._p(zs),
                 self._p(Rd), nb, self.norm_quats, self._p(fl), self._p(tx), self._p(tP), self._p(ea), self._p(ag), self._stream())
    else:
      self._run_stepwise(xv, Pv, kinds, dts, zs, Rd, nb, fl, tx, tP, ea, None if augment is None else np.asarray(augment).reshape(T),
                         symmetrise=not exact)
    if nb == self.batch:          # a strict subset leaves the orchestrator's clock alone: the other filters have not moved
      self._shift_augment_times(ts, augment)
      self.filter_time = float(ts[-1])
    self._keepalive = (kd, dd, Rd, ea, ag)      # the launch is asynchronous: keep its inputs alive
    return zs, tx, tP, fl

  def _trace_buffers(self, T, nb, pshape, trace, flags, out):
    """The trace and flag buffers of a fused run over nb filters -> (tx, tP, fl), None where not asked for: out = (tx, tP) as the caller
    preallocated them, checked against (T, nb, D) and pshape (the covariance trace: matrices or packed triangles), else fresh ones."""
    torch = self._torch
    if out is not None:
      tx, tP = out
      for t_, shp in ((tx, (T, nb, self.dim_x)), (tP, pshape)):
        assert t_.is_contiguous() and t_.dtype == torch.float64 and tuple(t_.shape) == shp and t_.device == self.device, "out: wrong trace buffer"
    else:
      tx = torch.empty((T, nb, self.dim_x), dtype=torch.float64, device=self.device) if trace else None
      tP = torch.empty(pshape, dtype=torch.float64, device=self.device) if trace else None
    return tx, tP, (torch.zeros((T, nb), dtype=torch.uint8, device=self.device) if flags else None)

  def _shift_augment_times(self, ts, augment):
    """The shared timeline's window-shift times (get_augment_times) along a schedule's augment (T,), None: no shifts."""
    if augment is not None and self.msckf:
      for t_, a_ in zip(ts, np.asarray(augment).reshape(len(ts))):
        if a_:
          self.augment_times = self.augment_times[1:] + [float(t_)]

  def _has_batch_run(self):
    """False for a library whose fused multi-step kernel did not fit the register file (gen_code fallback `no_run`: its
    {name}_batch_run returns ERR_UNSUPPORTED)."""
    fn = getattr(self._lib, f"{self.name}_has_batch_run", None)
    if fn is None:            # a library generated before the query existed: it has the kernel unless the call says otherwise
      return True
    fn.restype = ctypes.c_int
    return bool(fn())

  def _run_stepwise(self, xv, Pv, kinds, dts, zs, Rd, nb, fl, tx, tP, ea, augment, symmetrise=True):
    """run() for a library without the fused multi-step kernel, and run(exact=True) for every library: the same schedule, one fused
    predict + update launch per step through the step-granular entry points (same results as the reference's per-call path; the
    state crosses HBM every step)."""
    if symmetrise:      # one contract for the default run(), whichever path serves it: the fused kernels read (P + P^T) / 2 (include/rednose_amd_filter.h)
      Pv.copy_(0.5 * (Pv + Pv.transpose(1, 2)))
    for t in range(len(kinds)):
      k = int(kinds[t])
      Z = self.zdims[k]
      zt = zs[t, :, :Z].clone()              # own allocation: the C ABI wants 16-byte aligned observations
      Rt = Rd[t, :Z * Z]
      flp = None if fl is None else self._p(fl[t])
      eat = None if (ea is None or self.eadims.get(k, 0) == 0) else ea[t, :, :self.eadims[k]].contiguous()
      self._call(f"batch_predict_update_{k}", self._p(xv), self._p(Pv), self._p(self.Q), None, float(dts[t]), self._p(zt), self._p(Rt), 0,
                 self._p(eat), nb, self.norm_quats, flp, self._stream())
      zs[t, :, :Z] = zt
      if tx is not None:
        tx[t].copy_(xv)
      if tP is not None:
        tP[t].copy_(Pv)
      if augment is not None and augment[t]:
        self._call("batch_augment", self._p(xv), self._p(Pv), nb, self._stream())
      self._keepalive_step = (zt, Rt, eat)

  # -- N independent logs in one launch ---------------------------------------------------------------
  def _has_sym(self, sym):
    """{name}_has_{sym}() == 1; False for a library from before the symbol."""
    fn = getattr(self._lib, f"{self.name}_has_{sym}", None)
    return fn is not None and int(fn()) == 1

  # one per NoiseMode, looked up on the object when run_logs runs: an object may override one (a library "without" that kernel)
  def _has_batch_run_pf(self):
    return self._has_sym("batch_run_pf")

  def _has_batch_run_pf_r(self):
    return self._has_sym("batch_run_pf_r")

  def _has_batch_run_pf_rd(self):
    return self._has_sym("batch_run_pf_rd")

  def _has_batch_run_pf_ea(self):
    return self._has_sym("batch_run_pf_ea")

  def filter_augment_times(self):
    """(N, n_window) array: every filter's own last n_window window-shift times, as run_logs(augment=...) recorded them (the per-filter
    counterpart of get_augment_times(), which keeps the shifts of shared timelines); zeros until a filter has shifted, as the constructor's."""
    if self._augment_times_pf is None:
      self._augment_times_pf = np.zeros((self.batch, self.N))
    return self._augment_times_pf.copy()

  def run_logs(self, ts, kinds, zs, Rs, trace=False, flags=False, out=None, exact=False, extra_args=None, augment=None):
    """Replay N recorded logs, one per filter, in ONE launch ({name}_batch_run_pf: the fused run with a schedule per filter; objects built
    with per_filter=True).  ts (T, N): the time of entry t of filter i's log, NaN where the filter has none; kinds (T, N) ints, <= 0 = no
    entry (idle); zs (T, N, zmax): the first Z of a row are the observation, consumed -- overwritten by the residual, the rest of the row and
    the rows of idle entries pass through --; Rs {kind: (Z, Z)} shared by the entries of a kind.  trace / flags / out as run(): the trace is
    dense (an idle entry's row is the pair its filter had).  Returns (ys, trace_x, trace_P, flags); flags (T, N): 16 at idle entries.

    The noise may also come PER ENTRY, as every predict_and_update_batch call of a recorded log brings its own R: any value of the dict may be
    (T, N, Z, Z), read only where that kind occurs (the others stay (Z, Z)); or Rs is one tensor / array (T, N, zmax, zmax) or (T, N, zmax^2) in the
    kernel's layout -- the first Z * Z doubles of row (t, i) are the row-major R of that entry, the rest of the row and the rows of idle entries are
    never read and may hold anything; a contiguous float64 tensor on the device is used without a copy.  Such a run is one launch of
    {name}_batch_run_pf_r where the library has it ({name}_has_batch_run_pf_r()); without it, or with exact=True, the step walk below takes
    R[t] with r_per_filter = 1.  With (Z, Z) values only nothing changes: the same kernel, the same launches.  A wrong shape raises KalmanError.

    A per-entry noise that is DIAGONAL -- np.diag(std**2), what recorded logs carry -- comes as its variances: a dict value (T, N, Z), read only
    where that kind occurs, or one tensor / array (T, N, zmax) whose row (t, i) starts with the Z variances of that entry (the rest of the row and
    the rows of idle entries are never read and may hold anything; a contiguous float64 tensor on the device is used without a copy; with
    zmax == 1 that shape is (T, N, zmax^2) above: the same numbers, that path).  A dict takes ONE launch of {name}_batch_run_pf_rd (rows of zmax
    doubles in place of zmax^2) where the library has it ({name}_has_batch_run_pf_rd()), exact is false, no value is (T, N, Z, Z) and every
    shared (Z, Z) value is exactly diagonal (its diagonal fills the rows of its kind); the array under the first two conditions.  Otherwise the
    variances are expanded to full matrices in the layout (T, N, zmax^2) and take the path of the paragraph above.  (A three-dimensional dict
    value of Z * Z elements is the shared (Z, Z) it always was: a log with T * N == Z goes as the array or as (T, N, Z, Z).)

    Every filter predicts from its own time (filter_times(); a filter that has not started takes dt = 0 on its first entry, the rule of
    batch_timeline_plan) over its own previous entry.  A log must be in time order and must not start before its filter's time: a fused run
    does not rewind -- sort the log first (stable, by time).  A kind no filter of the model has raises KeyError, as in run().  Afterwards
    filter_times()[i] is the time of filter i's last entry, unchanged for a filter without one, and such a filter's x and P are untouched.
    With rewind_to_keep > 0 the rings are emptied as by reset_rewind(): their checkpoints are no longer the filters' past, so a later
    observation older than the run is "too old" by the usual rule.  pf_stats and rewind_stats do not count this call.
    The covariance is read as (P + P^T) / 2, the fused runs' contract.  exact=True, or a library without the kernel
    ({name}_has_batch_run_pf() == 0: MSCKF models, kinds with extra arguments, models without a fused run), walks the same schedule with the step-granular entry points, one
    batch_predict_update_kinds launch per step where the library has it, else one `_masked` launch per kind present in the step; exact=True
    leaves an asymmetric P as it is, like run(exact=True).

    extra_args (T, N, EA), EA the largest {name}_kind_eadim: row (t, i) starts with the extra arguments of filter i's entry t (a feature track's
    landmark); rows of idle entries and of kinds without extra arguments are never read and may hold anything.  A log with a kind that takes
    extra arguments and no extra_args raises KalmanError.  augment (T, N) bool / int, MSCKF models only (KalmanError otherwise): the window of
    filter i shifts after its entry t (EKF_sym.augment); set where kinds <= 0 it is ignored.  The trace row of such an entry is the estimate
    BEFORE the shift, as in run(); filter_augment_times() keeps every filter's own shift times.  An MSCKF model's logs with shared (Z, Z) noise
    are ONE launch of {name}_batch_run_pf_ea where the library has it ({name}_has_batch_run_pf_ea()); with exact=True, without the kernel or
    with a noise per entry the step walk passes each kind's extra arguments to its `_masked` launch and follows a step in which any filter
    shifts with one {name}_batch_augment_masked."""
    torch = self._torch
    if not self.per_filter:
      raise KalmanError("run_logs replays per-filter timelines: construct the orchestrator with per_filter=True")
    N, zmax = self.batch, max(self.zdims.values())
    tt, kd, kh, T = self._log_schedule(ts, kinds, "run_logs")
    present = [int(k) for k in (torch.unique(kd).tolist() if kh is None else np.unique(kh)) if int(k) > 0]
    if T == 0:
      return self._dev(zs, (0, N, zmax)), None, None, None
    for k in present:
      if k not in self.zdims or (isinstance(Rs, dict) and k not in Rs):
        raise KeyError(k)
      if self.eadims.get(k, 0) and extra_args is None:
        raise KalmanError(f"run_logs: kind {k} takes extra arguments: pass extra_args (T, N, {max(self.eadims.values())})")
    EA = max(list(self.eadims.values()) + [0])
    ea = None
    if extra_args is not None and EA > 0:
      shape = tuple(extra_args.shape) if hasattr(extra_args, "shape") else np.shape(extra_args)
      if shape != (T, N, EA):
        raise KalmanError(f"run_logs: extra_args must be (T, N, EA) = ({T}, {N}, {EA}), got {shape}")
      ea = self._dev(extra_args)
    ag = None
    if augment is not None:
      if not self.msckf:
        raise KalmanError("run_logs: augment shifts the window of an MSCKF model; this model has none")
      ag = augment if isinstance(augment, torch.Tensor) else torch.as_tensor(np.asarray(augment))
      if tuple(ag.shape) != (T, N):
        raise KalmanError(f"run_logs: augment must be (T, N) = ({T}, {N}), got {tuple(ag.shape)}")
      ag = ((ag.to(self.device) != 0) & (kd > 0)).to(torch.int32).contiguous()      # (ignored at idle entries)
    Rd, noise = self._run_logs_noise(Rs, kd, T, diag_ok=self._has_batch_run_pf_rd() and not exact)
    ft0 = self.filter_times()
    dts, last = self._log_dts(tt, kd, ft0, "run_logs")
    ft_new = torch.where(last[-1] >= 0, tt.gather(0, last[-1:].clamp(min=0))[0], ft0).contiguous()
    zs = self._dev(zs, (T, N, zmax))
    tx, tP, fl = self._trace_buffers(T, N, (T, N, self.dim_err, self.dim_err), trace, flags, out)
    # (DIAG comes only with its kernel and exact false: _run_logs_noise expands the variances otherwise)
    has = {TABLE: self._has_batch_run_pf, ENTRY: self._has_batch_run_pf_r, DIAG: self._has_batch_run_pf_rd}[noise]
    if self.msckf and noise is TABLE and not exact and self._has_batch_run_pf_ea():
      ea_k = ea if ea is not None else torch.zeros(2, dtype=torch.float64, device=self.device)      # (no kind of the log reads it)
      self._call("batch_run_pf_ea", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(kd), self._p(dts), T, self._p(zs), self._p(Rd), N,
                 self.norm_quats, self._p(fl), self._p(tx), self._p(tP), self._p(ea_k), self._p(ag), self._stream())
      self._keepalive_ea = (ea_k, ag)
    elif self.msckf or ea is not None:      # no kernel of batch_run_pf's family carries extra arguments or window shifts
      self._run_logs_stepwise(kd, dts, zs, Rd, fl, tx, tP, symmetrise=not exact, per_entry=noise.per_entry, ea=ea, ag=ag)
    elif has() and not exact:
      self._call(f"batch_run_pf{noise.sfx}", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(kd), self._p(dts), T, self._p(zs), self._p(Rd), N,
                 self.norm_quats, self._p(fl), self._p(tx), self._p(tP), self._stream())
    else:
      self._run_logs_stepwise(kd, dts, zs, Rd, fl, tx, tP, symmetrise=not exact, per_entry=noise.per_entry)
    if ag is not None:      # every filter's own shift times, in the order of its log
      at, agh, th = self.filter_augment_times(), ag.cpu().numpy() != 0, tt.cpu().numpy()
      for t in np.nonzero(agh.any(axis=1))[0]:
        m = agh[t]
        at[m] = np.concatenate([at[m, 1:], th[t, m, None]], axis=1)
      self._augment_times_pf = at
    self.filter_time = ft_new
    self._ft_dev = None
    if self.rewind_to_keep > 0:
      self.reset_rewind()
    self._keepalive = (kd, dts, Rd)
    return zs, tx, tP, fl

  def _log_schedule(self, ts, kinds, who):
    """ts and kinds of N logs on the device, KalmanError (in the name of `who`: run_logs, rts_smooth_logs) unless both are (T, N)
    -> (tt, kd int32, kh: the host array where kinds did not come as a tensor, else None, T)."""
    torch = self._torch
    tt, N = self._dev(ts), self.batch
    if tt.ndim != 2 or tt.shape[1] != N:
      raise KalmanError(f"{who}: ts must be (T, N) = (T, {N}), got {tuple(tt.shape)}")
    T = int(tt.shape[0])
    kh = None if isinstance(kinds, torch.Tensor) else np.array(kinds, dtype=np.int32)      # (a writable copy: torch does not take read-only arrays)
    kd = kinds.to(device=self.device, dtype=torch.int32) if kh is None else torch.as_tensor(kh).to(self.device)
    if tuple(kd.shape) != (T, N):
      raise KalmanError(f"{who}: kinds must be (T, N) = ({T}, {N}), got {tuple(kd.shape)}")
    return tt, kd.contiguous(), kh, T

  def _log_dts(self, tt, kd, ft0, who):
    """Every entry's dt from its filter's previous entry (or the filter's time ft0 in front of the first one; NaN there: dt = 0): a forward
    fill along T, shared by run_logs and rts_smooth_logs -> (dts (T, N), last (T, N): the latest entry of filter i up to step t, -1: none yet).
    Raises KalmanError for a log that is not in time order and for a real entry without a time."""
    torch = self._torch
    T, N = tt.shape
    has = kd > 0
    idx = torch.where(has, torch.arange(T, device=self.device)[:, None], torch.full((1, 1), -1, dtype=torch.int64, device=self.device))
    last = torch.cummax(idx, dim=0).values
    prev = torch.cat([torch.full((1, N), -1, dtype=torch.int64, device=self.device), last[:-1]], 0)
    t_prev = torch.where(prev >= 0, tt.gather(0, prev.clamp(min=0)), ft0[None, :])
    dts = torch.where(has, torch.nan_to_num(tt - t_prev, nan=0.0), torch.zeros_like(tt)).contiguous()
    bad = has & (torch.isnan(tt) | (tt < t_prev))
    if bool(bad.any()):
      t_, i_ = (int(v) for v in bad.nonzero()[0])
      if bool(torch.isnan(tt[t_, i_])):
        raise KalmanError(f"{who}: filter {i_}, step {t_}: kind {int(kd[t_, i_])} without a time (ts is NaN there; NaN marks idle entries, whose kind is <= 0)")
      raise KalmanError(f"{who}: filter {i_}, step {t_}: time {float(tt[t_, i_])} lies before the filter's previous time {float(t_prev[t_, i_])} "
                        "-- sort the log: a fused run does not rewind")
    return dts, last

  def _run_logs_noise(self, Rs, kd, T, diag_ok=False):
    """The observation noise of run_logs() on the device -> (Rd, its NoiseMode).  Shared by the entries of every kind: the per-kind table
    (num_kinds, zmax^2) of batch_run_pf, TABLE.  Otherwise the kernel's per-entry layout (T, N, zmax^2) of batch_run_pf_r: row (t, i)
    starts with the row-major (Z, Z) of entry (t, i), ENTRY.  A tensor or array in that layout is taken as it is (a device tensor of the
    right dtype without a copy); a dict is gathered into it, every kind's rows where that kind occurs.
    Variances per entry -- a dict value (T, N, Z), or one array (T, N, zmax) -- stay rows of zmax doubles, the layout of batch_run_pf_rd, and
    the mode is DIAG, where diag_ok (the library has that kernel and the run is not exact) and nothing in the dict needs a full matrix (no
    (T, N, Z, Z) value, every shared value exactly diagonal); otherwise they are expanded into the (T, N, zmax^2) layout, ENTRY."""
    torch = self._torch
    N, zmax = self.batch, max(self.zdims.values())
    ZZ = zmax * zmax

    def embed(v, Z):      # variances (T, N, Z) -> row-major diag(v) (T, N, Z * Z)
      return torch.diag_embed(v).reshape(T, N, Z * Z)

    def gather(width, rows):      # (T, N, width): rows(k) (T, N, w_k) where kind k occurs (a kind's values are read only there), zeros elsewhere
      Rd = torch.zeros((T, N, width), dtype=torch.float64, device=self.device)
      for k in self.kinds:
        v = rows(k)
        if v is not None:
          w = v.shape[2]
          Rd[:, :, :w] = torch.where((kd == k)[:, :, None], v, Rd[:, :, :w])
      return Rd

    if not isinstance(Rs, dict):
      shape = tuple(Rs.shape) if hasattr(Rs, "shape") else np.shape(Rs)
      if shape == (T, N, zmax) and zmax > 1:
        var = self._dev(Rs)
        if diag_ok:
          return var, DIAG
        return gather(ZZ, lambda k: embed(var[:, :, :self.zdims[k]], self.zdims[k])), ENTRY
      if shape not in ((T, N, zmax, zmax), (T, N, ZZ)):
        raise KalmanError(f"run_logs: Rs as one array is per entry, (T, N, zmax, zmax) = ({T}, {N}, {zmax}, {zmax}) or (T, N, zmax^2) = ({T}, {N}, {ZZ}), "
                          f"or its variances (T, N, zmax) = ({T}, {N}, {zmax}), got {shape}")
      return self._dev(Rs).reshape(T, N, ZZ), ENTRY
    shared, entry, var = {}, {}, {}
    for k in self.kinds:
      if k not in Rs:
        continue
      Z = self.zdims[k]
      shape = tuple(Rs[k].shape) if hasattr(Rs[k], "shape") else np.shape(Rs[k])
      if len(shape) == 4:
        if shape != (T, N, Z, Z):
          raise KalmanError(f"run_logs: Rs[{k}] per entry must be (T, N, Z, Z) = ({T}, {N}, {Z}, {Z}), got {shape}")
        entry[k] = Rs[k]
      elif shape == (T, N, Z) and T * N != Z:
        var[k] = Rs[k]
      else:
        if int(np.prod(shape)) != Z * Z:
          raise KalmanError(f"run_logs: Rs[{k}] must be (Z, Z) = ({Z}, {Z}), or (T, N, Z, Z) = ({T}, {N}, {Z}, {Z}) per entry, "
                            f"or that entry's variances (T, N, Z) = ({T}, {N}, {Z}), got {shape}")
        v = Rs[k].detach().cpu().numpy() if isinstance(Rs[k], torch.Tensor) else Rs[k]
        shared[k] = np.asarray(v, dtype=np.float64).reshape(Z * Z)
    if not entry and not var:
      tab = np.zeros((len(self.kinds), ZZ))
      for i, k in enumerate(self.kinds):
        if k in shared:
          tab[i, :self.zdims[k] ** 2] = shared[k]
      return self._dev(tab), TABLE
    if var and not entry and diag_ok and all(not (m - np.diag(np.diag(m))).any() for m in (shared[k].reshape(self.zdims[k], -1) for k in shared)):
      return gather(zmax, lambda k: self._dev(var[k]) if k in var else
                    self._dev(shared[k][::self.zdims[k] + 1].copy()).expand(T, N, self.zdims[k]) if k in shared else None), DIAG
    return gather(ZZ, lambda k: self._dev(entry[k]).reshape(T, N, self.zdims[k] ** 2) if k in entry else
                  embed(self._dev(var[k]), self.zdims[k]) if k in var else
                  self._dev(shared[k]).expand(T, N, self.zdims[k] ** 2) if k in shared else None), ENTRY

  def _run_logs_stepwise(self, kd, dts, zs, Rd, fl, tx, tP, symmetrise=True, per_entry=False, ea=None, ag=None):
    """run_logs() for a library without the fused kernel, and run_logs(exact=True): the same per-filter schedule, step by step.
    per_entry: Rd is (T, N, zmax^2), and step t takes Rd[t] with r_per_filter = 1 (the `_masked` walk: that kind's rows compacted to (N, Z^2)).
    ea (T, N, EA): a kind with extra arguments takes ea[t] in its `_masked` launch; ag (T, N) int32: a step in which any filter shifts its
    window is followed by one batch_augment_masked on those filters (the trace rows are taken before it)."""
    torch = self._torch
    T, N = kd.shape
    mixed = self._has_step_kinds() and ea is None
    ag_any = None if ag is None else ag.any(dim=1).cpu().numpy()
    if symmetrise:      # the fused kernel's contract: (P + P^T) / 2 for every filter that steps, a filter without an entry leaves as it came
      stepped = (kd > 0).any(dim=0)
      self.P.copy_(torch.where(stepped[:, None, None], 0.5 * (self.P + self.P.transpose(1, 2)), self.P))
    kh = None if mixed else kd.cpu().numpy()
    flt = torch.zeros(N, dtype=torch.uint8, device=self.device)
    keep = []
    for t in range(T):
      a8 = (kd[t] > 0).to(torch.uint8)
      dt = dts[t].clone()
      zt = zs[t].clone()                   # own allocation: the C ABI wants 16-byte aligned observations
      if mixed:
        kt = kd[t].clone()
        Rt = Rd[t].clone() if per_entry else Rd          # (own allocation, like zt)
        self._call("batch_predict_update_kinds", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt), 0.0, self._p(kt), self._p(zt), self._p(Rt),
                   int(per_entry), N, self.norm_quats, self._p(flt), self._p(a8), self._stream())
        keep = [(kt, a8, dt, zt, Rt)]      # (the stream orders the launches: the previous step's buffers may go)
      else:
        flt.fill_(16)
        for k in (int(k_) for k_ in np.unique(kh[t]) if int(k_) > 0):
          Z = self.zdims[k]
          m8 = (kd[t] == k).to(torch.uint8)
          zk = zt[:, :Z].contiguous()
          if per_entry:      # this kind's rows; the identity where a filter brings another kind or none (its row may hold anything)
            eye = torch.eye(Z, dtype=torch.float64, device=self.device).reshape(1, Z * Z)
            Rk = torch.where(m8[:, None] != 0, Rd[t, :, :Z * Z], eye).contiguous()
          else:
            Rk = Rd[self.kinds.index(k), :Z * Z].clone()
          fk = torch.zeros(N, dtype=torch.uint8, device=self.device)
          eak = None
          if self.eadims.get(k, 0):      # this kind's rows; zeros where a filter brings another kind or none (its row may hold anything)
            eak = torch.where(m8[:, None] != 0, ea[t, :, :self.eadims[k]], torch.zeros((), dtype=torch.float64, device=self.device)).contiguous()
          self._call(f"batch_predict_update_{k}_masked", self._p(self.x), self._p(self.P), self._p(self.Q), self._p(dt), 0.0, self._p(zk), self._p(Rk),
                     int(per_entry), self._p(eak), N, self.norm_quats, self._p(fk), self._p(m8), self._stream())
          zt[:, :Z] = torch.where(m8[:, None] != 0, zk, zt[:, :Z])
          flt.copy_(torch.where(m8 != 0, fk, flt))
          keep = keep[-len(self.kinds):] + [(m8, zk, Rk, fk, dt, eak)]
      zs[t].copy_(zt)
      if fl is not None:
        fl[t].copy_(flt)
      if tx is not None:
        tx[t].copy_(self.x)
      if tP is not None:
        tP[t].copy_(self.P)
      if ag_any is not None and ag_any[t]:
        g8 = (ag[t] != 0).to(torch.uint8)
        self._call("batch_augment_masked", self._p(self.x), self._p(self.P), self._p(g8), N, self._stream())
        keep = keep + [(g8,)]
    self._keepalive_step = keep

  # -- offline smoothing ----------------------------------------------------------------------------
  def smooth(self, ts, kinds, zs, Rs, passes=1, chunk=None, norm_quats=None, on_chunk=None, flags=False, extra_args=None, augment=None, packed=False):
    """Offline estimation over a whole observation stream: forward filter keeping the filtered trace, then the RTS
    backward pass -- `passes` times, each pass restarting the filter from the oldest smoothed estimate of the previous
    one ("multiple forward and backwards passes of the data", /root/reference/README.md:41-45, built on rts_smooth,
    ekf_sym.py:651-690).

    ts, kinds, zs, Rs, extra_args, augment: as for run() (zs (T, N, zmax) is NOT consumed here).  Pass 1 starts from the
    filter's current (x, P) at the filter time it had when smooth() was called (None: the first step has dt = 0); every later
    pass starts from the oldest smoothed estimate, which is an estimate AT ts[0], so its first step has dt = 0 (the
    reference's loop does init_state(x_s[0], P_s[0], None) between passes).  A chunk must start at an even filter index when
    the record sizes are odd (see run()).
    chunk: filters per forward/backward sweep.  The filtered trace of T steps costs T * (D + E*E) * 8 bytes per filter
    (live: 17 MB per filter at 2 100 steps, 279 GB for 16 384 filters with the predicted pairs the reference keeps,
    140 GB here); filters are independent, so the batch is swept in chunks whose trace fits -- the result is identical
    to one sweep.  on_chunk(lo, hi, xs, Ps, ys, flags) receives each chunk's smoothed trajectory (device tensors, valid
    only during the call: the buffers are reused); without it the whole smoothed trajectory is returned, which needs the
    trace of the full batch to fit.  On return x / P hold the FILTERED state after the last pass and filter_time = ts[-1].
    packed=True (has_tri_trace() libraries): the trace between the two passes holds packed lower triangles -- 2 208 B instead of 4 056 B per
    live filter-step written by the forward pass and read AND written by the backward pass; on_chunk then receives Ps as (T, m, E (E + 1) / 2)
    (unpack_tri() turns what it needs into matrices), the returned trajectory (no on_chunk) is unpacked to (T, N, E, E) as always.
    Returns (xs (T, N, D), Ps (T, N, E, E)) or None when on_chunk is given.
    """
    torch = self._torch
    ts = np.asarray(ts, dtype=np.float64)
    T = len(ts)
    assert passes >= 1 and T >= 1
    zmax = getattr(self._lib, f"{self.name}_zmax")()
    zs = self._dev(zs, (T, self.batch, zmax))
    step = self.batch if chunk is None else max(1, min(int(chunk), self.batch))
    if on_chunk is None and step < self.batch:
      raise KalmanError("smooth(chunk=...) hands the smoothed trajectory out chunk by chunk: pass on_chunk")
    t_init = self.filter_time
    aug0 = list(self.augment_times) if self.msckf else None      # run() shifts them when it covers the whole batch: once per pass
    if packed and not self.has_tri_trace():
      raise KalmanError(f"smooth(packed=True): lib{self.name}.so has no packed-triangle trace kernels ({self.name}_has_tri_trace)")
    tx = torch.empty((T, step, self.dim_x), dtype=torch.float64, device=self.device)
    tP = torch.empty((T, step, self.dim_tri) if packed else (T, step, self.dim_err, self.dim_err), dtype=torch.float64, device=self.device)
    for lo in range(0, self.batch, step):
      hi = min(self.batch, lo + step)
      m = hi - lo
      bx, bP = (tx, tP) if m == step else (tx[:, :m].contiguous(), tP[:, :m].contiguous())
      ea = None if extra_args is None else self._dev(extra_args)[:, lo:hi].contiguous()
      for p in range(passes):
        self.filter_time = t_init if p == 0 else float(ts[0])
        zc = zs[:, lo:hi].clone()               # run() consumes its observations (overwrites them with the residuals)
        ys, _, _, fl = self.run(ts, kinds, zc, Rs, flags=flags, out=(bx, bP), filters=(lo, hi), extra_args=ea, augment=augment, packed=packed)
        # the smoother works on the trace of this chunk only: a view of the orchestrator restricted to its filters
        xs, Ps = self._rts_on(bx, bP, ts, m, norm_quats, packed=packed)
        if p + 1 < passes:
          self.x[lo:hi].copy_(xs[0])
          self.P[lo:hi].copy_(self.unpack_tri(Ps[0]) if packed else Ps[0])
      if on_chunk is not None:
        on_chunk(lo, hi, xs, Ps, ys, fl)
    self.filter_time = float(ts[-1])
    if self.msckf:
      self.augment_times = aug0            # the window shifts of the schedule happened ONCE, whatever the passes / chunks
    self._shift_augment_times(ts, augment)
    if on_chunk is None:
      return xs, (self.unpack_tri(Ps) if packed else Ps)
    return None

  def _has_batch_rts_pf(self):
    return self._has_sym("batch_rts_pf")

  def rts_smooth_logs(self, trace_x, trace_P, ts, kinds, t0=None, norm_quats=None, inplace=False, last_predicted=None):
    """Batched Rauch-Tung-Striebel backward pass over the dense trace of run_logs(trace=True): N ragged logs, every filter with its own times,
    idle entries and length, in ONE launch ({name}_batch_rts_pf; objects built with per_filter=True).

    trace_x (T, N, D), trace_P (T, N, E, E): the trace; ts (T, N), kinds (T, N): as given to run_logs (NaN / kind <= 0: no entry).  t0 (N,): the
    filters' times before the run (filter_times() as it was then); default NaN = not started, so a filter's first entry has dt = 0, the rule of
    run_logs.  t0 only reaches the rows BEFORE a filter's first entry (below): every later dt is a difference of the log's own times.
    Per filter the semantics are rts_smooth's (the reference's, ekf_sym.py:651-690) over the entries that stepped it -- a kind of the model,
    whether or not the gate rejected the update.  An entry that did not step the filter (idle, or a kind the model does not have) is no predict
    at all: the predicted pair is the filtered one and the gain is the identity, also for models whose predict(0) is not.  The recursion starts
    at the filter's own last entry m from the PREDICTED pair of that entry (recomputed, or row i of last_predicted = (x (N, D), P (N, E, E)));
    rows behind m, and every row of a filter without an entry, come back bit for bit.  Rows before the filter's first entry f: step f - 1 is an
    ordinary step with that entry's dt, so it smooths the pair the filter started from, and the rows before it follow by identity steps -- the
    reference has no counterpart for them (its estimates begin with the first observation).
    The same refusals as run_logs: a log not in time order, a real entry without a time.  A library without the kernel
    ({name}_has_batch_rts_pf() == 0: MSCKF models, libraries without batch_rts, and models whose per-filter instantiation does not fit the register
    file -- of the shipped ones the dense test models rand17, rand40 and rand56) raises KalmanError: there is no other path.
    One pass, the whole batch, full E x E covariances: multi-pass, chunks and the packed-triangle trace are smooth()'s, on a shared schedule.
    Returns (states (T, N, D), covs (T, N, E, E)) device tensors."""
    torch = self._torch
    if not self.per_filter:
      raise KalmanError("rts_smooth_logs smooths per-filter timelines: construct the orchestrator with per_filter=True")
    if not self._has_batch_rts_pf():
      raise KalmanError(f"lib{self.name}.so has no smoother with a schedule per filter ({self.name}_has_batch_rts_pf() == 0)")
    N = self.batch
    tt, kd, _, T = self._log_schedule(ts, kinds, "rts_smooth_logs")
    xf, Pf = self._dev(trace_x), self._dev(trace_P)      # (converted first: a list has no shape to refuse; a device tensor of the right kind is not copied)
    for what, t_, shp in (("trace_x", xf, (T, N, self.dim_x)), ("trace_P", Pf, (T, N, self.dim_err, self.dim_err))):
      if tuple(t_.shape) != shp:
        raise KalmanError(f"rts_smooth_logs: {what} must be {shp}, got {tuple(t_.shape)}")
    if T == 0:
      return xf, Pf
    ft0 = torch.full((N,), float("nan"), dtype=torch.float64, device=self.device) if t0 is None else self._dev(t0, (N,))
    dts, _ = self._log_dts(tt, kd, ft0, "rts_smooth_logs")
    act = torch.zeros((T, N), dtype=torch.bool, device=self.device)
    for k in self.kinds:
      act |= kd == int(k)
    act = act.to(torch.uint8).contiguous()
    xs = xf if inplace else torch.empty_like(xf)
    Ps = Pf if inplace else torch.empty_like(Pf)
    xl = Pl = None
    if last_predicted is not None:
      xl = self._dev(last_predicted[0], (N, self.dim_x))
      Pl = self._dev(last_predicted[1], (N, self.dim_err, self.dim_err))
    self._call("batch_rts_pf", self._p(xf), self._p(Pf), self._p(dts), self._p(act), T, self._p(self.Q), N, self._nq(norm_quats), self._p(xs), self._p(Ps),
               self._p(xl), self._p(Pl), self._stream())
    self._keepalive_rts = (xf, Pf, dts, act, xl, Pl)
    return xs, Ps

  def smooth_logs(self, ts, kinds, zs, Rs, norm_quats=None, flags=False):
    """Offline estimation over N recorded logs: run_logs(trace=True) from the filters' current times, then rts_smooth_logs over that trace in
    place.  ts, kinds, zs, Rs: as for run_logs (Rs in every form it takes); zs is NOT consumed (it is cloned, as smooth() does).  On return x / P
    hold the FILTERED states and filter_times() is what run_logs leaves.  One pass over the whole batch with full covariances: multi-pass,
    chunks and the packed-triangle trace are not served for per-filter logs.  Returns (xs (T, N, D), Ps (T, N, E, E), ys, flags)."""
    torch = self._torch
    if not self.per_filter:
      raise KalmanError("smooth_logs smooths per-filter timelines: construct the orchestrator with per_filter=True")
    if not self._has_batch_rts_pf():
      raise KalmanError(f"lib{self.name}.so has no smoother with a schedule per filter ({self.name}_has_batch_rts_pf() == 0)")
    t0 = self.filter_times().clone()
    zc = self._dev(zs)
    zc = zc.clone() if isinstance(zs, torch.Tensor) else zc      # run_logs consumes its observations (overwrites them with the residuals)
    ys, tx, tP, fl = self.run_logs(ts, kinds, zc, Rs, trace=True, flags=flags)
    if tx is None:      # T == 0
      return tx, tP, ys, fl
    xs, Ps = self.rts_smooth_logs(tx, tP, ts, kinds, t0=t0, norm_quats=norm_quats, inplace=True)
    return xs, Ps, ys, fl

  def _nq(self, norm_quats):
    """The smoothers' nq argument.  bit 0: the recomputed predicted states are renormalised like the forward pass did (a property of the
    filter); bit 1: the reference's norm_quats argument (smoothed states; None: as the filter)."""
    return self.norm_quats | ((self.norm_quats if norm_quats is None else int(bool(norm_quats))) << 1)

  def _batch_rts(self, xf, Pf, td, m, norm_quats, xs, Ps, xl, Pl, packed):
    """The launch of rts_smooth (the whole batch) and _rts_on (m filters, in place): batch_rts, or batch_rts_tri over packed triangles."""
    self._call("batch_rts_tri" if packed else "batch_rts", self._p(xf), self._p(Pf), self._p(td), int(xf.shape[0]), self._p(self.Q), m, self._nq(norm_quats),
               self._p(xs), self._p(Ps), self._p(xl), self._p(Pl), self._stream())

  def _rts_on(self, tx, tP, ts, m, norm_quats, packed=False):
    """In-place backward pass over a trace of m filters (m <= batch); packed: tP holds packed lower triangles (batch_rts_tri)."""
    torch = self._torch
    if not hasattr(self._lib, f"{self.name}_batch_rts"):
      raise KalmanError(f"lib{self.name}.so has no batch_rts entry point")
    T = int(tx.shape[0])
    td = self._dev(np.asarray(ts, dtype=np.float64) if not isinstance(ts, torch.Tensor) else ts, (T,))
    self._batch_rts(tx, tP, td, m, norm_quats, tx, tP, None, None, packed)
    self._keepalive_rts = (tx, tP, td)
    return tx, tP

  def rts_smooth(self, trace_x, trace_P, ts, norm_quats=None, inplace=False, last_predicted=None, packed=False):
    """Batched Rauch-Tung-Striebel backward pass over the filtered trace returned by run(trace=True).

    trace_x (T, N, D), trace_P (T, N, E, E) filtered states/covariances, ts (T,) their times.  Semantics are the
    reference's rts_smooth (ekf_sym.py:651-690) applied to every filter -- the recursion starts from the predicted
    pair of the last step and, with norm_quats, all returned states but the oldest are renormalised; the
    predicted pairs are recomputed on the GPU from the filtered ones (templates/ekf_hip_rts.h).  MSCKF models: only
    the main block of the covariance and the main states are smoothed, the rest passes through (:675-686).
    last_predicted = (x (N, D), P (N, E, E)): the predicted pair of the last step (xk_km1, Pk_km1 of its estimate), which
    the reference returns verbatim as the newest smoothed estimate.  Default: its MAIN block is recomputed from the filtered
    pair of step T - 2 -- exact for models without an MSCKF window; for MSCKF models the window states and the window /
    cross-covariance blocks of that ONE estimate (index T - 1) are then the filtered ones of the trace, not the predicted
    ones (F_main P[main, window] is not formed), so pass last_predicted when the newest estimate's window blocks matter.
    Every older estimate is unaffected: the reference smooths the main block only (:675-686).
    packed=True (has_tri_trace() libraries): trace_P is a packed-triangle trace (T, N, E (E + 1) / 2) as run(packed=True) writes it and the
    smoothed covariances come back packed too (unpack_tri() gives matrices); last_predicted still takes a full (N, E, E) covariance.
    Returns (states (T, N, D), covs (T, N, E, E)) device tensors, oldest first.
    """
    torch = self._torch
    if not hasattr(self._lib, f"{self.name}_batch_rts"):
      raise KalmanError(f"lib{self.name}.so has no batch_rts entry point")
    if packed and not self.has_tri_trace():
      raise KalmanError(f"rts_smooth(packed=True): lib{self.name}.so has no packed-triangle trace kernels ({self.name}_has_tri_trace)")
    T = int(trace_x.shape[0])
    xf = self._dev(trace_x, (T, self.batch, self.dim_x))
    Pf = self._dev(trace_P, (T, self.batch, self.dim_tri) if packed else (T, self.batch, self.dim_err, self.dim_err))
    td = self._dev(np.asarray(ts, dtype=np.float64) if not isinstance(ts, torch.Tensor) else ts, (T,))
    xs = xf if inplace else torch.empty_like(xf)
    Ps = Pf if inplace else torch.empty_like(Pf)
    xl = Pl = None
    if last_predicted is not None:
      xl = self._dev(last_predicted[0], (self.batch, self.dim_x))
      Pl = self._dev(last_predicted[1], (self.batch, self.dim_err, self.dim_err))
      if packed:
        Pl = self.pack_tri(Pl)
    self._batch_rts(xf, Pf, td, self.batch, norm_quats, xs, Ps, xl, Pl, packed)
    self._keepalive_rts = (xf, Pf, td, xl, Pl)
    return xs, Ps
