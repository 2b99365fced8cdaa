"""Pieces shared by the kernel emitters: structured (sparse-at-generation-time) matrices, the per-filter scalar slot of the lane-group
family (SlotLayout), the per-routine device functions of the reference's scalar C ABI, and the launch text of the step-granular
kernels (launch_*), and the noise flavours of the fused run with a schedule per filter (NoiseMode)."""
from typing import NamedTuple

import sympy as sp

from rednose_amd.codegen.lower import Block, vector_names


class SMat:
  """Matrix whose entries are known at generation time to be zero, one, a constant or a named double."""

  def __init__(self, rows, cols):
    self.rows, self.cols = rows, cols
    self.e = [[None] * cols for _ in range(rows)]    # None == structural zero

  @classmethod
  def from_structure(cls, rows, cols, structure, fmt):
    m = cls(rows, cols)
    for i in range(rows):
      for j in range(cols):
        kind, val = structure[fmt(i, j)]
        if kind == 'zero':
          continue
        if kind == 'one':
          m.e[i][j] = ('one', None)
        elif kind == 'const':
          m.e[i][j] = ('const', repr(float(val)))
        else:
          m.e[i][j] = ('var', fmt(i, j))
    return m

  @classmethod
  def dense(cls, rows, cols, fmt):
    m = cls(rows, cols)
    for i in range(rows):
      for j in range(cols):
        m.e[i][j] = ('var', fmt(i, j))
    return m

  @classmethod
  def identity_padded(cls, inner, size):
    """blockdiag(inner, I): the MSCKF block predict (ekf_c.c:23-26) as one structured matrix."""
    m = cls(size, size)
    for i in range(size):
      for j in range(size):
        if i < inner.rows and j < inner.cols:
          m.e[i][j] = inner.e[i][j]
        elif i == j:
          m.e[i][j] = ('one', None)
    return m

  def nnz(self):
    return sum(1 for r in self.e for c in r if c is not None)

  def row_nz(self, i):
    return [(j, self.e[i][j]) for j in range(self.cols) if self.e[i][j] is not None]

  def col_nz(self, j):
    return [(i, self.e[i][j]) for i in range(self.rows) if self.e[i][j] is not None]


EADIM = 3        # extra-argument dimension of feature-track kinds, hard-coded in the reference (ekf_sym.py:151)


def ind(lines, n=2):
  pad = " " * n
  return [pad + s for s in lines]


class SlotLayout:
  """Per-filter scalar slot in LDS (doubles) of the lane-group family: the OFF_* of the fields emit_wide2.scalar_functions addresses and the
  stride SLOT.  A subclass says in pack() in which order and with which overlaps ITS fields are packed and returns the slot's length."""

  def __init__(self, spec, f_vars, he_vars_by_kind):
    self.zmax = max(k.zdim for k in spec.kinds)
    self.nf = len(f_vars)
    self.nh = max([len(v) for v in he_vars_by_kind.values()] + [0])
    self.zf = max([k.zdim for k in spec.kinds if k.He_sym is not None] + [0])      # rows of the feature-track kinds (MSCKF), 0: none
    self.OFF_X = 0
    n = self.pack(spec.dim_x, spec.dim_err)
    self.SLOT = n if n & 1 else n + 1      # odd stride: lane-per-filter ds_*_b64 accesses hit 32 distinct bank pairs

  def pack(self, D, E):
    raise NotImplementedError

  def feature_tail(self, n):
    """Appends the fields of feature-track kinds at n -> the slot's length.  EADIM Householder reflectors of the extra-argument Jacobian
    (EADIM x Z entries + EADIM betas: OFF_RF), the projected noise (Z - EADIM)^2 (OFF_RP), and the residual a second time: it exists in the
    orthonormal basis of the reflectors (what the update consumes: OFF_YP) and in the reference's fullPivLu basis (what goes back into z:
    the Y field)."""
    zp = self.zf - EADIM
    self.OFF_RF = n
    self.OFF_RP = self.OFF_RF + (EADIM * self.zf + EADIM if self.zf else 0)
    self.OFF_YP = self.OFF_RP + (zp ** 2 if self.zf else 0)
    return self.OFF_YP + (zp if self.zf else 0)


class NoiseMode(NamedTuple):
  """One flavour of the observation noise in the fused run with a schedule per filter: what the kernel emitters, emit's C ABI, gen_code's
  fallbacks and BatchedEKF.run_logs select on.  Where the flavours' wording differs irregularly the record carries the text as it is."""
  sfx: str               # C ABI: {name}_batch_run_pf{sfx} and {name}_has_batch_run_pf{sfx}
  kernel: str            # kernel stem ({kernel}_tr: the lane-per-filter family's kernel with the filtered trace)
  update: str            # update_{kind}_rows{update}: the lane-group family's predicated updates
  fallback: str          # of emit.FALLBACKS: the library without this kernel
  per_entry: bool        # gR is (T, n, row(zmax)), the lane's (group's) own rows staged in registers; False: one row per kind, a table in LDS
  diag: bool             # a row holds the entry's variances
  what: str              # the flavour in gen_code's log sentence, after "a schedule per filter"
  title_small: str       # emit_small.run_pf_kernel's title: untraced (K, ZZ) ...
  title_small_tr: str    # ... and with the filtered trace (K)
  title_wide: str        # emit_wide3.run_pf_kernel's title (zmax, ZZ)

  def row(self, zmax):
    """Doubles per row of gR."""
    return zmax if self.diag else zmax * zmax


TABLE = NoiseMode(
  sfx="", kernel="k_run_pf", update="_pf", fallback="no_run_pf", per_entry=False, diag=False, what="",
  title_small="// ---- fused run, a schedule per filter (kinds (T, n), dts (T, n)): blocks of {K} steps in registers (emit_small.run_pf_kernel) ----",
  title_small_tr="// ---- fused run, a schedule per filter, with the filtered trace: blocks of {K} steps (see emit_small.run_pf_kernel) ----------------",
  title_wide="""// ---- fused multi-step run, a schedule per filter: kinds (T, n), dts (T, n); z is (T, n, {zmax}) in: z, out: y; gR one row per kind -----------
// k_run's phases per step; a group takes part in those its own entry asks for (see emit_wide3.run_pf_kernel).""")
ENTRY = NoiseMode(
  sfx="_r", kernel="k_run_rpf", update="_rpf", fallback="no_run_pf_r", per_entry=True, diag=False, what=" and R per entry",
  title_small="// ---- fused run, a schedule per filter, R per entry (gR (T, n, {ZZ})): blocks of {K} steps in registers (emit_small.run_pf_kernel) ----",
  title_small_tr="// ---- fused run, a schedule per filter and R per entry, with the filtered trace: blocks of {K} steps (see emit_small.run_pf_kernel) ----",
  title_wide="""// ---- fused multi-step run, a schedule per filter and R per entry: kinds (T, n), dts (T, n); z is (T, n, {zmax}) in: z, out: y; gR (T, n, {ZZ}) -----------
// k_run_pf with the group's own row of R, a step ahead in registers (see emit_wide3.run_pf_kernel).""")
DIAG = NoiseMode(
  sfx="_rd", kernel="k_run_dpf", update="_dpf", fallback="no_run_pf_rd", per_entry=True, diag=True, what=" and a diagonal R per entry",
  title_small="// ---- fused run, a schedule per filter, diagonal R per entry (gR (T, n, {ZZ})): blocks of {K} steps in registers (emit_small.run_pf_kernel) ----",
  title_small_tr="// ---- fused run, a schedule per filter and a diagonal R per entry, with the filtered trace: blocks of {K} steps (see emit_small.run_pf_kernel) ----",
  title_wide="""// ---- fused multi-step run, a schedule per filter and a diagonal R per entry: kinds (T, n), dts (T, n); z is (T, n, {zmax}) in: z, out: y; gR (T, n, {ZZ}) -----------
// k_run_rpf with the group's own row of variances, a step ahead in registers (see emit_wide3.run_pf_kernel).""")
NOISE_MODES = (TABLE, ENTRY, DIAG)      # in the order of emission


def ea_count(k):
  """Number of extra arguments of kind k (0: the `ea` pointer is ignored)."""
  return 0 if k.ea_sym is None else int(sp.Matrix(k.ea_sym).shape[0])


def term(coef, operand):
  """C text of coef*operand (coef from an SMat entry, operand a C expression), None for zero."""
  if coef is None:
    return None
  kind, val = coef
  if kind == 'one':
    return operand
  return f"{val}*{operand}"


def sum_terms(terms):
  terms = [t for t in terms if t is not None]
  return " + ".join(terms) if terms else "0.0"


def coef_text(coef):
  if coef is None:
    return "0.0"
  kind, val = coef
  return "1.0" if kind == 'one' else val


def routine_device_function(routine):
  """One `__device__` function per sympy routine with the reference's argument order (inputs, then the
  flat row-major output).  Dense: every output entry is written, zeros included, like the reference's
  generated C."""
  names = {}
  params = []
  for idx, a in enumerate(routine.args):
    if a is None:
      params.append(("ptr", f"unused{idx}", 1))
      continue
    if isinstance(a, sp.MatrixSymbol):
      cname = str(a.name)
      names.update(vector_names(a, cname))
      params.append(("ptr", cname, int(a.shape[0] * a.shape[1])))
    elif isinstance(a, sp.Symbol):
      names[a] = str(a.name)
      params.append(("scalar", str(a.name), 1))
    else:  # a sympy Matrix of plain symbols (e.g. extra args)
      cname = f"ea{idx}"
      names.update(vector_names(a, cname))
      params.append(("ptr", cname, len(sp.Matrix(a))))
  expr = sp.Matrix(routine.expr)
  blk = Block(names, tmp_prefix="t")
  n_out = int(expr.shape[0] * expr.shape[1])
  for i in range(expr.shape[0]):
    for j in range(expr.shape[1]):
      blk.add(f"out[{i * expr.shape[1] + j}]", expr[i, j])
  stmts, _ = blk.lower(materialize_all=True, decl="")
  sig = ", ".join((f"const double* __restrict__ {n}" if k == "ptr" else f"double {n}") for k, n, _ in params)
  text = [f"__device__ __forceinline__ void {routine.name}({sig}, double* __restrict__ out) {{"]
  text += ["  " + s for s in stmts]
  text.append("}")
  return "\n".join(text), params, n_out


def innovation_solver(Z, general, y_terms, thresh=None):
  """Text pieces for the Z x Z innovation covariance S held in `S` (with `HPH`, `Rl` beside it): -> (factor, gate, solve) where
  `factor` factors S into (L, iL), `gate` (when `thresh` is given) is the Mahalanobis test of ekf_c.c:88-94 on the residual `y_terms`
  -- R *= 1e16 and a second factorisation when it trips --, and `solve(v)` is the call that overwrites the array v with S^-1 v.
  general=True: S is taken as a general matrix (L D U, templates/ekf_hip_rt.h: ldu_*) -- the step-granular kernels, which follow the
  reference on asymmetric covariances; False: L D L^T from the lower triangle (spd_*) -- the fused multi-step kernels, whose covariance
  is symmetric by contract."""
  pre = "rn::ldu" if general else "rn::spd"
  factor = f"{pre}_factor<{Z}>(S, L, iL);"
  gate = []
  if thresh is not None:
    ys = ", ".join(y_terms)
    if general:
      gate = ["{", f"  double v[{Z}] = {{{ys}}}, w[{Z}] = {{{ys}}};", f"  rn::ldu_forward<{Z}>(L, iL, v);", f"  rn::ldu_forward_t<{Z}>(L, iL, w);",
              "  const double d2 = " + " + ".join(f"v[{i}]*w[{i}]*iL[{i}]" for i in range(Z)) + ";"]
    else:
      gate = ["{", f"  double v[{Z}] = {{{ys}}};", f"  rn::spd_forward<{Z}>(L, iL, v);",
              "  const double d2 = " + " + ".join(f"v[{i}]*v[{i}]*iL[{i}]" for i in range(Z)) + ";"]
    gate += [f"  if (d2 > {thresh!r}) {{", "    gated = 1;", "#pragma unroll",
             f"    for (int i = 0; i < {Z * Z}; i++) {{ Rl[i] = 1.0e16 * Rl[i]; S[i] = HPH[i] + Rl[i]; }}", f"    {factor}", "  }", "}"]
  return factor, gate, (lambda v: f"{pre}_solve<{Z}>(L, iL, {v});")


# ---- launch text of the step-granular kernels, the same in both kernel families but for `tiles`, the family's count of wavefront tiles in n ----
def _launch(tiles, kernel, args):
  return f"""  const int64_t tiles = {tiles};
  hipLaunchKernelGGL({kernel}, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     {args});"""


def launch_predict(tiles):
  return _launch(tiles, "k_predict", "x, P, Q, dt_vec, dt, n, norm_quats, active")


def _step_args(obs, do_predict, head=0):
  """Arguments of a step kernel in its own order.  head=1 (the lane-per-filter family, emit_small._step_signature): what the requests of a full tile need
  comes first, within the 14 dwords that arrive preloaded in SGPRs, r_per_filter and norm_quats packed into one int (bits 0 and 1)."""
  if head:
    return (f"x, P, z, n, {'Q' if do_predict else 'nullptr'}, R, (r_per_filter != 0 ? 1 : 0) | (norm_quats != 0 ? 2 : 0), {obs}, "
            f"{'dt_vec, dt' if do_predict else 'nullptr, 0.0'}, flags, active")
  return f"x, P, z, R, r_per_filter, {obs}, {'Q, dt_vec, dt' if do_predict else 'nullptr, nullptr, 0.0'}, n, norm_quats, flags, active"


def launch_step(tiles, kind, do_predict, head=0):
  return _launch(tiles, f"k_step_{kind}<{'true' if do_predict else 'false'}>", _step_args("ea", do_predict, head))


def launch_step_ckpt(tiles, kind, head=0):
  return _launch(tiles, f"k_stepc_{kind}<true>", _step_args("ea", True, head) + ", ckpt_x, ckpt_P, ckpt_z")


def launch_kinds(tiles, do_predict, head=0):
  return _launch(tiles, f"k_kinds<{'true' if do_predict else 'false'}>", _step_args("kinds", do_predict, head))


def launch_maha(tiles, kind, ea=True):
  return _launch(tiles, f"k_maha_{kind}", f"x, P, z, R, r_per_filter, {'ea, ' if ea else ''}n, d2")
