"""Kernel family W, step-granular kernels, second structure: scalar phase lane-per-filter, matrix phase lane-group.

emit_wide.py evaluates the x-dependent scalars (f, F, h, H.H_mod, err_fun: ~2 000 instructions with the
accelerometer kind's gravity/rotation terms) redundantly in all 32 lanes of a filter's lane group, twice per
wavefront, and keeps them in VGPRs next to the covariance rows: 256 VGPRs + AGPR spills, 1 wave per SIMD, 13.7 % of
the HBM roofline on live (round-1 profile).  Here a wavefront owns a tile of FT filters and works in three phases:

  phase 1  lane l = filter l of the tile (FT lanes active): x, z -> f, F non-zeros, normalise, h, He = H.H_mod
           non-zeros, y = z - h; results go to the filter's scalar SLOT in LDS.  One evaluation per filter.
  phase 2  for each GROUP of filters (as many as fit a wavefront with one lane per row of P: 64 // dim_err, see
           filters_per_wave): the lane-group-per-filter covariance algebra of emit_wide.py, but every x-dependent
           coefficient is an LDS broadcast read from the slot; the next group's P records stream HBM -> LDS
           asynchronously (global_load_lds_dwordx4, double buffer) while the current group computes -- or, for small
           records, a single buffer and several wavefronts per SIMD (double_buffered).  dx goes back to the slot.
           Feature-track kinds of MSCKF models project G, Gt and He P He^T on the left null space of the
           extra-argument Jacobian with the reflectors phase 1 left in the slot (_lean_update).
  phase 3  lane l = filter l again: x' = err_fun(x, dx), renormalise, x / y / flags leave through LDS, coalesced.

The algebra and its order are unchanged (see emit_wide.py / emit_small.py docstrings); only who evaluates the
scalars changed.  Results agree with the first structure to rounding (different instruction streams contract
FMAs differently), which tests/test_gpu_run.py bounds.

Where things are: slot_tables() lowers a model once against a slot layout (Layout here; the fused runs and the smoother pass their own);
scalar_functions(), mat_predict_fn(), mat_predict_rts_fn(), mat_update_fns() return the phase functions, device_functions() all of them; the
update bodies and step_kernel() / maha_kernels() are each put together from the named pieces above them.
"""
import functools
import re
import types

import sympy as sp

from rednose_amd.codegen import emit_common, tuning
from rednose_amd.codegen.lower import Block, vector_names
from rednose_amd.codegen.emit_common import EADIM, SMat, SlotLayout, ea_count, ind, term, sum_terms, innovation_solver


def group_lanes(spec):
  """Lanes per filter in the matrix phase: one lane per row/column of P, groups packed back to back."""
  fpw = filters_per_wave(spec)
  if fpw == 1:
    return 64              # 33 .. 64 error states: the whole wavefront works on one filter
  return 32 if fpw == 2 else spec.dim_err     # two groups: one per 32-lane half (fewest LDS conflicts)


def filters_per_wave(spec):
  """Filters whose covariance algebra one wavefront does at a time (64 // dim_err, e.g. 3 for 21 error states:
  63 of 64 lanes busy instead of 42 with two 32-lane groups)."""
  if spec.dim_err > 32:
    return 1
  fpw = tuning.current().wide_fpw
  return fpw if fpw else max(2, 64 // spec.dim_err)


def tile_filters(spec):
  """Filters per wavefront tile: the tuning value rounded up to whole groups."""
  fpw = filters_per_wave(spec)
  ft = tuning.current().wide_ft
  if ft == 0:      # auto: small records (<= 16 error states) -> two groups per tile, several wavefronts per SIMD; else 16;
    #                above 40 error states 8, to keep the block's LDS (P buffer + per-filter slots) under 64 KB
    ft = 2 * fpw if spec.dim_err <= 16 else (16 if spec.dim_err <= 40 else 8)
  return -(-ft // fpw) * fpw


def double_buffered(spec):
  """Asynchronous double-buffered prefetch of the next group's covariance records, or a single buffer.  With small records
  several wavefronts fit per SIMD and hide each other's HBM latency, and the second buffer only costs occupancy
  (kinematic9: 25.5-26.3 us per launch with a single buffer and tiles of 14 filters, 30.5 us with the live-tuned 16 / double)."""
  db = tuning.current().wide_db
  return bool(db) if db >= 0 else 16 < spec.dim_err <= 40       # above 40 error states a second E x E buffer does not fit 64 KB


class Layout(SlotLayout):
  """Per-filter scalar slot in LDS (doubles)."""

  def pack(self, D, E):
    self.OFF_F = D
    self.OFF_Y = self.OFF_F + self.nf
    self.OFF_HE = self.OFF_Y + self.zmax
    self.OFF_DX = self.OFF_HE + self.nh
    self.OFF_DT = self.OFF_DX + E
    self.OFF_FL = self.OFF_DT + 1
    return self.feature_tail(self.OFF_FL + 1)


def _lowered_predict(spec):
  D, M = spec.dim_x, spec.dim_main_err
  names = {**vector_names(spec.x_sym, 'x'), spec.dt_sym: 'dt'}
  blk = Block(names, tmp_prefix="pt")
  for i in range(D):
    blk.add(f"xn_{i}", spec.f_sym[i])
  fmtF = lambda i, j: f"F_{i}_{j}"  # noqa: E731
  for i in range(M):
    for j in range(M):
      blk.add(fmtF(i, j), spec.F_sym[i, j])
  stmts, st = blk.lower()
  F = SMat.identity_padded(SMat.from_structure(M, M, st, fmtF), spec.dim_err)
  f_vars = [c[1] for row in F.e for c in row if c is not None and c[0] == 'var']
  return stmts, st, F, f_vars


def _lowered_obs(spec, k):
  E, Z = spec.dim_err, k.zdim
  names = dict(vector_names(spec.x_sym, 'x'))
  names.update(vector_names(k.ea_sym, 'ea'))
  Herr = sp.Matrix(k.H_sym) * sp.Matrix(spec.H_mod_sym)
  blk = Block(names, tmp_prefix="ut")
  for i in range(Z):
    blk.add(f"hx_{i}", k.h_sym[i])
  fmtH = lambda i, j: f"He_{i}_{j}"  # noqa: E731
  for i in range(Z):
    for j in range(E):
      blk.add(fmtH(i, j), Herr[i, j])
  if k.He_sym is not None:      # d h / d extra args (the reference's He_{kind}), Z x EADIM
    assert tuple(k.He_sym.shape) == (Z, EADIM), "feature-track kinds take EADIM = 3 extra arguments (ekf_sym.py:151)"
    for i in range(Z):
      for j in range(EADIM):
        blk.add(f"Hea_{i}_{j}", k.He_sym[i, j])
  stmts, st = blk.lower()
  He = SMat.from_structure(Z, E, st, fmtH)
  he_vars = [c[1] for row in He.e for c in row if c is not None and c[0] == 'var']
  return stmts, st, He, he_vars


def _obs_call(k, project):
  """Phase-1 call of kind k's scalar function for filter `lane` of the tile (extra args / R are per filter)."""
  Z = k.zdim
  feat = k.He_sym is not None
  args = f"sl, s_z + lane * {Z}"
  if ea_count(k):
    args += f", gea + (base + lane) * {ea_count(k)}"
  if feat:
    args += f", r_per_filter ? gR + (base + lane) * {Z * Z} : gR"
  return f"scal_obs_{k.kind}{'<' + project + '>' if feat else ''}({args})"


def _slotted(smat, var_list, off):
  """Copy of `smat` whose named entries read the filter's LDS slot instead of a register."""
  m = SMat(smat.rows, smat.cols)
  index = {v: i for i, v in enumerate(var_list)}
  for i in range(smat.rows):
    for j in range(smat.cols):
      e = smat.e[i][j]
      if e is not None and e[0] == 'var':
        m.e[i][j] = ('var', f"sl[{off + index[e[1]]}]")
      else:
        m.e[i][j] = e
  return m


def slot_tables(spec, lay_cls=None, with_obs=True):
  """The model lowered ONCE -> (slot layout of class `lay_cls`, slot-addressed F, {kind: slot-addressed He}, low); `low` = (_lowered_predict's,
  {kind: _lowered_obs's}) is for scalar_functions.  with_obs=False leaves the kinds alone (the smoother has no observation)."""
  pred = _lowered_predict(spec)
  obs = {k.kind: _lowered_obs(spec, k) for k in spec.kinds} if with_obs else {}
  lay = (lay_cls or Layout)(spec, pred[3], {kk: v[3] for kk, v in obs.items()})
  return lay, _slotted(pred[2], pred[3], lay.OFF_F), {kk: _slotted(v[2], v[3], lay.OFF_HE) for kk, v in obs.items()}, (pred, obs)


COEF_BATCH_MAX = 40      # coefficients held in registers at once by _in_registers (live: 33 of F, 27 of He; a denser model -- the 24-state
                         # random test model has 86 -- would spill under the 256-register budget of two wavefronts per SIMD: it keeps
                         # the slot reads where they are used)


def _in_registers(smat, name):
  """-> (copy of `smat` whose named entries are `name[i]`, C statements loading them from where the original read them): every
  coefficient of the register-lean matrix phase is read from the slot ONCE, all reads issued before the first use and held there by a
  scheduling barrier -- left alone hipcc sinks each LDS broadcast read next to its use, and every output of the phase becomes a
  read -> wait -> FMA -> write chain of its own.  live, dt > 0 launch at 16 384 filters, same call: 40.5 -> 37.8 us, results bit-identical."""
  m = SMat(smat.rows, smat.cols)
  src = []
  for i in range(smat.rows):
    for j in range(smat.cols):
      e = smat.e[i][j]
      if e is not None and e[0] == 'var':
        if e[1] not in src:
          src.append(e[1])
        m.e[i][j] = ('var', f"{name}[{src.index(e[1])}]")
      else:
        m.e[i][j] = e
  if not src or len(src) > COEF_BATCH_MAX:
    return (m if not src else smat), []
  loads = [f"double {name}[{len(src)}];"] + [f"{name}[{i}] = {v};" for i, v in enumerate(src)] + ["__builtin_amdgcn_sched_barrier(0);"]
  return m, loads


WIDE_Z_LDS = 7      # observation dimension from which the general update keeps the innovation covariance in LDS (below: in registers)


def wide_z(k, E):
  """The LDS path of the innovation covariance (_wide_obs_update: lane z forms row z of S, so Z <= E lanes of the filter's group are needed);
  a kind with more rows than the model has error states (Z > E) keeps the in-register general update whatever its size."""
  return WIDE_Z_LDS <= k.zdim <= E


def wide_s_doubles(k):
  """LDS doubles per filter of a wide kind's innovation covariance: S / its L D U factor in place, the reciprocal pivots, and a copy of
  S for the gated second factorisation."""
  Z = k.zdim
  return Z * Z + Z + (Z * Z if k.maha_test else 0)


# ---- the Joseph-form update, in the pieces its four bodies share (general, wide-Z, lean, and mat_maha_* up to the solve) --------------
# G = He P (lane cc holds column cc of it), Gt = P He^T (row cc), S = G He^T + R, K = Gt S^-1 (the lane's row of it: kk), dx = K y,
# P' = (P - K G) + Dm K^T with the Joseph correction Dm = K R - B He^T, B = P - K G.  He's generation-time non-zeros carry every product.
def _row_dot(m, i, operand):
  """C text of row i of the structured matrix m (He, F) against a vector whose entry j is the text operand(j): a term per non-zero."""
  return sum_terms(term(cf, operand(j)) for j, cf in m.row_nz(i))


def _load_row(E, more=""):
  return [f"double row[{E}]{more};", "#pragma unroll", f"for (int j = 0; j < {E}; j++) row[j] = sP[cc * {E} + j];"]


def _load_col(E, more=""):
  return [f"double col[{E}]{more};", "#pragma unroll", f"for (int kq = 0; kq < {E}; kq++) col[kq] = sP[kq * {E} + cc];"]


def _g_gt(Hs, Z, col, row=None, gt="const double Gt_{z} = {e};"):
  """G_z from the lane's column of P (entry k: col(k)) and, with `row`, Gt_z from its row, declared as the line `gt`."""
  b = []
  for zi in range(Z):
    b.append(f"const double G_{zi} = {_row_dot(Hs, zi, col)};")
    if row:
      b.append(gt.format(z=zi, e=_row_dot(Hs, zi, row)))
  return b


def _store_g(Z, E):
  return ["if (act) { " + " ".join(f"sG[{zi} * {E} + cc] = G_{zi};" for zi in range(Z)) + " }", "rn::wave_lds_sync();"]


def _hph(Hs, Z, E, dst="HPH", plus_r=False):
  """He P He^T from the rows of G in sG (every lane forms all of it), into `dst`; plus_r: + R at once."""
  return [f"{dst}[{zi * Z + w}] = " + _row_dot(Hs, w, lambda j, zi=zi: f"sG[{zi} * {E} + {j}]") + (f" + R[{zi * Z + w}];" if plus_r else ";")
          for zi in range(Z) for w in range(Z)]


def _s_decl(Z):
  return f"double HPH[{Z * Z}], Rl[{Z * Z}], S[{Z * Z}], L[{Z * Z}], iL[{Z}];"


def _solve_gain(k, Z, yoff):
  """S = HPH + R factored, the gate on the residual at sl[yoff ..], and kk <- S^-1 Gt.
  S is solved as a GENERAL matrix (L D U): the step-granular kernels follow the reference on asymmetric covariances (ekf_c.c:100-101)."""
  factor, gate, solve = innovation_solver(Z, True, [f"sl[{yoff + i}]" for i in range(Z)], k.maha_thresh if k.maha_test else None)
  return (["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) {{ Rl[i] = R[i]; S[i] = HPH[i] + Rl[i]; }}", factor, "int gated = 0;"] + gate +
          [f"double kk[{Z}] = {{{', '.join(f'Gt_{zi}' for zi in range(Z))}}};", solve("kk")])


def _dxc(Z, yoff):
  return "const double dxc = " + " + ".join(f"kk[{zi}]*sl[{yoff + zi}]" for zi in range(Z)) + ";"


def _dm(Z, c, r="Rl", rs="", guard=""):
  """Dm_z = [rs *] (K R)_z - c(z), c(z) the text of (B He^T)_z; `guard`: the condition prefix under which it is zero instead."""
  return [f"const double Dm_{zi} = {guard}{rs}(" + " + ".join(f"kk[{w}]*{r}[{w * Z + zi}]" for w in range(Z)) + f") - ({c(zi)});" for zi in range(Z)]


def _store_k(Z, E, lay, fl="(double)gated"):
  """The lane's row of K to sK, its dx and (lane 0) the filter's flag to the slot."""
  return ["if (act) { " + " ".join(f"sK[{zi} * {E} + cc] = kk[{zi}];" for zi in range(Z)) + f" sw[{lay.OFF_DX} + cc] = dxc; if (cc == 0) sw[{lay.OFF_FL}] = {fl}; }}",
          "rn::wave_lds_sync();"]


def _rank_z(E, Z, op, coef, src):
  """Rank-Z pass over the lane's row in registers, unrolled: row[j] op= sum_z coef_z * src[z][j]."""
  return [f"row[{j}] {op} " + " + ".join(f"{coef.format(zi)}*{src}[{zi * E + j}]" for zi in range(Z)) + ";" for j in range(E)]


def _store_row(E):
  return ["if (act) {", "#pragma unroll", f"  for (int j = 0; j < {E}; j++) sP[cc * {E} + j] = row[j];", "}", "rn::wave_lds_sync();"]


def _rank_z_rolled(E, Z, src, unroll):
  """Both rank-Z passes in ONE rolled pass over the lane's row (`src`: its registers or LDS), the result going to LDS as it is formed."""
  return ["if (act) {", unroll, f"  for (int j = 0; j < {E}; j++) {{",
          f"    const double bj = {src} - (" + " + ".join(f"kk[{zi}]*sG[{zi * E} + j]" for zi in range(Z)) + ");",
          "    pr[j] = bj + (" + " + ".join(f"Dm_{zi}*sK[{zi * E} + j]" for zi in range(Z)) + ");", "  }", "}", "rn::wave_lds_sync();"]


def _finish_in_registers(Hs, Z, E, lay, **dm):
  """From the gain kk, the lane's row in registers: dx, B = P - K G, Dm (`dm`: its R and scale), K to sK, P' = B + Dm K^T to sP."""
  return ([_dxc(Z, lay.OFF_Y)] + _rank_z(E, Z, "-=", "kk[{}]", "sG") + _dm(Z, lambda zi: _row_dot(Hs, zi, "row[{}]".format), **dm) + _store_k(Z, E, lay) +
          _rank_z(E, Z, "+=", "Dm_{}", "sK") + _store_row(E))


def _general_update(k, Hs, lay, E):
  """The update as the reference writes it (on asymmetric P too), everything in registers."""
  Z = k.zdim
  b = _load_row(E, f", R[{Z * Z}]") + _load_col(E)
  b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = gR[i];", "rn::wave_lds_sync();"]
  b += _g_gt(Hs, Z, "col[{}]".format, "row[{}]".format) + _store_g(Z, E)
  b += [_s_decl(Z)] + _hph(Hs, Z, E) + _solve_gain(k, Z, lay.OFF_Y)
  return b + _finish_in_registers(Hs, Z, E, lay)


def _wide_obs_update(k, Hs, lay, E):
  """The general (reference-on-asymmetric-P) update for a WIDE observation kind: Z >= 7.  In registers the five Z x Z matrices of the
  ordinary path (R, He P He^T, the gated copy, S, its factor) are 405 doubles for Z = 9 -- the 10-state test model with a 9-dimensional
  kind shipped with 516 B of scratch.  Here S lives in the filter's LDS buffer sS: lane z < Z forms row z of S = G He^T + R (the
  generation-time sparsity is in He's rows, the lane only picks its row of G), the group factors it IN PLACE as L D U without pivoting
  -- column by column, lane i eliminating its own row against the broadcast pivot row (two fences per column) -- and every lane solves
  its own right-hand side against the factor with broadcast reads.  R is read from memory where it is used (the gate's 1e16 as a scalar)."""
  Z = k.zdim
  ZZ = Z * Z
  b = _load_row(E) + _load_col(E) + ["rn::wave_lds_sync();", f"double kk[{Z}];"]
  b += _g_gt(Hs, Z, "col[{}]".format, "row[{}]".format, gt="kk[{z}] = {e};      // Gt") + _store_g(Z, E)
  b.append(f"static_assert({Z} <= {E}, \"a lane per row of the innovation covariance\");")
  b.append(f"const bool zrow = act && cc < {Z};")
  b.append(f"const int zc = cc < {Z} ? cc : 0;")
  b.append(f"const double* gz_ = sG + zc * {E};")
  b.append("{")
  for w in range(Z):
    b.append(f"  const double s_{w} = {_row_dot(Hs, w, 'gz_[{}]'.format)} + gR[zc * {Z} + {w}];")
  b.append("  if (zrow) { " + " ".join(f"sS[cc * {Z} + {w}] = s_{w};" + (f" sS[{ZZ + Z} + cc * {Z} + {w}] = s_{w};" if k.maha_test else "") for w in range(Z)) + " }")
  b.append("}")
  b.append("rn::wave_lds_sync();")

  def factor():
    f = []
    for j in range(Z):
      f.append("{")
      f.append(f"  const double id_ = rn::fast_recip(sS[{j * Z + j}]);")
      if j + 1 < Z:
        f.append(f"  double pj[{Z - j - 1}], rw[{Z - j - 1}];")
        f += ["#pragma unroll", f"  for (int m = {j + 1}; m < {Z}; m++) {{ pj[m - {j + 1}] = sS[{j * Z} + m]; rw[m - {j + 1}] = sS[zc * {Z} + m]; }}"]
        f.append(f"  const double l_ = sS[zc * {Z} + {j}] * id_;")
      f.append("  rn::wave_lds_sync();")
      f.append("  if (zrow) {")
      if j + 1 < Z:
        f.append(f"    if (cc > {j}) {{")
        f.append(f"      sS[cc * {Z} + {j}] = l_;")
        f += ["#pragma unroll", f"      for (int m = {j + 1}; m < {Z}; m++) sS[cc * {Z} + m] = rw[m - {j + 1}] - l_ * pj[m - {j + 1}];", "    }"]
        f.append(f"    if (cc == {j}) {{")
        f += ["#pragma unroll", f"      for (int m = {j + 1}; m < {Z}; m++) sS[{j * Z} + m] = pj[m - {j + 1}] * id_;", "    }"]
      f.append(f"    if (cc == {j}) sS[{ZZ + j}] = id_;")
      f.append("  }")
      f.append("  rn::wave_lds_sync();")
      f.append("}")
    return f
  b += factor()
  b.append("int gated = 0;")
  b.append("double rs = 1.0;")
  if k.maha_test:
    ys = [f"sl[{lay.OFF_Y + i}]" for i in range(Z)]
    b += ["{", f"  double v[{Z}] = {{{', '.join(ys)}}}, w[{Z}] = {{{', '.join(ys)}}};"]
    for i in range(Z):
      if i:
        b.append(f"  v[{i}] -= " + " + ".join(f"sS[{i * Z + kq}]*v[{kq}]" for kq in range(i)) + ";")
        b.append(f"  w[{i}] -= " + " + ".join(f"sS[{kq * Z + i}]*w[{kq}]" for kq in range(i)) + ";")
    b.append("  const double d2 = " + " + ".join(f"v[{i}]*w[{i}]*sS[{ZZ + i}]" for i in range(Z)) + ";")
    b.append(f"  gated = d2 > {k.maha_thresh!r} ? 1 : 0;      // (uniform over the filter's lanes: every lane evaluates the same numbers)")
    b.append("}")
    b.append("rn::wave_lds_sync();")
    b.append("if (gated) {      // R *= 1e16 (ekf_c.c:88-94) and a second factorisation, from the kept copy of S = He P He^T + R")
    b.append("  rs = 1.0e16;")
    b.append("  if (zrow) { " + " ".join(f"sS[cc * {Z} + {w}] = sS[{ZZ + Z} + cc * {Z} + {w}] + (1.0e16 - 1.0) * gR[cc * {Z} + {w}];" for w in range(Z)) + " }")
    b.append("  rn::wave_lds_sync();")
    b += ind(factor())
    b.append("}")
  # kk <- (L D U)^-1 Gt: the factor by broadcast reads
  for i in range(1, Z):
    b.append(f"kk[{i}] -= " + " + ".join(f"sS[{i * Z + kq}]*kk[{kq}]" for kq in range(i)) + ";")
  for i in range(Z - 1, -1, -1):
    tail = "".join(f" - sS[{i * Z + kq}]*kk[{kq}]" for kq in range(i + 1, Z))
    b.append(f"kk[{i}] = kk[{i}]*sS[{ZZ + i}]{tail};")
  return b + _finish_in_registers(Hs, Z, E, lay, r="gR", rs="rs*")


def _lean_update(k, Hs, lay, E, rows_in_regs=False):
  """Update with the Joseph correction Dm = K R - B He^T formed from Gt - K (He P He^T) (the same quantity, B = P - K G
  never materialised), only the columns of P that He touches read, and ONE pass over the lane's row:
  P'[cc, j] = (P[cc, j] - sum_z K_z G[z, j]) + sum_z Dm_z K[j, z].  rows_in_regs=False leaves the row in LDS (rolled
  in-place pass, a few dozen live registers: two or more wavefronts per SIMD).

  Feature-track kinds (k.He_sym, MSCKF): G, Gt and the rows of He P He^T are taken to the left null space of the
  extra-argument Jacobian by the reflectors phase 1 left in the slot (ekf_c.c:66-76: H <- A^T H); everything after
  that is the ordinary update with Z - EADIM rows and the projected y / R of the slot."""
  Zf = k.zdim
  feat = k.He_sym is not None
  Z = Zf - EADIM if feat else Zf
  used = sorted({kk for zi in range(Zf) for kk, _ in Hs.row_nz(zi)})
  reflect = f"rn::apply_reflectors<{Zf}, {EADIM}>(sl + {lay.OFF_RF}, sl + {lay.OFF_RF + EADIM * Zf}, {{}});"
  b = [f"double R[{Z * Z}];", f"double* pr = sP + cc * {E};"]
  if not feat:      # the non-zeros of He (27 for live) are read from the slot once, up front, behind a scheduling barrier (_in_registers)
    Hs, coef_loads = _in_registers(Hs, "hc")
    b += coef_loads
  if rows_in_regs:
    b += [f"double row[{E}];", "#pragma unroll", f"for (int j = 0; j < {E}; j++) row[j] = pr[j];"]
  b += [f"const double col_{kk} = sP[{kk} * {E} + cc], row_{kk} = {'row' if rows_in_regs else 'pr'}[{kk}];" for kk in used]
  if feat:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = sl[{lay.OFF_RP} + i];      // A^T R A (phase 1)", "(void)gR;"]
    b.append(f"double G0[{Zf}] = {{" + ", ".join(_row_dot(Hs, zi, "col_{}".format) for zi in range(Zf)) + "};")
    b.append(f"double Gt0[{Zf}] = {{" + ", ".join(_row_dot(Hs, zi, "row_{}".format) for zi in range(Zf)) + "};")
    b += [reflect.format("G0"), reflect.format("Gt0")]
    for zi in range(Z):
      b.append(f"const double G_{zi} = G0[{EADIM + zi}], Gt_{zi} = Gt0[{EADIM + zi}];")
    b.append(f"const double rank_deficient = sl[{lay.OFF_FL}];      // 4.0 when phase 1 found Hea rank deficient")
  else:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = gR[i];"]
    b += _g_gt(Hs, Z, "col_{}".format, "row_{}".format)
  b += _store_g(Z, E)
  b.append(_s_decl(Z))
  if feat:
    for zi in range(Z):
      b.append("{")
      b.append(f"  double m[{Zf}] = {{" + ", ".join(_row_dot(Hs, w, lambda j, zi=zi: f"sG[{zi} * {E} + {j}]") for w in range(Zf)) + "};")
      b.append("  " + reflect.format("m"))
      b += ["#pragma unroll", f"  for (int w = 0; w < {Z}; w++) HPH[{zi * Z} + w] = m[{EADIM} + w];", "}"]
  else:
    b += _hph(Hs, Z, E)
  YO = lay.OFF_YP if feat else lay.OFF_Y      # the residual the update consumes (feature-track kinds: the one in the reflectors' basis)
  b += _solve_gain(k, Z, YO)
  if feat:     # the reference's numpy path ignores a measurement whose null-space projection failed (ekf_sym.py:589-591)
    b += ["if (rank_deficient != 0.0) {", "#pragma unroll", f"  for (int i = 0; i < {Z}; i++) kk[i] = 0.0;", "}"]
  b.append(_dxc(Z, YO))
  b += _dm(Z, lambda zi: f"Gt_{zi} - (" + " + ".join(f"kk[{w}]*HPH[{w * Z + zi}]" for w in range(Z)) + ")", guard="rank_deficient != 0.0 ? 0.0 : " if feat else "")
  b += _store_k(Z, E, lay, fl="(double)gated + rank_deficient" if feat else "(double)gated")
  return b + (_rank_z_rolled(E, Z, "row[j]", "#pragma unroll") if rows_in_regs else _rank_z_rolled(E, Z, "pr[j]", "#pragma unroll 2"))


def _update_body(k, E):
  """-> (the builder of kind k's matrix update, does it take the LDS buffer sS)."""
  if tuning.current().wide_lean == 1:
    return _lean_update, False
  if k.He_sym is not None:
    return functools.partial(_lean_update, rows_in_regs=True), False
  return (_wide_obs_update, True) if wide_z(k, E) else (_general_update, False)


# ---- phase functions.  They have pointer-only interfaces (state lives in LDS between them) and are inlined by default: inlined
# into the group loop hipcc keeps ~460 registers live (1 wave/SIMD); __noinline__ (tuning knob wide_inline=0) keeps each
# under 256 but pays scratch frames and is 5x slower.
def _inl():
  return "__forceinline__" if tuning.current().wide_inline else "__noinline__"


def _normq(spec):
  quat = "".join(f" rn::normalize_quat<{spec.dim_x}>(x, {q});" for q in spec.quaternion_idxs)
  return f"if (norm_quats) {{{quat} }}" if spec.quaternion_idxs else "(void)norm_quats;"


def _x_in(D, src):
  return [f"double x[{D}];", "#pragma unroll", f"for (int i = 0; i < {D}; i++) x[i] = {src};"]


def _x_out(D, dst):
  return ["#pragma unroll", f"for (int i = 0; i < {D}; i++) {dst} = x[i];"]


def _scal_predict(spec, lay, low, sfx):
  """phase 1, scalars of predict: x <- f(x) [normalised], the non-trivial entries of F and dt to the slot."""
  D = spec.dim_x
  pst, pstruct, _, f_vars = low[0]
  b = _x_in(D, "xin[i]")
  # every non-trivial entry of F goes to the slot as soon as it exists (short live ranges: a dense F is hundreds of values)
  f_at = {v: i for i, v in enumerate(f_vars)}
  stored = set()
  for st_ in pst:
    b.append(st_)
    mm = re.match(r"\s*const double (\w+) =", st_)
    if mm and mm.group(1) in f_at:
      b.append(f"sl[{lay.OFF_F + f_at[mm.group(1)]}] = {mm.group(1)};")
      stored.add(mm.group(1))
      if len(stored) % 32 == 0:
        b.append("rn::wave_lds_sync();      // (a scheduling boundary: keeps hipcc from computing everything before storing anything)")
  for i, v in enumerate(f_vars):
    if v not in stored:
      b.append(f"sl[{lay.OFF_F + i}] = {v};")
  for i in range(D):
    kind, val = pstruct[f"xn_{i}"]
    b.append(f"x[{i}] = xn_{i};" if kind == 'expr' else f"x[{i}] = {float(val)!r};")
  b += [_normq(spec), f"sl[{lay.OFF_DT}] = dt;"] + _x_out(D, f"sl[{lay.OFF_X} + i]")
  return "\n".join([f"__device__ {_inl()} void scal_predict{sfx}(const double* xin, const double dt, double* sl, const int norm_quats) {{"] + ind(b) + ["}"])


def _scal_keep(spec, lay, low, sfx):
  """phase 1 without a predict: x [normalised] to the slot."""
  D = spec.dim_x
  b = _x_in(D, "xin[i]") + [_normq(spec)] + _x_out(D, f"sl[{lay.OFF_X} + i]")
  return "\n".join([f"__device__ {_inl()} void scal_keep{sfx}(const double* xin, double* sl, const int norm_quats) {{"] + ind(b) + ["}"])


def _scal_obs(spec, lay, low, sfx, k):
  """phase 1, scalars of observation kind k: the non-zeros of He = H H_mod and y = z - h(x) to the slot."""
  D, Z, EA = spec.dim_x, k.zdim, ea_count(k)
  stmts, st, _, he_vars = low[1][k.kind]
  feat = k.He_sym is not None
  b = [f"double x[{D}], z[{Z}];", "#pragma unroll", f"for (int i = 0; i < {D}; i++) x[i] = sl[{lay.OFF_X} + i];",
       "#pragma unroll", f"for (int i = 0; i < {Z}; i++) z[i] = zin[i];"]
  if EA:
    b += [f"double ea[{EA}];", "#pragma unroll", f"for (int i = 0; i < {EA}; i++) ea[i] = eain[i];"]
  b += list(stmts)
  val = lambda nm: nm if st[nm][0] == 'expr' else repr(float(st[nm][1] or 0.0))  # noqa: E731
  for i, v in enumerate(he_vars):
    b.append(f"sl[{lay.OFF_HE + i}] = {v};")
  if not feat:
    for i in range(Z):
      b.append(f"sl[{lay.OFF_Y + i}] = z[{i}] - {val(f'hx_{i}')};")
  else:
    # ekf_c.c:66-76: residual and R go to the left null space of Hea; the reflectors stay in the slot for phase 2
    Zp = Z - EADIM
    b.append(f"double y[{Z}] = {{{', '.join(f'z[{i}] - ' + val(f'hx_{i}') for i in range(Z))}}};")
    b.append("if (PROJECT) {")
    hea = ", ".join(("0.0" if st[f"Hea_{i}_{j}"][0] == 'zero' else ("1.0" if st[f"Hea_{i}_{j}"][0] == 'one' else val(f"Hea_{i}_{j}")))
                    for i in range(Z) for j in range(EADIM))
    b += [f"  double Hea[{Z * EADIM}] = {{{hea}}};", f"  double u[{EADIM * Z}], beta[{EADIM}], yref[{Zp}];",
          f"  const bool ok2 = rn::nullspace_residual<{Z}, {EADIM}>(Hea, y, yref);      // y in the reference's basis (ekf_c.c:71-73); Hea and y are modified below",
          f"  const bool ok = rn::householder_qr<{Z}, {EADIM}>(Hea, u, beta) && ok2;",
          f"  rn::apply_reflectors<{Z}, {EADIM}>(u, beta, y);",
          "#pragma unroll", f"  for (int i = 0; i < {EADIM * Z}; i++) sl[{lay.OFF_RF} + i] = u[i];",
          "#pragma unroll", f"  for (int i = 0; i < {EADIM}; i++) sl[{lay.OFF_RF + EADIM * Z} + i] = beta[i];",
          "#pragma unroll", f"  for (int i = 0; i < {Zp}; i++) {{ sl[{lay.OFF_YP} + i] = ok ? y[{EADIM} + i] : 0.0; sl[{lay.OFF_Y} + i] = ok ? yref[i] : 0.0; }}",
          "#pragma unroll", f"  for (int i = {Zp}; i < {Z}; i++) sl[{lay.OFF_Y} + i] = z[i];      // y has Z - EADIM rows (ekf_c.c:120)",
          f"  sl[{lay.OFF_FL}] = ok ? 0.0 : 4.0;",
          f"  double Rm[{Z * Z}];", "#pragma unroll", f"  for (int i = 0; i < {Z * Z}; i++) Rm[i] = gRf[i];",
          f"  rn::project_noise<{Z}, {EADIM}>(u, beta, Rm);",
          "#pragma unroll", f"  for (int a = 0; a < {Zp}; a++) {{", "#pragma unroll",
          f"    for (int c = 0; c < {Zp}; c++) sl[{lay.OFF_RP} + a * {Zp} + c] = Rm[({EADIM} + a) * {Z} + {EADIM} + c];", "  }",
          "} else {", "#pragma unroll", f"  for (int i = 0; i < {Z}; i++) sl[{lay.OFF_Y} + i] = y[i];", "}"]
  tmpl = "template <bool PROJECT>\n" if feat else ""
  sig = "double* sl, const double* zin" + (", const double* eain" if EA else "") + (", const double* gRf" if feat else "")
  return "\n".join([f"{tmpl}__device__ {_inl()} void scal_obs_{k.kind}{sfx}({sig}) {{"] + ind(b) + ["}"])


def _scal_inject(spec, lay, low, sfx):
  """phase 3: x <- err_fun(x, dx) [normalised]; -> 2 when the new state is not finite."""
  D, E = spec.dim_x, spec.dim_err
  nom, delta = spec.err_eqs[1], spec.err_eqs[2]
  enames = dict(vector_names(nom, 'x'))
  enames.update({(delta, i, 0): f"sl[{lay.OFF_DX + i}]" for i in range(E)})
  eblk = Block(enames, tmp_prefix="et")
  for i in range(D):
    eblk.add(f"xi_{i}", sp.Matrix(spec.err_eqs[0])[i])
  estmts, est = eblk.lower()
  b = _x_in(D, f"sl[{lay.OFF_X} + i]") + list(estmts)
  for i in range(D):
    kind, val = est[f"xi_{i}"]
    b.append(f"x[{i}] = xi_{i};" if kind == 'expr' else f"x[{i}] = {float(val)!r};")
  b.append(_normq(spec))
  b += _x_out(D, "xout[i]") + ["double acc = 0.0;", "#pragma unroll",
        f"for (int i = 0; i < {D}; i++) acc += x[i];", "return (acc - acc == 0.0) ? 0 : 2;"]
  return "\n".join([f"__device__ {_inl()} int scal_inject{sfx}(const double* sl, double* xout, const int norm_quats) {{"] + ind(b) + ["}"])


def scalar_functions(spec, lay, low, sfx="", only=None):
  """Texts of the scalar phase functions against the slot layout `lay` under names suffixed `sfx`: scal_predict, scal_keep, scal_obs_{kind},
  scal_inject.  `low`: slot_tables()'s; `only`: the (unsuffixed) names to emit instead of all."""
  fns = [("scal_predict", _scal_predict), ("scal_keep", _scal_keep)]
  fns += [(f"scal_obs_{k.kind}", functools.partial(_scal_obs, k=k)) for k in spec.kinds] + [("scal_inject", _scal_inject)]
  return [fn(spec, lay, low, sfx) for name, fn in fns if only is None or name in only]


def mat_predict_fn(spec, lay, Fs):
  """phase 2, matrix part of predict: P in sP -> F P F^T + dt Q in sP."""
  E = spec.dim_err
  tune = tuning.current()
  lean_p = tune.wide_lean == 1      # predict through LDS only in the fully lean variant
  dt = f"const double dt = sl[{lay.OFF_DT}];"
  if lean_p:
    # rows, then columns, pass through ONE register array; every result goes straight back to LDS (in place: the lane's
    # own row / column is in registers, other lanes' are untouched), so nothing but the array stays live
    b = [dt, f"double v[{E}];"]
    Fp, coef_loads = _in_registers(Fs, "fc")      # the non-zeros of F (33 for live): one batch of slot reads, not one read-wait-FMA chain per output
    b += coef_loads
    b += ["if (act) {", "#pragma unroll", f"  for (int j = 0; j < {E}; j++) v[j] = sP[cc * {E} + j];"]
    for i in range(E):
      b.append(f"  sP[cc * {E} + {i}] = {_row_dot(Fp, i, 'v[{}]'.format)};")
    b += ["}", "rn::wave_lds_sync();", "if (act) {", "#pragma unroll", f"  for (int k = 0; k < {E}; k++) v[k] = sP[k * {E} + cc];"]
    for i in range(E):
      qv = f"qcol[{i}]" if tune.wide_lean_q else f"sQ[{i} * {E} + cc]"
      b.append(f"  sP[{i} * {E} + cc] = {_row_dot(Fp, i, 'v[{}]'.format)} + dt*{qv};")
    b += ["}", "rn::wave_lds_sync();"]
  else:
    b = [dt, f"double row[{E}], a[{E}], col[{E}];", "#pragma unroll",
         f"for (int j = 0; j < {E}; j++) row[j] = sP[cc * {E} + j];"]
    for i in range(E):
      b.append(f"a[{i}] = {_row_dot(Fs, i, 'row[{}]'.format)};")
    b += ["if (act) {", "#pragma unroll", f"  for (int i = 0; i < {E}; i++) sP[cc * {E} + i] = a[i];", "}", "rn::wave_lds_sync();",
          "#pragma unroll", f"for (int k = 0; k < {E}; k++) a[k] = sP[k * {E} + cc];"]
    for i in range(E):
      b.append(f"col[{i}] = {_row_dot(Fs, i, 'a[{}]'.format)} + dt*qcol[{i}];")
    b += ["rn::wave_lds_sync();", "if (act) {", "#pragma unroll", f"  for (int k = 0; k < {E}; k++) sP[k * {E} + cc] = col[k];", "}",
          "rn::wave_lds_sync();"]
  qarg = "const double* sQ" if (lean_p and not tune.wide_lean_q) else f"const double (&qcol)[{E}]"
  return "\n".join([f"__device__ {_inl()} void mat_predict(double* sP, {qarg}, const double* sl, const int cc, const bool act) {{"] + ind(b) + ["}"])


def mat_predict_rts_fn(spec, lay, Fs):
  """Smoother (templates/ekf_hip_rts.h, k_rts_group): main block of the predicted pair from a row held in registers.
  row = row c of Pk_k[:M, :M]; y <- column c of F Pk_k^T; sB (M x M, stride M) <- F Pk_k F^T + dt Q[:M, :M].
  Only two register vectors are live at a time (y + the column of P F^T): each entry of the result goes to LDS as soon as
  it is formed -- the lane rewrites its OWN column of sB, which no other lane reads in this function."""
  E, M = spec.dim_err, spec.dim_main_err
  b = [f"const double dt = sl[{lay.OFF_DT}];"]
  for i in range(M):
    b.append(f"y[{i}] = {sum_terms(term(cf, f'row[{kk}]') for kk, cf in Fs.row_nz(i) if kk < M)};")
  b += ["if (act) {", "#pragma unroll", f"  for (int i = 0; i < {M}; i++) sB[cc * {M} + i] = y[i];", "}", "rn::wave_lds_sync();",
        f"double a[{M}];", "#pragma unroll", f"for (int k = 0; k < {M}; k++) a[k] = sB[k * {M} + cc];", "rn::wave_lds_sync();"]
  for i in range(M):
    b.append(f"{{ const double v = {sum_terms(term(cf, f'a[{kk}]') for kk, cf in Fs.row_nz(i) if kk < M)} + dt*gQc[{i * E}]; if (act) sB[{i * M} + cc] = v; }}")
  b += ["rn::wave_lds_sync();"]
  return "\n".join([f"__device__ __forceinline__ void mat_predict_rts(const double (&row)[{M}], double* sB, const double* __restrict__ gQc, "
                    f"const double* sl, const int cc, const bool act, double (&y)[{M}]) {{"] + ind(b) + ["}"])


def mat_update_fns(spec, lay, Hss):
  """phase 2, matrix part of the update, a function per kind: its body is _update_body()'s."""
  E = spec.dim_err
  out = []
  for k in spec.kinds:
    body, takes_ss = _update_body(k, E)
    out.append("\n".join([f"__device__ {_inl()} void mat_update_{k.kind}(double* sP, const double* __restrict__ gR, const double* sl, double* sw, "
                          f"double* sG, double* sK{', double* sS' if takes_ss else ''}, const int cc, const bool act) {{"] + ind(body(k, Hss[k.kind], lay, E)) + ["}"]))
  return out


def device_functions(spec, lay_cls=None, sfx=""):
  """Phase functions of the three-phase kernels -> (text, slot layout).  With `lay_cls` / `sfx` only the scalar phases are
  emitted, against another slot layout and under suffixed names (the fused runs keep more compact slots: emit_wide3, emit_run2)."""
  lay, Fs, Hss, low = slot_tables(spec, lay_cls)
  scal = scalar_functions(spec, lay, low, sfx)
  if lay_cls is not None:
    return "\n\n".join(scal), lay
  return "\n".join(scal + [mat_predict_fn(spec, lay, Fs), mat_predict_rts_fn(spec, lay, Fs)] + mat_update_fns(spec, lay, Hss)), lay


# ---- the pieces step_kernel and maha_kernels put their kernels together from: lines of kernel text, a parameter where the two texts differ
def _geometry(spec, maha=False):
  """Sizes of a kernel.  DB: double buffer; ODD: can a group's record start on an odd double?  PBUF: doubles of a buffer of P (one slack double for
  the shifted image, whole 16-byte vectors), CPIN: the copy that fills it (k_maha_* always has the room and the copy for the shift, and one buffer)."""
  g = types.SimpleNamespace(D=spec.dim_x, E=spec.dim_err, EE=spec.dim_err ** 2, FT=tile_filters(spec), FPW=filters_per_wave(spec), GL=group_lanes(spec))
  g.DB = 1 if double_buffered(spec) and not maha else 0
  g.ODD = (g.FPW * g.EE) % 2 == 1 or (g.FT * g.EE) % 2 == 1
  g.PBUF = (g.FPW * g.EE + (3 if g.ODD or maha else 1)) // 2 * 2
  g.CPIN = "rn::async_copy_g2l_any" if g.ODD or maha else "rn::async_copy_g2l"
  return g


def _stamp(on, idx):
  """Debug stamp (tuning knob wide_timeline): [block][slot idx][0] = shader cycles, [1] = 100 MHz wall clock."""
  return [f"    if (lane == 0 && blockIdx.x < 256) {{ const int ti_ = {idx}; if (ti_ < 64) {{ g_tl[(blockIdx.x * 64 + ti_) * 2] = __builtin_readcyclecounter(); "
          "g_tl[(blockIdx.x * 64 + ti_) * 2 + 1] = wall_clock64(); } }"] if on else []


def _stamp_block(on, which):
  """Start (0) / end (1) of EVERY workgroup's first tile."""
  return [f"    if (lane == 0 && tile == blockIdx.x && blockIdx.x < 4096) g_tlb[blockIdx.x * 2{' + 1' if which else ''}] = wall_clock64();"] if on else []


def _signature(kname, upd, mixed, ckpt):
  tune = tuning.current()
  lbs = f"__launch_bounds__(64, {tune.wide_lb})" if tune.wide_lb else "__launch_bounds__(64)"
  tmpl = "template <bool DO_PREDICT>\n" if upd else ""
  sig_obs = ("double* __restrict__ gz, const double* __restrict__ gR, const int r_per_filter, " +
             ("const int32_t* __restrict__ gkinds" if mixed else "const double* __restrict__ gea") + ",\n    " if upd else "")
  flags_arg = (", uint8_t* __restrict__ flags" if upd else "") + ", const uint8_t* __restrict__ active"
  if ckpt:
    flags_arg += ", double* __restrict__ cx, double* __restrict__ cP, double* __restrict__ cz"
  return [f"{tmpl}__global__ {lbs} void {kname}(double* __restrict__ gx, double* __restrict__ gP,",
          f"    {sig_obs}const double* __restrict__ gQ, const double* __restrict__ gdt, const double dt_scalar, const int64_t n,",
          f"    const int norm_quats{flags_arg}) {{"]


def _lds_decls(g, p_decl, Z=0, K=True, S=0, mixed=False):
  """The block's LDS: the buffer(s) of P, the tile's x and z, a group's G / K^T, S doubles per filter of a wide kind, the slots, a mixed tile's kinds."""
  sh = "  __shared__ __attribute__((aligned(16))) double "
  L = [sh + p_decl, sh + f"s_x[FT2 * {g.D} + 2];"]
  if Z:
    L += [sh + f"s_z[FT2 * {Z} + 2];", sh + f"s_G[{g.FPW} * {Z * g.E}];"]
    if K:
      L.append(sh + f"s_K[{g.FPW} * {Z * g.E}];")
    if S:
      L.append(sh + f"s_S[{g.FPW} * {S}];      // the wide kind's innovation covariance, factored in place (_wide_obs_update)")
  L.append(sh + "s_sl[FT2 * SLOT];")
  if mixed:
    L.append("  __shared__ int s_kd[FT2];      // the kind each filter of the tile is updated with; 0: none (masked out, or not a kind of this model)")
  return L


def _lanes(g):
  return ["  const int lane = threadIdx.x;", f"  const int g = lane / {g.GL};", f"  const int c = lane % {g.GL};",
          f"  const bool act = c < {g.E} && g < {g.FPW};", "  const int cc = act ? c : 0;"]


def _q_fetch(g, dop, off=""):
  return f"qcol[i] = ({dop} && gQ != nullptr) ? gQ[i * {g.E} + cc{off}] : 0.0;"


def _q_staging(g, dop):
  tune = tuning.current()
  if tune.wide_lean == 1 and not tune.wide_lean_q:
    return [f"  __shared__ __attribute__((aligned(16))) double s_Q[{g.EE}];      // process noise, staged once per wavefront",
            f"  for (int i = lane; i < {g.EE}; i += 64) s_Q[i] = ({dop} && gQ != nullptr) ? gQ[i] : 0.0;", "  const double* qcol = s_Q;"]
  if tune.wide_lean == 1:
    return [f"  double qcol[{g.E}];                          // column cc of Q: loaded per tile AFTER the scalar phase (see below)"]
  return [f"  double qcol[{g.E}];                          // column cc of Q, resident for the whole launch", "#pragma unroll",
          f"  for (int i = 0; i < {g.E}; i++) {_q_fetch(g, dop)}"]


def _late_q(g, dop):
  tune = tuning.current()
  if not (tune.wide_lean == 1 and tune.wide_lean_q):
    return []
  return ["    {",
          "      // Q's column is fetched here, behind an opaque zero, so that its 2 x dim_err registers are not live during the scalar",
          "      // phase above (the widest point of the kernel: with them it spilled); an L2 hit per tile, hidden under the first P wait",
          "      int qoff = 0;", "      asm volatile(\"\" : \"+v\"(qoff) :: \"memory\");", "#pragma unroll",
          f"      for (int i = 0; i < {g.E}; i++) {_q_fetch(g, dop, ' + qoff')}", "    }"]


def _do_pred(spec, dop):
  if spec.identity_at_dt0():
    return ["  // predict with a uniform dt == 0 (a second observation at the same timestamp) is the identity on (x, P) for finite",
            "  // states: f(x, 0) == x and F(x, 0) == I were checked SYMBOLICALLY for this model at generation time",
            "  // (FilterSpec.identity_at_dt0) and dt Q = 0, so the covariance phase is skipped; results are unchanged.",
            f"  const bool do_pred = {dop} && !(gdt == nullptr && dt_scalar == 0.0);"]
  return ["  // this model's f(x, 0) != x or F(x, 0) != I: predict runs on every call, dt == 0 included (ekf_c.c:15-28)",
          f"  const bool do_pred = {dop};"]


TILE_LOOP = ["  const int64_t tiles = (n + FT2 - 1) / FT2;", "  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {",
             "    const int64_t base = tile * FT2;", "    const int cnt = (n - base) < FT2 ? (int)(n - base) : FT2;"]


def _tile_in(g, Z, prefetch=False):
  """The tile's x (and z) to LDS; prefetch: the first group's records of P behind them."""
  L = [f"    rn::copy_g2l<FT2 * {g.D}>(gx + base * {g.D}, cnt * {g.D}, s_x, lane);"]
  if Z:
    L.append(f"    rn::copy_g2l<FT2 * {Z}>(gz + base * {Z}, cnt * {Z}, s_z, lane);")
  if prefetch:
    L.append(f"    {g.CPIN}<{g.PBUF}>(gP + base * {g.EE}, (cnt < {g.FPW} ? cnt : {g.FPW}) * {g.EE}, s_P[0], lane);")
  return L + ["    rn::wave_lds_sync();"]


def _phase1(spec, g, k, Z, dop, mixed):
  upd = k is not None or mixed
  L = []
  if mixed:
    known = " || ".join(f"kd_ == {kk_.kind}" for kk_ in spec.kinds)
    L += ["    int kd1 = 0;", "    if (lane < cnt) {", "      const int kd_ = gkinds[base + lane];",
          f"      if ((active == nullptr || active[base + lane] != 0) && ({known})) kd1 = kd_;", "      s_kd[lane] = kd1;", "    }"]
  L += ["    if (lane < cnt" + (" && kd1 != 0" if mixed else "") + ") {",
        "      double* sl = s_sl + lane * SLOT;",
        "      if (do_pred) {",
        "        int ld_ = lane;",
        '        asm volatile("" : "+v"(ld_));      // (the address gdt + lane is otherwise formed at the kernel\'s entry and kept -- in scratch, where registers are short -- for this one use)',
        "        const double dt = gdt != nullptr ? gdt[base + ld_] : dt_scalar;",
        f"        scal_predict(s_x + lane * {g.D}, dt, sl, norm_quats);",
        "      } else {",
        f"        scal_keep(s_x + lane * {g.D}, sl, {dop} ? norm_quats : 0);      // predict(dt = 0) still renormalises",
        "      }"]
  if upd:
    L.append("      __builtin_amdgcn_sched_barrier(0);       // f / F first, then h / H: interleaved for ILP they need the sum of both register sets")
    if mixed:
      L.append("      switch (kd1) {")
      L += [f"        case {kk_.kind}: scal_obs_{kk_.kind}(sl, s_z + lane * {Z}); break;" for kk_ in spec.kinds]
      L += ["        default: break;", "      }"]
    else:
      L.append(f"      {_obs_call(k, 'true')};")
  return L + ["    }", "    rn::wave_lds_sync();"]


def _group_head(g, const_p=False):
  L = [f"    const int ngroups = (cnt + {g.FPW - 1}) / {g.FPW};", "    for (int p = 0; p < ngroups; p++) {",
       f"      const int pcnt = (cnt - {g.FPW} * p) < {g.FPW} ? (cnt - {g.FPW} * p) : {g.FPW};",
       f"      {'const ' if const_p else ''}double* gPp = gP + (base + {g.FPW} * p) * {g.EE};"]
  if const_p:
    return L + [f"      const int sh = {'rn::odd_start(gPp)' if g.ODD else '0'};"]
  return L + ["      // a group record may start on an odd double (odd dim_err^2 x odd group index): the LDS image is then shifted",
              "      // by one double so that the 16-byte transfers stay aligned on both sides",
              "      const int sh = rn::odd_start(gPp);" if g.ODD else "      constexpr int sh = 0;                    // records of this model always start 16-byte aligned"]


def _group_load(g, buf=None):
  """Group p's records land in `buf` (None: the step kernels' sPb, declared here); with two buffers group p + 1 is requested."""
  if g.DB:
    return ["      double* sPb = s_P[p & 1];", "      rn::async_wait();                        // group p has landed (issued one iteration ago)", "      rn::wave_lds_sync();",
            f"      if (p + 1 < ngroups) {g.CPIN}<{g.PBUF}>(gP + (base + {g.FPW} * (p + 1)) * {g.EE}, ((cnt - {g.FPW} * (p + 1)) < {g.FPW} ? (cnt - {g.FPW} * (p + 1)) : {g.FPW}) * {g.EE}, s_P[(p + 1) & 1], lane);"]
  decl = [] if buf else ["      double* sPb = s_P[0];                   // single buffer: the co-resident wave hides the HBM latency"]
  return decl + [f"      {g.CPIN}<{g.PBUF}>(gPp, pcnt * {g.EE}, {buf or 'sPb'}, lane);", "      rn::async_wait();", "      rn::wave_lds_sync();"]


def _group_compute(spec, g, k, Z, mixed, tl):
  ZZ, E, EE, FPW = Z * Z, g.E, g.EE, g.FPW
  L = ["      double* sPc = sPb + sh;", "      const int gg = g < pcnt ? g : 0;",
       "      // a masked-out filter (active[i] == 0) is not `on`: every LDS store of the matrix phase is predicated, so its image",
       "      // of P goes back to HBM as it came"]
  if mixed:
    L += [f"      const int kd = (act && g < pcnt) ? s_kd[{FPW} * p + gg] : 0;", "      const bool on = kd != 0;"]
  else:
    L.append(f"      const bool on = act && g < pcnt && (active == nullptr || active[base + {FPW} * p + gg] != 0);")
  L += [f"      double* sl = s_sl + ({FPW} * p + gg) * SLOT;", f"      if (do_pred) mat_predict(sPc + gg * {EE}, qcol, sl, cc, on);"]
  L += _stamp(tl, "5 + 4 * p")
  if mixed:
    for ki_, kk_ in enumerate(spec.kinds):      # a kind no filter of the pass has is skipped (wave-uniform test)
      L.append(f"      if (any_lane(kd == {kk_.kind}))")
      L.append(f"        mat_update_{kk_.kind}(sPc + gg * {EE}, r_per_filter ? gR + (base + {FPW} * p + gg) * {ZZ} : gR + {ki_ * ZZ}, sl, sl, s_G + gg * {Z * E}, s_K + gg * {Z * E}, cc, kd == {kk_.kind});")
  elif k is not None:
    ss_ = f", s_S + gg * {wide_s_doubles(k)}" if _update_body(k, E)[1] else ""
    L.append(f"      mat_update_{k.kind}(sPc + gg * {EE}, r_per_filter ? gR + (base + {FPW} * p + gg) * {ZZ} : gR, sl, sl, s_G + gg * {Z * E}, s_K + gg * {Z * E}{ss_}, cc, on);")
  return L


def _group_out(g, dst):
  """The group's image back to its records at `dst` (16-byte aligned like gP: the record starts on the same parity)."""
  return [f"      rn::copy_l2g_any<{g.PBUF}>({dst}, pcnt * {g.EE}, sPb, sh, lane);" if g.ODD else f"      rn::copy_l2g<{g.PBUF}>({dst}, pcnt * {g.EE}, sPb, lane);"]


def _phase3(spec, g, lay, k, Z, mixed):
  upd = k is not None or mixed
  D = g.D
  L = ["    if (lane < cnt && kd1 != 0) {" if mixed else "    if (lane < cnt && (active == nullptr || active[base + lane] != 0)) {",
       "      const double* sl = s_sl + lane * SLOT;"]
  if upd:
    L.append(f"      int fl = scal_inject(sl, s_x + lane * {D}, norm_quats);")
  if mixed:
    zcases = " ".join(f"case {kk_.kind}: zk_ = {kk_.zdim}; break;" for kk_ in spec.kinds)
    L += ["      int zk_ = 0;", f"      switch (kd1) {{ {zcases} default: break; }}", "#pragma unroll",
          f"      for (int i = 0; i < {Z}; i++) if (i < zk_) s_z[lane * {Z} + i] = sl[{lay.OFF_Y} + i];      // the rest of the row passes through",
          f"      if (flags != nullptr) flags[base + lane] = (uint8_t)(fl | (int)sl[{lay.OFF_FL}]);     // 1 gated",
          "    } else if (lane < cnt && flags != nullptr) {",
          "      flags[base + lane] = (active != nullptr && active[base + lane] == 0) ? 16 : 8;       // masked out / not a kind of this model: x, P and z pass through untouched"]
  elif upd:
    L += ["#pragma unroll", f"      for (int i = 0; i < {Z}; i++) s_z[lane * {Z} + i] = sl[{lay.OFF_Y} + i];",
          f"      if (flags != nullptr) flags[base + lane] = (uint8_t)(fl | (int)sl[{lay.OFF_FL}]);     // 1 gated, 4 projection failed",
          "    } else if (lane < cnt && flags != nullptr) {",
          "      flags[base + lane] = 16;       // masked out: x, P and z pass through untouched"]
  else:
    L += ["#pragma unroll", f"      for (int i = 0; i < {D}; i++) s_x[lane * {D} + i] = sl[{lay.OFF_X} + i];"]
  return L + ["    }", "    rn::wave_lds_sync();"]


def _tile_out(g, Z, ckpt):
  L = [f"    rn::copy_l2g<FT2 * {g.D}>(gx + base * {g.D}, cnt * {g.D}, s_x, lane);"]
  if Z:
    L.append(f"    rn::copy_l2g<FT2 * {Z}>(gz + base * {Z}, cnt * {Z}, s_z, lane);")
  if ckpt:
    L.append(f"    rn::copy_l2g<FT2 * {g.D}>(cx + base * {g.D}, cnt * {g.D}, s_x, lane);")
  return L + ["    rn::wave_lds_sync();"]


def step_kernel(spec, lay, kname, k=None, ckpt=False, mixed=False):
  """One step-granular kernel: k_predict (k None), k_step_{kind} of kind k, k_stepc_{kind}, k_kinds.
  mixed: k_kinds, a kind per filter (kinds[i]) -- z rows at stride zmax, per-filter R at stride zmax^2 or a table in the order of the model's
  kinds; phase 1 and phase 3 switch per lane, phase 2 runs the matrix update of every kind a pass holds on the filters of that kind
  ckpt: the kernel also writes a CHECKPOINT -- the observations as they came (cz), the filtered pair (cx, cP) --, what the orchestrators' rewind
  rings keep of every call (ekf_sym.cc:142-156, 191); a kernel of its own (k_stepc_{kind}), k_step_{kind} stays as it is"""
  upd = k is not None or mixed
  Z = (max(kk_.zdim for kk_ in spec.kinds) if mixed else k.zdim) if upd else 0
  dop = "DO_PREDICT" if upd else "true"
  g = _geometry(spec)
  tl = tuning.current().wide_timeline and not mixed
  wide_s = wide_s_doubles(k) if upd and not mixed and _update_body(k, g.E)[1] else 0
  L = _signature(kname, upd, mixed, ckpt)
  L += _lds_decls(g, f"s_P[{1 + g.DB}][{g.PBUF}];     // double buffer: group p computes, group p+1 lands", Z, S=wide_s, mixed=mixed)
  L += _lanes(g) + _q_staging(g, dop) + _do_pred(spec, dop) + TILE_LOOP
  L += _stamp(tl, 0) + _stamp_block(tl, 0)
  L.append("    // ---------------- phase 1: lane l = filter l, x-dependent scalars -> LDS slot ----------------")
  L += _tile_in(g, Z, prefetch=g.DB)
  if ckpt:
    L.append(f"    rn::copy_l2g<FT2 * {Z}>(cz + base * {Z}, cnt * {Z}, s_z, lane);      // the observations, before the residuals take their place")
  L += _stamp(tl, 1) + _phase1(spec, g, k, Z, dop, mixed) + _late_q(g, dop) + _stamp(tl, 2)
  L.append(f"    // ---------------- phase 2: {g.GL}-lane group per filter, {g.FPW} filters at a time, covariance algebra ----------")
  L += _group_head(g) + _group_load(g) + _stamp(tl, "4 + 4 * p") + _group_compute(spec, g, k, Z, mixed, tl) + _stamp(tl, "6 + 4 * p")
  L += _group_out(g, "gPp") + (_group_out(g, f"cP + (base + {g.FPW} * p) * {g.EE}") if ckpt else [])
  L += _stamp(tl, "7 + 4 * p") + ["      rn::wave_lds_sync();", "    }"] + _stamp(tl, 3)
  L.append("    // ---------------- phase 3: lane l = filter l, inject the error state, write x / y / flags ---------")
  L += _phase3(spec, g, lay, k, Z, mixed) + _tile_out(g, Z, ckpt) + _stamp(tl, 63) + _stamp_block(tl, 1)
  return "\n".join(L + ["  }", "}"]) + "\n"


ANY_LANE = """
// Does any lane of the wavefront hold `p`?  (k_kinds skips the matrix update of a kind no filter of a pass has: an optimisation only, every
// store of the matrix phase is predicated.  A host build of this text, the kernels running lane by lane as threads, takes every update.)
#ifdef __HIP__
__device__ __forceinline__ bool any_lane(const bool p) { return __ballot(p) != 0ull; }
#else
inline bool any_lane(bool) { return true; }
#endif
"""


def kernels(spec):
  fn_text, lay = device_functions(spec)
  out = [f"// ---- family W, three-phase step kernels (tile of {tile_filters(spec)} filters per wavefront, slot = {lay.SLOT} doubles) ----",
         f"constexpr int FT2 = {tile_filters(spec)};", f"constexpr int SLOT = {lay.SLOT};", f"constexpr int SLOT_OFF_X = {lay.OFF_X};",
         f"constexpr int SLOT_OFF_DT = {lay.OFF_DT};", fn_text]
  if tuning.current().wide_timeline:
    out.append("__device__ unsigned long long g_tl[256 * 64 * 2];      // debug timeline (tuning knob wide_timeline)")
    out.append("__device__ unsigned long long g_tlb[4096 * 2];         // start / end of EVERY workgroup's first tile")
  out.append(step_kernel(spec, lay, "k_predict"))
  for k in spec.kinds:
    out.append(step_kernel(spec, lay, f"k_step_{k.kind}", k))
    out.append(step_kernel(spec, lay, f"k_stepc_{k.kind}", k, ckpt=True))
  from rednose_amd.codegen import emit      # (emit imports this module: see its docstring)
  if emit.step_kinds(spec):
    out += [ANY_LANE, step_kernel(spec, lay, "k_kinds", mixed=True)]
  return "\n".join(out)


def maha_kernels(spec):
  """Standalone Mahalanobis distance (reference: EKF_sym.maha_test, ekf_sym.py:626-649): d2 per filter, state untouched."""
  g = _geometry(spec, maha=True)
  E, EE, FPW = g.E, g.EE, g.FPW
  lay, _, Hss, _ = slot_tables(spec)
  out = []
  for k in spec.kinds:
    Z = k.zdim
    ZZ = Z * Z
    Hs = Hss[k.kind]
    b = _load_col(E, f", R[{ZZ}]") + ["#pragma unroll", f"for (int i = 0; i < {ZZ}; i++) R[i] = gR[i];"]
    b += _g_gt(Hs, Z, "col[{}]".format) + _store_g(Z, E)
    b.append(f"double S[{ZZ}], L[{ZZ}], iL[{Z}], v[{Z}], w[{Z}];")
    b += _hph(Hs, Z, E, dst="S", plus_r=True)
    for i in range(Z):
      b.append(f"v[{i}] = w[{i}] = sl[{lay.OFF_Y + i}];")
    b += [f"rn::ldu_factor<{Z}>(S, L, iL);", f"rn::ldu_forward<{Z}>(L, iL, v);", f"rn::ldu_forward_t<{Z}>(L, iL, w);", "rn::wave_lds_sync();",
          "return " + " + ".join(f"v[{i}]*w[{i}]*iL[{i}]" for i in range(Z)) + ";"]
    out.append("\n".join([f"__device__ __forceinline__ double mat_maha_{k.kind}(const double* sP, const double* __restrict__ gR, const double* sl, "
                          "double* sG, const int cc, const bool act) {"] + ind(b) + ["}"]))
    L = ["", f"__global__ __launch_bounds__(64) void k_maha_{k.kind}(const double* __restrict__ gx, const double* __restrict__ gP,",
         "    const double* __restrict__ gz, const double* __restrict__ gR, const int r_per_filter, const double* __restrict__ gea,",
         "    const int64_t n, double* __restrict__ d2) {", "  (void)gea;"]
    L += _lds_decls(g, f"s_P[{g.PBUF}];", Z, K=False) + _lanes(g) + TILE_LOOP + _tile_in(g, Z)
    L += ["    if (lane < cnt) {", "      double* sl = s_sl + lane * SLOT;", f"      scal_keep(s_x + lane * {g.D}, sl, 0);", f"      {_obs_call(k, 'false')};", "    }",
          "    rn::wave_lds_sync();"]
    L += _group_head(g, const_p=True) + _group_load(g, buf="s_P")
    L += ["      const int gg = g < pcnt ? g : 0;",
          f"      const double d = mat_maha_{k.kind}(s_P + sh + gg * {EE}, r_per_filter ? gR + (base + {FPW} * p + gg) * {ZZ} : gR, s_sl + ({FPW} * p + gg) * SLOT,",
          f"                                  s_G + gg * {Z * E}, cc, act && g < pcnt);",
          f"      if (c == 0 && g < pcnt) d2[base + {FPW} * p + g] = d;", "      rn::wave_lds_sync();", "    }", "  }", "}", ""]
    out.append("\n".join(L))
  return "\n".join(out)


TILES = "(n + FT2 - 1) / FT2"      # tiles of a launch: FT2 filters per wavefront (tile_filters)
launch_predict, launch_step, launch_step_ckpt, launch_kinds, launch_maha = (functools.partial(f, TILES) for f in (
  emit_common.launch_predict, emit_common.launch_step, emit_common.launch_step_ckpt, emit_common.launch_kinds, emit_common.launch_maha))
