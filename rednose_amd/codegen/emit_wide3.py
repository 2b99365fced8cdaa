"""Kernel family W, fused multi-step run `k_run`: state resident in registers, SEVERAL ROWS PER LANE.

The first version of this kernel (round 1) gave every filter a 32-lane group, one row of P per lane, and evaluated the
x-dependent scalars (f, F, h, H.H_mod, err_fun: ~1 600 instructions for live's accelerometer kind) in every lane of the
group -- per wavefront that is the same instruction count whether 2 or 8 filters share it, so with 2 filters per
wavefront the scalars alone cost 3 us per step, the rank-Z passes ran at 22 busy lanes of 32, each FMA fetched one
broadcast operand from LDS, and the kernel needed 256 + 166 registers with a thousand AGPR moves: 343 M steps/s on
live's config-4 forward pass, SLOWER per step than one launch per step.

Here a filter gets GL = 8 lanes (16 above 22 error states) and lane c owns rows c, c + GL, c + 2 GL ... of P
(R = ceil(E / GL) rows per lane), so a wavefront carries 8 (4) filters:
  * the scalar phases run ONCE per filter (one lane per filter, through an LDS slot -- the step kernels' generated functions,
    instantiated against RunLayout), amortised over 4x as many filters per wavefront;
  * every broadcast operand of the rank-Z passes (a row of G or K^T from LDS) feeds R FMAs instead of one;
  * live: 22 of 24 row slots busy instead of 22 of 32 lanes.
P lives in registers as rows only (R x E doubles per lane: 132 VGPRs for live).  LDS holds per filter one E x E image -- the
scratch of predict's single transposition and the staging buffer of the trace / MSCKF window shift, written only then --, one
Z x E buffer shared by G and K^T, and the scalar slot.  P = P^T (up to the Joseph form's rounding, as in the reference) is used
twice: columns of A = P F^T are rows of F P (predict_fn), and column j of G = He P is row j of P against He (update_fn).

  predict (ekf_c.c:8-33)   rows of A = P F^T (row-local) -> image -> columns of A -> P'[r] = (F P)[r] F^T + dt Q[r] (row-local)
  update  (ekf_c.c:37-121) Joseph form with its rank-Z structure, per row slot; S is factored redundantly per lane;
                           feature-track kinds project on the null space of the extra-argument Jacobian with Householder
                           reflectors (ekf_c.c:66-76)
Results agree with the step-granular path to rounding (different association of the same sums); tests/test_gpu_run.py,
test_gpu_random.py, test_gpu_msckf.py, test_gpu_fullsize.py bound it.  Measurements and what hipcc needed: DESIGN.md section 3.

(The same layout for the step-granular entry points was built in round 2 and measured slower than the three-phase kernels of
emit_wide2 -- one wavefront per SIMD cannot overlap its own HBM round trip; numbers in profiles/tuning_notes.md.)
"""
import types

from rednose_amd.codegen import emit_wide2 as w2, tuning
from rednose_amd.codegen.emit_common import EADIM, SlotLayout, ea_count, ind, term, sum_terms, NOISE_MODES, TABLE


def ea_max(spec):
  return max([ea_count(k) for k in spec.kinds] + [0])


def layout(spec):
  """-> (GL lanes per filter, R rows per lane, FPW filters per wavefront).  8 lanes while 8 covariance images fit the LDS
  budget of a wavefront (E <= 22), 16 up to 32 error states; above that the row sets of several rows per lane no longer fit the
  register file (feature36 at 16 lanes x 3 rows: 120 spilled registers) and a filter takes the whole wavefront, a row per lane."""
  E = spec.dim_err
  GL = 8 if E <= 22 else (16 if E <= 32 else 64)       # above 32 error states: one filter per wavefront, one row per lane
  return GL, -(-E // GL), 64 // GL


def _tl(ph):
  """Debug stamp inside the matrix phases (tuning knob wide_timeline): slot 20 * (t % 3) + ph of the workgroup's timeline."""
  if not tuning.current().wide_timeline:
    return []
  return [f"if (threadIdx.x == 0 && blockIdx.x < 256) {{ const int ti_ = tl_t * 20 + {ph}; g_tl[(blockIdx.x * 64 + ti_) * 2] = "
          "__builtin_readcyclecounter(); g_tl[(blockIdx.x * 64 + ti_) * 2 + 1] = wall_clock64(); }"]


def _tl_arg(call=False):
  if not tuning.current().wide_timeline:
    return ""
  return ", (int)(t % 3)" if call else ", const int tl_t"


def rank_pass(E, Z, R, src, op, coef, JB=None):
  """Straight-line rank-Z pass over the register rows: row_s[j] op= sum_z coef_s[z] * src[z][j] for all j, in blocks of JB
  columns.  Two things hipcc does not do by itself here:
    * the broadcast operands of block b + 1 are loaded before the FMAs of block b and a compiler fence closes every block, so
      one block of loads is in flight under the arithmetic and no more (left alone it issues all Z*E LDS loads first: 2*Z*E
      registers on top of the rows -> hundreds of spills);
    * inside a block the FMAs are emitted term by term ACROSS the block's JB * R entries, so consecutive instructions belong to
      different accumulation chains: a dependent fp64 FMA issues ~40 cycles after its predecessor with one wavefront per SIMD
      (tools/fp64_ilp.hip), entry-by-entry order made every FMA wait for the one before it."""
  JB = JB or 4      # columns per block (6 and 8 measured in round 5: 21.21 / 20.90 ms per config-4 chunk against 21.04 / 21.24 -- noise; profiles/tuning_notes.md)
  out = []
  blocks = [list(range(j, min(j + JB, E))) for j in range(0, E, JB)]
  sg = "-=" if op == "-=" else "+="

  def loads(bl):
    return [f"const double q_{zi}_{j} = {src}[{zi} * {E} + {j}];" for j in bl for zi in range(Z)]
  out += loads(blocks[0])
  for bi, bl in enumerate(blocks):
    if bi + 1 < len(blocks):
      out += loads(blocks[bi + 1])
    for zi in range(Z):
      for j in bl:
        for s in range(R):
          out.append(f"row{s}[{j}] {sg} {coef}{s}[{zi}]*q_{zi}_{j};")
    out.append(" ".join(f"rn::pin(row{s}[{j}]);" for j in bl for s in range(R)))
    out.append("rn::wave_lds_sync();")
  return ["{"] + ind(out) + ["}"]


class RunLayout(SlotLayout):
  """Per-filter scalar slot of the fused run (doubles).  Same fields as emit_wide2.Layout, packed by lifetime so that eight
  filters of a 22-state model, their covariance images and the G / K^T buffers stay under 40 KB (4 wavefronts per CU):
  the non-trivial entries of F (dead once predict's matrix phase is through), those of He = H H_mod (written after that, dead
  once the Joseph-form coefficients exist) and dx (written after that) share one region; x lives ONLY here (no separate
  copy), and z comes in / y goes out through the Y field."""

  def pack(self, D, E):
    self.OFF_F = self.OFF_HE = self.OFF_DX = D
    self.OFF_Y = D + max(self.nf, self.nh, E)
    self.OFF_DT = self.OFF_Y + self.zmax
    self.OFF_FL = self.OFF_DT + 1
    return self.feature_tail(self.OFF_FL + 1)


def predict_fn(spec, qdiag=False, pf=False, sfx="_pf"):
  """Matrix part of predict on register rows; F's non-trivial entries are broadcast reads of the filter's slot.

  P' = F P F^T + dt Q with ONE transposition through LDS: rows of A = P F^T are row-local; under P = P^T the columns of A are the
  rows of B = F P (B[r][m] = sum_k F[r][k] P[k][m] = sum_k F[r][k] P[m][k] = A[m][r]), and P'[r][:] = B[r][:] F^T + dt Q[r][:] is
  row-local again, so the new rows land in the registers that hold them for the next step.  (P is symmetric up to the rounding
  of the Joseph form, in the reference as here; the reference multiplies F P F^T out entry by entry, ekf_c.c:8-33.)

  qdiag=True emits the variant for a DIAGONAL process noise (detected once per launch by k_run): the lane's diagonal entries of Q
  arrive as register operands and no global memory is read.  That matters beyond the 3 R E loads saved: a load's s_waitcnt
  vmcnt also waits for every EARLIER store of the wavefront (the counter retires in order), so with the trace enabled the rows
  of Q fetched here drained the previous step's 32 KB of trace stores on every step -- the only vector load consumed in the
  middle of a step (profiles/r3a: 11.6 us per step with the trace against 8.7 without).

  pf=True emits `predict_rows_pf` / `predict_rows_qd_pf` for the fused run with a schedule per filter (k_run_pf): the same statements with
  one more argument, `pd` -- does this lane's GROUP predict at this step? --, and every assignment to a register row selects between
  the new value and the row as it is.  Every lane walks every statement (and meets every wave_lds_sync); a group that is idle keeps its
  rows bit for bit.  What such a group writes into its own image of P is scratch (all LDS exchange is group-local)."""
  E = spec.dim_err
  GL, R, _ = layout(spec)
  lay, Fs, _, _ = w2.slot_tables(spec, RunLayout)
  b = [f"const double dt = sl[{lay.OFF_DT}];"]
  # rows of A, whole rows at a time: 16-byte LDS stores of a lane's contiguous row (entry-wise 8-byte stores at a row stride
  # collide on banks)
  for s in range(R):
    b.append("{")
    b.append(f"  double a[{E}];")
    for i in range(E):
      b.append(f"  a[{i}] = {sum_terms(term(cf, f'row{s}[{k}]') for k, cf in Fs.row_nz(i))};")
    b += [f"  if (ok{s}) {{", "#pragma unroll", f"    for (int i = 0; i < {E}; i++) sP[rr{s} * {E} + i] = a[i];", "  }"]
    b.append("}")
  b.append("rn::wave_lds_sync();")
  b += _tl(8)
  if qdiag:
    for s in range(R):
      b.append(f"const double dq{s} = dt * qd{s};")
      b.append("{")
      b.append(f"  double a[{E}];")
      b += ["#pragma unroll", f"  for (int m = 0; m < {E}; m++) a[m] = sP[m * {E} + rc{s}];      // column of A = row of B"]
      for j in range(E):
        diag = f" + (rc{s} == {j} ? dq{s} : 0.0)" if GL * s <= j < GL * (s + 1) else ""      # the lane's own row index is c + {GL} s
        val = f"{sum_terms(term(cf, f'a[{m}]') for m, cf in Fs.row_nz(j))}{diag}"
        b.append(f"  row{s}[{j}] = pd ? ({val}) : row{s}[{j}];" if pf else f"  row{s}[{j}] = {val};")
      b.append("}")
  else:
    # Q is read from HBM / L2 (no LDS left for it): slot s's row of Q is requested one slot ahead of its use
    b.append(f"double q0[{E}];")
    b += ["#pragma unroll", f"for (int j = 0; j < {E}; j++) q0[j] = gQ[rc0 * {E} + j];"]
    for s in range(R):
      if s + 1 < R:
        b.append(f"double q{s + 1}[{E}];")
      b.append("{")
      b.append(f"  double a[{E}];")
      b += ["#pragma unroll", f"  for (int m = 0; m < {E}; m++) a[m] = sP[m * {E} + rc{s}];      // column of A = row of B"]
      if s + 1 < R:
        b += ["#pragma unroll", f"  for (int j = 0; j < {E}; j++) q{s + 1}[j] = gQ[rc{s + 1} * {E} + j];"]
      for j in range(E):
        val = f"{sum_terms(term(cf, f'a[{m}]') for m, cf in Fs.row_nz(j))} + dt*q{s}[{j}]"
        b.append(f"  row{s}[{j}] = pd ? ({val}) : row{s}[{j}];" if pf else f"  row{s}[{j}] = {val};")
      b.append("}")
  b.append("rn::wave_lds_sync();      // the image is free again")
  b += _tl(9)
  rows = ", ".join(f"double (&row{s})[{E}]" for s in range(R))
  idx = ", ".join(f"const int rr{s}, const int rc{s}, const bool ok{s}" for s in range(R))
  sfx, pda = (sfx, ", const bool pd") if pf else ("", "")      # (sfx="_epf": the same text under the names k_run_epf calls)
  if qdiag:
    qarg = ", ".join(f"const double qd{s}" for s in range(R))
    head = (f"__device__ __forceinline__ void predict_rows_qd{sfx}({rows}, double* sP, {qarg}, const double* sl, {idx}{pda}{_tl_arg()}) {{")
  else:
    head = (f"__device__ __forceinline__ void predict_rows{sfx}({rows}, double* sP, const double* __restrict__ gQ, const double* sl, {idx}{pda}{_tl_arg()}) {{")
  return "\n".join([head] + ind(b) + ["}"])


def update_fn(spec, k, pf=False, noise=TABLE, sfx=None):
  """Matrix part of the update of kind k on register rows.  y, the non-trivial entries of He = H H_mod and, for feature-track
  kinds, the Householder reflectors and the projected noise are read from the filter's slot (phase 1 put them there); dx and
  the gate / rank flags go back to it.

  pf=True emits `update_{kind}_rows_pf` for k_run_pf, with one more argument: `mine` -- does this lane's GROUP carry this kind at this step?
  Every lane walks every statement; a group that is idle, flagged 8 or of another kind puts zeros where G and K^T go in its own buffer and
  takes zero coefficients into both rank-Z passes (row -+= 0 * 0: the rows come out unchanged, whatever stale numbers its slot holds), and
  writes nothing into its slot.

  A feature-track kind with pf=True (k_run_epf, MSCKF models; sfx="_epf" names the function `update_{kind}_rows_epf`): `mine` goes through the null-space
  projection.  The projected noise, rank_deficient and the reflectors of the slot mean something only where `mine`; any other group's slot is stale (NaN at
  first), and it takes R = I, rank_deficient = 0 and HPH = 0 by select -- S = I --, beside the zeroed coefficients and the guarded slot writes above.

  noise=ENTRY (with pf) emits `update_{kind}_rows_rpf` for k_run_rpf, whose R is per entry: the same statements, except that `gR` is the group's OWN
  row and its Z * Z doubles are taken only where `mine` -- the row of a group that is idle, flagged 8 or of another kind may hold anything, NaN
  included, and such a group factors the identity instead (its coefficients are zeroed either way, but 0 * NaN is NaN).

  noise=DIAG (with pf) emits `update_{kind}_rows_dpf` for k_run_dpf, whose R is the group's own row of Z variances, taken only where `mine` (ones
  otherwise: the identity as above).  The noise stays a vector through the update -- S = HPH with S[i][i] += r[i], the gate's 1e16 on the Z
  variances, the Joseph term K R as kk[zi] * r[zi] -- so Z doubles live where the other flavours hold Z * Z."""
  assert (pf or noise is TABLE) and not (k.He_sym is not None and noise is not TABLE)
  E, Zf = spec.dim_err, k.zdim
  _, R, _ = layout(spec)
  lay, _, Hss, _ = w2.slot_tables(spec, RunLayout)
  Hs = Hss[k.kind]
  feat = k.He_sym is not None
  Z = Zf - EADIM if feat else Zf
  RF, RB = lay.OFF_RF, lay.OFF_RF + EADIM * Zf
  # The shared table's R of a kind whose Z * Z doubles do not fit the scalar register file (2 Z^2 of its ~100 registers: Z >= 8, randz10's kind 1):
  # `gR + row` is the same address in every lane, hipcc fetches it with scalar loads, and 162 SGPRs of R and Rl held through the update left
  # k_run_pf on 312 of its 320 SGPR-spill lane slots with wrong results on the device (batch_rts_pf, "Found on the way").  Such a kind
  # holds no copy: R is read through a vector address where S and the Joseph term take it, as k_run_dpf reads its Z variances.
  lean = pf and noise is TABLE and not feat and not k.maha_test and 2 * Z * Z > 96
  b = ["(void)sP;"] + ([] if lean else [f"double R[{Z if noise.diag else Z * Z}];"])
  if lean:
    b += ["int rz = 0;", 'asm volatile("" : "+v"(rz));', "const double* gRv = gR + rz;      // a vector address: R stays out of the scalar registers"]
  elif feat and pf:      # the slot of a group that is not `mine` is stale (NaN at first): the identity and 0 by select, never by product
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = mine ? sl[{lay.OFF_RP} + i] : ((i % {Z + 1} == 0) ? 1.0 : 0.0);      // A^T R A (phase 1)",
          "(void)gR;", f"const double rank_deficient = mine ? sl[{lay.OFF_FL}] : 0.0;      // 4.0 when phase 1 found Hea rank deficient"]
  elif feat:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = sl[{lay.OFF_RP} + i];      // A^T R A (phase 1)", "(void)gR;",
          f"const double rank_deficient = sl[{lay.OFF_FL}];      // 4.0 when phase 1 found Hea rank deficient"]
  elif noise.diag:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z}; i++) R[i] = mine ? gR[i] : 1.0;      // the variances of the group's entry"]
  elif noise.per_entry:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = (i % {Z + 1} == 0) ? 1.0 : 0.0;",
          "if (mine) {", "#pragma unroll", f"  for (int i = 0; i < {Z * Z}; i++) R[i] = gR[i];", "}"]
  else:
    b += ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) R[i] = gR[i];"]
  # G = He P: G[z][j] = sum_k He[z][k] P[k][j]; with P = P^T (up to the Joseph form's rounding) that is row j of P against
  # He[z][:] -- row-local, so the lane that owns row j has column j of G in registers; the same numbers are the row view
  # P He^T that is solved into K below.  Nothing of the update reads the LDS image of P.
  for s in range(R):
    if feat:
      b.append(f"double t0_{s}[{Zf}] = {{" + ", ".join(sum_terms(term(cf, f'row{s}[{kk}]') for kk, cf in Hs.row_nz(zi)) for zi in range(Zf)) + "};")
      b.append(f"rn::apply_reflectors<{Zf}, {EADIM}>(sl + {RF}, sl + {RB}, t0_{s});")
      b.append(f"double kk{s}[{Z}] = {{{', '.join(f't0_{s}[{EADIM + zi}]' for zi in range(Z))}}};")
    else:
      b.append(f"double kk{s}[{Z}] = {{" + ", ".join(sum_terms(term(cf, f'row{s}[{kk}]') for kk, cf in Hs.row_nz(zi)) for zi in range(Z)) + "};")
    if pf:
      b += [f"if (!mine) {{", "#pragma unroll", f"  for (int i = 0; i < {Z}; i++) kk{s}[i] = 0.0;", "}"]
    b.append(f"if (ok{s}) {{ " + " ".join(f"sG[{zi} * {E} + rr{s}] = kk{s}[{zi}];" for zi in range(Z)) + " }")
  b.append("rn::wave_lds_sync();")
  b += _tl(10)
  b.append(f"double HPH[{Z * Z}], " + ("" if lean else f"Rl[{Z if noise.diag else Z * Z}], ") + f"S[{Z * Z}], L[{Z * Z}], iL[{Z}];")
  if noise.diag:      # S = HPH + diag(Rl), `scale` in front of the variances
    s_of = lambda scale: ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) S[i] = HPH[i];",      # noqa: E731
                          "#pragma unroll", f"for (int i = 0; i < {Z}; i++) {{ Rl[i] = {scale}[i]; S[i * {Z + 1}] += Rl[i]; }}"]
  if feat:
    for zi in range(Z):
      b.append("{")
      b.append(f"  double m[{Zf}] = {{" + ", ".join(sum_terms(term(cf, f'sG[{zi} * {E} + {j}]') for j, cf in Hs.row_nz(w)) for w in range(Zf)) + "};")
      b.append(f"  rn::apply_reflectors<{Zf}, {EADIM}>(sl + {RF}, sl + {RB}, m);")
      # (pf: a group that is not `mine` put zeros where G goes, but its reflectors are stale: S = R = I for it, by select)
      b += ["#pragma unroll", f"  for (int w = 0; w < {Z}; w++) HPH[{zi * Z} + w] = {'mine ? ' if pf else ''}m[{EADIM} + w]{' : 0.0' if pf else ''};", "}"]
  else:
    for zi in range(Z):
      for w in range(Z):
        b.append(f"HPH[{zi * Z + w}] = {sum_terms(term(cf, f'sG[{zi} * {E} + {j}]') for j, cf in Hs.row_nz(w))};")
  b += (s_of("R") if noise.diag else ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) S[i] = HPH[i] + gRv[i];"] if lean else
        ["#pragma unroll", f"for (int i = 0; i < {Z * Z}; i++) {{ Rl[i] = R[i]; S[i] = HPH[i] + Rl[i]; }}"]) + [
        f"rn::spd_factor<{Z}>(S, L, iL);", "int gated = 0;"]
  if k.maha_test:
    b += ["{", f"  double v[{Z}] = {{{', '.join(f'sl[{(lay.OFF_YP if feat else lay.OFF_Y) + i}]' for i in range(Z))}}};", f"  rn::spd_forward<{Z}>(L, iL, v);",
          "  const double d2 = " + " + ".join(f"v[{i}]*v[{i}]*iL[{i}]" for i in range(Z)) + ";", f"  if (d2 > {k.maha_thresh!r}) {{", "    gated = 1;"] + (
          ["    " + l_ if not l_.startswith("#") else l_ for l_ in s_of("1.0e16 * Rl")] if noise.diag else
          ["#pragma unroll", f"    for (int i = 0; i < {Z * Z}; i++) {{ Rl[i] = 1.0e16 * Rl[i]; S[i] = HPH[i] + Rl[i]; }}"]) + [
          f"    rn::spd_factor<{Z}>(S, L, iL);", "  }", "}"]
  b += _tl(11)
  for s in range(R):
    b.append(f"rn::spd_solve<{Z}>(L, iL, kk{s});                       // K[row][:]")
    if feat:     # the reference's numpy path ignores a measurement whose null-space projection failed (ekf_sym.py:589-591)
      b += ["if (rank_deficient != 0.0) {", "#pragma unroll", f"  for (int i = 0; i < {Z}; i++) kk{s}[i] = 0.0;", "}"]
    if pf:      # (S = R for such a group: the solve above ran on zeros)
      b += [f"if (!mine) {{", "#pragma unroll", f"  for (int i = 0; i < {Z}; i++) kk{s}[i] = 0.0;", "}"]
    b.append(f"const double dx{s} = " + " + ".join(f"kk{s}[{zi}]*sl[{(lay.OFF_YP if feat else lay.OFF_Y) + zi}]" for zi in range(Z)) + ";")
  # B = P - K G: every broadcast row of G feeds all R row slots
  b += _tl(12)
  b += rank_pass(E, Z, R, "sG", "-=", "kk")
  b += _tl(13)
  for s in range(R):
    if feat:
      b.append(f"double Cf{s}[{Zf}] = {{" + ", ".join(sum_terms(term(cf, f'row{s}[{j}]') for j, cf in Hs.row_nz(w)) for w in range(Zf)) + "};")
      b.append(f"rn::apply_reflectors<{Zf}, {EADIM}>(sl + {RF}, sl + {RB}, Cf{s});")
    b.append(f"double Dm{s}[{Z}];")
    for zi in range(Z):
      c = f"Cf{s}[{EADIM + zi}]" if feat else sum_terms(term(cf, f"row{s}[{j}]") for j, cf in Hs.row_nz(zi))
      kr = (f"kk{s}[{zi}]*Rl[{zi}]" if noise.diag else " + ".join(f"kk{s}[{w}]*gRv[{w * Z + zi}]" for w in range(Z)) if lean else
            " + ".join(f"kk{s}[{w}]*Rl[{w * Z + zi}]" for w in range(Z)))
      b.append(f"Dm{s}[{zi}] = " + ("rank_deficient != 0.0 ? 0.0 : " if feat else "") + ("!mine ? 0.0 : " if pf else "") + f"({kr}) - ({c});")
  b.append("rn::wave_lds_sync();      // every lane has taken G (and y): the buffer takes K^T, the slot takes dx and the flags")
  fl = "(double)gated + rank_deficient" if feat else "(double)gated"
  for s in range(R):
    slot = f" sw[{lay.OFF_DX} + rr{s}] = dx{s};" + (f" if (rr{s} == 0) sw[{lay.OFF_FL}] = {fl};" if s == 0 else "")
    if pf:
      slot = f" if (mine) {{{slot} }}"
    b.append(f"if (ok{s}) {{ " + " ".join(f"sG[{zi} * {E} + rr{s}] = kk{s}[{zi}];" for zi in range(Z)) + slot + " }")
  b.append("rn::wave_lds_sync();")
  b += _tl(14)
  b += rank_pass(E, Z, R, "sG", "+=", "Dm")
  b += _tl(15)
  b.append("rn::wave_lds_sync();      // the broadcast buffer is free again")
  rows = ", ".join(f"double (&row{s})[{E}]" for s in range(R))
  idx = ", ".join(f"const int rr{s}, const int rc{s}, const bool ok{s}" for s in range(R))
  head = (f"__device__ __forceinline__ void update_{k.kind}_rows{(sfx or noise.update) if pf else ''}({rows}, const double* __restrict__ gR, double* sP, "
          f"double* sG, const double* sl, double* sw, {idx}{', const bool mine' if pf else ''}{_tl_arg()}) {{")
  return "\n".join([head] + ind(b) + ["}"])


def kernels(spec, with_run=True):
  """Matrix-phase device functions + the fused multi-step kernel (the phase-1 / phase-3 functions are emit_wide2's, which must
  precede this text in the generated file).  with_run=False: only the layout constants -- the model's fused run is emit_run2's k_run2
  (the smoother emitters use these constants and emit their own functions)."""
  from rednose_amd.codegen import emit      # (emit imports this module)
  GL, R, FPW = layout(spec)
  scal_text, lay = w2.device_functions(spec, lay_cls=RunLayout, sfx="_r")
  slot_note = "fused run: doubles per scalar slot" if with_run else "doubles per scalar slot of the single-wavefront layout"
  consts = [f"constexpr int GLR = {GL};    // fused run: lanes per filter", f"constexpr int RPL = {R};    // rows of P per lane",
            f"constexpr int FPWR = {FPW};   // filters per wavefront", f"constexpr int SLOT_R = {lay.SLOT};   // {slot_note}", ""]
  # the fused run with a schedule per filter: the predicated predict once, then per noise flavour its predicated updates (per entry: they take
  # R, or the Z variances, only where `mine`) + its kernel: k_run_pf, k_run_rpf, k_run_dpf
  pf = [predict_fn(spec, pf=True), predict_fn(spec, qdiag=True, pf=True)] if emit.run_pf(spec) else []
  for noise in NOISE_MODES:
    if emit.has_run_pf(spec, noise):
      pf += [update_fn(spec, k, pf=True, noise=noise) for k in spec.kinds] + [run_pf_kernel(spec, noise)]
  # MSCKF models: the same run with extra arguments per entry, the predicated null-space projection and a window shift per group (k_run_epf)
  if emit.has_run_pf_ea(spec):
    pf += ([predict_fn(spec, pf=True, sfx="_epf"), predict_fn(spec, qdiag=True, pf=True, sfx="_epf")] +
           [update_fn(spec, k, pf=True, sfx="_epf") for k in spec.kinds] + [run_epf_kernel(spec)])
  if not with_run:
    # the model's batch_run is emit_run2's k_run2; the fused run with a schedule per filter is this module's single-wavefront structure:
    # the scalar phases against RunLayout, the predicated matrix phases and k_run_pf follow the constants
    return "\n".join(consts + (["", scal_text, ""] + pf if pf else []))
  return "\n".join(consts + [scal_text, "", predict_fn(spec), predict_fn(spec, qdiag=True)] + [update_fn(spec, k) for k in spec.kinds] + [run_kernel(spec)] + pf)


def _obs_fragments(lay, zmax, FPW, indexed, count_note):
  """How the observations travel: the entries a lane carries between HBM and the slots, FPW * zmax values per tile and step, one per lane and
  pass (a single pass up to 8-dimensional observations at 8 filters per wavefront; the reference puts no limit on ZDIM, ekf_c.c:37).
  indexed=False (a single pass) prints the names without an index, zf / slz / zn, as k_run does; count_note: the comment behind the indexed
  declaration."""
  NZ = -(-(FPW * zmax) // 64)
  z = types.SimpleNamespace()
  if not indexed:
    assert NZ == 1
    z.decl = f"const int zf = lane / {zmax}, zc = lane % {zmax};                // observation entry this lane carries between HBM and the slots"
    z.tile_a = "    const bool zlive = zf < cnt;\n"
    z.tile_b = f"    double* slz = s_sl + (zlive ? zf : 0) * SLOT_R + {lay.OFF_Y} + zc;\n"
    z.first = f"    if (zlive) *slz = gz[base * {zmax} + lane];"
    z.next = ("      double zn = 0.0;                                 // next step's observation, in flight during this step\n"
              f"      if (t + 1 < T && zlive) zn = gz[((t + 1) * n + base) * {zmax} + lane];")
    z.out = f"      if (zlive) gz[(t * n + base) * {zmax} + lane] = *slz;          // y (the observation itself after an unknown kind)"
    z.commit = "      if (zlive) *slz = zn;"
    return z
  q_ = range(NZ)
  z.decl = " ".join(f"const int zf{q} = (lane + {64 * q}) / {zmax}, zc{q} = (lane + {64 * q}) % {zmax};" for q in q_) + \
           (f"      // {NZ} observation entries per lane ({FPW} filters x {zmax})" if count_note else "")
  z.tile_a = "".join(f"    const bool zlive{q} = zf{q} < cnt;\n" for q in q_)
  z.tile_b = "".join(f"    double* slz{q} = s_sl + (zlive{q} ? zf{q} : 0) * SLOT_R + {lay.OFF_Y} + zc{q};\n" for q in q_)
  z.first = "\n".join(f"    if (zlive{q}) *slz{q} = gz[base * {zmax} + lane + {64 * q}];" for q in q_)
  z.next = "\n".join([f"      double zn[{NZ}] = {{{', '.join('0.0' for _ in q_)}}};                 // next step's observations, in flight during this step"] +
                     [f"      if (t + 1 < T && zlive{q}) zn[{q}] = gz[((t + 1) * n + base) * {zmax} + lane + {64 * q}];" for q in q_])
  z.out = "\n".join(f"      if (zlive{q}) gz[(t * n + base) * {zmax} + lane + {64 * q}] = *slz{q};" for q in q_)
  z.commit = "\n".join(f"      if (zlive{q}) *slz{q} = zn[{q}];" for q in q_)
  return z


def _row_args(R):
  """The register rows and their indices as call arguments."""
  return ", ".join(f"row{s}" for s in range(R)), ", ".join(f"rr{s}, rc{s}, ok{s}" for s in range(R))


def _img(E, R, cond="", pad=""):
  """rows -> LDS image (only where something reads the image: trace, window shift, the final store)"""
  return "\n".join(f"{pad}        if (ok{s}{cond}) {{\n#pragma unroll\n{pad}          for (int j = 0; j < {E}; j++) sP[rr{s} * {E} + j] = row{s}[j];\n{pad}        }}" for s in range(R))


def _stamp(ph):
  """A line of k_run with a debug stamp (tuning knob wide_timeline; tools/timeline.py run): the last three steps, twenty stamps each."""
  if not tuning.current().wide_timeline:
    return "\n      "
  return (f"\n      if (lane == 0 && blockIdx.x < 256) {{ const int ti_ = (int)(t % 3) * 20 + {ph}; "
          "g_tl[(blockIdx.x * 64 + ti_) * 2] = __builtin_readcyclecounter(); g_tl[(blockIdx.x * 64 + ti_) * 2 + 1] = wall_clock64(); }")


def _fused_run(spec, pf, *, title, sched, update, flags_rule, args="", unused="", pre_loop="", after_step="", kname=None, fsfx="_pf"):
  """The text of a single-wavefront fused run, once: kernel head, LDS, the tile prologue (images, slots, observations, rows into registers), the
  step loop (predict, update, inject, y and the trace out, the next observation in) and the write-back.  `pf`: a schedule per filter (k_run_pf)
  instead of a shared one (k_run) -- the predicates of the predict phase, the predicated matrix functions, the write-back into the image
  loaded again, and without k_run's notes and debug stamps.  The keyword arguments are the text the two kernels do not share: title, trailing
  arguments, what precedes the loop, the schedule fetch (through the predicates), the update's scalar and matrix dispatch, the flags rule
  and what follows a step."""
  D, E = spec.dim_x, spec.dim_err
  EE = E * E
  GL, R, FPW = layout(spec)
  lay = w2.slot_tables(spec, RunLayout)[0]
  zmax = max(k.zdim for k in spec.kinds)
  z = _obs_fragments(lay, zmax, FPW, indexed=pf or FPW * zmax > 64, count_note=not pf)
  rows, idx = _row_args(R)
  img = _img(E, R)
  nt_trace = "true" if tuning.current().nt_trace else "false"
  qd_decl = "\n".join(f"  const double qd{s} = gQ[((c + {GL * s}) < {E} ? (c + {GL * s}) : 0) * {E + 1}];" for s in range(R))
  qd_args = ", ".join(f"qd{s}" for s in range(R))
  decl_rows = "\n".join(f"    double row{s}[{E}];" for s in range(R))
  decl_idx = "\n".join(f"    const int rr{s} = c + {GL * s}; const bool ok{s} = live && rr{s} < {E}; const int rc{s} = rr{s} < {E} ? rr{s} : 0;" for s in range(R))
  # the fused run's covariance is symmetric by contract (include/rednose_amd_filter.h): (P + P^T) / 2 of the caller's matrix, once, as
  # the rows enter the registers -- predict_fn / update_fn use P = P^T, the reference's dense products use both halves
  load_rows = "\n".join(f"#pragma unroll\n    for (int j = 0; j < {E}; j++) row{s}[j] = 0.5 * (sP[rc{s} * {E} + j] + sP[j * {E} + rc{s}]);" for s in range(R))

  def copy_in(l):
    return f"    rn::copy_g2l<FPWR * {EE}>(gP + base * {EE}, cnt * {EE}, s_P, {l});"

  def note(text):      # k_run's remarks; k_run_pf refers to k_run
    return "" if pf else text
  stamp = (lambda ph: "") if pf else _stamp
  step, pd, any_pd, fsfx, pda = ("step", "pd", "__any(pd)", fsfx, ", pd") if pf else ("live", "do_pred", "do_pred", "", "")
  le_decl = f"""    int le = lane;
    asm volatile("" : "+v"(le));{note("         // (same: nothing of the first copy's index arithmetic is kept alive across the step loop)")}
"""
  if pf:      # a filter that no entry stepped is not written back: the image that came in, again, and only the groups that stepped put their rows into it
    write_back = f"""    // the image the filters came with, again: a filter that no entry stepped leaves as it came (x: its slot was never written)
{le_decl}{copy_in("le")}
    rn::wave_lds_sync();
{_img(E, R, " && stepped")}
    rn::wave_lds_sync();
"""
  else:
    write_back = f"""{img}
    rn::wave_lds_sync();
{le_decl}"""
  # (Measured and not kept, round 4: the trace straight from the register rows as 8-byte stores to the TRANSPOSED positions -- lane c of
  # a group holds P[c + GL s][j]; written to [j][c + GL s] the lanes of a group cover 64 contiguous bytes per instruction, no LDS image,
  # no read-back -- config 4 forward 70.6 ms per chunk against 22.6 ms through the image: 66 store instructions per lane and step, each
  # a scatter of eight 64-byte pieces.  Round 3 measured the row-wise 16-byte variant at 25.3 ms.  profiles/tuning_notes.md.)
  # (Measured and not kept, round 4, profiles/tuning_notes.md: the copy of a step's covariance trace DEFERRED into the next step and woven
  # between the statements of its scalar phase when that step has no predict -- LDS / store throughput under a chain of dependent fp64
  # instructions, the arithmetic run redundantly on all lanes so that no divergent region separates the two streams.  Host-verified,
  # parity-green on the device, and 8 % SLOWER: config 4 forward 23.6 ms per chunk against 21.8.)
  return f"""
{title}
__global__ __launch_bounds__(64) void {kname or ("k_run_pf" if pf else "k_run")}(double* __restrict__ gx, double* __restrict__ gP, const double* __restrict__ gQ,
    const int32_t* __restrict__ kinds, const double* __restrict__ dts, const int64_t T, double* __restrict__ gz,
    const double* __restrict__ gR, const int64_t n, const int norm_quats, uint8_t* __restrict__ flags,
    double* __restrict__ tx, double* __restrict__ tP{args}) {{{unused}
  __shared__ __attribute__((aligned(16))) double s_P[FPWR * {EE} + 2];      // one image of P per filter{note(" (see emit_wide3.py)")}
  __shared__ __attribute__((aligned(16))) double s_G[FPWR * {zmax * E}];     // G, then K^T
  __shared__ __attribute__((aligned(16))) double s_sl[FPWR * SLOT_R];
  const int lane = threadIdx.x;
  const int g = lane / GLR;
  const int c = lane % GLR;
  {z.decl}{note(chr(10) + "  // a diagonal process noise (the usual case) lives in registers: see predict_fn(qdiag=True)")}
  int qoff = 0;
  for (int i = lane; i < {EE}; i += 64) qoff |= (i / {E} != i % {E}) && (gQ[i] != 0.0);
  const bool qdiag = !__any(qoff);
{qd_decl}
  const int64_t tiles = (n + FPWR - 1) / FPWR;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {{
    const int64_t base = tile * FPWR;
    const int cnt = (n - base) < FPWR ? (int)(n - base) : FPWR;
    const int gg = g < cnt ? g : 0;
    const bool live = g < cnt;
{z.tile_a}    double* sP = s_P + gg * {EE};
    double* sl = s_sl + gg * SLOT_R;
{z.tile_b}{decl_idx}
    int lb = lane;
    asm volatile("" : "+v"(lb));{note("         // opaque copy of the lane index: the copies' index arithmetic stays inside the tile")}
{copy_in("lb")}
    for (int i = lane; i < cnt * {D}; i += 64) s_sl[(i / {D}) * SLOT_R + {lay.OFF_X} + i % {D}] = gx[base * {D} + i];
{z.first}
    rn::wave_lds_sync();
{decl_rows}
{load_rows}
{pre_loop}    for (int64_t t = 0; t < T; t++) {{
{z.next}
{sched}
      // ---- phase 1a / 2a: predict{", per group on its own dt" if pf else ""} ----
      if (c == 0 && {step}) {{
        if ({pd}) scal_predict_r(sl + {lay.OFF_X}, dt, sl, norm_quats);
        else scal_keep_r(sl + {lay.OFF_X}, sl, norm_quats);                 // predict(dt = 0) still renormalises
      }}
      rn::wave_lds_sync();{stamp(1)}
      if ({any_pd}) {{
        if (qdiag) {{
          predict_rows_qd{fsfx}({rows}, sP, {qd_args}, sl, {idx}{pda}{_tl_arg(True)});
        }} else {{
          int qz = 0;
          asm volatile("" : "+v"(qz));{note("                 // Q behind an opaque zero: its addresses are not worth registers across the step loop")}
          predict_rows{fsfx}({rows}, sP, gQ + qz, sl, {idx}{pda}{_tl_arg(True)});
        }}
      }}{stamp(2)}
      // ---- phase 1b / 2b: update{", every kind present among the wavefront's filters" if pf else ""} ----
{update}{stamp(4)}
      // ---- phase 3: lane 0 of each group injects the error state ----
      if (c == 0 && live) {{
{flags_rule}
        if (flags != nullptr) flags[t * n + base + g] = (uint8_t)fl;
      }}
      rn::wave_lds_sync();{stamp(5)}
{z.out}
      int lz = lane;
      asm volatile("" : "+v"(lz));{note("       // the copies' per-iteration indices are not worth registers across the step loop")}
      if (tx != nullptr) {{
        for (int i = lz; i < cnt * {D}; i += 64) tx[(t * n + base) * {D} + i] = s_sl[(i / {D}) * SLOT_R + {lay.OFF_X} + i % {D}];
      }}
      if (tP != nullptr) {{
{img}
        rn::wave_lds_sync();
        rn::copy_l2g<FPWR * {EE}, {nt_trace}>(tP + (t * n + base) * {EE}, cnt * {EE}, s_P, lz);
      }}
      rn::wave_lds_sync();{stamp(6)}
{z.commit}
      rn::wave_lds_sync();{stamp(7)}{after_step}
    }}
{write_back}    rn::copy_l2g<FPWR * {EE}>(gP + base * {EE}, cnt * {EE}, s_P, le);
    for (int i = le; i < cnt * {D}; i += 64) gx[base * {D} + i] = s_sl[(i / {D}) * SLOT_R + {lay.OFF_X} + i % {D}];
    rn::wave_lds_sync();
  }}
}}
"""


def run_kernel(spec):
  """k_run: the schedule is shared, kinds[t] and dts[t] are wave-uniform, and so is every branch of a step.  Extra arguments, feature-track
  kinds and the MSCKF window shift exist here and, per filter, in k_run_epf (_fused_run holds the kernel's text, _window_shift the shift's)."""
  E = spec.dim_err
  _, R, _ = layout(spec)
  lay = w2.slot_tables(spec, RunLayout)[0]
  zmax = max(k.zdim for k in spec.kinds)
  EAM = ea_max(spec)
  rows, idx = _row_args(R)
  scal_cases, mat_cases = [], []
  for k in spec.kinds:
    EA = ea_count(k)
    feat = k.He_sym is not None
    args = f"sl, sl + {lay.OFF_Y}"
    guard = ""
    if EA:
      args += f", gea + ((int64_t)t * n + base + g) * {EAM}"
      guard = "if (gea == nullptr) { bad = 8; break; } "
    if feat:
      args += f", gR + t * {zmax * zmax}"
    scal_cases.append(f"          case {k.kind}: {{ {guard}scal_obs_{k.kind}_r{'<true>' if feat else ''}({args}); break; }}")
    mat_cases.append(f"        case {k.kind}: update_{k.kind}_rows({rows}, gR + t * {zmax * zmax}, sP, s_G + gg * {zmax * E}, sl, sl, {idx}{_tl_arg(True)}); break;")
  aug = "" if spec.N <= 0 else f"""
      // MSCKF window shift after this step (EKF_sym.augment, ekf_sym.py:365-391; the schedule's augment[t]): a fixed permutation
      // of the state (one lane per filter) and of the rows / columns of P, read out of the LDS image (the trace above holds the
      // estimate BEFORE the shift, like the reference's Estimate)
{_window_shift(spec, cond="augs != nullptr && augs[t] != 0")}"""
  # predict(dt = 0) is skipped only for models where it is symbolically the identity (FilterSpec.identity_at_dt0)
  id0_guard = "true" if not spec.identity_at_dt0() else "dt != 0.0"
  nlc = chr(10)
  return _fused_run(
    spec, False, title=f"""// ---- fused multi-step run: kinds[t], dts[t] shared by all filters; z is (T, n, {zmax}) in: z, out: y -----------
// Per step, with P in registers: (1a) one lane per filter evaluates f and the non-trivial entries of F into the filter's LDS
// slot, (2a) all lanes run predict's covariance algebra on their rows, (1b) one lane per filter evaluates h and He for the
// observation kind, (2b) all lanes run the update's covariance algebra, (3) one lane per filter injects the error state.
// x lives in the slot between the phases.""",
    args=", const double* __restrict__ gea, const int32_t* __restrict__ augs", unused="\n  (void)gea; (void)augs;",
    sched=f"""      const int kind = kinds[t];
      const double dt = dts[t];
      const bool do_pred = {id0_guard};{_stamp(0)}""",
    update=f"""      int bad = 0;
      if (c == 0 && live) {{
        switch (kind) {{
{nlc.join(scal_cases)}
          default: bad = 8; break;      // unknown kind
        }}
      }}
      bad = __builtin_amdgcn_readfirstlane(__any(bad) ? 8 : 0);
      rn::wave_lds_sync();{_stamp(3)}
      if (!bad) {{
        switch (kind) {{
{nlc.join(mat_cases)}
          default: break;
        }}
      }}""",
    flags_rule=f"""        int fl = bad;
        if (!bad) fl = scal_inject_r(sl, sl + {lay.OFF_X}, norm_quats) | (int)sl[{lay.OFF_FL}];""",
    after_step=aug)


def run_pf_kernel(spec, noise=TABLE, msckf=False):
  """k_run_pf of the lane-group family: k_run's structure (GL lanes per filter, rows of P in registers, FPW filters per wavefront) with a
  SCHEDULE PER FILTER, kinds (T, n) and dts (T, n).  Every lane of a group fetches its filter's kind and dt (one address per group), a step
  ahead like the observations.  The scalar phases run on lane c == 0 of the groups that step, each on its own kind and dt.  The matrix phases
  are the predicated functions (predict_fn / update_fn with pf=True): predict runs when any group of the wavefront predicts, and for every
  kind present among the wavefront's filters (a wave-uniform test) that kind's rows update runs on all lanes, changing the rows of the
  groups that carry it.  An idle group (kind <= 0, flag 16) and a group whose kind the model does not have (flag 8) keep slot and rows.
  A filter that no entry stepped is not written back: the image of the final store is the one that came in, loaded again, and only the
  groups that stepped put their rows into it.  Above 32 error states a filter owns the wavefront and the tests are uniform anyway.
  (_fused_run holds the kernel's text.)

  noise=ENTRY: k_run_rpf, a NOISE MATRIX PER ENTRY -- gR is (T, n, zmax^2), row (t, i) the R of filter i's entry t.  Every lane of a group reads its
  filter's row (one address per group, like the schedule) a step ahead: the row of step t + 1 is requested once the update of step t has consumed
  the registers, and lands under the rest of the step with the next kind, dt and observation.  The request is unconditional on a row inside the
  buffer (group gg, the last row again at t + 1 == T); what it brings may be NaN (idle entries, entries of an unknown kind, the tail of a row), and
  `update_{kind}_rows_rpf` takes the values only where `mine`.

  noise=DIAG: k_run_dpf, a DIAGONAL NOISE PER ENTRY -- gR is (T, n, zmax), the leading Z doubles of row (t, i) the variances of filter i's entry t.
  k_run_rpf with rows of zmax doubles, Re[zmax]: requested, waited for and predicated in the same places (`update_{kind}_rows_dpf`).

  msckf=True (with noise=TABLE): k_run_epf, the same schedule text with what run_epf_kernel's docstring lists."""
  assert noise is TABLE or not msckf
  E = spec.dim_err
  _, R, _ = layout(spec)
  lay = w2.slot_tables(spec, RunLayout)[0]
  zmax = max(k.zdim for k in spec.kinds)
  ZZ, EAM = noise.row(zmax), ea_max(spec)      # doubles per row of gR, of gea
  rows, idx = _row_args(R)
  nlc = chr(10)
  known = " ".join(f"case {k.kind}:" for k in spec.kinds)
  psfx, usfx = ("_epf", "_epf") if msckf else ("_pf", noise.update)      # the names of the predicated predict / update functions
  scal_cases, mat = [], []
  for i, k in enumerate(spec.kinds):      # (extra arguments and feature-track kinds: MSCKF models only, emit.has_run_pf)
    feat = k.He_sym is not None
    args = f"sl, sl + {lay.OFF_Y}" + (f", gea + ((int64_t)t * n + base + g) * {EAM}" if ea_count(k) else "") + (f", gR + {i * ZZ}" if feat else "")
    scal_cases.append(f"          case {k.kind}: scal_obs_{k.kind}_r{'<true>' if feat else ''}({args}); break;")
    mat.append(f"""      {{
        const bool mine = step && kind == {k.kind};
        if (__any(mine)) update_{k.kind}_rows{usfx}({rows}, {"Re" if noise.per_entry else f"gR + {i * ZZ}"}, sP, s_G + gg * {zmax * E}, sl, sl, {idx}, mine{_tl_arg(True)});
      }}""")
  id0_guard = "true" if not spec.identity_at_dt0() else "dt != 0.0"
  title, kname, args, after_step = noise.title_wide.format(zmax=zmax, ZZ=ZZ), noise.kernel, "", ""
  aug_first = aug_now = aug_next = ""
  if msckf:      # the MSCKF flavour's own (run_epf_kernel), beside the names and the scalar cases' arguments above
    title = (f"// ---- fused multi-step run, a schedule per filter, MSCKF models: k_run_pf (gR one row per kind) with gea (T, n, {EAM}) extra arguments per entry "
             "and augs (T, n) or NULL, a window shift after the entry, per group (see emit_wide3.run_epf_kernel) -----------")
    aug_first = "    int aug_n = augs != nullptr ? augs[base + gg] : 0;\n"
    aug_now = "      const int aug = aug_n;\n"
    aug_next = "        if (augs != nullptr) aug_n = augs[tn * n + base + gg];\n"
    kname, args = "k_run_epf", ", const double* __restrict__ gea, const int32_t* __restrict__ augs"
    after_step = f"""
      // MSCKF window shift after this step, per group (k_run's block under the group's own predicate; the trace above holds the estimate
      // BEFORE the shift): every lane meets the fences, only the shifting groups take the new rows and write x
      {{
        const bool sh = step && aug != 0;
{_window_shift(spec, pad="  ", cond="__any(sh)", guard="sh")}
      }}"""
  r_first, r_next = "", ""
  if noise.per_entry:
    r_first = f"""    // the group's own row of R, a step ahead like its schedule entry; taken by the updates only where the group carries their kind
    double Re[{ZZ}];
#pragma unroll
    for (int i = 0; i < {ZZ}; i++) Re[i] = gR[(base + gg) * {ZZ} + i];
"""
    r_next = f"""
      {{      // the update has consumed the row: the next entry's, under the rest of this step (the last row again at the end: inside the buffer)
        const int64_t tn = t + 1 < T ? t + 1 : t;
        const double* rp_ = gR + (tn * n + base + gg) * {ZZ};
#pragma unroll
        for (int i = 0; i < {ZZ}; i++) Re[i] = rp_[i];
      }}"""
  return _fused_run(
    spec, True, title=title, kname=kname, fsfx=psfx, args=args, after_step=after_step,
    pre_loop="""    bool stepped = false;
    // the group's own schedule entry, a step ahead (every lane of a group reads its filter's: one address per group)
    int kind_n = kinds[base + gg];
    double dt_n = dts[base + gg];
""" + aug_first + r_first,
    sched=f"""      const int kind = live ? kind_n : 0;
      const double dt = dt_n;
{aug_now}      {{
        const int64_t tn = t + 1 < T ? t + 1 : t;
        kind_n = kinds[tn * n + base + gg];
        dt_n = dts[tn * n + base + gg];
{aug_next}      }}
      bool step = false;
      switch (kind) {{ {known} step = true; break; default: break; }}
      const bool pd = step && ({id0_guard});
      stepped = stepped || step;""",
    update=f"""      if (c == 0 && step) {{
        switch (kind) {{
{nlc.join(scal_cases)}
          default: break;
        }}
      }}
      rn::wave_lds_sync();
{nlc.join(mat)}{r_next}""",
    flags_rule=f"""        int fl = kind <= 0 ? 16 : 8;          // idle entry; a kind the model does not have: untouched either way
        if (step) fl = scal_inject_r(sl, sl + {lay.OFF_X}, norm_quats) | (int)sl[{lay.OFF_FL}];""")


def _shift_maps(spec):
  """The MSCKF window shift (EKF_sym.augment, ekf_sym.py:365-391) as fixed permutations -> (src_x, se): new state entry i is old entry
  src_x[i], new row / column i of P is old row / column se(i)."""
  D, E = spec.dim_x, spec.dim_err
  d1, d2, d3, d4 = spec.dim_main, spec.dim_main_err, spec.dim_augment, spec.dim_augment_err
  src_x = [i if i < d1 else (i + d3 if i < D - d3 else i - (D - d3)) for i in range(D)]

  def se(i):
    r = i if i < E - d4 else i - (E - d4)
    return r if r < d2 else r + d4
  return src_x, se


def _window_shift(spec, cond, pad="", guard=""):
  """The block `if (cond) { ... }` of the MSCKF window shift, for k_run and k_run_epf alike: the image is written from the rows, lane 0 of a group
  permutes x, and the rows are re-read out of the image through the fixed permutation (_shift_maps); every lane meets both fences.
  k_run: `cond` is the wave-uniform augs[t], every live group shifts.  k_run_epf: the block sits `pad` deeper, `cond` asks whether any group of
  the wavefront shifts and `guard` is the group's own predicate: only the shifting groups write x and take the new rows."""
  D, E = spec.dim_x, spec.dim_err
  _, R, _ = layout(spec)
  lay = w2.slot_tables(spec, RunLayout)[0]
  d2, d4 = spec.dim_main_err, spec.dim_augment_err
  src_x, se = _shift_maps(spec)
  nl = chr(10)
  shift = []
  for s in range(R):
    # (guard: a branch on the group's predicate, not a select per entry: with `row = sh ? image : row` hipcc kept the row arrays in scratch memory,
    # 256 bytes per lane on the 15-state model; the lanes of the other groups are masked off through the same statements)
    shift.append(f"{pad}        {f'if ({guard}) ' if guard else ''}{{ const int sr = (rc{s} < {E - d4} ? rc{s} : rc{s} - {E - d4}); const int srow = sr < {d2} ? sr : sr + {d4};")
    shift += [f"{pad}          row{s}[{j}] = sP[srow * {E} + {se(j)}];" for j in range(E)]
    shift.append(f"{pad}        }}")
  return f"""{pad}      if ({cond}) {{
{_img(E, R, pad=pad)}
{pad}        rn::wave_lds_sync();
{pad}        if (c == 0 && {guard or "live"}) {{
{pad}          double xo[{D}];
#pragma unroll
{pad}          for (int i = 0; i < {D}; i++) xo[i] = sl[{lay.OFF_X} + i];
{nl.join(f"{pad}          sl[{lay.OFF_X + i}] = xo[{src_x[i]}];" for i in range(D) if src_x[i] != i)}
{pad}        }}
{nl.join(shift)}
{pad}        rn::wave_lds_sync();
{pad}      }}"""


def run_epf_kernel(spec):
  """k_run_epf, MSCKF models: k_run_pf (one R per kind) with what k_run alone carried so far, per filter.
    * EXTRA ARGUMENTS PER ENTRY: gea is (T, n, EA), EA the largest kind_eadim.  Lane c == 0 of a group that steps a kind with extra arguments
      reads its own row (t n + base + g) EA inside that kind's scalar phase; no other row is read (idle entries, entries of an unknown kind
      and of kinds without extra arguments may hold NaN there).
    * FEATURE-TRACK KINDS: `update_{kind}_rows_epf` (update_fn(pf=True)) carries `mine` through the null-space-projected update.  The projected
      noise, rank_deficient and the reflectors of the slot mean something only where `mine`; any other group takes the identity, 0 and zero
      coefficients by SELECT (its slot is stale, NaN at first, and 0 * NaN is NaN) and writes nothing into its slot.
    * A WINDOW SHIFT PER FILTER: augs is (T, n) or NULL, fetched a step ahead with kind and dt.  After step t the groups with step && aug != 0
      shift, with the arithmetic of k_run's block: the image is written from the rows, lane 0 permutes x, the rows are re-read through the
      fixed permutation -- every lane meets both fences, only the shifting groups take the new rows and write x (the others masked off).
      The block is skipped when no group of the wavefront shifts.  An entry that did not step its filter (idle, unknown kind) does not shift
      it; one whose projection was rank deficient (flag 4) does, as in k_run.  The trace row is the estimate BEFORE the shift.
  (_fused_run holds the kernel's text.)"""
  return run_pf_kernel(spec, msckf=True).strip("\n")      # (one title line, no blank line around: tools/emit_digest.py --without k_run_epf takes exactly this text out)


def launch_run_epf():
  return _launch("k_run_epf", ", ea, augment")


def _launch(kname, more=""):
  return f"""  const int64_t tiles = (n + FPWR - 1) / FPWR;
  hipLaunchKernelGGL({kname}, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, trace_x, trace_P{more});"""


def launch_run_pf(noise=TABLE):
  return _launch(noise.kernel)


def launch_run():
  return _launch("k_run", ", ea, augment")
