"""Kernel family W, smoother `k_rts4`: the RTS backward pass with EVERY BROADCAST OPERAND TAKEN FROM REGISTERS (`row_newbcast`).

Reference: the Python-only `EKF_sym.rts_smooth` (/root/reference/rednose/helpers/ekf_sym.py:651-690); per backward step k
    Fk = F(xk_k, t[k+1] - t[k]);  Ck = solve(Pk1_k, Fk Pk_k^T)^T;  xk_n = err(xk_k, Ck inv_err(xk1_k, xk1_n));
    Pk_n = Pk_k + Ck (Pk1_n - Pk1_k) Ck^T
with the predicted pair (xk1_k, Pk1_k) recomputed from the filtered one (templates/ekf_hip_rts.h explains the recursion's quirks,
which are kept: start from the PREDICTED pair of the last step, in-place renormalisation of xk1_n).

Why this layout.  Its predecessor `k_rts3` (the fused run's layout: 8 lanes x 3 rows per filter; deleted in round 6) ran ONE wavefront per
SIMD (two row sets of 132 registers each + an LDS image per filter) and took every operand another lane owns through LDS: one 8-byte
broadcast read feeds three FMAs, four wavefronts share a CU's LDS, and a lone wavefront issues an fp64 instruction every ~10 cycles (a
dependent one every ~27-40): 0.25 of the HBM roofline for two rounds, whatever was moved inside it (profiles/tuning_notes.md).  CDNA3/4 have exactly one cross-lane form for fp64
arithmetic: `v_fmac_f64_dpp ... row_newbcast:L` -- lane L of every 16-lane row feeds all 16 lanes of that row, at the plain FMA's
issue rate (tools/dpp_probe.hip: 5.4-5.8 cycles per instruction with two wavefronts per SIMD, 6.5 alone; semantics checked there).
So here a filter is ONE 16-LANE ROW (4 filters per wavefront), row r of every matrix lives in slot r // RS of lane r % RS (RS = rows per
slot: 22 error states = 2 slots x 11 lanes), and
  * the right-looking L D L^T factorisation, both substitutions and both E^3 products read the other lanes' rows straight out of
    their registers: no LDS broadcast, no LDS round trip inside a dependent chain, 22 independent accumulation chains per pass;
  * the smoothed covariance of step k + 1 is CARRIED in registers (k_rts3 stored it and read it back: +11 % traffic, a wait for
    the previous step's stores in the middle of every step);
  * at most two row sets (2 x 88 registers for 22 error states) + one half set are live at any point, the third matrix of each
    phase waits in the filter's single E x E image of LDS -- 19.5 KB per wavefront for live: EIGHT wavefronts per CU, two per
    SIMD, which is what hides the dependent chains (pivot reciprocals, the one-lane scalar phase) that a lone wavefront exposes.
The price: 22 of 32 row slots busy (k_rts3: 22 of 24), i.e. ~1.15 x the vector instructions per filter-step.

  step k (image I per filter; register row sets in capitals):
    Pk_k HBM -> I (one coalesced asynchronous burst); lead lanes evaluate f / F non-zeros (scal_predict) meanwhile
    rows of Pk_k <- I (lower triangle mirrored: the batch_rts contract);  rows of A = Pk_k Fk^T (row-local, sparse) -> I
    Pp <- rows of Pk1_k = (columns of A) Fk^T + dt Q;   D <- PS - Pp  (PS: smoothed covariance of step k + 1, carried)
    Pp <- its L D L^T factor, right-looking: column j scaled by the broadcast pivot's reciprocal, trailing columns updated with
          v_fmac_f64_dpp (unscaled entry of row m from lane m, own scaled entry as the other factor)
    per row slot: Y <- row of A from I; forward substitution, scaling, backward substitution (axpy form, 21 .. 1 independent
          FMAs per pivot); Y = row of Ck -> I
    state: delta = Ck inv_err(xk1_k, xk1_n), xk_n = err(xk_k, delta)  (lead lanes + one E-term dot per row)
    T <- Ck D per row slot (coefficients: the lane's own row of Ck from I; operands: rows of D by row_newbcast)
    CK <- I;  U = T Ck^T per row slot (operands: rows of Ck by row_newbcast); symmetric: slot 0 forms columns 0 .. 15 only
    I <- U (mirrored);  Pk_n = Pk_k + U: one coalesced read-add-write over the tile's records, the sum also goes back into I
    PS <- rows of I
  step k with t[k + 1] == t[k] (models whose predict(0) is the identity; not the recursion's first step): Ck = I, see dt0_path() / identity_step():
    Pk_k HBM -> I;  xk_n = err(xk_k, inv_err(xk_k, xk1_n));  D <- PS - lower(Pk_k);  Pk_n = Pk_k + D row by row in place;  I -> HBM;  PS <- rows of I
  `k_rts4_tri` (kernel(tri=True)): the same on a trace of PACKED lower triangles -- elements are scattered to / gathered from the images' lower
  positions through a byte table of row indices in LDS.

Generated for ordinary (non-MSCKF) lane-group models whose 4 images + vectors fit 20 KB of LDS (8 .. 22 error states, odd counts
included: live, kinematic9); every other lane-group model -- MSCKF, more states, a dense F whose non-zeros do not fit the slot --
keeps rn::k_rts_group, which is also the fallback (`no_rts4`).  (k_rts3, the round-4 smoother in the fused run's layout, served the
odd counts until round 6 and is gone.)
"""
from rednose_amd.codegen import emit_wide2 as w2, tuning
from rednose_amd.codegen.emit_common import SlotLayout, term, sum_terms

GL = 16            # lanes per filter: one DPP row
FPW = 4            # filters per wavefront
LDS_BUDGET = 20480  # bytes per wavefront: eight wavefronts on a CU's 160 KB


MACROS = r"""
// ---- fp64 cross-lane operands without LDS: lane L of every 16-lane row feeds the row (the only DPP form double-precision ALU
// instructions have on gfx90a / gfx94x / gfx950).  tools/dpp_probe.hip: semantics, and the same issue rate as a plain v_fma_f64.
// EXEC must be full where these execute (a disabled source lane is not a valid source): the kernel keeps them out of divergent code.
#ifndef RN4_FMAC
#define RN4_FMAC(acc, src, coef, L)  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #L " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(coef))
#define RN4_FNMAC(acc, src, coef, L) asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:" #L " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(coef))
// (s_nop 1: a DPP read of a register the previous vector instruction wrote wants two wait states; inline asm is opaque to hipcc's hazard pass)
#define RN4_BC(dst, src, L)          asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:" #L " row_mask:0xf bank_mask:0xf" : "=v"(dst) : "v"(src))
// RN4_FMAC / RN4_FNMAC carry no wait states (two per instruction would cost the products a third of their issue rate).  Their DPP sources are
// register rows that ordinary C statements wrote (the rows of Pk1_k, the factor's scaled columns): hipcc may sink such a statement to right in
// front of its first reader.  So at the head of every phase that reads a row set through DPP the rows are pinned (rn::pin: the writers cannot sink
// below) and RN4_SETTLE() puts the two wait states between them and the phase -- volatile asm statements keep their order.  What remains possible is
// a register copy hipcc's allocator places in front of a reader: rednose_amd.build.dpp_hazards checks every built k_rts4 for that.
#define RN4_SETTLE()                 asm volatile("s_nop 1")
#endif
"""


def rows_per_lane(spec):
  return -(-spec.dim_err // GL)


def lds_bytes(spec, slot, tri=False):
  D, E = spec.dim_x, spec.dim_err
  base = 8 * (FPW * E * E + 2 + FPW * slot + 2 * (FPW * D + 2) + FPW * E + 2 + E + 2 * FPW * (GL - -(-E // rows_per_lane(spec))) + 2)
  return base + (8 * -(-(E * (E + 1) // 2) // 8) if tri else 0)      # k_rts4_tri: the row of every packed index, one byte each


def tri_applicable(spec):
  """k_rts4_tri (the packed-triangle trace, see kernel()) needs E (E + 1) / 2 more bytes of LDS under the same budget."""
  if not applicable(spec):
    return False
  lay = w2.slot_tables(spec, RtsLayout, with_obs=False)[0]
  return lds_bytes(spec, lay.SLOT, tri=True) <= LDS_BUDGET


class RtsLayout(SlotLayout):
  """Scalar slot of the smoother (doubles per filter): x' = f(x) [normalised], the non-trivial entries of F, dt."""

  def pack(self, D, E):
    self.nh = self.zf = 0
    self.OFF_F = D
    self.OFF_DT = D + self.nf
    n = self.OFF_DT + 1
    # fields the shared scalar functions of emit_wide2.scalar_functions address but the smoother never calls
    self.OFF_HE = self.OFF_DX = self.OFF_Y = self.OFF_FL = self.OFF_RF = self.OFF_RP = self.OFF_YP = n
    return n


def dt0_path(spec):
  """Steps with dt == 0 take the identity-gain path (see identity_step()): only for models whose predict(dt = 0) is the identity symbolically."""
  return bool(tuning.current().rts_dt0) and spec.identity_at_dt0()


def applicable(spec):
  """Ordinary (non-MSCKF) lane-group models with 8 .. 32 error states whose four images + vectors fit LDS_BUDGET."""
  msckf = any(k.He_sym is not None for k in spec.kinds) or spec.N > 0
  if msckf or spec.dim_main_err != spec.dim_err:
    return False
  E = spec.dim_err
  if E < 8 or E > 2 * GL:
    return False
  lay = w2.slot_tables(spec, RtsLayout, with_obs=False)[0]
  return lds_bytes(spec, lay.SLOT) <= LDS_BUDGET


# Issue priority: the two E^3 products (stamps 7 .. 9) are straight FMA streams that can run any time; everything else in a step is a chain of
# dependent latencies (LDS round trips, the pivots' reciprocals, the one-lane scalar phase, memory).  With the products at priority 0 and the
# rest at 3 the co-resident wavefront's chains issue ahead of this one's FMA stream: 8.31 -> 7.73 ms on 8 192 x 300 steps, same call
# (other windows measured: products + substitutions low 8.07, substitutions only 8.27, levels 1 / 2 instead of 3: 7.85; tools/rts4_time.py).
# (first stamp, last stamp, level outside): phase_h opens the window behind its stamp 7 with level 0, phase_i closes it behind its stamp 9.
PRIO = (7, 9, 3)
U = "#pragma unroll"


def setprio(level, ind="      "):
  return [f"{ind}__builtin_amdgcn_s_setprio({level});"]


class Geometry:
  """What the phase builders of one kernel (k_rts4, tri: k_rts4_tri) share: sizes, the slot layout, where a row lives, the record provider."""

  def __init__(self, spec, tri, pf=False):
    self.tri, self.pf = tri, pf
    self.D, self.E = D, E = spec.dim_x, spec.dim_err
    self.EE = E * E
    self.TRI = E * (E + 1) // 2
    self.REC = self.TRI if tri else self.EE          # doubles per covariance record in memory
    self.ITT = -(-(FPW * self.TRI) // 64)       # packed elements per lane of a tile
    self.kname = "k_rts4_pf" if pf else ("k_rts4_tri" if tri else "k_rts4")
    self.R = rows_per_lane(spec)
    self.S = range(self.R)
    self.RS = -(-E // self.R)        # rows per slot: row r lives in slot r // RS of lane r % RS (22 states: 2 x 11 -- balanced slots keep the block lower
                                     # triangles of the symmetric matrices at 11 + 22 columns per lane instead of 16 + 22, and lanes RS .. 15 idle)
    self.lay, self.Fs, _, low = w2.slot_tables(spec, RtsLayout, with_obs=False)
    self.scal, = w2.scalar_functions(spec, self.lay, low, sfx="_s4", only=("scal_predict",))      # the only scalar phase the smoother calls
    self.quat = "".join(f" rn::normalize_quat<{D}>(xv, {q});" for q in spec.quaternion_idxs)
    self.XT = -(-(FPW * D) // 64)
    self.IT = -(-(FPW * self.EE // 2) // 64)
    self.ITF = (FPW * self.EE // 2) // 64          # iterations of the coalesced passes that are whole for a full tile
    self.dt0 = dt0_path(spec)
    self.busy, self.groups = fk_groups(self.Fs, E)
    self.rec = (Packed if tri else Full)(self)

  def slot_of(self, r):
    return r // self.RS

  def lane_of(self, r):
    return r % self.RS

  def last_row(self, s):       # last row index a slot can hold
    return min(self.E, self.RS * s + self.RS) - 1

  def ncol(self, s):           # columns a row slot keeps of a SYMMETRIC matrix: up to its last row (block lower triangle)
    return self.last_row(s) + 1

  def upd_slots(self, m):          # slots that hold a row >= m
    return [s for s in self.S if self.last_row(s) >= m]

  def rows_decl(self, name, sym_=False):
    return " ".join(f"double {name}{s}[{self.ncol(s) if sym_ else self.E}];" for s in self.S)


# ---- fragments that occur more than once: each takes its indentation and, where they differ, its names ----

def opaque(ind, names, srcs=None, note="", note2=""):
  """opaque copies `names` of the lane / row indices `srcs` (None: the names themselves, afresh): index arithmetic derived from them stays where it is"""
  decl = [f"{ind}int " + ", ".join(f"{n} = {v}" for n, v in zip(names, srcs)) + ";" + note] if srcs else []
  return decl + [f'{ind}asm volatile("" : ' + ", ".join(f'"+v"({n})' for n in names) + ");" + note2]


def settle(g, name, ind="      "):
  """the block-lower rows `name` are about to be read through DPP: see RN4_SETTLE"""
  return [ln for s in g.S for ln in (U, f"{ind}for (int j = 0; j < {g.ncol(s)}; j++) rn::pin({name}{s}[j]);")] + [f"{ind}RN4_SETTLE();"]


def sym_row(g, s, ind, dst, rc, op="=", note="", full=False):
  """`dst[j] op M[rc][j]` for row rc (of slot s) of a symmetric matrix from the LOWER triangle of the image: entry j is M[rc][j] for j <= rc, M[j][rc]
  above (full=False: only the columns up to the slot's last row)."""
  E, lo, hi = g.E, g.RS * s, g.ncol(s)
  o = [U, f"{ind}for (int j = 0; j < {lo}; j++) {dst}[j] {op} sI[{rc} * {E} + j];"] if lo else []
  o += [U, f"{ind}for (int j = {lo}; j < {hi}; j++) {dst}[j] {op} sI[{E} * max({rc}, j) + min({rc}, j)];{note}"]
  if hi < E and full:
    o += [U, f"{ind}for (int j = {hi}; j < {E}; j++) {dst}[j] {op} sI[j * {E} + {rc}];"]
  return o


def lower_rows(g, name, ind="      ", rc="rq", full=False):
  """the lane's rows `name{s}` of a symmetric matrix from the image (sym_row per slot)"""
  note = "      // (max / min / mad: no compare-select pair per entry)"
  return [ln for s in g.S for ln in sym_row(g, s, ind, f"{name}{s}", f"{rc}{s}", note=note, full=full)]


def renormalise(g, ind):
  """xk1_n is renormalised in place (the recursion's quirk, templates/ekf_hip_rts.h)"""
  return [f"""{ind}if (lead && (norm_quats & 2)) {{
{ind}  double xv[{g.D}];
#pragma unroll
{ind}  for (int i = 0; i < {g.D}; i++) xv[i] = sxn[i];
{ind} {g.quat}
#pragma unroll
{ind}  for (int i = 0; i < {g.D}; i++) sxn[i] = xv[i];
{ind}}}"""]


def store_xs(g, ind):
  """(through an opaque lane index of its own: lo)"""
  return opaque(ind, ["lo"], ["lb"]) + [f"{ind}for (int i = lo; i < cnt * {g.D}; i += 64) xs[((k + 1) * n + base) * {g.D} + i] = s_xn[i];      // smoothed state of step k + 1 (after its renormalisation)"]


def request_xnext(g, ind, lane):
  """xk_k of the next (older) step is requested early and committed to LDS (commit_xnext) once the lead lanes have read this step's"""
  return [U, f"{ind}for (int it = 0; it < {g.XT}; it++) {{ const int i = {lane} + 64 * it; xnext[it] = xf[((k > 0 ? k - 1 : 0) * n + base) * {g.D} + (i < cnt * {g.D} ? i : 0)]; }}"]


def commit_xnext(g, ind, lane):
  return [U, f"{ind}for (int it = 0; it < {g.XT}; it++) {{ const int i = {lane} + 64 * it; if (i < cnt * {g.D}) s_xk[i] = xnext[it]; }}"]


def read_add_write(g, guard):
  """one pass of Pk_n = Pk_k + U over the tile's full records (v: Pk_k as requested under the last product block); the sum also returns to the image"""
  return [f"""#pragma unroll
        for (int it = 0; it < {g.IT}; it++) {{
          const int idx = le + 64 * it;
          if ({guard}) {{
            rts4_d2* im = reinterpret_cast<rts4_d2*>(s_I + 2 * idx);
            const rts4_d2 w_ = v[it] + *im;
            out2[idx] = w_;
            *im = w_;
          }}
        }}"""]


def fk_groups(Fs, E):
  """-> (rows of Fk that have entries off the diagonal, the same in groups of at most 10 run-time coefficients)"""
  busy = [j for j in range(E) if any(m != j or cf[0] != 'one' for m, cf in Fs.row_nz(j))]
  groups, cur, ncoef = [], [], 0
  for j in busy:
    nv_ = sum(1 for _, cf in Fs.row_nz(j) if cf[0] == 'var')
    if cur and ncoef + nv_ > 10:
      groups.append(cur)
      cur, ncoef = [], 0
    cur.append(j)
    ncoef += nv_
  if cur:
    groups.append(cur)
  return busy, groups


def grouped(Fs, groups, tag, ind, emit_row):
  """emit_row(j, reg_term) -> C lines for row j of Fk, with the coefficients of the groups software-pipelined one group ahead."""
  regname = {}

  def gl(grp):
    out = []
    for j in grp:
      for _, cf in Fs.row_nz(j):
        if cf[0] == 'var' and cf[1] not in regname:
          regname[cf[1]] = f"{tag}{len(regname)}"
          out.append(f"{ind}const double {regname[cf[1]]} = {cf[1]};")
    return out

  def reg_term(cf, operand):
    return f"{regname[cf[1]]}*{operand}" if cf[0] == 'var' else term(cf, operand)
  o = gl(groups[0]) if groups else []
  for gi, grp in enumerate(groups):
    if gi + 1 < len(groups):
      o += gl(groups[gi + 1])
    o.append(f"{ind}__builtin_amdgcn_sched_barrier(0);")
    for j in grp:
      o += [ind + ln for ln in emit_row(j, reg_term)]
  return o + [f"{ind}__builtin_amdgcn_sched_barrier(0);"]


# ---- the two record layouts: every place where a covariance record crosses memory takes its fragment from one of these (Geometry.rec) ----

class Full:
  """Records are E x E matrices.  An even record length moves HBM -> LDS directly; an odd one is staged through registers (request_tile)."""
  table = ""

  def __init__(self, g):
    self.g = g

  def newest_in(self):
    EE = self.g.EE
    return [f"""      rn::async_copy_g2l<{FPW} * {EE}>(Pl + base * {EE}, cnt * {EE}, s_I, lt);
      for (int i = lt; i < cnt * {EE}; i += 64) Ps[((T - 1) * n + base) * {EE} + i] = Pl[base * {EE} + i];
      rn::async_wait();"""]

  def request_tile(self):
    EE = self.g.EE
    if EE % 2:
      # Records of an odd number of doubles: the tile of step k starts at (k n + base) E^2 doubles, 16-byte aligned only when k n is even.  The
      # direct HBM -> LDS transfer wants 16-byte aligned global addresses; ordinary 16-byte vector loads do not (dword alignment is enough on the
      # device), so these models stage the tile through registers -- the copy is not hidden under the scalar phase (the test models and kinematic9).
      return [f"      rn::copy_g2l<{FPW} * {EE}>(Pf + (k * n + base) * {EE}, cnt * {EE}, s_I, lb);"]
    return [f"""      if (cnt == {FPW}) {{      // (full tile: unguarded transfers -- sixteen predicated regions otherwise)
        const double* __restrict__ gp = Pf + (k * n + base) * {EE};
#pragma unroll
        for (int it = 0; it < {self.g.IT}; it++) {{
          if (it < {self.g.ITF} || lb + 64 * it < {FPW * EE // 2})
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp + 2 * (lb + 64 * it)), rn::lds_offset_ptr(s_I + 2 * 64 * it), 16, 0, 0);
        }}
      }} else {{
        rn::async_copy_g2l<{FPW} * {EE}>(Pf + (k * n + base) * {EE}, cnt * {EE}, s_I, lb);      // no register staging: lands under the scalar phase
      }}"""]

  def land(self, ind):
    return []      # (the transfer writes the image itself: the phases wait for it)

  def identity_step(self):
    """Covariance of the identity-gain step.  U = D = Pk1_n - Pk1_k with Pk1_k = the LOWER triangle of Pk_k mirrored (the contract of batch_rts); a lane
    holds D on the block lower triangle of its rows (in place of the carried rows); what a row needs of D beyond its slot's last row belongs to the lanes
    of the later slots, which put it where the row's own entries of that block were (the upper-right block of the image, read into registers first).  The
    sum Pk_k + U is then formed row by row in place, with the entries of Pk_k as stored (above the diagonal too)."""
    g = self.g
    E, EE, RS, S, ncol = g.E, g.EE, g.RS, g.S, g.ncol
    o = []
    for s in S:
      o += sym_row(g, s, "        ", f"ps{s}", f"rq{s}", op="-=") + ["        __builtin_amdgcn_sched_barrier(0);"]
    for s in S:
      if ncol(s) < E:
        o += [f"        double pu{s}[{E - ncol(s)}];", U, f"        for (int j = {ncol(s)}; j < {E}; j++) pu{s}[j - {ncol(s)}] = sI[rq{s} * {E} + j];"]
    if g.R > 1:
      o.append("        rn::wave_lds_sync();      // every lane has read what the exchange overwrites")
      for s in S:
        if RS * s:
          o += [f"        {{ double* swc = ok{s} ? sI + rq{s} : strash; const int st = ok{s} ? {E} : 0;      // column rq{s} of the rows above the slot (idle lanes: one trash entry)",
                U, f"          for (int j = 0; j < {RS * s}; j++) swc[j * st] = ps{s}[j]; }}"]
      o.append("        rn::wave_lds_sync();")
    else:
      o.append("        rn::wave_lds_sync();      // every lane has read what it mirrors from other rows: the rows take the sums")
    for s in S:
      o += ["        {", f"          double o_[{E}];", U, f"          for (int j = 0; j < {E}; j++) o_[j] = sI[rq{s} * {E} + j];",
            U, f"          for (int j = 0; j < {ncol(s)}; j++) o_[j] += ps{s}[j];      // Pk_n = Pk_k + U, U = D (Ck = I)"]
      if ncol(s) < E:
        o += [U, f"          for (int j = {ncol(s)}; j < {E}; j++) o_[j] += pu{s}[j - {ncol(s)}];      // (the sum commutes: U arrived in the image, Pk_k waits in pu)"]
      o += [U, f"          for (int j = 0; j < {E}; j++) sw{s}[j] = o_[j];", "        }", "        __builtin_amdgcn_sched_barrier(0);"]
    o += [f"""        rn::wave_lds_sync();
        {{      // Pk_n leaves: one coalesced pass over the tile's records
          typedef double rts4_d2 __attribute__((ext_vector_type(2)));
          rts4_d2* __restrict__ out2 = reinterpret_cast<rts4_d2*>(Ps + (k * n + base) * {EE});
          const int nv = (cnt * {EE}) / 2;
#pragma unroll
          for (int it = 0; it < {g.IT}; it++) {{
            const int idx = lo + 64 * it;
            if ((cnt == {FPW} && it < {g.ITF}) || idx < nv) out2[idx] = *reinterpret_cast<const rts4_d2*>(s_I + 2 * idx);
          }}"""]
    if EE % 2:
      o.append(f"          if (((cnt * {EE}) & 1) && lo == 0) Ps[(k * n + base) * {EE} + cnt * {EE} - 1] = s_I[cnt * {EE} - 1];      // (odd record length, ragged tile: the last double)")
    return (o + ["        }"] + opaque("        ", [f"rq{s}" for s in S]) + lower_rows(g, "ps", ind="        ")
            + ["        rn::wave_lds_sync();      // every lane has its rows: the image is free for the next step's burst"])

  def store_predicted(self, also=""):
    """(also: a further condition of the lane, k_rts4_pf's `&& fresh`)"""
    g = self.g
    o = [f"          double* __restrict__ po = Ps + ((k + 1) * n + base + gg) * {g.EE};      // the recomputed Pk1_k leaves mirrored from the block lower triangle the lanes hold"]
    for s in g.S:
      o += [U, f"          for (int j = 0; j < {g.ncol(s)}; j++) {{ if (ok{s}{also}) po[rr{s} * {g.E} + j] = a{s}[j]; }}"]
      if g.RS * s:
        o += [U, f"          for (int j = 0; j < {g.RS * s}; j++) {{ if (ok{s}{also}) po[j * {g.E} + rr{s}] = a{s}[j]; }}"]
    return o

  def final_decl(self):
    EE = self.g.EE
    return [f"""      const rts4_d2* __restrict__ in2 = reinterpret_cast<const rts4_d2*>(Pf + (k * n + base) * {EE});
      rts4_d2* __restrict__ out2 = reinterpret_cast<rts4_d2*>(Ps + (k * n + base) * {EE});
      const int nv = (cnt * {EE}) / 2;
      rts4_d2 v[{self.g.IT}];"""]

  def final_request(self):
    g, half = self.g, FPW * self.g.EE // 2
    return [f"""      if (cnt == {FPW}) {{
#pragma unroll
        for (int it = 0; it < {g.IT}; it++) {{ const int idx = le + 64 * it; v[it] = in2[(it < {g.ITF} || idx < {half}) ? idx : {half - 1}]; }}
      }} else {{
#pragma unroll
        for (int it = 0; it < {g.IT}; it++) {{ const int idx = le + 64 * it; v[it] = in2[idx < nv ? idx : nv - 1]; }}
      }}"""]

  def mirror_u(self):
    """upper-right blocks of U, inside the image (the records hold whole matrices)"""
    g = self.g
    if all(g.ncol(s) == g.E for s in g.S):
      return []
    o = ["      {      // upper-right blocks: U[r][j] = U[j][r] for the columns beyond a slot's last row"]
    for s in g.S:
      nc_ = g.ncol(s)
      if nc_ < g.E:
        o += ["        {", f"          double m_[{g.E - nc_}];", U, f"          for (int j = {nc_}; j < {g.E}; j++) m_[j - {nc_}] = sI[j * {g.E} + rq{s}];",
              U, f"          for (int j = {nc_}; j < {g.E}; j++) sw{s}[j] = m_[j - {nc_}];", "        }"]
    return o + ["      }", "      rn::wave_lds_sync();"]

  def final_pass(self):
    g, EE = self.g, self.g.EE
    o = [f"      if (cnt == {FPW}) {{      // full tile: the first {g.ITF} passes of the wavefront are whole"]
    o += read_add_write(g, f"it < {g.ITF} || idx < {FPW * EE // 2}") + ["      } else {"] + read_add_write(g, "idx < nv")
    if EE % 2:
      o += [f"""        if (((cnt * {EE}) & 1) && le == 0) {{      // odd record length, ragged tile: the last double
          const int e_ = cnt * {EE} - 1;
          const double w_ = Pf[(k * n + base) * {EE} + e_] + s_I[e_];
          Ps[(k * n + base) * {EE} + e_] = w_;
          s_I[e_] = w_;
        }}"""]
    return o + ["      }"]


class Packed:
  """Records are packed lower triangles (row-major, E (E + 1) / 2 doubles).  The image stays E x E: an element goes to / comes from its LOWER position
  through s_tr, the row of every packed index."""

  def __init__(self, g):
    self.g = g
    self.table = f"""  __shared__ unsigned char s_tr[{-(-g.TRI // 8) * 8}];      // row of every packed index (p = r (r + 1) / 2 + j, j <= r)
  for (int p = lane; p < {g.TRI}; p += 64) {{ int r = 0; while ((r + 1) * (r + 2) / 2 <= p) r++; s_tr[p] = (unsigned char)r; }}
  rn::wave_lds_sync();
"""

  def off(self, idx, ind):
    """C line: image offset `o_` (filter f_, lower position of packed index p_) of the tile's packed element `idx`"""
    g = self.g
    return f"{ind}const int f_ = ({idx}) / {g.TRI}; const int p_ = ({idx}) - f_ * {g.TRI}; const int r_ = s_tr[p_]; const int o_ = f_ * {g.EE} + r_ * {g.E} + p_ - (r_ * (r_ + 1)) / 2;"

  def each(self, ind, lane, body):
    """`body` for every packed element of the tile the lane owns: idx in the tile, o_ in the images"""
    g = self.g
    shell = [U, f"{ind}for (int it = 0; it < {g.ITT}; it++) {{", f"{ind}  const int idx = {lane} + 64 * it;", f"{ind}  if (idx < cnt * {g.TRI}) {{"]
    return shell + [self.off("idx", ind + "    ")] + [f"{ind}    {ln}" for ln in body] + [f"{ind}  }}", f"{ind}}}"]

  def newest_in(self):
    TRI = self.g.TRI
    return [f"""      for (int i = lt; i < cnt * {TRI}; i += 64) {{
        const double v_ = Pl[base * {TRI} + i];
        Ps[((T - 1) * n + base) * {TRI} + i] = v_;
{self.off("i", "        ")}
        s_I[o_] = v_;
      }}"""]

  def request_tile(self):
    g = self.g
    return [f"      double wt[{g.ITT}];      // the tile's packed triangles, requested now, scattered to the lower positions of the images after the scalar phase",
            f"      const double* __restrict__ gpt = Pf + (k * n + base) * {g.TRI};", U,
            f"      for (int it = 0; it < {g.ITT}; it++) {{ const int idx = lb + 64 * it; wt[it] = gpt[idx < cnt * {g.TRI} ? idx : cnt * {g.TRI} - 1]; }}"]

  def land(self, ind):
    """the packed tile requested at A lands in the images (lower positions)"""
    return self.each(ind, "lb", ["s_I[o_] = wt[it];"])

  def identity_step(self):
    """Covariance of the identity-gain step: only lower triangles exist.  Row by row on the block lower triangle: pk = the entry of Pk_k (mirrored inside the
    diagonal block), Pk_n = pk + (Pk1_n - pk) as written -- which IS the carried row of the next step, so nothing is read back.  The rows go to the
    image (lower positions) for the coalesced packed store; every read of another row's entry precedes every write (fence)."""
    g, o = self.g, []
    for s in g.S:
      o += ["        {", f"          double pk_[{g.ncol(s)}];"] + sym_row(g, s, "          ", "pk_", f"rq{s}")
      o += [U, f"          for (int j = 0; j < {g.ncol(s)}; j++) {{ ps{s}[j] -= pk_[j]; ps{s}[j] = pk_[j] + ps{s}[j]; }}      // D = Pk1_n - Pk1_k, then Pk_n = Pk_k + D (Ck = I)",
            "        }", "        __builtin_amdgcn_sched_barrier(0);"]
    o.append("        rn::wave_lds_sync();")
    for s in g.S:
      o += [U, f"        for (int j = 0; j < {g.ncol(s)}; j++) sw{s}[j] = ps{s}[j];"]
    o += ["        rn::wave_lds_sync();", f"        double* __restrict__ gpo = Ps + (k * n + base) * {g.TRI};"]
    return o + self.each("        ", "lo", ["gpo[idx] = s_I[o_];"]) + ["        rn::wave_lds_sync();      // the image is free for the next step's tile"]

  def store_predicted(self):
    g = self.g
    o = [f"          double* __restrict__ po = Ps + ((k + 1) * n + base + gg) * {g.TRI};      // the recomputed Pk1_k leaves as its packed lower triangle (once per tile: predicated stores)"]
    for s in g.S:
      o += [U, f"          for (int j = 0; j < {g.ncol(s)}; j++) {{ if (ok{s} && j <= rr{s}) po[(rr{s} * (rr{s} + 1)) / 2 + j] = a{s}[j]; }}"]
    return o

  def final_decl(self):
    g = self.g
    return [f"      const double* __restrict__ in1 = Pf + (k * n + base) * {g.TRI};", f"      double* __restrict__ out1 = Ps + (k * n + base) * {g.TRI};", f"      double v[{g.ITT}];"]

  def final_request(self):
    g = self.g
    return [U, f"      for (int it = 0; it < {g.ITT}; it++) {{ const int idx = le + 64 * it; v[it] = in1[idx < cnt * {g.TRI} ? idx : cnt * {g.TRI} - 1]; }}"]

  def mirror_u(self):
    return []      # (packed output: only lower positions are read)

  def final_pass(self):
    return self.each("      ", "le", ["const double w_ = v[it] + s_I[o_];", "out1[idx] = w_;", "s_I[o_] = w_;"])


# ---- the phases, in the order of the kernel's text (letters: the module docstring's step list and the kernel's own comments) ----

def head(g):
  """title, what k_rts4_tri shares with the k_rts4 in front of it (macros, scalar phase), signature, LDS, per-launch values"""
  D, E, EE = g.D, g.E, g.EE
  o = [f"// ---- smoother, operands by row_newbcast: {GL} lanes x {g.R} rows per filter, {FPW} filters per wavefront (emit_rts4.py){' -- covariances as packed lower triangles' if g.tri else ''} ----"]
  if g.pf:
    o[0] = o[0][:-5] + " -- a schedule per filter: dts (T, n) in `ts`, ga (T, n) = 1 where the entry stepped its filter; see pf_step_flags() ----"
  if not g.tri and not g.pf:
    o += [MACROS, f"constexpr int RTS4_SLOT = {g.lay.SLOT};", g.scal]
  return o + [f"""
__global__ __launch_bounds__(64, 2) void {g.kname}(const double* __restrict__ xf, const double* __restrict__ Pf, const double* __restrict__ ts,
    const int64_t T, const double* __restrict__ gQ, const int64_t n, const int norm_quats, double* __restrict__ xs,
    double* __restrict__ Ps, const double* __restrict__ xl, const double* __restrict__ Pl{", const unsigned char* __restrict__ ga" if g.pf else ""}) {{
  __shared__ __attribute__((aligned(16))) double s_I[{FPW} * {EE} + 2];          // the one matrix image per filter (see emit_rts4.py)
  __shared__ __attribute__((aligned(16))) double s_sl[{FPW} * RTS4_SLOT];        // x' = f(xk_k), F non-zeros, dt
  __shared__ __attribute__((aligned(16))) double s_xk[{FPW} * {D} + 2];          // xk_k
  __shared__ __attribute__((aligned(16))) double s_xn[{FPW} * {D} + 2];          // xk1_n, then xk_n
  __shared__ __attribute__((aligned(16))) double s_dv[{FPW} * {E} + 2];          // inv_err(xk1_k, xk1_n), then Ck delta
  __shared__ __attribute__((aligned(16))) double s_trash[{E} + 2 * {FPW * (GL - g.RS)} + 2];      // where the idle lanes' row stores go (no predicated regions around LDS stores): overlapping rows, 16 bytes apart
  const int lane = threadIdx.x;
{g.rec.table}  int qoff = 0;
  for (int i = lane; i < {EE}; i += 64) qoff |= (i / {E} != i % {E}) && (gQ[i] != 0.0);
  const bool qdiag = !__any(qoff);      // a diagonal process noise (the usual case): its row entry is requested at the head of every step
  const int64_t tiles = (n + {FPW} - 1) / {FPW};"""]


def tile_prologue(g):
  """the tile's lanes and pointers, T == 1, xk_k of the first step, the carried rows and the newest pair where it is passed in"""
  D, E, EE, RS, S, REC = g.D, g.E, g.EE, g.RS, g.S, g.REC
  pf_single = "" if not g.pf else f"""      // (a filter whose only entry is row 0: its predicted pair where it was passed in)
      if (xl != nullptr) {{ rn::async_wait(); for (int i = lt; i < cnt * {D}; i += 64) {{ if (ga[base + i / {D}]) xs[base * {D} + i] = xl[base * {D} + i]; }} }}
      if (Pl != nullptr) {{ rn::async_wait(); for (int i = lt; i < cnt * {REC}; i += 64) {{ if (ga[base + i / {REC}]) Ps[base * {REC} + i] = Pl[base * {REC} + i]; }} }}
"""
  o = [f"""  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {{
    const int64_t base = tile * {FPW};
    const int cnt = (n - base) < {FPW} ? (int)(n - base) : {FPW};"""]
  o += opaque("    ", ["lt"], ["lane"], note="      // opaque per tile: index arithmetic derived from it is not hoisted to the kernel's entry (where it was ~80 spilled registers)")
  o += [f"""    const int g = lt / {GL};
    const int c = lt % {GL};
    const bool live = g < cnt;
    const int gg = live ? g : 0;
    const bool lead = live && c == 0;
    double* sI = s_I + gg * {EE};
    double* sl = s_sl + gg * RTS4_SLOT;
    double* sxk = s_xk + gg * {D};
    double* sxn = s_xn + gg * {D};
    double* sdv = s_dv + gg * {E};"""] + opaque("    ", ["ct"], ["c"])
  o += [f"    const int rr{s} = ct + {RS * s}; const bool ok{s} = live && ct < {RS} && rr{s} < {E}; const int rc{s} = (ct < {RS} && rr{s} < {E}) ? rr{s} : 0;" for s in S]
  o += [f"""    if (T == 1) {{      // nothing to smooth, the single estimate's predicted pair is not available: the filtered pair passes through
      if (Ps != Pf) {{ for (int i = lt; i < cnt * {REC}; i += 64) Ps[base * {REC} + i] = Pf[base * {REC} + i]; }}
      if (xs != xf) {{ for (int i = lt; i < cnt * {D}; i += 64) xs[base * {D} + i] = xf[base * {D} + i]; }}
{pf_single}      continue;
    }}
    // xk_k of the first step to process; every later one is committed to LDS by the step before it (nothing read from memory crosses the
    // loop's back edge in registers: hipcc waits for such a value with vmcnt(0) at the loop header -- behind the previous step's stores)
    for (int i = lt; i < cnt * {D}; i += 64) s_xk[i] = xf[((T - 2) * n + base) * {D} + i];
    {g.rows_decl('ps', True)}      // rows of the smoothed covariance of step k + 1 (block lower triangle), carried from step to step; D = Pk1_n - Pk1_k inside a step"""]
  for s in S:
    o += [U, f"    for (int j = 0; j < {g.ncol(s)}; j++) ps{s}[j] = 0.0;"]
  if g.pf:
    return o + [f"""    // rows behind a filter's last entry pass through: the carried state starts as the raw newest row (it leaves with the first step), the newest
    // covariance row is copied where the outputs are separate (every older row leaves as Pk_k + U with U = -0 until the recursion starts)
    for (int i = lt; i < cnt * {D}; i += 64) s_xn[i] = xf[((T - 1) * n + base) * {D} + i];
    if (Ps != Pf) {{ for (int i = lt; i < cnt * {REC}; i += 64) Ps[((T - 1) * n + base) * {REC} + i] = Pf[((T - 1) * n + base) * {REC} + i]; }}
    bool started = false;      // an entry that stepped this lane's filter lies at or behind row k + 1
    rn::wave_lds_sync();"""] + setprio(PRIO[2], "    ")
  o += ["    if (Pl != nullptr) {      // newest smoothed covariance := the predicted one of the last step as passed in (ekf_sym.py:658-659): through the image,",
        "      // like every later step's (lower triangle mirrored), and out to Ps[T - 1]"]
  o += g.rec.newest_in() + ["      rn::wave_lds_sync();"] + lower_rows(g, "ps", rc="rc") + ["      rn::wave_lds_sync();", "    }"]
  return o + ["    double dtc = ts[T - 1] - ts[T - 2];      // the step's time difference, read one step ahead (a scalar load's latency at the head of every step otherwise)"] + setprio(PRIO[2], "    ")


def pf_step_flags(g):
  """k_rts4_pf: what `first` and the identity test of k_rts4 become, per filter -- i.e. per 16-lane row; the compiler keeps such lane predicates as wave
  masks in scalar registers.  Every DPP phase stays outside divergent code (EXEC full): the four rows walk the full path together and differ by selects.
    st     entry k + 1 stepped the filter (act); an entry that did not is no predict: the rows of A and of Pk1_k are those of Pk_k, x' = xk_k
    fresh  st and no entry behind k + 1 stepped it: the recursion starts here from the predicted pair just computed (or x_last / P_last)
    ns     not started: row k + 1 lies behind the filter's last entry.  The carried state is the raw row (it leaves as it came), Ck = I and
           U = -0, so Pk_n = Pk_k + U leaves with the bits of Pk_k
    idn    an identity-gain step: Ck is forced to I, and T = Ck D, U = T Ck^T give U = D exactly (sums of exact zeros)"""
  return [f"""      const bool st = ga[(k + 1) * n + base + gg] != 0;
      const bool fresh = st && !started;
      started = started || st;
      const bool ns = !started;
      const double dt = st ? ts[(k + 1) * n + base + gg] : 0.0;
      const bool idn = !ns && !fresh && (!st{" || dt == 0.0" if g.dt0 else ""});
      const bool eye = idn || ns;"""]


def step_prologue(g):
  """the step's opaque lane and row indices, its store targets, its entries of a diagonal Q"""
  E, RS, S = g.E, g.RS, g.S
  o = ["    for (int64_t k = T - 2; k >= 0; k--) {"] + (pf_step_flags(g) if g.pf else ["      const bool first = (k == T - 2);"])
  o += opaque("      ", ["lb"], ["lt"], note2="         // opaque copy of the lane index: the copies' index arithmetic stays inside the step")
  o += opaque("      ", [f"rq{s}" for s in S], [f"rc{s}" for s in S], note="      // (same for the row indices: hoisted out of the step loop, the LDS addresses they feed were ~150 spilled registers)")
  o.append(f"      double* strash = s_trash + 2 * ((g * {GL - RS} + (ct >= {RS} ? ct - {RS} : ct)) % {max(1, FPW * (GL - RS))});      // (an idle lane's own 16 bytes of every row store: stores of many lanes to ONE address serialise)")
  o += [f"      double* sw{s} = ok{s} ? sI + rq{s} * {E} : strash;      // the lane's row of the image as a store target (idle lanes: a trash row)" for s in S]
  o += [f"      const double qd{s} = gQ[rq{s} * {E + 1}];      // (not kept across steps: four registers of a kernel that has none to spare)" for s in S]
  return o + ["      RN_RTS_STAMP(0);"]


def phase_a(g):
  return (["      // ---- A. filtered pair of step k: Pk_k -> image in one coalesced burst, xk_k -> LDS ----"] + g.rec.request_tile()
          + ([] if g.pf else ["      const double dt = dtc;"]) + ["      rn::wave_lds_sync();", "      RN_RTS_STAMP(1);"])


def identity_step(g):
  """Steps with dt == 0 of a model whose predict(dt = 0) is the identity (FilterSpec.identity_at_dt0: f(x, 0) == x, F(x, 0) == I symbolically, and
  dt Q = 0): the predicted pair of step k IS the filtered one, bit for bit -- what the full path computes there is Pk1_k = sym(Pk_k), A = Pk_k and
  Ck = Pk1_k^-1-solve of itself = I up to the rounding of the factorisation (|Ck - I| <= 2.3e-9 in the reference's own golden, np.linalg.solve).
  With Ck = I (ekf_sym.py:672-686):  xk_n = err(xk_k, inv_err(xk1_k, xk1_n))  -- NOT xk1_n: err o inv_err is not the identity for finite
  rotations --,  Pk_n = Pk_k + (Pk1_n - Pk1_k)  evaluated as written.  No factorisation, no substitutions, no products: the step is one read and
  one write of the covariance.  dt is a scalar of the launch (ts is shared by the batch): the branch is uniform.  The recursion's first step always
  takes the full path (it also produces the newest pair).  Tuning knob rts_dt0 = 0 keeps the full solve on every step."""
  if not g.dt0 or g.pf:      # (k_rts4_pf: one path; a row at an identity step has Ck forced to I inside it)
    return []
  D, E, ind = g.D, g.E, "        "
  o = ["      if (dt == 0.0 && !first) {"] + renormalise(g, ind) + ["        rn::wave_lds_sync();"] + store_xs(g, ind)
  o += [f"        double xnext[{g.XT}];      // filtered state of the next (older) step"] + request_xnext(g, ind, "lo")
  o += [f"""        dtc = k > 0 ? ts[k] - ts[k - 1] : 0.0;
        rn::wave_lds_sync();      // every lane has read xk1_n: the buffer takes xk_n
        if (lead) {{      // xk1_k = f(xk_k, 0) = xk_k [renormalised like the forward pass]; delta = inv_err(xk1_k, xk1_n); xk_n = err(xk_k, delta)
          double xa[{D}], xv[{D}], x1n[{D}], xnew[{D}], delta[{E}];
#pragma unroll
          for (int i = 0; i < {D}; i++) {{ xa[i] = sxk[i]; xv[i] = xa[i]; x1n[i] = sxn[i]; }}
          if (norm_quats & 1) {{{g.quat} }}
          inv_err_fun(xv, x1n, delta);
          err_fun(xa, delta, xnew);
#pragma unroll
          for (int i = 0; i < {D}; i++) sxn[i] = xnew[i];       // xk_n: becomes xk1_n of the next (older) step
        }}"""]
  o += g.rec.land(ind) or ["        rn::async_wait();"]      # (full records: the transfer writes the image itself, only waited for)
  o += ["        rn::wave_lds_sync();      // Pk_k has landed; the lead lanes have read xk_k: the buffer takes the next step's"] + commit_xnext(g, ind, "lo")
  return o + g.rec.identity_step() + ["        RN_RTS_STAMP(10);", "        continue;", "      }"]


def phase_b(g):
  return (["      // ---- B. f(xk_k) [renormalised like the forward pass], non-zeros of Fk: once per filter -> slot ----",
           "      if (lead) scal_predict_s4(sxk, dt, sl, norm_quats & 1);" if not g.pf else
           f"      if (lead) {{ if (st) scal_predict_s4(sxk, dt, sl, norm_quats & 1); else {{ for (int i = 0; i < {g.D}; i++) sl[{g.lay.OFF_X} + i] = sxk[i]; }} }}      // (no predict happened: x' = xk_k)"] + g.rec.land("      ")
          + ["      rn::async_wait();", "      rn::wave_lds_sync();", "      RN_RTS_STAMP(2);"])


def phase_c(g):
  """Both passes of the predict (here and in predicted_covariance) touch only the rows of Fk that have entries off the diagonal; their coefficients
  are read from the slot in GROUPS, the next group requested before the current group's FMAs (read where it is used, every pair of FMAs waited for
  its own LDS round trip: 3.5 us of a 24 us step; all 33 at once cost 66 registers under two row sets)."""
  E, S, Fs = g.E, g.S, g.Fs
  o = ["      {", f"        {g.rows_decl('pf')}      // rows of Pk_k (lower triangle mirrored: the contract of batch_rts, include/rednose_amd_filter.h)"]
  o += lower_rows(g, "pf", ind="        ", full=True)
  o += ["        rn::wave_lds_sync();      // every lane has its rows: the image takes A", "        RN_RTS_STAMP(3);",
        "        // ---- C. rows of A = Pk_k Fk^T (row-local, F's structural zeros cost nothing): the right-hand sides; they wait in the image,",
        "        // whose columns are the rows of Fk Pk_k (P = P^T up to rounding, as in the fused run's predict) ----"]
  for s in S:      # the columns Fk leaves alone first: most of the row set is dead before the sums are formed
    o += [U, f"        for (int j = 0; j < {E}; j++) {{ if (" + (" && ".join(f"j != {jb}" for jb in g.busy) or "true") + f") sw{s}[j] = pf{s}[j]; }}"]
  o.append("        __builtin_amdgcn_sched_barrier(0);")
  sel = (lambda s, j, v: f"st ? ({v}) : pf{s}[{j}]") if g.pf else (lambda s, j, v: v)
  o += grouped(Fs, g.groups, "fp", "        ", lambda j, rt: [f"sw{s}[{j}] = {sel(s, j, sum_terms(rt(cf, f'pf{s}[{kk}]') for kk, cf in Fs.row_nz(j)))};" for s in S])
  return o + ["      }", "      rn::wave_lds_sync();"]


def predicted_covariance(g):
  """rows of Pk1_k = (columns of A) Fk^T + dt Q, one row slot at a time"""
  E, RS, S, Fs, ncol = g.E, g.RS, g.S, g.Fs, g.ncol
  o = [f"      {g.rows_decl('a', True)}      // rows of Pk1_k up to each slot's last row (symmetric: the block lower triangle is all anything reads), then its L D L^T factor (unit lower triangle, reciprocal pivots on the diagonal)"]
  for s in S:
    o += ["      {", f"        double col[{E}];", U, f"        for (int m = 0; m < {E}; m++) col[m] = sI[m * {E} + rq{s}];      // column of A = row of Fk Pk_k"]
    sel = (lambda j, v: f"st ? ({v}) : col[{j}]") if g.pf else (lambda j, v: v)
    o += grouped(Fs, g.groups, f"fq{s}_", "        ", lambda j, rt, s=s, sel=sel: ([f"a{s}[{j}] = {sel(j, sum_terms(rt(cf, f'col[{m}]') for m, cf in Fs.row_nz(j)))};"] if j < ncol(s) else []))
    o += [f"        a{s}[{j}] = col[{j}];" for j in range(ncol(s)) if j not in g.busy] + ["      }"]
  o.append("      if (qdiag) {")
  for s in S:
    o.append(f"        const double dq{s} = dt * qd{s};")
    o += [f"        a{s}[{j}] += (rq{s} == {j} ? dq{s} : 0.0);" for j in range(RS * s, ncol(s))]
  o.append("      } else {")
  for s in S:
    H2 = (ncol(s) + 1) // 2
    o += ["        {", f"          double q[{H2}];"]
    for lo_, hi_ in ((0, H2), (H2, ncol(s))):
      o += [U, f"          for (int j = {lo_}; j < {hi_}; j++) q[j - {lo_}] = gQ[rq{s} * {E} + j];",
            U, f"          for (int j = {lo_}; j < {hi_}; j++) a{s}[j] = fma(dt, q[j - {lo_}], a{s}[j]);"]
    o.append("        }")
  return o + ["      }", "      RN_RTS_STAMP(4);"]


def phase_d_pf(g):
  """k_rts4_pf: the recursion starts per filter (pf_step_flags)"""
  D, E, EE, S = g.D, g.E, g.EE, g.S
  o = [f"""      // ---- D. recursion start of the filters that are `fresh` / difference matrix (the image keeps A) ----
      if (__any(fresh)) {{
        if (live && fresh) {{      // newest estimate := the predicted pair of the filter's last entry (passed in, or recomputed just now): ekf_sym.py:658-659
          const int cf = lb % {GL};
          if (xl != nullptr) {{ for (int i = cf; i < {D}; i += {GL}) sxn[i] = xl[(base + lb / {GL}) * {D} + i]; }}
          else {{ for (int i = cf; i < {D}; i += {GL}) sxn[i] = sl[{g.lay.OFF_X} + i]; }}
        }}
        rn::async_wait();      // row k + 1 left raw with the step before (Pk_k + U, U = -0): that store has landed before this one is issued
        if (Pl == nullptr) {{"""]
  o += g.rec.store_predicted(also=" && fresh") + ["        } else {", f"          double* __restrict__ po = Ps + ((k + 1) * n + base + gg) * {EE};",
                                                   f"          const double* __restrict__ pi = Pl + (base + gg) * {EE};"]
  for s in S:
    o += [U, f"          for (int j = 0; j < {E}; j++) {{ if (ok{s} && fresh) po[rr{s} * {E} + j] = pi[rr{s} * {E} + j]; }}",
          U, f"          for (int j = 0; j < {g.ncol(s)}; j++) {{ if (fresh) ps{s}[j] = pi[{E} * max(rq{s}, j) + min(rq{s}, j)]; }}      // (lower triangle mirrored, like every carried row)"]
  o += ["        }", "      }", "      rn::wave_lds_sync();"]
  o += [ln.replace("if (lead && (norm_quats & 2))", "if (lead && (norm_quats & 2) && started)") for ln in renormalise(g, "      ")] + ["      rn::wave_lds_sync();"]
  o += ["      {"] + store_xs(g, "        ") + ["      }"]
  o += [f"""      // D = Pk1_n - Pk1_k; a fresh row that recomputed its predicted pair has Pk1_n = Pk1_k: D = 0
      const bool dzero = fresh && Pl == nullptr;
      if (lead) inv_err_fun(sl + {g.lay.OFF_X}, sxn, sdv);"""]
  for s in S:
    o += [U, f"      for (int j = 0; j < {g.ncol(s)}; j++) {{ ps{s}[j] = dzero ? 0.0 : fma(-1.0, a{s}[j], ps{s}[j]); rn::pin(ps{s}[j]); }}"]
  return o + ["      RN_RTS_STAMP(5);"]


def phase_d(g):
  if g.pf:
    return phase_d_pf(g)
  D, S = g.D, g.S
  o = [f"""      // ---- D. recursion start / difference matrix (the image keeps A: the substitutions take their right-hand sides from it) ----
      if (first) {{
        // newest estimate := the predicted pair of the last step (passed in, or recomputed just now): ekf_sym.py:658-659
        if (live) {{       // (two loops, not one select between a global and an LDS source: hipcc 7.2 trips over the generic pointer)
          const int cf = lb % {GL};      // (from the step's opaque lane index: addresses formed from c are hoisted to the kernel's entry and held in registers for this one step)
          if (xl != nullptr) {{ for (int i = cf; i < {D}; i += {GL}) sxn[i] = xl[(base + lb / {GL}) * {D} + i]; }}
          else {{ for (int i = cf; i < {D}; i += {GL}) sxn[i] = sl[{g.lay.OFF_X} + i]; }}
        }}
        if (Pl == nullptr) {{      // (a covariance that was passed in went into ps* before the loop)"""]
  o += g.rec.store_predicted() + ["        }", "      }", "      rn::wave_lds_sync();"] + renormalise(g, "      ") + ["      rn::wave_lds_sync();"]
  o += ["      {"] + store_xs(g, "        ") + ["      }"]
  o += [f"""      // D = Pk1_n - Pk1_k as fma(-1, Pk1_k, Pk1_n) -- the subtraction, bit for bit.  When the recursion starts from the predicted pair it has just
      // recomputed, Pk1_n IS Pk1_k: the carried rows are still zero and the weight is 0, so D = 0 without a copy of the row set
      const double dw = (first && Pl == nullptr) ? 0.0 : -1.0;
      // state, first half: delta = inv_err(xk1_k, xk1_n) by the lead lanes (its chain runs under the factorisation of the other wavefront)
      if (lead) inv_err_fun(sl + {g.lay.OFF_X}, sxn, sdv);      // (straight from / to LDS: staged through arrays, the two states were 4 D registers next to two row sets)"""]
  for s in S:
    o += [U, f"      for (int j = 0; j < {g.ncol(s)}; j++) {{ ps{s}[j] = fma(dw, a{s}[j], ps{s}[j]); rn::pin(ps{s}[j]); }}      // D = Pk1_n - Pk1_k, block lower triangle (the product takes D[kk][j] = D[j][kk] from whichever lane holds it).  (pinned: hipcc sinks the subtraction to its first use after the substitutions and keeps BOTH operands -- a copy of Pk1_k beside its factor -- alive until then)"]
  return o + ["      RN_RTS_STAMP(5);"]


def phase_e(g):
  E, S, slot_of, lane_of, last_row = g.E, g.S, g.slot_of, g.lane_of, g.last_row
  o = ["      // ---- E. L D L^T of Pk1_k, right-looking, lower triangle.  Column j: the pivot comes from lane j by row_newbcast, every lane",
       "      // forms its reciprocal (v_rcp_f64 + two Newton steps) and its scaled entries; the trailing update of column m reads the",
       "      // UNSCALED entry (m, j) from lane m's register and multiplies with the lane's own scaled entry.  Column j + 1 is",
       "      // completed first and its pivot's reciprocal chain started before the rest of column j's update is issued. ----"]
  o += settle(g, "a") + ["      double dj_0;", f"      RN4_BC(dj_0, a{slot_of(0)}[0], {lane_of(0)});", "      double id_0 = rn::fast_recip(dj_0);"]
  o += [f"      double l{s}_0 = a{s}[0] * id_0;" for s in S if last_row(s) > 0]
  for j in range(E):
    if j + 1 < E:
      m = j + 1
      o += [f"      RN4_FNMAC(a{s}[{m}], a{slot_of(m)}[{j}], l{s}_{j}, {lane_of(m)});" for s in g.upd_slots(m)]
      o += [f"      double dj_{m};", f"      RN4_BC(dj_{m}, a{slot_of(m)}[{m}], {lane_of(m)});", f"      const double id_{m} = rn::fast_recip(dj_{m});"]
      o += [f"      RN4_FNMAC(a{s}[{m2}], a{slot_of(m2)}[{j}], l{s}_{j}, {lane_of(m2)});" for m2 in range(j + 2, E) for s in g.upd_slots(m2)]
    o += [f"      a{s}[{j}] = (rr{s} == {j}) ? id_{j} : l{s}_{j};" if last_row(s) > j else f"      a{s}[{j}] = id_{j};" for s in S if last_row(s) >= j]
    o += [f"      const double l{s}_{j + 1} = a{s}[{j + 1}] * id_{j + 1};" for s in S if j + 1 < E and last_row(s) > j + 1]
  return o + settle(g, "a") + ["      RN_RTS_STAMP(6);"]


def phase_f(g):
  E, slot_of, lane_of = g.E, g.slot_of, g.lane_of
  o = ["      // ---- F. Ck^T = Pk1_k^-1 M, one row slot at a time (its right-hand side = the lane's row of A, waiting in the image):",
       "      // forward substitution with the unit factor, scaling by the reciprocal pivots, backward substitution, all in axpy form --",
       "      // the factor's entry comes from its owner's register by row_newbcast, 21 .. 1 independent FMAs per pivot. ----"]
  for s in g.S:
    o += ["      {", f"        double y[{E}];", U, f"        for (int j = 0; j < {E}; j++) y[j] = sI[rq{s} * {E} + j];"]
    o += [f"        RN4_FNMAC(y[{i}], a{slot_of(i)}[{m}], y[{m}], {lane_of(i)});" for m in range(E) for i in range(m + 1, E)]
    # y[m] *= 1 / d_m as ONE multiply-add with the reciprocal pivot broadcast by the instruction itself (0 + (1 / d_m) y[m]: the product, bit for bit)
    o += [f"        {{ double t_ = 0.0; RN4_FMAC(t_, a{slot_of(m)}[{m}], y[{m}], {lane_of(m)}); y[{m}] = t_; }}" for m in range(E)]
    o += [f"        RN4_FNMAC(y[{i}], a{slot_of(m)}[{i}], y[{m}], {lane_of(m)});" for m in range(E - 1, 0, -1) for i in range(m - 1, -1, -1)]
    if g.pf:
      o += [U, f"        for (int j = 0; j < {E}; j++) sw{s}[j] = eye ? (rq{s} == j ? 1.0 : 0.0) : y[j];      // row of Ck, the identity's where the filter's step is an identity-gain step", "      }"]
    else:
      o += [U, f"        for (int j = 0; j < {E}; j++) sw{s}[j] = y[j];      // row of Ck (each lane overwrites the row it read; idle lanes: the trash row)", "      }"]
  return o + ["      rn::wave_lds_sync();", "      RN4_SETTLE();      // (the rows of D were pinned where they were formed)"]


def phase_h(g):
  """(the products' priority window opens here: PRIO)"""
  E, S, slot_of, lane_of = g.E, g.S, g.slot_of, g.lane_of
  o = ["      RN_RTS_STAMP(7);"] + setprio(0)
  o += ["      // ---- H. T = Ck D, one row slot at a time: coefficients = the lane's row of Ck, operands = rows of D from their owners ----", f"      {g.rows_decl('t')}",
        "      double " + ", ".join(f"dx{s}" for s in S) + ";      // state, second half: Ck delta (one E-term dot per row), formed while the row of Ck is in registers anyway"]
  for s in S:
    o += ["      {", f"        double ck[{E}];", U, f"        for (int j = 0; j < {E}; j++) ck[j] = sI[rq{s} * {E} + j];", f"        double dxa{s} = 0.0, dxb{s} = 0.0;"]
    for c0_ in range(0, E, 8):      # (delta in pieces of eight: all E at once are 2 E registers next to three row sets)
      c1_ = min(E, c0_ + 8)
      o += ["        {", f"          double de[{c1_ - c0_}];", U, f"          for (int j = {c0_}; j < {c1_}; j++) de[j - {c0_}] = sdv[j];"]
      o += [f"          dx{'ab'[j & 1]}{s} = fma(ck[{j}], de[{j - c0_}], dx{'ab'[j & 1]}{s});" for j in range(c0_, c1_)]
      o += [f"          rn::pin(dxa{s}); rn::pin(dxb{s});", "        }"]
    o += [f"        dx{s} = dxa{s} + dxb{s};", f"        rn::pin(dx{s});",
          "        rn::wave_lds_sync();      // (compiler fence: delta is re-read by the next slot instead of staying in 2 E registers under this slot's product)",
          U, f"        for (int j = 0; j < {E}; j++) t{s}[j] = 0.0;"]
    for kk in range(E):      # (D[kk][j] above the block triangle of row kk: D[j][kk] from row j's lane)
      o += [f"        RN4_FMAC(t{s}[{j}], ps{slot_of(kk)}[{j}], ck[{kk}], {lane_of(kk)});" if j < g.ncol(slot_of(kk)) else
            f"        RN4_FMAC(t{s}[{j}], ps{slot_of(j)}[{kk}], ck[{kk}], {lane_of(j)});" for j in range(E)]
    o.append("      }")
  return o + ["      RN_RTS_STAMP(8);"]


def phase_i(g):
  """(the products' priority window closes behind this phase: PRIO)"""
  E, RS, S = g.E, g.RS, g.S
  o = ["      // ---- I. U = T Ck^T: operands = rows of Ck from their owners' registers.  U is symmetric (D is, up to rounding): a row slot",
       "      // forms the columns up to its last row, the upper-right block is mirrored inside the image ----", f"      {g.rows_decl('ck')}"]
  for s in S:
    o += [U, f"      for (int j = 0; j < {E}; j++) ck{s}[j] = sI[rq{s} * {E} + j];"]
  o.append("      rn::wave_lds_sync();      // every lane has read delta and has its rows of Ck: the buffer takes Ck delta, the image U")
  o += [f"      *(ok{s} ? sdv + rq{s} : strash) = dx{s};" for s in S]
  o += ["      typedef double rts4_d2 __attribute__((ext_vector_type(2)));"] + opaque("      ", ["le"], ["lb"]) + g.rec.final_decl()
  o.append(f"      double xnext[{g.XT}];      // filtered state of the next (older) step")
  # U in column blocks of one slot's rows each, ordered so that row sets die early: a block of columns [RS q, RS q + RS) broadcasts only
  # slot q's rows of Ck.  Last slot first, its own (diagonal) block first: after it slot R - 1's rows of Ck are dead; the last block of
  # all is slot 0's, under which the tile's filtered records for the final read-add-write are requested (below).
  blocks = [(s_, q) for s_ in reversed(S) for q in reversed(range(s_ + 1))]
  for bi, (s, q) in enumerate(blocks):
    c0, c1 = RS * q, min(E, RS * q + RS)
    if bi == len(blocks) - 1:
      # The tile's filtered records for the final read-add-write are requested HERE, in front of the last product block: the other
      # slots' rows of T and of Ck are dead, their registers take the loads, and the HBM / Infinity Cache round trip passes under the
      # block's FMAs instead of being waited for after them.
      o += g.rec.final_request() + request_xnext(g, "      ", "le") + ["      __builtin_amdgcn_sched_barrier(0);"]
    o += ["      {", f"        double u[{c1 - c0}];", U, f"        for (int j = 0; j < {c1 - c0}; j++) u[j] = 0.0;"]
    o += [f"        RN4_FMAC(u[{j - c0}], ck{q}[{kk}], t{s}[{kk}], {g.lane_of(j)});" for kk in range(E) for j in range(c0, c1)]
    o += [U, f"        for (int j = 0; j < {c1 - c0}; j++) sw{s}[{c0} + j] = {'ns ? -0.0 : ' if g.pf else ''}u[j];", "      }", "      __builtin_amdgcn_sched_barrier(0);"]
  return o + ["      rn::wave_lds_sync();", "      RN_RTS_STAMP(9);"] + setprio(PRIO[2])


def phase_j(g):
  D, E = g.D, g.E
  o = ["      // ---- J. Pk_n = Pk_k + U leaves: one coalesced read-add-write over the tile's records; the sum also returns to the image,",
       "      // from which every lane takes its rows of the smoothed covariance for the next (older) step ----"] + g.rec.mirror_u()
  o += [f"""      if (lead) {{      // state update, last part: one lane per filter, while the loads above are in flight
        double xa[{D}], xnew[{D}], delta[{E}];
#pragma unroll
        for (int i = 0; i < {D}; i++) xa[i] = sxk[i];
#pragma unroll
        for (int i = 0; i < {E}; i++) delta[i] = sdv[i];
        err_fun(xa, delta, xnew);
#pragma unroll
        for (int i = 0; i < {D}; i++) sxn[i] = {"ns ? xa[i] : " if g.pf else ""}xnew[i];       // xk_n: becomes xk1_n of the next (older) step
      }}
{"" if g.pf else "      dtc = k > 0 ? ts[k] - ts[k - 1] : 0.0;" + chr(10)}      rn::wave_lds_sync();      // the lead lanes have read xk_k: the buffer takes the next step's"""]
  o += commit_xnext(g, "      ", "le") + g.rec.final_pass() + ["      rn::wave_lds_sync();"]
  o += opaque("      ", [f"rq{s}" for s in g.S], note2="      // (fresh addresses: those of the step's first row read are not worth registers across the step)")
  return o + lower_rows(g, "ps") + ["      rn::wave_lds_sync();      // every lane has its rows: the image is free for the next step's burst", "      RN_RTS_STAMP(10);", "    }"]


def epilogue(g):
  o = []
  if g.pf:
    o = [f"""    if ((xl != nullptr || Pl != nullptr) && __any(live && !started && ga[base + gg] != 0)) {{      // a filter whose only entry is row 0: its predicted pair where it was passed in
      const bool only0 = live && !started && ga[base + gg] != 0;
      if (xl != nullptr && only0) {{ for (int i = c; i < {g.D}; i += {GL}) sxn[i] = xl[(base + gg) * {g.D} + i]; }}
      if (Pl != nullptr) {{
        rn::async_wait();      // row 0 left with the last step: before this store
        double* __restrict__ po = Ps + (base + gg) * {g.EE};
        const double* __restrict__ pi = Pl + (base + gg) * {g.EE};"""]
    for s in g.S:
      o += [U, f"        for (int j = 0; j < {g.E}; j++) {{ if (ok{s} && only0) po[rr{s} * {g.E} + j] = pi[rr{s} * {g.E} + j]; }}"]
    o += ["      }", "      rn::wave_lds_sync();", "    }"]
  o += ["    // ---- the oldest smoothed state goes out un-normalised (ekf_sym.py:665-667 never reaches it); its covariance left above ----", "    {"]
  o += opaque("      ", ["lz"], ["lane"]) + [f"      for (int i = lz; i < cnt * {g.D}; i += 64) xs[base * {g.D} + i] = s_xn[i];", "    }"]
  return o + ["    rn::wave_lds_sync();", "  }", "}"]


def kernel(spec, tri=False, pf=False):
  """tri=True: `k_rts4_tri` -- the same recursion on a trace whose covariances are PACKED lower triangles (row-major, E (E + 1) / 2 doubles:
  what batch_run_tri writes): Pf, Ps and Pl are (.., E (E + 1) / 2) arrays.  The kernel's matrix image stays E x E; a packed element goes to /
  comes from the image's LOWER position (row of a packed index: a byte table in LDS, filled once per launch), which is all the kernel reads
  of a covariance anyway (the contract of batch_rts) -- the upper-right exchange of the identity-gain step and the mirroring of U drop out."""
  g = Geometry(spec, tri, pf)
  phases = (head, tile_prologue, step_prologue, phase_a, identity_step, phase_b, phase_c, predicted_covariance, phase_d, phase_e, phase_f, phase_h, phase_i,
            phase_j, epilogue)
  return "\n".join(ln for phase in phases for ln in phase(g))


def launch_pf():
  """k_rts4_pf (kernel(spec, pf=True)): the smoother with a schedule per filter; `ts` carries dts (T, n)."""
  return f"""  const int64_t tiles = (n + {FPW - 1}) / {FPW};
  hipLaunchKernelGGL(k_rts4_pf, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     xf, Pf, dts, T, Q, n, norm_quats, xs, Ps, x_last, P_last, act);"""


def launch(spec, tri=False):
  return f"""  const int64_t tiles = (n + {FPW - 1}) / {FPW};
  hipLaunchKernelGGL({'k_rts4_tri' if tri else 'k_rts4'}, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     xf, Pf, ts, T, Q, n, norm_quats, xs, Ps, x_last, P_last);"""
