"""Kernel family S ("lane per filter"): the whole filter state lives in one lane's VGPRs.

Used when E is small (kinematic: D=E=2; kinematic6: D=E=6 -> 6 + 36 doubles = 84 VGPRs).  A
wavefront owns 64 consecutive filters: it pulls their x / P / z records out of HBM as one
contiguous, 16-byte-vectorised burst per array, transposes through its private LDS slice so that
lane l ends up holding filter l, runs the fully unrolled predict / update algebra below in
registers, and writes back the same way.  All sparsity of F and H.H_mod is resolved here, at
generation time: structural zeros emit no instruction, unit entries no multiply.

Algebra emitted (reference lines in /root/reference/rednose/templates/ekf_c.c):
  predict :8-33   x' = f(x,dt); F = F(x,dt) at the PRE-propagation state; P' = (F P) F^T + dt Q
                  (MEDIM < EDIM handled as F_full = blockdiag(F_main, I), identical to :23-26)
  update  :37-121 y = z - h(x); He = H(x) H_mod(x); G = He P; Gt = He P^T; S = G He^T + R;
                  optional gate d2 = y^T S^-1 y > thresh => R *= 1e16 (:88-94);
                  K^T = S^-1 Gt via Cholesky (:101 uses fullPivLu; S is SPD);
                  dx = K y; x = err_fun(x, dx);
                  Joseph form (:115) evaluated with its rank-Z structure:
                     B = P - K G            (= I_KH P)
                     C = B He^T             (E x Z)
                     P' = B + (K R - C) K^T (= B I_KH^T + K R K^T)
                  which is the same polynomial in the same inputs -- including the property that the
                  rounding error of B is cancelled to first order by the correction term.

Where things are: predict_regs / update_regs / maha_regs print the algebra on registers.  kernels() strings the library's kernels together:
predict_kernel() for k_predict, then step_kernel() for k_step_{kind}, k_stepc_{kind} (+ checkpoint) and -- through kinds_kernel() -- k_kinds (a kind
per filter).  The step kernels have ONE structure -- the first tile requested at the very top out of the preloaded arguments, Q by LDS-DMA among the
requests, the observation tile last behind a counted wait, the tile loop rotated, x and the residual leaving ahead of P -- and step_kernel() joins it
from the pieces above it: the timeline stamps (_stamp*), the request list (_step_requests, the one source of the requests' text and of the counted
wait's operand), what happens once the tile has landed (_step_landed), the update with its write-back (_step_update per kind, _kinds_update mixed),
the flags (_step_flags) and the signature with its host-order shim (_step_signature).  The smaller pieces (LDS images, TILE_LOOP / FIRST_TILE /
NEXT_TILE, tile copies, pins, the non-finite test) also serve k_predict, k_maha_{kind} and k_run.  kind_cases() is the per-kind `switch` of k_kinds,
k_run, k_run_blk and k_run_blk_tr.  The launch text of the step-granular kernels is emit_common's, bound to this family's TILES and to the preloaded
argument order; launch_run is this family's own.
"""
import functools

import sympy as sp

from rednose_amd.codegen import emit_common, tuning
from rednose_amd.codegen.lower import Block, vector_names
from rednose_amd.codegen.emit_common import SMat, term, sum_terms, innovation_solver, ea_count, NOISE_MODES, TABLE, ENTRY, DIAG
from rednose_amd.codegen.emit_common import ind as _ind

TILES = "(n + 63) >> 6"      # tiles of a launch: 64 filters per wavefront


def predict_regs(spec, sym=False):
  """-> text of `predict_regs(x, P, Q, dt)` operating on registers.

  sym=True emits `predict_regs_sym` for the fused multi-step kernels (k_run*), whose contract is a SYMMETRIC covariance: they read
  (P + P^T) / 2 of the caller's matrix once, when the state enters the registers (include/rednose_amd_filter.h), and from then on only
  the upper triangle is read and formed, mirrored at the end of every function -- register renames the compiler drops wherever the
  lower triangle is not consumed.  kinematic6: 548 -> 446 fp64 instructions per step, 42 -> 56 G steps/s in the blocked run (MI355X,
  same call).  The step-granular kernels keep the full product: they use both halves of P exactly as the reference does
  (ekf_c.c:24)."""
  D, E, M = spec.dim_x, spec.dim_err, spec.dim_main_err
  names = {**vector_names(spec.x_sym, 'x'), spec.dt_sym: 'dt'}
  blk = Block(names, tmp_prefix="pt")
  for i in range(D):
    blk.add(f"xn_{i}", spec.f_sym[i])
  fmtF = lambda i, j: f"F_{i}_{j}"  # noqa: E731
  for i in range(M):
    for j in range(M):
      blk.add(fmtF(i, j), spec.F_sym[i, j])
  stmts, st = blk.lower()
  F = SMat.identity_padded(SMat.from_structure(M, M, st, fmtF), E)

  U = (lambda i, j: f"P[{min(i, j) * E + max(i, j)}]") if sym else (lambda i, j: f"P[{i * E + j}]")      # noqa: E731
  body = list(stmts)
  # T = F P   (rows of F that are a bare unit diagonal alias the row of P)
  T = [[None] * E for _ in range(E)]
  for i in range(E):
    nz = F.row_nz(i)
    if len(nz) == 1 and nz[0][0] == i and nz[0][1][0] == 'one':
      for j in range(E):
        T[i][j] = U(i, j)
      continue
    for j in range(E):
      body.append(f"const double T_{i}_{j} = {sum_terms(term(c, U(k, j)) for k, c in nz)};")
      T[i][j] = f"T_{i}_{j}"
  # P' = T F^T + dt Q
  newP = []
  for i in range(E):
    for j in range(i if sym else 0, E):
      s = sum_terms(term(c, T[i][k]) for k, c in F.row_nz(j))
      newP.append(f"const double Pn_{i}_{j} = {s} + dt*Q[{i * E + j}];")
  body += newP
  for i in range(E):
    for j in range(i if sym else 0, E):
      body.append(f"P[{i * E + j}] = Pn_{i}_{j};")
  if sym:
    body += [f"P[{j * E + i}] = P[{i * E + j}];" for i in range(E) for j in range(i + 1, E)]
  for i in range(D):
    kind, val = st[f"xn_{i}"]
    body.append(f"x[{i}] = xn_{i};" if kind == 'expr' else f"x[{i}] = {float(val)!r};")
  head = (f"__device__ __forceinline__ void predict_regs{'_sym' if sym else ''}(double (&x)[{D}], double (&P)[{E * E}], "
          "const double* Q, const double dt) {")
  return "\n".join([head] + _ind(body) + ["}"]), F


def update_regs(spec, k, sym=False, split=False):
  """-> text of `update_<kind>_regs(x, P, z, R)`; returns the gate flag.  sym=True: `update_<kind>_regs_sym`, see predict_regs.

  split=True (what the step-granular kernels call): `update_<kind>_regs_split(x, P, z, R, mid)` -- the same statements in the same
  order, but x and the residual are assigned where they are final, between the gain and the Joseph form, and `mid()` is called there: the
  kernel sends them on their way while the bulk of the update's arithmetic is still to come."""
  assert not (sym and split)
  D, E, Z = spec.dim_x, spec.dim_err, k.zdim
  names = dict(vector_names(spec.x_sym, 'x'))
  if k.ea_sym is not None:
    names.update(vector_names(k.ea_sym, 'ea'))
  Herr = sp.Matrix(k.H_sym) * sp.Matrix(spec.H_mod_sym)
  blk = Block(names, tmp_prefix="ut")
  for i in range(Z):
    blk.add(f"hx_{i}", k.h_sym[i])
  fmtH = lambda i, j: f"He_{i}_{j}"  # noqa: E731
  for i in range(Z):
    for j in range(E):
      blk.add(fmtH(i, j), Herr[i, j])
  stmts, st = blk.lower()
  He = SMat.from_structure(Z, E, st, fmtH)

  b = list(stmts)
  for i in range(Z):
    kind, val = st[f"hx_{i}"]
    hx = f"hx_{i}" if kind == 'expr' else repr(float(val))
    b.append(f"const double y_{i} = z[{i}] - {hx};")
  # G = He P ; Gt = He P^T   (sym: P = P^T, upper triangle only -- see predict_regs -- and Gt IS G)
  U = (lambda i, j: f"P[{min(i, j) * E + max(i, j)}]") if sym else (lambda i, j: f"P[{i * E + j}]")      # noqa: E731
  for zi in range(Z):
    nz = He.row_nz(zi)
    for j in range(E):
      b.append(f"const double G_{zi}_{j} = {sum_terms(term(c, U(kk, j)) for kk, c in nz)};")
      b.append(f"const double Gt_{zi}_{j} = " + (f"G_{zi}_{j};" if sym else f"{sum_terms(term(c, f'P[{j * E + kk}]') for kk, c in nz)};"))
  # HPHt, S, Cholesky, optional gate
  b.append(f"double HPH[{Z * Z}], Rl[{Z * Z}], S[{Z * Z}], L[{Z * Z}], iL[{Z}];")
  for zi in range(Z):
    for w in range(Z):
      b.append(f"HPH[{zi * Z + w}] = {sum_terms(term(c, f'G_{zi}_{j}') for j, c in He.row_nz(w))};")
  b.append("#pragma unroll")
  b.append(f"for (int i = 0; i < {Z * Z}; i++) {{ Rl[i] = R[i]; S[i] = HPH[i] + Rl[i]; }}")
  factor, gate, solve = innovation_solver(Z, not sym, [f"y_{i}" for i in range(Z)], k.maha_thresh if k.maha_test else None)
  b.append(factor)
  b.append("int gated = 0;")
  b += gate
  # K (E x Z): column j of Gt solved against S
  for j in range(E):
    b.append(f"double k_{j}[{Z}] = {{{', '.join(f'Gt_{zi}_{j}' for zi in range(Z))}}};")
    b.append(solve(f"k_{j}"))
  K = lambda i, zi: f"k_{i}[{zi}]"  # noqa: E731
  for j in range(E):
    b.append(f"const double dx_{j} = " + " + ".join(f"{K(j, zi)}*y_{zi}" for zi in range(Z)) + ";")
  # error injection
  nom, delta = spec.err_eqs[1], spec.err_eqs[2]
  enames = dict(vector_names(nom, 'x'))
  enames.update({(delta, i, 0): f"dx_{i}" for i in range(E)})
  eblk = Block(enames, tmp_prefix="et")
  for i in range(D):
    eblk.add(f"xi_{i}", sp.Matrix(spec.err_eqs[0])[i])
  estmts, est = eblk.lower()
  b += estmts
  final = []
  for i in range(D):
    kind, val = est[f"xi_{i}"]
    final.append(f"x[{i}] = xi_{i};" if kind == 'expr' else f"x[{i}] = {float(val)!r};")
  for i in range(Z):
    final.append(f"z[{i}] = y_{i};")
  if split:      # nothing below reads x, z or y: the model's expressions were all evaluated above
    b += final + ["mid();"]
  # B = P - K G (in place).  sym: B = (I - K He) P is NOT symmetric -- its upper triangle is needed for the result and the
  # columns He touches for C below, all rows of those; an entry below the diagonal starts from its mirror image and lives in the
  # (otherwise unused) lower half of the array until the final mirroring overwrites it.
  hcols = sorted({j for zi in range(Z) for j, _ in He.row_nz(zi)})
  # The rank-Z passes are printed as nested multiply-adds, acc -+ a0 b0 -+ a1 b1 .. = fma(-+a0, b0, fma(-+a1, b1, .. acc)): Z instructions per
  # entry.  Printed as `acc -= a0*b0 + a1*b1 + ..` hipcc contracts the sum (1 multiply + Z - 1 multiply-adds) but does not reassociate it into
  # the accumulator: one more add per entry, 20-25 % of this issue-bound kernel's fp64 instructions (ekf_c.c:105,115: same products, the sum
  # taken in another order).
  def chain(acc, pairs, neg=False):
    out = acc
    for a_, b_ in reversed(list(pairs)):
      out = f"fma({'-' if neg else ''}{a_}, {b_}, {out})"
    return out
  if sym:       # the entries below the diagonal first: they start from upper-triangle values the in-place pass below overwrites
    for i in range(E):
      for j in (c_ for c_ in hcols if c_ < i):
        b.append(f"P[{i * E + j}] = {chain(U(i, j), ((K(i, zi), f'G_{zi}_{j}') for zi in range(Z)), neg=True)};")
  for i in range(E):
    for j in range(i if sym else 0, E):
      b.append(f"P[{i * E + j}] = {chain(f'P[{i * E + j}]', ((K(i, zi), f'G_{zi}_{j}') for zi in range(Z)), neg=True)};")
  # C = B He^T, D = K R - C
  for i in range(E):
    for zi in range(Z):
      c = sum_terms(term(cf, f"P[{i * E + j}]") for j, cf in He.row_nz(zi))
      b.append(f"const double Dm_{i}_{zi} = {chain(f'-({c})', ((K(i, w), f'Rl[{w * Z + zi}]') for w in range(Z)))};")
  for i in range(E):
    for j in range(i if sym else 0, E):
      b.append(f"P[{i * E + j}] = {chain(f'P[{i * E + j}]', ((f'Dm_{i}_{zi}', K(j, zi)) for zi in range(Z)))};")
  if sym:
    b += [f"P[{j * E + i}] = P[{i * E + j}];" for i in range(E) for j in range(i + 1, E)]
  if not split:
    b += final
  b.append("return gated;")
  ea_arg = ", const double* __restrict__ ea" if k.ea_sym is not None else ""
  head = (("template <class Mid>\n" if split else "") +
          f"__device__ __forceinline__ int update_{k.kind}_regs{'_sym' if sym else ('_split' if split else '')}(double (&x)[{D}], double (&P)[{E * E}], "
          f"double (&z)[{Z}], const double (&R)[{Z * Z}]{ea_arg}{', Mid&& mid' if split else ''}) {{")
  return "\n".join([head] + _ind(b) + ["}"]), He


def maha_regs(spec, k):
  """d2 = y^T (He P He^T + R)^-1 y for one observation, state untouched (reference: EKF_sym.maha_test, ekf_sym.py:626-649)."""
  D, E, Z = spec.dim_x, spec.dim_err, k.zdim
  names = dict(vector_names(spec.x_sym, 'x'))
  Herr = sp.Matrix(k.H_sym) * sp.Matrix(spec.H_mod_sym)
  blk = Block(names, tmp_prefix="mt")
  for i in range(Z):
    blk.add(f"hx_{i}", k.h_sym[i])
  fmtH = lambda i, j: f"He_{i}_{j}"  # noqa: E731
  for i in range(Z):
    for j in range(E):
      blk.add(fmtH(i, j), Herr[i, j])
  stmts, st = blk.lower()
  He = SMat.from_structure(Z, E, st, fmtH)
  b = list(stmts)
  b.append(f"double v[{Z}], S[{Z * Z}], L[{Z * Z}], iL[{Z}];")
  for i in range(Z):
    kind, val = st[f"hx_{i}"]
    hx = f"hx_{i}" if kind == 'expr' else repr(float(val))
    b.append(f"v[{i}] = z[{i}] - {hx};")
  for zi in range(Z):
    nz = He.row_nz(zi)
    for j in range(E):
      b.append(f"const double G_{zi}_{j} = {sum_terms(term(c, f'P[{kk * E + j}]') for kk, c in nz)};")
  for zi in range(Z):
    for w in range(Z):
      b.append(f"S[{zi * Z + w}] = {sum_terms(term(c, f'G_{zi}_{j}') for j, c in He.row_nz(w))} + R[{zi * Z + w}];")
  b.append(f"double w[{Z}];")
  b += ["#pragma unroll", f"for (int i = 0; i < {Z}; i++) w[i] = v[i];"]
  b.append(f"rn::ldu_factor<{Z}>(S, L, iL);")
  b.append(f"rn::ldu_forward<{Z}>(L, iL, v);")
  b.append(f"rn::ldu_forward_t<{Z}>(L, iL, w);")
  b.append("return " + " + ".join(f"v[{i}]*w[{i}]*iL[{i}]" for i in range(Z)) + ";")
  head = (f"__device__ __forceinline__ double maha_{k.kind}_regs(const double (&x)[{D}], const double (&P)[{E * E}], "
          f"const double (&z)[{Z}], const double (&R)[{Z * Z}]) {{")
  return "\n".join([head] + _ind(b) + ["}"])


def maha_kernels(spec):
  D, E = spec.dim_x, spec.dim_err
  EE = E * E
  out = []
  for k in spec.kinds:
    Z = k.zdim
    ZZ = Z * Z
    out.append(maha_regs(spec, k))
    out.append(f"""
__global__ __launch_bounds__(64) void k_maha_{k.kind}(const double* __restrict__ gx, const double* __restrict__ gP,
    const double* __restrict__ gz, const double* __restrict__ gR, const int r_per_filter, const int64_t n,
    double* __restrict__ d2) {{
{_lds(x=D, P=EE, z=Z, R=ZZ)}
  const int lane = threadIdx.x;
{TILE_LOOP}
    rn::tile_g2l_async<{D}>(gx + base * {D}, cnt, s_x, lane);
    rn::tile_g2l_async<{EE}>(gP + base * {EE}, cnt, s_P, lane);
    rn::tile_g2l_async<{Z}>(gz + base * {Z}, cnt, s_z, lane);
    if (r_per_filter) rn::tile_g2l_async<{ZZ}>(gR + base * {ZZ}, cnt, s_R, lane);
    rn::async_wait();
    rn::wave_lds_sync();
    double x[{D}], P[{EE}], z[{Z}], R[{ZZ}];
    rn::lds_to_regs<{D}>(s_x, lane, x);
    rn::lds_to_regs<{EE}>(s_P, lane, P);
    rn::lds_to_regs<{Z}>(s_z, lane, z);
    if (r_per_filter) {{
      rn::lds_to_regs<{ZZ}>(s_R, lane, R);
    }} else {{
#pragma unroll
      for (int i = 0; i < {ZZ}; i++) R[i] = gR[i];
    }}
    const double d = maha_{k.kind}_regs(x, P, z, R);
    if (lane < cnt) d2[base + lane] = d;
    rn::wave_lds_sync();
  }}
}}
""")
  return "\n".join(out)


def norm_text(spec):
  """Quaternion renormalisation after predict / update (EKFSym::normalize_quaternions, ekf_sym.cc:69-77,207,213)."""
  quat = "".join(f" rn::normalize_quat<{spec.dim_x}>(x, {q});" for q in spec.quaternion_idxs)
  return f"if (norm_quats) {{{quat} }}" if spec.quaternion_idxs else "(void)norm_quats;"


# ---- pieces of the kernels' text: a tile of 64 filters between HBM, the wavefront's LDS slice and the lanes' registers -------------------------
TILE_LOOP = """  const int64_t tiles = (n + 63) >> 6;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile << 6;
    const int cnt = (n - base) < 64 ? (int)(n - base) : 64;"""
# the rotated loop of the step kernels and k_predict: the first tile is requested in front of `for (;;)`, whose body ends with the next tile's requests
FIRST_TILE = """  const int64_t tiles = (n + 63) >> 6;
  int64_t tile = blockIdx.x;
  if (tile >= tiles) return;
  int64_t base = tile << 6;
  int cnt = (n - base) < 64 ? (int)(n - base) : 64;"""
NEXT_TILE = """    tile += gridDim.x;
    if (tile >= tiles) break;
    base = tile << 6;
    cnt = (n - base) < 64 ? (int)(n - base) : 64;"""


def _lds(flat=False, **doubles):
  """LDS declarations.  s_{name}: the image of a tile, `doubles` per filter in rows padded to an odd count; flat: an array of that many doubles."""
  return "\n".join(f"  __shared__ __attribute__((aligned(16))) double s_{a}[{n if flat else f'64 * {n | 1}'}];" for a, n in doubles.items())


def _tile_in(n, g, s):
  return f"rn::tile_g2l_async<{n}>({g} + base * {n}, cnt, {s}, lane);"


def _tile_out(n, g, s):
  return f"rn::tile_l2g<{n}>({g} + base * {n}, cnt, {s}, lane);"


def _pin(n, reg):
  return f"#pragma unroll\n    for (int i = 0; i < {n}; i++) rn::pin({reg}[i]);"


def _flag_acc(D):
  """The non-finite test on the state: a sum that is not finite fails acc - acc == 0."""
  return f"""double acc = 0.0;
#pragma unroll
      for (int i = 0; i < {D}; i++) acc += x[i];
      if (!(acc - acc == 0.0)) nf = 2;          // non-finite state"""


def kind_cases(spec, suffix, z, R, R_shared=None, extra="", ea_lane=None, ind=8):
  """The `case {kind}: { .. }` blocks of a switch over the model's kinds.  The observation and its covariance are copied into arrays of the kind's
  own size -- zk from `z`[i], Rk from the expression `R` in i (or R(idx) when callable; R_shared(idx): the expression for `!r_per_filter`, idx the
  kind's position in the model) --, fl = update_{kind}{suffix}(x, P, zk, Rk ..) runs, the residual goes back to `z`.  `extra`: text behind the call's arguments.  `ea_lane`:
  the lane's filter within the tile in the (T, n, EA) array of per-step extra arguments; a kind that takes them sets flag 8 without the array."""
  pad = " " * ind
  EAM = max(ea_count(k) for k in spec.kinds)
  cases = []
  R_of = R if callable(R) else (lambda idx: R)      # (k_run_pf: a per-kind table, the expression depends on the kind's position)
  for idx, k in enumerate(spec.kinds):
    Z = k.zdim
    R_k = R_of(idx)
    ea, guard = "", ""
    if k.ea_sym is not None and ea_lane is not None:
      ea = f", gea + ((int64_t)t * n + base + {ea_lane}) * {EAM}"
      guard = f"{pad}  if (gea == nullptr) {{ fl = 8; break; }}\n"
    copy_R = f"#pragma unroll\n{pad}  for (int i = 0; i < {Z * Z}; i++) Rk[i] = {R_k};"
    if R_shared is not None:
      copy_R = f"""{pad}  if (r_per_filter) {{
#pragma unroll
{pad}    for (int i = 0; i < {Z * Z}; i++) Rk[i] = {R_k};
{pad}  }} else {{
#pragma unroll
{pad}    for (int i = 0; i < {Z * Z}; i++) Rk[i] = {R_shared(idx)};
{pad}  }}"""
    cases.append(f"""{pad}case {k.kind}: {{
{guard}{pad}  double zk[{Z}], Rk[{Z * Z}];
#pragma unroll
{pad}  for (int i = 0; i < {Z}; i++) zk[i] = {z}[i];
{copy_R}
{pad}  fl = update_{k.kind}{suffix}(x, P, zk, Rk{ea}{extra});
#pragma unroll
{pad}  for (int i = 0; i < {Z}; i++) {z}[i] = zk[i];
{pad}  break;
{pad}}}""")
  return "\n".join(cases)


def kernels(spec):
  """Device functions + __global__ kernels of family S for every kind."""
  tline = bool(tuning.current().small_timeline)
  E = spec.dim_err
  EE = E * E
  out = []
  for sym in (False, True):          # full products (and the split update) for the step-granular kernels, symmetric arithmetic for the fused runs
    ptxt, _ = predict_regs(spec, sym)
    out.append(ptxt)
    for k in spec.kinds:
      utxt, _ = update_regs(spec, k, sym, split=not sym)
      out.append(utxt)
  out.append(f"""
// the fused multi-step kernels read (P + P^T) / 2 of the caller's covariance, once, as the state enters the registers
__device__ __forceinline__ void symmetrize_regs(double (&P)[{EE}]) {{
#pragma unroll
  for (int i = 0; i < {E}; i++) {{
#pragma unroll
    for (int j = i + 1; j < {E}; j++) {{ P[i * {E} + j] = 0.5 * (P[i * {E} + j] + P[j * {E} + i]); P[j * {E} + i] = P[i * {E} + j]; }}
  }}
}}
""")
  # (wait_but_tile is emitted although no kernel calls it: taking its two lines out changes every library's text and digest, a change of its own)
  out.append("""
// What the step kernels use of the runtime beyond the tile copies: the counted waits, the per-filter dt and the shared Q as LDS-DMA transfers
// (templates/ekf_hip_rt.h), and the point the instruction scheduler moves nothing across.  A host build of this text (the kernels run lane by
// lane as threads, every copy synchronous) has nothing to wait for and nothing to hold.
#ifdef __HIP__
template <int EPF> __device__ __forceinline__ void wait_but_tile(int cnt) { rn::async_wait_but_tile<EPF>(cnt); }
template <int N> __device__ __forceinline__ void wait_but_loads(int cnt) { rn::async_wait_but_loads<N>(cnt); }
__device__ __forceinline__ void lane_dt_request(const double* g_lane, double* lds, int lane) { (void)lane; rn::lane_double_g2l_async(g_lane, lds); }
__device__ __forceinline__ double lane_dt(const double* lds, int lane) { return rn::lane_double_from_lds(lds, lane); }
template <int ND> __device__ __forceinline__ void shared_request(const double* g, double* lds, int lane) { rn::doubles_g2l_async<ND>(g, lds, lane); }
__device__ __forceinline__ void hold_order() { __builtin_amdgcn_sched_barrier(0); }
#else
template <int EPF> inline void wait_but_tile(int) {}
template <int N> inline void wait_but_loads(int) {}
inline void lane_dt_request(const double* g_lane, double* lds, int lane) { lds[lane] = *g_lane; }
inline double lane_dt(const double* lds, int lane) { return lds[lane]; }
template <int ND> inline void shared_request(const double* g, double* lds, int lane) { for (int i = lane; i < ND; i += 64) lds[i] = g[i]; }
inline void hold_order() {}
#endif
""")
  norm = norm_text(spec)
  if tline:
    out.append("__device__ unsigned long long g_tl[256 * 8 * 2];      // debug timeline (tuning knob small_timeline)")
  out.append(predict_kernel(spec, norm))
  # k_stepc_{kind}: the same kernel writing a CHECKPOINT on its way -- the observations as they came (cz) and the filtered pair (cx, cP): what the
  # orchestrators' rewind rings keep of every call (ekf_sym.cc:142-156, 191).  A kernel of its own, so that k_step_{kind} stays as it is.
  out += [step_kernel(spec, norm, k, ckpt, tline) for k in spec.kinds for ckpt in (False, True)]
  from rednose_amd.codegen import emit      # (emit imports this module: see its docstring)
  if emit.step_kinds(spec):
    out.append(kinds_kernel(spec, norm))
  if run_block(spec) > 0:          # blocked fused runs: k_run_blk (no trace) and k_run_blk_tr (filtered trace)
    out.append(run_kernel_blk(spec, norm))
    out.append(run_kernel_blk(spec, norm, trace=True))
  else:                            # fallback "no_run_blk" (the blocked kernels spilled): the step-at-a-time k_run serves both
    out.append(run_kernel(spec, norm))
  # the fused run with a schedule per filter, R per kind, per entry, its variances per entry: k_run_pf, k_run_rpf, k_run_dpf (no trace) and
  # their `_tr` (filtered trace)
  out += [run_pf_kernel(spec, norm, trace, noise) for noise in NOISE_MODES if emit.has_run_pf(spec, noise) for trace in (False, True)]
  return "\n".join(out)


# ---- pieces of the step kernels (k_step_{kind}, k_stepc_{kind}, k_kinds), joined by step_kernel() ---------------------------------------------
def _stamp(tline, i, pad="    "):
  """Stamp i of the debug timeline (tuning knob small_timeline; tools/timeline.py small): shader cycles and the 100 MHz wall clock, in scalar registers."""
  return f"\n{pad}if (tl_on) {{ tl_c[{i}] = __builtin_readcyclecounter(); tl_w[{i}] = wall_clock64(); }}" if tline else ""


def _stamp_decl(tline):
  """The stamps' registers and the entry stamp, in front of the first tile's requests: outside the rotated loop, so only a workgroup's first tile is stamped."""
  return f"""
  bool tl_on = blockIdx.x < 256;
  unsigned long long tl_c[7] = {{0, 0, 0, 0, 0, 0, 0}}, tl_w[7] = {{0, 0, 0, 0, 0, 0, 0}};{_stamp(tline, 0, "  ")}""" if tline else ""


def _stamp_out(tline):
  """The last stamp, and lane 0 storing all seven when the tile is done (no store is in flight while a phase is timed)."""
  return f"""{_stamp(tline, 6)}
    if (tl_on && lane == 0) {{
#pragma unroll
      for (int i = 0; i < 7; i++) {{ g_tl[(blockIdx.x * 8 + i) * 2] = tl_c[i]; g_tl[(blockIdx.x * 8 + i) * 2 + 1] = tl_w[i]; }}
    }}
    tl_on = false;""" if tline else ""


def _loads(epf):
  """global_load_lds instructions of tile_g2l_async<epf> on a full tile (rn::tile_async_loads)."""
  return (32 * epf + 63) // 64


def _step_requests(D, EE, Z, ZZ, mixed):
  """The requests of a tile in issue order: [(text, transfers it issues on a full tile, first tile only, read by the predict or before it)].

  This one list makes both the requests' text (_requests_text) and the operand of the counted wait (_in_flight): vmcnt retires in issue order, so
  what may stay in flight under the predict is what stands behind the last request the predict reads -- the observation tile.  It goes last because
  the update is the first to read it, after 42 LDS reads and the whole predict; in a stream it is also the slowest tile (a buffer nothing has touched
  since it was written: HBM, while x and P were written by the previous launch and sit in the L2 / Infinity Cache).  The mask and the kinds are
  ordinary loads in front of it.  (hipcc may move an ordinary load; whichever way it moves, no fewer transfers than counted are issued behind the
  predict's last operand, so the wait can only be stronger than written, never weaker.)  A ragged tile goes through registers and waits for
  everything, Q included.  Q comes by LDS-DMA into s_Q, once; a shared R is an ordinary load, once as well."""
  lane_c = "base + (lane < cnt ? lane : cnt - 1)"      # clamped inside a ragged tile
  shared_R = "" if mixed else f"""// a shared R: ordinary loads, once (it does not change from tile to tile), first used by the update
  double R[{ZZ}];
  if (!r_per_filter) {{
#pragma unroll
    for (int i = 0; i < {ZZ}; i++) R[i] = gR[i];
  }}"""
  return [(_tile_in(D, "gx", "s_x"), _loads(D), False, True), (_tile_in(EE, "gP", "s_P"), _loads(EE), False, True),
          ("if (r_per_filter) " + _tile_in(ZZ, "gR", "s_R"), _loads(ZZ), False, True),
          (shared_R, 0, True, True),
          (f"if (DO_PREDICT) shared_request<{EE}>(gQ, s_Q, lane);", (2 * EE + 63) // 64, True, True),
          ("hold_order();      // the arguments beyond the preloaded ones are first used below: their wait stands behind the requests above", 0, False, True),
          # the per-filter dt rides with the tiles (LDS-DMA: a lane without a filter stores nothing)
          (f"if (DO_PREDICT && gdt != nullptr) lane_dt_request(gdt + {lane_c}, s_dt, lane);", 2, False, True),
          (f"if (active != nullptr) act = active[{lane_c}];", 0, False, True)] + ([(f"kind = gkinds[{lane_c}];", 0, False, True)] if mixed else []) + [
          (_tile_in(Z, "gz", "s_z"), _loads(Z), False, False), ("hold_order();", 0, False, False)]


def _requests_text(reqs, first, pad, tline):
  """The requests of the first tile (in front of the loop) or of a later one (at the end of the loop's body), and the stamp behind them."""
  return ("\n" + pad).join(text for text, _, first_only, _ in reqs if text and (first or not first_only)) + _stamp(tline, 1)


def _in_flight(reqs):
  """The operand of the counted wait: the transfers issued behind the last request the predict reads."""
  last_needed = max(i for i, r in enumerate(reqs) if r[3])
  return sum(r[1] for r in reqs[last_needed + 1:])


def _step_landed(D, EE, Z, ZZ, mixed, norm, ckpt, tline):
  """Behind the counted wait: x, P and dt from LDS to registers, the predict, pins that end its arithmetic there, the wait for the observation tile."""
  pin_note = "" if mixed else "\n    // (the predict's arithmetic ends here: without the pins hipcc sinks it below the wait, into the update's)"
  cz_store = f"\n    {_tile_out(Z, 'cz', 's_z')}      // the observations, before the residuals take their place" if ckpt else ""
  return f"""
    rn::wave_lds_sync();{_stamp(tline, 2)}
    double x[{D}], P[{EE}], z[{Z}]{f', Rf[{ZZ}]' if mixed else ''};
    const double dt = (DO_PREDICT && gdt != nullptr) ? lane_dt(s_dt, lane) : dt_scalar;
    rn::lds_to_regs<{D}>(s_x, lane, x);
    rn::lds_to_regs<{EE}>(s_P, lane, P);
    if (DO_PREDICT) {{
      predict_regs(x, P, s_Q, dt);
      {norm}
    }}{pin_note}
{_pin(D, "x")}
{_pin(EE, "P")}{_stamp(tline, 4)}
    rn::async_wait();
    rn::wave_lds_sync();{_stamp(tline, 3)}{cz_store}
    rn::lds_to_regs<{Z}>(s_z, lane, z);
    if (r_per_filter) rn::lds_to_regs<{ZZ}>(s_R, lane, {'Rf' if mixed else 'R'});"""


def _step_update(spec, k, norm, ckpt, tline):
  """Update of kind k and the write-back: x and the residual are final before the Joseph form, the bulk of the update's arithmetic -- they leave
  there (with the checkpoint's x and the non-finite test), P follows alone."""
  D, EE, Z = spec.dim_x, spec.dim_err ** 2, k.zdim
  # extra arguments are per observation, i.e. per filter of the batch: (n, len(ea)) row-major
  ea = f", gea + (base + (lane < cnt ? lane : 0)) * {ea_count(k)}" if k.ea_sym is not None else ""
  cx_store = f"\n      {_tile_out(D, 'cx', 's_x')}" if ckpt else ""
  cP_store = f"\n    {_tile_out(EE, 'cP', 's_P')}" if ckpt else ""
  tl_pin = "\n" + _pin(EE, "P") if tline else ""      # stamped builds: a phase's arithmetic ends at its stamp
  return f"""const bool on = active == nullptr || (lane < cnt && act != 0);
    int nf = 0;
    int fl = update_{k.kind}_regs_split(x, P, z, R{ea}, [&]() {{
      {norm}
      rn::wave_lds_sync();
      if (on) {{
        rn::regs_to_lds<{D}>(s_x, lane, x);
        rn::regs_to_lds<{Z}>(s_z, lane, z);
      }}
      rn::wave_lds_sync();
      {_tile_out(D, "gx", "s_x")}
      {_tile_out(Z, "gz", "s_z")}{cx_store}
      {_flag_acc(D)}
    }});{tl_pin}{_stamp(tline, 5)}
    rn::wave_lds_sync();
    if (on) rn::regs_to_lds<{EE}>(s_P, lane, P);
    rn::wave_lds_sync();
    {_tile_out(EE, "gP", "s_P")}{cP_store}"""


def _kinds_update(spec, norm):
  """Update of k_kinds and the write-back: a per-lane switch over the model's kinds, then x, P and the residual leave together.  A shared R is read
  from the table inside the switch (one load per kind present in the wavefront)."""
  D, EE, Z = spec.dim_x, spec.dim_err ** 2, max(k.zdim for k in spec.kinds)
  cases = kind_cases(spec, "_regs_split", "z", "Rf[i]", R_shared=lambda idx: f"gR[{idx * Z * Z} + i]", extra=", []() {}")
  return f"""const bool live = lane < cnt && act != 0;
    bool on = live;
    int fl = 0, nf = 0;
    if (live) {{
      switch (kind) {{
{cases}
        default: on = false; break;      // not a kind of this model: untouched, flag 8
      }}
    }}
    {norm}
    rn::wave_lds_sync();
    if (on) {{
      rn::regs_to_lds<{D}>(s_x, lane, x);
      rn::regs_to_lds<{EE}>(s_P, lane, P);
      rn::regs_to_lds<{Z}>(s_z, lane, z);
    }}
    rn::wave_lds_sync();
    {_tile_out(D, "gx", "s_x")}
    {_tile_out(EE, "gP", "s_P")}
    {_tile_out(Z, "gz", "s_z")}
    {{
      {_flag_acc(D)}
    }}"""


def _step_flags(mixed, tline):
  """The flags of the tile's filters: what the update and the non-finite test set, or why the filter was left untouched; the stamps behind them."""
  return f"if (flags != nullptr && lane < cnt) flags[base + lane] = (uint8_t)(on ? (fl | nf) : {'(live ? 8 : 16)' if mixed else '16'});{_stamp_out(tline)}"


def _step_signature(kn, mixed, ckpt):
  """Head of kernel `kn`.  gx, gP, gz, n, gQ, gR and `opts` (bit 0: r_per_filter, bit 1: norm_quats) are the first 13 dwords of the kernel arguments,
  which arrive preloaded in SGPRs (rednose_amd/build.py: -amdgpu-kernarg-preload-count): the requests of x, P, a per-filter R and Q wait for no
  s_load.  Host builds of this text (tests/test_emit_host*.py) call the kernels in the argument order of the C ABI: a shim in that order forwards."""
  obs = "const int32_t* __restrict__ gkinds" if mixed else "const double* __restrict__ gea"
  cargs = ", double* __restrict__ cx, double* __restrict__ cP, double* __restrict__ cz" if ckpt else ""
  cnames = ", cx, cP, cz" if ckpt else ""
  return f"""#ifndef __HIP__
template <bool DO_PREDICT> void {kn}(double* gx, double* gP, double* gz, const int64_t n, const double* gQ, const double* gR, const int opts, {obs.replace("__restrict__ ", "")}, const double* gdt, const double dt_scalar, uint8_t* flags, const uint8_t* active{cargs.replace("__restrict__ ", "")});
template <bool DO_PREDICT> inline void {kn}(double* gx, double* gP, double* gz, const double* gR, const int r_per_filter, {obs.replace("__restrict__ ", "")}, const double* gQ, const double* gdt, const double dt_scalar, const int64_t n, const int norm_quats, uint8_t* flags, const uint8_t* active{cargs.replace("__restrict__ ", "")}) {{ {kn}<DO_PREDICT>(gx, gP, gz, n, gQ, gR, (r_per_filter != 0 ? 1 : 0) | (norm_quats != 0 ? 2 : 0), {'gkinds' if mixed else 'gea'}, gdt, dt_scalar, flags, active{cnames}); }}
#endif
template <bool DO_PREDICT>
__global__ __launch_bounds__(64) void {kn}(double* __restrict__ gx, double* __restrict__ gP, double* __restrict__ gz, const int64_t n,
    const double* __restrict__ gQ, const double* __restrict__ gR, const int opts, {obs},
    const double* __restrict__ gdt, const double dt_scalar, uint8_t* __restrict__ flags, const uint8_t* __restrict__ active{cargs}) {{"""


def step_kernel(spec, norm, k, ckpt=False, tline=False):
  """The step kernels, [predict +] update with the state round-tripping HBM once per launch: k_step_{kind} of kind k, k_stepc_{kind} (ckpt: the same
  writing the call's checkpoint), and with k = None k_kinds (see kinds_kernel).  tline: the stamped build of the tuning knob small_timeline.

  Nothing stands in front of the first tile's requests: what they need is in the preloaded arguments (_step_signature), the other arguments are
  loaded at the top as before and their wait stands behind those requests, in front of the per-filter dt, the mask, the kinds.  The tile loop is
  rotated: the first tile is requested outside it, its body is wait, compute, store, request the next tile.  hipcc cannot hoist the loop's
  invariants (the addresses of the write-back, the lane masks of the ragged copies) in front of requests that stand outside the loop, and
  hold_order() keeps its scheduler from moving anything across the end of the requests."""
  mixed = k is None
  D, EE = spec.dim_x, spec.dim_err ** 2
  Z = max(kk.zdim for kk in spec.kinds) if mixed else k.zdim
  kn = "k_kinds" if mixed else (f"k_stepc_{k.kind}" if ckpt else f"k_step_{k.kind}")
  title = ("// ---- a kind per filter: [predict +] update of kinds[i], state round-trips HBM once per launch whatever the mix of kinds ------------" if mixed else
           f"// ---- kind {k.kind}: [predict +] update{' + checkpoint' if ckpt else ''}, state round-trips HBM once per launch --------------------------")
  mask_note = ("// a filter that is masked out, or whose kind the model does not have, is not written back (flags 16 / 8)" if mixed else
               "// masked-out filters (active[i] == 0) pass through untouched: x, P and z leave as they came, flag bit 4 is set")
  reqs = _step_requests(D, EE, Z, Z * Z, mixed)
  update = _kinds_update(spec, norm) if mixed else _step_update(spec, k, norm, ckpt, tline)
  kind_decl = "\n  int kind = 0;" if mixed else ""
  return f"""
{title}
{_step_signature(kn, mixed, ckpt)}
{_lds(x=D, P=EE, z=Z, R=Z * Z)}
{_lds(True, Q=EE, dt=64)}
  const int lane = threadIdx.x;
  const int r_per_filter = opts & 1, norm_quats = opts & 2;
{FIRST_TILE}{_stamp_decl(tline)}
  uint8_t act = 1;{kind_decl}
  {_requests_text(reqs, True, "  ", tline)}
  for (;;) {{
    {mask_note}
    wait_but_loads<{_in_flight(reqs)}>(cnt);{_step_landed(D, EE, Z, Z * Z, mixed, norm, ckpt, tline)}
    {update}
    {_step_flags(mixed, tline)}
    rn::wave_lds_sync();
{NEXT_TILE}
    {_requests_text(reqs, False, "    ", tline)}
  }}
}}
"""


def kinds_kernel(spec, norm):
  """k_kinds: the step kernel in which every filter brings its own observation kind (kinds[i]).  The tile is loaded once -- z rows and per-filter
  R at the strides of the fused run, zmax and zmax^2 --, predicted once, and a per-lane switch over the model's kinds calls update_{k}_regs_split:
  a wavefront pays the sum of the kinds present among its 64 filters in arithmetic, and one trip through HBM.  A filter that is masked out, or
  whose kind the model does not have, is not written back (flags 16 / 8): its lane leaves the LDS image as it was loaded.
  s_R is allocated whether or not R comes per filter.  The kernel has no stamped build.  It is covered by tests; its time has not been measured."""
  return step_kernel(spec, norm, None)


def predict_kernel(spec, norm):
  """k_predict, with the step kernels' prologue (see step_kernel): its arguments but the mask are all within the preloaded ones as they stand."""
  D, E = spec.dim_x, spec.dim_err
  EE = E * E
  dt = "dt = (gdt != nullptr && lane < cnt) ? gdt[base + lane] : dt_scalar;"
  return f"""
// ---- predict only: one launch propagates n filters by dt -------------------------------------------
__global__ __launch_bounds__(64) void k_predict(double* __restrict__ gx, double* __restrict__ gP,
    const double* __restrict__ gQ, const double* __restrict__ gdt, const double dt_scalar, const int64_t n,
    const int norm_quats, const uint8_t* __restrict__ active) {{
{_lds(x=D, P=EE)}
{_lds(True, Q=EE)}
  const int lane = threadIdx.x;
{FIRST_TILE}
  {_tile_in(D, "gx", "s_x")}
  {_tile_in(EE, "gP", "s_P")}
  shared_request<{EE}>(gQ, s_Q, lane);       // Q as LDS broadcast operands (36 SGPR pairs spilled otherwise), requested with the first tile
  double {dt}
  hold_order();
  for (;;) {{
    rn::async_wait();
    rn::wave_lds_sync();
    double x[{D}], P[{EE}];
    rn::lds_to_regs<{D}>(s_x, lane, x);
    rn::lds_to_regs<{EE}>(s_P, lane, P);
    predict_regs(x, P, s_Q, dt);
    {norm}
    rn::wave_lds_sync();
    // a masked-out filter (active[i] == 0: no observation for it in this call) keeps the record it came with: its lane
    // does not overwrite the LDS image, so the coalesced write-back returns the loaded bytes
    if (active == nullptr || (lane < cnt && active[base + lane] != 0)) {{
      rn::regs_to_lds<{D}>(s_x, lane, x);
      rn::regs_to_lds<{EE}>(s_P, lane, P);
    }}
    rn::wave_lds_sync();
    {_tile_out(D, "gx", "s_x")}
    {_tile_out(EE, "gP", "s_P")}
    rn::wave_lds_sync();
{NEXT_TILE}
    {_tile_in(D, "gx", "s_x")}
    {_tile_in(EE, "gP", "s_P")}
    {dt}
    hold_order();
  }}
}}
"""


# the step kernels take their arguments in the preloaded order (_step_signature)
launch_step, launch_step_ckpt, launch_kinds = (functools.partial(f, TILES, head=1) for f in (
  emit_common.launch_step, emit_common.launch_step_ckpt, emit_common.launch_kinds))
launch_predict = functools.partial(emit_common.launch_predict, TILES)
launch_maha = functools.partial(emit_common.launch_maha, TILES, ea=False)      # this family's k_maha_{kind} has no extra-argument parameter


def run_unroll(spec):
  """Steps of the schedule per iteration of the traced fused run's loop (= depth of its observation prefetch ring)."""
  zmax = max(k.zdim for k in spec.kinds)
  return 8 if zmax <= 2 else 4          # observation rows in flight per wavefront (zmax doubles of staging registers per lane each)


def run_block(spec):
  """Steps per block of the untraced fused run (k_run_blk): observation rows of one block are in flight while the previous block is
  computed, so a block has to outlast one HBM round trip (~2 us); a step of the 2-state model takes ~0.1 us, of a 6-state model
  ~1 us.  Bounded by the staging registers (2 x K x zmax doubles per lane) and the code size (the K steps are unrolled)."""
  from rednose_amd.codegen import emit      # (emit imports this module: see its docstring)
  forced = -1 if "no_run_blk" in emit._active else tuning.current().run_block      # pylint: disable=protected-access
  if forced:
    return max(0, forced)
  zmax = max(k.zdim for k in spec.kinds)
  # measured (tools/ab_run.cpp, 65 536 filters, one wavefront per SIMD): 2-state model 8 / 16 / 32 / 64 steps per block ->
  # 322 / 331 / 273 / 233 G steps/s (the traced kernel's structure: 138); 6-state model 2 / 4 / 8 -> 42.1 / 40.5 / 42.2 (31.5)
  K = 16 if spec.dim_err <= 2 else 8
  while K > 2 and (K * zmax > 32 or K * len(spec.kinds) > 16):      # staging registers; code size (K steps x every kind, unrolled)
    K //= 2
  return K


def run_kernel(spec, norm):
  """T steps per launch: x and P stay in VGPRs, only z (in) / y (out) and the optional trace touch HBM."""
  D, E = spec.dim_x, spec.dim_err
  EE = E * E
  zmax = max(k.zdim for k in spec.kinds)
  KP = run_unroll(spec)
  cases = kind_cases(spec, "_regs_sym", "z", f"gR[t * {zmax * zmax} + i]", ea_lane="(lane < cnt ? lane : 0)")
  return f"""
// ---- fused multi-step run: kinds[t], dts[t] shared by all filters; z is (T, n, {zmax}) in: z, out: y -----------
__global__ __launch_bounds__(64) void k_run(double* __restrict__ gx, double* __restrict__ gP, const double* __restrict__ gQ,
    const int32_t* __restrict__ kinds, const double* __restrict__ dts, const int64_t T, double* __restrict__ gz,
    const double* __restrict__ gR, const int64_t n, const int norm_quats, uint8_t* __restrict__ flags,
    double* __restrict__ tx, double* __restrict__ tP, const double* __restrict__ gea, const int32_t* __restrict__ augs) {{
  (void)gea; (void)augs;      // lane-per-filter models are never MSCKF models (those use the lane-group family): no window shift here
{_lds(x=D, P=EE, z=zmax)}
{_lds(True, Q=EE)}
  const int lane = threadIdx.x;
  for (int i = lane; i < {EE}; i += 64) s_Q[i] = gQ[i];
{TILE_LOOP}
    rn::tile_g2l<{D}>(gx + base * {D}, cnt, s_x, lane);
    rn::tile_g2l<{EE}>(gP + base * {EE}, cnt, s_P, lane);
    rn::tile_g2l<{zmax}>(gz + base * {zmax}, cnt, s_z, lane);
    rn::wave_lds_sync();
    double x[{D}], P[{EE}], z[{zmax}];
    rn::lds_to_regs<{D}>(s_x, lane, x);
    rn::lds_to_regs<{EE}>(s_P, lane, P);
    symmetrize_regs(P);
    // Observation prefetch, {KP} steps deep: a step of a small model takes a fraction of a microsecond, less than one HBM round
    // trip, so with the next step's row alone in flight every step waited for its observation (r3a counters of the 2-state
    // model: 59 % of the wave cycles in s_waitcnt, 13 % issuing).  ring[j] carries the row of the step t = j (mod {KP}); the
    // step loop is unrolled {KP} times so that the ring index is a compile-time constant (a runtime index would put the staging
    // registers into scratch memory).  Loads are issued unconditionally on a clamped row (see TilePrefetch).
    rn::TilePrefetch<{zmax}> ring[{KP}];
#pragma unroll
    for (int u = 1; u < {KP}; u++) ring[u].issue(gz + ((u < T ? u : T - 1) * n + base) * {zmax}, cnt, lane);
    for (int64_t tb = 0; tb < T; tb += {KP}) {{
#pragma unroll
    for (int u = 0; u < {KP}; u++) {{
      const int64_t t = tb + u;
      if (t < T) {{
      rn::lds_to_regs<{zmax}>(s_z, lane, z);
      rn::wave_lds_sync();
      ring[u].issue(gz + ((t + {KP} < T ? t + {KP} : T - 1) * n + base) * {zmax}, cnt, lane);
      const int kind = kinds[t];
      const double dt = dts[t];
      predict_regs_sym(x, P, s_Q, dt);
      {norm}
      int fl = 0;
      switch (kind) {{
{cases}
        default: fl = 8; break;      // kind not available in the fused run (unknown, or it takes extra arguments)
      }}
      {norm}
      // y(t) and the optional trace go out through LDS as coalesced 16-byte stores
      rn::regs_to_lds<{zmax}>(s_z, lane, z);
      if (tx != nullptr) rn::regs_to_lds<{D}>(s_x, lane, x);
      if (tP != nullptr) rn::regs_to_lds<{EE}>(s_P, lane, P);
      rn::wave_lds_sync();
      rn::tile_l2g<{zmax}>(gz + (t * n + base) * {zmax}, cnt, s_z, lane);
      if (tx != nullptr) rn::tile_l2g<{D}>(tx + (t * n + base) * {D}, cnt, s_x, lane);
      if (tP != nullptr) rn::tile_l2g<{EE}>(tP + (t * n + base) * {EE}, cnt, s_P, lane);
      if (flags != nullptr && lane < cnt) flags[t * n + base + lane] = (uint8_t)fl;
      rn::wave_lds_sync();
      if (t + 1 < T) ring[(u + 1) % {KP}].commit(s_z, cnt, lane);
      rn::wave_lds_sync();
      }}
    }}
    }}
    rn::regs_to_lds<{D}>(s_x, lane, x);
    rn::regs_to_lds<{EE}>(s_P, lane, P);
    rn::wave_lds_sync();
    rn::tile_l2g<{D}>(gx + base * {D}, cnt, s_x, lane);
    rn::tile_l2g<{EE}>(gP + base * {EE}, cnt, s_P, lane);
    rn::wave_lds_sync();
  }}
}}
"""


def _blocked_run(spec, norm, trace, K, *, kname, title, ragged_note, step, trace_note, helpers="", args="", unused="", lds=None, fill="",
                 sched_ptrs="", decl_d="", decl_i="", decl_more="", issue_sched="", issue_ptrs="", issue_row="", issue_step="",
                 pin_row="", pin_block="", rot_row="", rot_block="", reload_note="", wb_guard=""):
  """The text of a blocked fused run, once: kernel head, LDS, tile prologue, the block loop (everything in flight lands, the previous block's y
  and flags leave, the registers rotate, the next block is requested, K steps run), the last block's tail and the write-back.  The keyword
  arguments are the fragments in which the kernels of a shared schedule (run_kernel_blk) and of a schedule per filter (run_pf_kernel) differ:
  names, arguments and LDS tables, the schedule's registers with their part of `issue`, of the pins and of the rotation (`_row`: per step
  of the block, `_block`: once per block), the body of a step, and the reload and guard of the write-back."""
  D, E = spec.dim_x, spec.dim_err
  EE = E * E
  zmax = max(k.zdim for k in spec.kinds)
  load_img = f"""    rn::tile_g2l<{D}>(gx + base * {D}, cnt, s_x, lane);
    rn::tile_g2l<{EE}>(gP + base * {EE}, cnt, s_P, lane);
    rn::wave_lds_sync();"""

  def to_lds(pad):
    return f"{pad}rn::regs_to_lds<{D}>(s_x, lane, x);\n{pad}rn::regs_to_lds<{EE}>(s_P, lane, P);"
  # rows are addressed by pointer increments (one 64-bit multiply per block, none per row): a row past the end of the schedule
  # re-reads row T - 1 (the increment is zero there), so the loads stay unconditional
  issue = f"""{{
      const int64_t tb0_ = TB_ < T ? TB_ : T - 1;{issue_sched}
      const double* zp_ = zrow + tb0_ * rowstride;{issue_ptrs}
      const int64_t left_ = T - 1 - tb0_;          // rows of the schedule after row tb0_
#pragma unroll
      for (int u = 0; u < {K}; u++) {{{issue_row}
#pragma unroll
        for (int i = 0; i < {zmax}; i++) nxt[u][i] = zp_[i];
        zp_ += (u < left_) ? rowstride : 0;{issue_step}
      }}
    }}"""
  store = f"""#pragma unroll
          for (int i = 0; i < {zmax}; i++) yp_[i] = cur[u][i];
          if (flags != nullptr) fp_[0] = (uint8_t)flb[u];
          yp_ += rowstride;
          fp_ += n;"""
  targs = ",\n    double* __restrict__ tx, double* __restrict__ tP" if trace else ""
  tstore = f"""
          {trace_note}
{to_lds(" " * 10)}
          rn::wave_lds_sync();
          if (tx != nullptr) rn::tile_l2g<{D}>(tx + (t * n + base) * {D}, cnt, s_x, lane);
          if (tP != nullptr) rn::tile_l2g<{EE}>(tP + (t * n + base) * {EE}, cnt, s_P, lane);
          rn::wave_lds_sync();""" if trace else ""
  reload = f"\n    {reload_note}\n{load_img}" if trace and reload_note else ""
  write_back = f"{wb_guard} {{\n{to_lds(' ' * 6)}\n    }}" if wb_guard else to_lds(" " * 4)
  return f"""{helpers}
{title}
__global__ __launch_bounds__(64) void {kname}(double* __restrict__ gx, double* __restrict__ gP, const double* __restrict__ gQ,
    const int32_t* __restrict__ kinds, const double* __restrict__ dts, const int64_t T, double* gz,
    const double* __restrict__ gR, const int64_t n, const int norm_quats, uint8_t* __restrict__ flags{args}{targs}) {{{unused}
{_lds(x=D, P=EE)}
{_lds(True, Q=EE, **(lds or {}))}
  const int lane = threadIdx.x;
  for (int i = lane; i < {EE}; i += 64) s_Q[i] = gQ[i];{fill}
  const int64_t tiles = (n + 63) >> 6;
  const int64_t rowstride = n * {zmax};               // doubles between the rows of one filter in consecutive steps
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {{
    const int64_t base = tile << 6;
    const int cnt = (n - base) < 64 ? (int)(n - base) : 64;
{load_img}
    double x[{D}], P[{EE}];
    rn::lds_to_regs<{D}>(s_x, lane, x);
    rn::lds_to_regs<{EE}>(s_P, lane, P);
    symmetrize_regs(P);
    {ragged_note}
    const int lc = lane < cnt ? lane : cnt - 1;
    const bool live = lane < cnt;
    double* zrow = gz + (base + lc) * {zmax};{sched_ptrs}
    double cur[{K}][{zmax}], nxt[{K}][{zmax}]{decl_d};
    int flb[{K}]{decl_i};{decl_more}
    {issue.replace("TB_", "((int64_t)0)")}
    for (int64_t tb = 0; tb < T; tb += {K}) {{
      // everything in flight lands: this block's rows and schedule (and the stores issued one block ago)
#pragma unroll
      for (int u = 0; u < {K}; u++) {{
#pragma unroll
        for (int i = 0; i < {zmax}; i++) rn::pin(nxt[u][i]);{pin_row}
      }}{pin_block}
      if (tb > 0 && live) {{
        double* yp_ = zrow + (tb - {K}) * rowstride;
        uint8_t* fp_ = flags + (tb - {K}) * n + base + lane;
#pragma unroll
        for (int u = 0; u < {K}; u++) {{
{store}
        }}
      }}
#pragma unroll
      for (int u = 0; u < {K}; u++) {{
#pragma unroll
        for (int i = 0; i < {zmax}; i++) cur[u][i] = nxt[u][i];{rot_row}
      }}{rot_block}
      {issue.replace("TB_", f"(tb + {K})")}
#pragma unroll
      for (int u = 0; u < {K}; u++) {{
        const int64_t t = tb + u;
        flb[u] = 0;
        if (t < T) {{
{step}
          flb[u] = fl;{tstore}
        }}
      }}
    }}
    if (live) {{
      const int64_t tl = ((T - 1) / {K}) * {K};          // first step of the last block
      double* yp_ = zrow + tl * rowstride;
      uint8_t* fp_ = flags + tl * n + base + lane;
#pragma unroll
      for (int u = 0; u < {K}; u++) {{
        if (tl + u < T) {{
{store}
        }}
      }}
    }}{reload}
{write_back}
    rn::wave_lds_sync();
    rn::tile_l2g<{D}>(gx + base * {D}, cnt, s_x, lane);
    rn::tile_l2g<{EE}>(gP + base * {EE}, cnt, s_P, lane);
    rn::wave_lds_sync();
  }}
}}
"""


def run_kernel_blk(spec, norm, trace=False):
  """The fused run without trace (tx == tP == nullptr), restructured around what the counters of k_run show for small models: the
  arithmetic of a step is tens of fp64 instructions, the step took thousands of cycles, because every step (a) waited for its own
  y store to retire -- vmcnt counts loads and stores in issue order, and the wait for the prefetched observation row behind the
  (conditional) stores degrades to vmcnt(0) --, (b) waited twice for scalar loads (kind / dt, then R), and (c) crossed the LDS
  three times (row in, y out, Q).  Here a wavefront works in blocks of K steps entirely in registers:
    * lane l reads / writes its own filter's observation row directly (zmax doubles per step, contiguous per lane);
    * the K rows of block b + 1, and the block's schedule (dt, kind: lane u of a schedule register holds step u of the block; R: the block's
      K x zmax^2 doubles spread over the lanes; all broadcast with v_readlane when the step runs), are loaded while block b is computed -- ONE vmcnt(0) per block;
    * y (which replaces z in its registers) and the flags of block b are stored at the start of block b + 1, AFTER that wait, so no
      load the wavefront is waiting for ever queues behind a store it has just issued.
  Same arithmetic as k_run (predict_regs / update_*_regs); results agree to the last bits (FMA contraction may differ per kernel).

  trace=True: the same structure writing the filtered trace -- every step's x / P leave through the LDS image as coalesced stores that
  nothing waits for until the next block starts (k_run_blk_tr; the step-at-a-time k_run paid a store wait per step: MI355X, same call,
  8 192 x 200 kinematic6 3.04 -> 3.38 G steps/s, 65 536 x 200 kinematic 59 -> 75 G steps/s, results bit-identical).

  The kernel's text is _blocked_run's; what is here is the shared schedule: fetched by the lanes, a step each, and broadcast when the step runs."""
  ZZ = max(k.zdim for k in spec.kinds) ** 2
  K = run_block(spec)
  NR = (K * ZZ + 63) // 64
  cases = kind_cases(spec, "_regs_sym", "cur[u]", f"lane_bcast(Rv[(u * {ZZ} + i) >> 6], (u * {ZZ} + i) & 63)", ea_lane="lc", ind=10)
  return _blocked_run(
    spec, norm, trace, K, kname="k_run_blk_tr" if trace else "k_run_blk",
    title=(f"// ---- fused multi-step run with the filtered trace: blocks of {K} steps, no store is waited for inside a block -----------------"
           if trace else
           f"// ---- fused multi-step run without trace: blocks of {K} steps in registers (see emit_small.run_kernel_blk) -------------------"),
    helpers="" if trace else """
__device__ __forceinline__ double lane_bcast(const double v, const int l) {      // lane l's value in every lane (l uniform): two v_readlane_b32
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ void pin_i(int& v) { asm volatile("" : "+v"(v)); }
""",
    args=",\n    const double* __restrict__ gea", unused="\n  (void)gea;",
    ragged_note="// lanes past the end of a ragged tile compute on a copy of the last filter's rows and store nothing",
    decl_d=f", Rv[{NR}], Rn[{NR}], dtv, dtn", decl_i=", kv, kn",
    issue_sched=f"""
      const int64_t ts_ = TB_ + (lane < {K} ? lane : {K - 1});
      const int64_t tsc_ = ts_ < T ? ts_ : T - 1;
      dtn = dts[tsc_];
      kn = kinds[tsc_];
#pragma unroll
      for (int r = 0; r < {NR}; r++) {{           // R of the block's steps, flat: lane l of register r holds double r * 64 + l
        const int64_t ri_ = tb0_ * {ZZ} + r * 64 + lane;
        Rn[r] = gR[ri_ < T * {ZZ} ? ri_ : T * {ZZ} - 1];
      }}""",
    pin_block=f"""
      rn::pin(dtn);
      pin_i(kn);
#pragma unroll
      for (int r = 0; r < {NR}; r++) rn::pin(Rn[r]);""",
    rot_block=f"""
      dtv = dtn;
      kv = kn;
#pragma unroll
      for (int r = 0; r < {NR}; r++) Rv[r] = Rn[r];""",
    step=f"""          const double dt = lane_bcast(dtv, u);
          const int kind = __builtin_amdgcn_readlane(kv, u);
          predict_regs_sym(x, P, s_Q, dt);
          {norm}
          int fl = 0;
          switch (kind) {{
{cases}
            default: fl = 8; break;      // kind not available in the fused run (unknown, or it takes extra arguments)
          }}
          {norm}""",
    trace_note="// filtered pair of step t: through the LDS image, coalesced; the stores drain under the following steps")


def run_pf_block(spec):
  """Steps per block of k_run_pf: run_block's, or run_unroll's where the blocked kernels were dropped (fallback no_run_blk)."""
  return run_block(spec) or run_unroll(spec)


def run_pf_r_block(spec):
  """Steps per block of k_run_rpf: run_pf_block's, halved until the rows of R of a block fit the staging registers.  The kernel stages zmax^2 more
  doubles per step and buffer than k_run_pf (2 x K x zmax^2 on top of 2 x K x zmax: attitude at K = 8 would hold 288 VGPRs of R alone); at
  K x zmax^2 <= 36 the rows of R take at most 144 VGPRs of the 512 a lone wavefront has.  (kinematic6 built at K = 8: 256 + 256 registers, 148 spilled
  VGPRs and 580 B of scratch in k_run_rpf, 216 and 804 B in k_run_rpf_tr; at K = 4: 256 + 178 / 182 and none.  DESIGN.md section 12.)"""
  K, ZZ = run_pf_block(spec), max(k.zdim for k in spec.kinds) ** 2
  while K > 2 and K * ZZ > 36:
    K //= 2
  return K


def run_pf_rd_block(spec):
  """Steps per block of k_run_dpf: run_pf_block's, halved while the diagonal rows of a block exceed the staging budget run_pf_r_block states
  (K x zmax <= 36 doubles per buffer), or while the rows of both buffers with x and P take more than 172 VGPRs: what kinematic6's k_run_pf_tr
  (256 + 168 registers at K = 8, 84 of them x and P) leaves of the 512 a lone wavefront has.  kinematic6 built at K = 8 (96 VGPRs of rows): k_run_dpf
  256 + 218 and none spilled, k_run_dpf_tr 256 + 256 with 6 spilled VGPRs and 28 B of scratch; at K = 4 both fit.  A row is zmax doubles, not
  zmax^2: kinematic keeps 16, the 3- and 5-state models their 4, the 6-state models take 4 of k_run_pf's 8 like k_run_rpf.  The register table
  decides, not this rule: DESIGN.md section 12."""
  K, zmax = run_pf_block(spec), max(k.zdim for k in spec.kinds)
  while K > 2 and (K * zmax > 36 or 4 * K * zmax + 2 * (spec.dim_x + spec.dim_err ** 2) > 172):
    K //= 2
  return K


def run_pf_kernel(spec, norm, trace=False, noise=TABLE):
  """The fused run with a SCHEDULE PER FILTER (kinds (T, n), dts (T, n)): N independent logs replayed in one launch.  run_kernel_blk's
  structure -- blocks of K steps in registers, ONE vmcnt(0) per block, y and the flags of block b stored at the start of block b + 1 --
  with the schedule per lane: the lane of filter i loads its own kinds[t * n + i] and dts[t * n + i] of the next block's K steps with that
  block's observation rows (coalesced across the lanes; K more int + double registers per buffer), nothing is broadcast, the per-kind
  table of R sits in LDS beside Q, and the switch over kinds runs per lane as in k_kinds: a wavefront pays for the kinds present among its
  64 filters.  An idle entry (kind <= 0, flag 16) and an entry whose kind the model does not have (flag 8) skip predict and update: the
  lane's registers and its z row stay as they are.  A filter without a stepped entry in the whole schedule is not written back: its lane
  leaves the LDS image as it was loaded (the `_masked` kernels' rule).
  trace=True: k_run_pf_tr, every step's pair of every filter (stepped or not: the trace is dense) leaves through the LDS image as in
  k_run_blk_tr; the image of the final write-back is loaded again in front of it, since the trace has overwritten the one that came in.

  noise=ENTRY: k_run_rpf / k_run_rpf_tr, a NOISE MATRIX PER ENTRY: gR is (T, n, zmax^2) and row (t, i) is the R of filter i's entry t (the `r_per_filter`
  row of k_kinds).  No table in LDS: the lane of filter i stages its own rows of the next block in registers, loaded with that block's observation
  rows and schedule under the same single wait (zmax^2 doubles per step and buffer, hence the shorter block run_pf_r_block), clamped like them at
  rows past T and lanes past cnt.  A lane copies the leading Z^2 doubles of a row inside the case of its own kind, which an idle or flag-8 lane never
  enters: whatever such a row and the tail of the others hold (NaN included) stays in staging registers nothing reads.

  noise=DIAG: k_run_dpf / k_run_dpf_tr, a DIAGONAL NOISE PER ENTRY: k_run_rpf's structure with rows of zmax doubles -- gR is (T, n, zmax), the leading Z
  doubles of row (t, i) the variances of filter i's entry t.  Staged, clamped and waited for exactly like k_run_rpf's rows (a third of the registers
  at zmax = 3; the block is run_pf_rd_block's).  Inside the case of its own kind a lane fills the update's
  Rk[Z * Z] with its Z variances on the diagonal and literal zeros elsewhere; the update's statements are those of the other two kernels.

  The kernel's text is _blocked_run's; what is here is the schedule per lane, a register per step of the block, the table of R and `stepped`."""
  zmax = max(k.zdim for k in spec.kinds)
  ZZ = noise.row(zmax)      # doubles per row of gR
  NK = len(spec.kinds)
  K = {TABLE: run_pf_block, ENTRY: run_pf_r_block, DIAG: run_pf_rd_block}[noise](spec)
  names = dict(kname=noise.kernel + ("_tr" if trace else ""), title=(noise.title_small_tr if trace else noise.title_small).format(K=K, ZZ=ZZ))
  if noise.per_entry:
    # Rk of a kind: the lane's staged row, or its Z variances on the diagonal (i a constant of the unrolled loop)
    r_expr = (lambda idx: f"(i % {spec.kinds[idx].zdim + 1} == 0) ? Rc[u][i / {spec.kinds[idx].zdim + 1}] : 0.0") if noise.diag else "Rc[u][i]"
    # the rows of R travel like the schedule: the lane's own row of every step of the block, addressed by pointer increments
    table = dict(sched_ptrs=f"\n    const double* rrow = gR + (base + lc) * {ZZ};", decl_d=f", Rc[{K}][{ZZ}], Rn[{K}][{ZZ}]",
                 issue_ptrs=f"\n      const double* rp_ = rrow + tb0_ * (n * {ZZ});",
                 issue_row=f"\n#pragma unroll\n        for (int i = 0; i < {ZZ}; i++) Rn[u][i] = rp_[i];",
                 issue_step=f"\n        rp_ += (u < left_) ? n * {ZZ} : 0;",
                 pin_row=f"\n#pragma unroll\n        for (int i = 0; i < {ZZ}; i++) rn::pin(Rn[u][i]);",
                 rot_row=f"\n#pragma unroll\n        for (int i = 0; i < {ZZ}; i++) Rc[u][i] = Rn[u][i];")
  else:
    r_expr = lambda idx: f"s_R[{idx * ZZ} + i]"      # noqa: E731
    names.update(lds=dict(R=NK * ZZ), fill=f"\n  for (int i = lane; i < {NK * ZZ}; i += 64) s_R[i] = gR[i];      // one row per kind, in the order of the model's kinds")
    table = dict.fromkeys(("sched_ptrs", "decl_d", "issue_ptrs", "issue_row", "issue_step", "pin_row", "rot_row"), "")
  cases = kind_cases(spec, "_regs_sym", "cur[u]", r_expr, ind=12)
  known = " ".join(f"case {k.kind}:" for k in spec.kinds)
  return _blocked_run(
    spec, norm, trace, K, **names,
    helpers="" if trace or noise.per_entry else """
__device__ __forceinline__ void pin_k(int& v) { asm volatile("" : "+v"(v)); }
""",
    ragged_note="// lanes past the end of a ragged tile follow a copy of the last filter's schedule and rows and store nothing",
    sched_ptrs="\n    const int32_t* krow = kinds + base + lc;\n    const double* drow = dts + base + lc;" + table["sched_ptrs"],
    decl_d=f", dtv[{K}], dtn[{K}]" + table["decl_d"], decl_i=f", kv[{K}], kn[{K}]", decl_more="\n    bool stepped = false;",
    # the schedule is addressed by pointer increments like the rows
    issue_ptrs="\n      const int32_t* kp_ = krow + tb0_ * n;\n      const double* dp_ = drow + tb0_ * n;" + table["issue_ptrs"],
    issue_row="\n        kn[u] = kp_[0];\n        dtn[u] = dp_[0];" + table["issue_row"],
    issue_step="\n        kp_ += (u < left_) ? n : 0;\n        dp_ += (u < left_) ? n : 0;" + table["issue_step"],
    pin_row="\n        rn::pin(dtn[u]);\n        pin_k(kn[u]);" + table["pin_row"], rot_row="\n        dtv[u] = dtn[u];\n        kv[u] = kn[u];" + table["rot_row"],
    step=f"""          const int kind = kv[u];
          int fl = 16;                             // idle entry: no predict, the row passes through
          if (kind > 0) {{
            switch (kind) {{
              {known} {{
                const double dt = dtv[u];
                predict_regs_sym(x, P, s_Q, dt);
                {norm}
                stepped = true;
                fl = 0;
                break;
              }}
              default: fl = 8; break;      // not a kind of this model: untouched like an idle entry
            }}
          }}
          if (fl == 0) {{
            switch (kind) {{
{cases}
              default: break;
            }}
            {norm}
          }}""",
    trace_note="// pair of every filter after step t (an idle filter's is the one it had): through the LDS image, coalesced",
    reload_note="// the image the filters came with, again (the trace has overwritten it; x and P in HBM are still untouched)",
    wb_guard="    // a filter that no entry of its schedule stepped keeps the record it came with: its lane does not touch the image\n"
             "    if (live && stepped)")


def _launch_blocked(kname, more=""):
  """Launch text of a blocked run: `kname` without a trace, `kname`_tr with one."""
  return f"""  const int64_t tiles = (n + 63) >> 6;
  if (trace_x == nullptr && trace_P == nullptr) {{
    hipLaunchKernelGGL({kname}, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                       x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags{more});
  }} else {{
    hipLaunchKernelGGL({kname}_tr, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                       x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags{more}, trace_x, trace_P);
  }}"""


def launch_run_pf(noise=TABLE):
  return _launch_blocked(noise.kernel)


def launch_run(spec=None):
  blk = spec is not None and run_block(spec) > 0
  if not blk:
    return """  const int64_t tiles = (n + 63) >> 6;
  hipLaunchKernelGGL(k_run, dim3(rn::grid_for_tiles(tiles)), dim3(64), 0, (hipStream_t)stream,
                     x, P, Q, kinds, dts, T, z, R, n, norm_quats, flags, trace_x, trace_P, ea, augment);"""
  return "  (void)augment;\n" + _launch_blocked("k_run_blk", ", ea")
