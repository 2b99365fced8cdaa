"""What a DIAGONAL noise per log entry costs in the fused run with a schedule per filter: {name}_batch_run_pf_rd (rows of zmax variances) against
batch_run_pf_r on the same log with the diagonal expanded to full rows of zmax^2 -- what such a log costs without this entry point -- and against
batch_run_pf with the shared per-kind table.

  python tools/run_pf_rd_time.py [--reps 9] [--out profiles/run_pf_rd_times.txt]

One process, device warmed (two untimed rounds of every shape), HIP events around each alternative, the alternatives interleaved round by
round, every timed call from the same state; median with [min, max] over the rounds.  The workloads of tools/run_pf_r_time.py: kinds drawn per
filter, 20 % idle entries, NaN in everything the contract calls never read (the rows of idle entries, the positions beyond Z and Z * Z).
Rows per workload:
  (a)  batch_run_pf, R the shared per-kind table
  (b)  the yardstick: batch_run_pf_r, the same schedule, every entry's diag(variances) as a full row (T, n, zmax^2)
  (c)  batch_run_pf_rd, the same schedule, the variances (T, n, zmax)
randz10 (a 9-dimensional kind) has no batch_run_pf_r kernel: its yardstick (w) is what run_logs does with such a log without (c), the step walk
of `_masked` launches with R[t] (BatchedEKF._run_logs_stepwise, host work included).
The acceptance rule, for kinematic6 (lane per filter, a memory kernel: 84 B per entry against 132 B): the median of (c) lies below the minimum
sample of (b); the tool exits non-zero otherwise.  kinematic9 (lane group: R is 3 % of its time) is reported, with a note if the median of (c)
lies above the maximum sample of (b).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

#            model         n      T    kinds      bounded
WORKLOADS = (("kinematic6", 65536, 200, (1,), True), ("kinematic9", 65536, 100, (1, 2, 3), False), ("randz10", 16384, 50, None, False))


def stat(v):
  return "not measured" if not v else f"median {np.median(v):9.3f} ms   [min {np.min(v):9.3f}, max {np.max(v):9.3f}]"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=9)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import torch
  from examples import ensure_generated, model_class_of
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  lines = [f"# tools/run_pf_rd_time.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  failed = []
  for name, n, T, kinds, bounded in WORKLOADS:
    M = model_class_of(name)
    gen = ensure_generated([name])
    D, E = len(M.initial_x), len(M.initial_P_diag)
    f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, per_filter=True)
    kinds = tuple(sorted(f.zdims)) if kinds is None else kinds
    dev, zmax = f.device, max(f.zdims.values())
    ZZ = zmax * zmax
    has_r, has_rd = f._has_batch_run_pf_r(), f._has_batch_run_pf_rd()
    if not has_rd:
      lines.append(f"\n== {name}: lib{name}.so has no batch_run_pf_rd kernel, nothing to measure ==")
      continue
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
    tab, var = np.zeros((len(f.kinds), ZZ)), np.full((len(f.kinds), zmax), np.nan)
    for i, k in enumerate(f.kinds):
      if k in Rs:
        Rk = np.diag(np.diag(Rs[k]))      # the same diagonal noise in all three forms
        tab[i, :Rk.size] = Rk.reshape(-1)
        var[i, :Rk.shape[0]] = np.diag(Rk)
    kd = rng.choice(np.array(kinds, dtype=np.int32), size=(T, n)).astype(np.int32)
    kd[rng.random((T, n)) < 0.2] = 0
    # the variances per entry on the device: the kind's diagonal scaled per entry (log-uniform in [0.25, 4]); NaN beyond Z and in the rows of idle entries
    kdd = t(kd, torch.int32)
    idx = torch.zeros((T, n), dtype=torch.int64, device=dev)
    for i, k in enumerate(f.kinds):
      idx[kdd == k] = i
    scale = torch.exp(torch.empty((T, n, 1), dtype=torch.float64, device=dev).uniform_(np.log(0.25), np.log(4.0)))
    Rv = (t(var)[idx] * scale).contiguous()
    Rv[kdd <= 0] = float("nan")
    # the same numbers as full rows: diag(variances) in the leading Z * Z doubles, NaN beyond and in the rows of idle entries
    Re = torch.full((T, n, ZZ), float("nan"), dtype=torch.float64, device=dev)
    for k in kinds:
      Z = f.zdims[k]
      m = kdd == k
      Re[:, :, :Z * Z] = torch.where(m[:, :, None], torch.diag_embed(torch.nan_to_num(Rv[:, :, :Z])).reshape(T, n, Z * Z), Re[:, :, :Z * Z])
    del idx, scale
    x0, P0 = f.x.clone(), f.P.clone()
    z0 = t(rng.normal(size=(T, n, zmax)) * 0.1)
    zs = z0.clone()
    d = dict(tab=t(tab), kd=kdd, dts=t(np.full((T, n), 0.01)))
    assert (n * ZZ) % 2 == 0 and (n * zmax) % 2 == 0, "the rows of a step stay 16-byte aligned"

    def reset():
      f.x.copy_(x0)
      f.P.copy_(P0)
      zs.copy_(z0)

    def launch(sym, R):
      return lambda: f._call(sym, f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["kd"]), f._p(d["dts"]), T, f._p(zs), f._p(R), n, f.norm_quats, None, None, None,
                             f._stream())

    def walk():
      f._run_logs_stepwise(d["kd"], d["dts"], zs, Re, None, None, None, per_entry=True)

    alts = [("a", launch("batch_run_pf", d["tab"])), ("c", launch("batch_run_pf_rd", Rv))] + ([("b", launch("batch_run_pf_r", Re))] if has_r else [("w", walk)])
    rows = {key: [] for key in "abcw"}
    for it in range(args.reps + 2):
      for key, fn in alts:
        reset()
        torch.cuda.synchronize()
        ms = timed(fn)
        if it >= 2:
          rows[key].append(ms)
    assert bool(torch.isfinite(f.x).all()) and bool(torch.isfinite(f.P).all()), "NaN doubles of R have reached the state"
    entries = n * T
    lines.append(f"\n== {name}, {n} filters x {T} steps, kinds {list(kinds)} drawn per filter, 20 % idle" +
                 ("" if has_r else f"  (lib{name}.so has no batch_run_pf_r kernel)") + " ==")
    lines.append(f"(a)  batch_run_pf, the shared per-kind table                       {stat(rows['a'])}")
    if has_r:
      lines.append(f"(b)  batch_run_pf_r, that schedule, diag(variances) as full rows   {stat(rows['b'])}")
    else:
      lines.append(f"(w)  that schedule walked with `_masked` launches, R[t]            {stat(rows['w'])}")
    lines.append(f"(c)  batch_run_pf_rd, that schedule, the variances                 {stat(rows['c'])}")
    a_, c_ = float(np.median(rows["a"])), float(np.median(rows["c"]))
    rate = f"(c): {entries / c_ / 1e6:.2f} G entries/s, {entries * zmax * 8 / c_ / 1e6:.1f} GB/s of R"
    if has_r:
      b_ = float(np.median(rows["b"]))
      if bounded and not c_ < min(rows["b"]):
        failed.append(name)
        lines.append(f"     FAILED: median (c) {c_:.3f} ms is not below the minimum sample of (b) {min(rows['b']):.3f} ms")
      if not bounded and c_ > max(rows["b"]):
        lines.append(f"     NOTE: median (c) {c_:.3f} ms lies above the maximum sample of (b) {max(rows['b']):.3f} ms")
      lines.append(f"     (b)/(c) = {b_ / c_:.2f}   (c)/(a) = {c_ / a_:.2f}   median (c) {'<' if c_ < min(rows['b']) else '>='} min (b) = {min(rows['b']):.3f} ms   {rate}")
    else:
      lines.append(f"     (w)/(c) = {float(np.median(rows['w'])) / c_:.1f}   (c)/(a) = {c_ / a_:.2f}   {rate}")
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)
  if failed:
    sys.exit(f"median (c) >= min (b) for {failed}")


if __name__ == "__main__":
  main()
