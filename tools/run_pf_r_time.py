"""What a noise matrix per log entry costs in the fused run with a schedule per filter: {name}_batch_run_pf_r against batch_run_pf with the
shared per-kind table and against the step walk it replaces.

  python tools/run_pf_r_time.py [--reps 9] [--out profiles/run_pf_r_times.txt]

One process, device warmed (two untimed rounds of every shape), HIP events around each alternative, the alternatives interleaved round by
round, every timed call from the same state; median with [min, max] over the rounds.  The workloads of tools/run_pf_time.py: kinds drawn per
filter, 20 % idle entries.  Rows per workload:
  (a)  batch_run_pf, R the shared per-kind table
  (b)  batch_run_pf_r, the same schedule, R per entry (T, n, zmax^2): every stepped entry's row filled, the rows of idle entries NaN
  (c)  the yardstick: the same schedule as T batch_predict_update_kinds launches with R[t] and r_per_filter = 1
The acceptance rule: the median of (b) lies below the minimum sample of (c) on every workload (the tool exits non-zero otherwise).  (b)/(a) is
reported, not bounded: the kernel reads up to 8 zmax^2 more bytes per entry.  A library without the kernel reports (b) as "not measured".
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = (("kinematic6", 65536, 200, (1,)), ("kinematic9", 65536, 100, (1, 2, 3)))


def stat(v):
  return "not measured" if not v else f"median {np.median(v):9.3f} ms   [min {np.min(v):9.3f}, max {np.max(v):9.3f}]"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=9)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import torch
  import bench
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  lines = [f"# tools/run_pf_r_time.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  failed = []
  for name, n, T, kinds in WORKLOADS:
    M = bench.model_class(name)
    gen = ensure_generated([name])
    D, E = M.initial_x.shape[0], M.initial_P_diag.shape[0]
    f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, per_filter=True)
    dev, zmax = f.device, max(f.zdims.values())
    ZZ = zmax * zmax
    has_r = f._has_batch_run_pf_r()
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
    tab = np.zeros((len(f.kinds), ZZ))
    for i, k in enumerate(f.kinds):
      if k in Rs:
        tab[i, :Rs[k].size] = Rs[k].reshape(-1)
    kd = rng.choice(np.array(kinds, dtype=np.int32), size=(T, n)).astype(np.int32)
    kd[rng.random((T, n)) < 0.2] = 0
    # R per entry on the device: the kind's row scaled per entry (log-uniform in [0.25, 4]), NaN in the rows of idle entries
    kdd = t(kd, torch.int32)
    idx = torch.zeros((T, n), dtype=torch.int64, device=dev)
    for i, k in enumerate(f.kinds):
      idx[kdd == k] = i
    scale = torch.exp(torch.empty((T, n, 1), dtype=torch.float64, device=dev).uniform_(np.log(0.25), np.log(4.0)))
    Re = (t(tab)[idx] * scale).contiguous()
    Re[kdd <= 0] = float("nan")
    del idx, scale
    x0, P0 = f.x.clone(), f.P.clone()
    z0 = t(rng.normal(size=(T, n, zmax)) * 0.1)
    zs = z0.clone()
    d = dict(tab=t(tab), kd=kdd, dts=t(np.full((T, n), 0.01)), act=t(kd > 0, torch.uint8))
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert (n * ZZ) % 2 == 0 and (n * zmax) % 2 == 0, "the rows of a step stay 16-byte aligned"

    def reset():
      f.x.copy_(x0)
      f.P.copy_(P0)
      zs.copy_(z0)

    def table():
      f._call("batch_run_pf", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["kd"]), f._p(d["dts"]), T, f._p(zs), f._p(d["tab"]), n, f.norm_quats, None, None, None,
              f._stream())

    def entry():
      f._call("batch_run_pf_r", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["kd"]), f._p(d["dts"]), T, f._p(zs), f._p(Re), n, f.norm_quats, None, None, None,
              f._stream())

    def walk():
      for s in range(T):
        f._call("batch_predict_update_kinds", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["dts"][s]), 0.0, f._p(d["kd"][s]), f._p(zs[s]), f._p(Re[s]), 1, n,
                f.norm_quats, f._p(fl), f._p(d["act"][s]), f._stream())

    alts = [("a", table), ("c", walk)] + ([("b", entry)] if has_r else [])
    rows = {key: [] for key in "abc"}
    for it in range(args.reps + 2):
      for key, fn in alts:
        reset()
        torch.cuda.synchronize()
        ms = timed(fn)
        if it >= 2:
          rows[key].append(ms)
    assert bool(torch.isfinite(f.x).all()) and bool(torch.isfinite(f.P).all()), "NaN rows of R have reached the state"
    entries = n * T
    lines.append(f"\n== {name}, {n} filters x {T} steps, kinds {list(kinds)} drawn per filter, 20 % idle" +
                 ("" if has_r else f"  (lib{name}.so has no batch_run_pf_r kernel)") + " ==")
    lines.append(f"(a)  batch_run_pf, the shared per-kind table                 {stat(rows['a'])}")
    lines.append(f"(b)  batch_run_pf_r, that schedule, R per entry              {stat(rows['b'])}")
    lines.append(f"(c)  that schedule as {T} batch_predict_update_kinds, R[t]    {stat(rows['c'])}")
    if has_r:
      a_, b_, c_ = (float(np.median(rows[k])) for k in "abc")
      if not b_ < min(rows["c"]):
        failed.append(name)
        lines.append(f"     FAILED: median (b) {b_:.3f} ms is not below the minimum sample of (c) {min(rows['c']):.3f} ms -- one launch loses to {T} launches")
      lines.append(f"     (b)/(a) = {b_ / a_:.2f}   (c)/(b) = {c_ / b_:.1f}   median (b) {'<' if b_ < min(rows['c']) else '>='} min (c) = {min(rows['c']):.3f} ms"
                   f"   (b): {entries / b_ / 1e6:.2f} G entries/s, {entries * ZZ * 8 / b_ / 1e6:.1f} GB/s of R")
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)
  if failed:
    sys.exit(f"median (b) >= min (c) for {failed}")


if __name__ == "__main__":
  main()
