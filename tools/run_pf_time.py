"""What replaying N recorded logs costs: the fused run with a schedule per filter ({name}_batch_run_pf) against batch_run on a shared
schedule and against the step walk it replaces.

  python tools/run_pf_time.py [--reps 9] [--out profiles/run_pf_times.txt]

One process, device warmed (two untimed rounds of every shape), HIP events around each alternative, the alternatives interleaved round by
round, every timed call from the same state; median with [min, max] over the rounds.  Rows per workload:
  (a)  batch_run on a shared schedule
  (b)  batch_run_pf with that schedule replicated per filter
  (c)  batch_run_pf with kinds drawn per filter and 20 % idle entries
  (d)  the yardstick: the schedule of (c) walked with T batch_predict_update_kinds launches
A library without the kernel ({name}_has_batch_run_pf() == 0) reports (b) and (c) as "not measured".
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
  lines = [f"# tools/run_pf_time.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

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
    has_pf = f._has_batch_run_pf()
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    Rs = {k: np.atleast_2d(M.obs_noise[k]) for k in kinds}
    tab = np.zeros((len(f.kinds), zmax * zmax))
    for i, k in enumerate(f.kinds):
      if k in Rs:
        tab[i, :Rs[k].size] = Rs[k].reshape(-1)
    sched = np.array([kinds[s % len(kinds)] for s in range(T)], dtype=np.int32)
    Rt = np.stack([tab[f.kinds.index(int(k))] for k in sched])
    kd_mixed = rng.choice(np.array(kinds, dtype=np.int32), size=(T, n)).astype(np.int32)
    kd_mixed[rng.random((T, n)) < 0.2] = 0
    x0, P0 = f.x.clone(), f.P.clone()
    z0 = t(rng.normal(size=(T, n, zmax)) * 0.1)
    zs = z0.clone()
    d = dict(tab=t(tab), sched=t(sched, torch.int32), dts=t(np.full(T, 0.01)), Rt=t(Rt), kd_rep=t(np.tile(sched[:, None], (1, n)), torch.int32),
             kd_mixed=t(kd_mixed, torch.int32), dts_pf=t(np.full((T, n), 0.01)), act=t(kd_mixed > 0, torch.uint8))
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)

    def reset():
      f.x.copy_(x0)
      f.P.copy_(P0)
      zs.copy_(z0)

    def shared():
      f._call("batch_run", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["sched"]), f._p(d["dts"]), T, f._p(zs), f._p(d["Rt"]), n, f.norm_quats, None, None, None,
              None, None, f._stream())

    def fused(kd):
      f._call("batch_run_pf", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d[kd]), f._p(d["dts_pf"]), T, f._p(zs), f._p(d["tab"]), n, f.norm_quats, None, None, None,
              f._stream())

    def walk():
      for s in range(T):
        f._call("batch_predict_update_kinds", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["dts_pf"][s]), 0.0, f._p(d["kd_mixed"][s]), f._p(zs[s]), f._p(d["tab"]), 0, n,
                f.norm_quats, f._p(fl), f._p(d["act"][s]), f._stream())

    alts = [("a", shared), ("d", walk)] + ([("b", lambda: fused("kd_rep")), ("c", lambda: fused("kd_mixed"))] if has_pf else [])
    rows = {key: [] for key in "abcd"}
    for it in range(args.reps + 2):
      for key, fn in alts:
        reset()
        torch.cuda.synchronize()
        ms = timed(fn)
        if it >= 2:
          rows[key].append(ms)
    steps = n * T
    lines.append(f"\n== {name}, {n} filters x {T} steps, kinds {list(kinds)}" + ("" if has_pf else f"  (lib{name}.so has no batch_run_pf kernel)") + " ==")
    lines.append(f"(a)  batch_run, shared schedule                              {stat(rows['a'])}")
    lines.append(f"(b)  batch_run_pf, that schedule per filter                  {stat(rows['b'])}")
    lines.append(f"(c)  batch_run_pf, kinds per filter, 20 % idle               {stat(rows['c'])}")
    lines.append(f"(d)  the schedule of (c) as {T} batch_predict_update_kinds    {stat(rows['d'])}")
    if has_pf:
      a_, b_, c_, d_ = (float(np.median(rows[k])) for k in "abcd")
      if not c_ < min(rows["d"]):
        failed.append(name)
        lines.append(f"     FAILED: median (c) {c_:.3f} ms is not below the minimum sample of (d) {min(rows['d']):.3f} ms -- one launch loses to {T} launches")
      lines.append(f"     (b)/(a) = {b_ / a_:.2f}   (c)/(a) = {c_ / a_:.2f}   (d)/(c) = {d_ / c_:.1f}   median (c) {'<' if c_ < min(rows['d']) else '>='} min (d) = {min(rows['d']):.3f} ms"
                   f"   (a): {steps / a_ / 1e6:.2f} G filter-steps/s, (c): {steps / c_ / 1e6:.2f} G entries/s")
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)
  if failed:
    sys.exit(f"median (c) >= min (d) for {failed}")


if __name__ == "__main__":
  main()
