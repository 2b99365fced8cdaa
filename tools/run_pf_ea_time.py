"""What replaying N recorded MSCKF logs costs: the fused run with a schedule per filter, landmarks and window shifts per entry
({name}_batch_run_pf_ea) against batch_run on a shared schedule and against the step walk it replaces.

  python tools/run_pf_ea_time.py [--reps 9] [--out profiles/run_pf_ea_times.txt]

One process, device warmed (two untimed rounds of every shape), HIP events around each alternative, the alternatives interleaved round by
round, every timed call from the same state; median with [min, max] over the rounds.  The schedule is the golden stream's pattern repeated
(POSITION followed by a window shift, then two FEATURE tracks); per filter, 20 % of the entries are idle, so kinds and shifts differ between
the filters of a wavefront.  Rows per workload:
  (a)  batch_run with the pattern as a shared schedule (the kernel that existed before: the baseline)
  (b)  batch_run_pf_ea, one launch, kinds / landmarks / shifts per filter, 20 % idle
  (c)  the schedule of (b) walked: per step one batch_predict_update_{k}_masked launch per kind and one batch_augment_masked
No target is fixed in advance; the tool reports (b)/(a) next to k_run_pf's own ratio to batch_run from profiles/run_pf_times.txt.
"""
import argparse
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = (("feature", 16384, 90), ("feature36", 4096, 45))
POSITION, FEATURE = 1, 2


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
  lines = [f"# tools/run_pf_ea_time.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  for name, n, T in WORKLOADS:
    M = model_class_of(name)
    f = BatchedEKF(ensure_generated([name]), name, M.Q, M.initial_x, np.diag(M.initial_P_diag), 6, 6, batch=n, per_filter=True, **M.filter_kwargs())
    dev, zmax = f.device, max(f.zdims.values())
    has = f._has_batch_run_pf_ea()
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    tab = np.zeros((len(f.kinds), zmax * zmax))
    for i, k in enumerate(f.kinds):
      tab[i, :M.obs_noise[k].size] = np.asarray(M.obs_noise[k]).reshape(-1)
    sched = np.array([POSITION if s % 3 == 0 else FEATURE for s in range(T)], dtype=np.int32)
    aug = (sched == POSITION).astype(np.int32)
    Rt = np.stack([tab[f.kinds.index(int(k))] for k in sched])
    idle = rng.random((T, n)) < 0.2
    kd = np.where(idle, 0, sched[:, None]).astype(np.int32)
    ag = np.where(idle, 0, aug[:, None]).astype(np.int32)
    ea = np.array([2.0, 1.0, 8.0]) + rng.normal(size=(T, n, 3)) * 0.5
    z = np.zeros((T, n, zmax))
    z[:, :, :3] = rng.normal(size=(T, n, 3)) * 0.2                                    # POSITION: the camera near the origin
    feat = np.tile(ea[:, :, :2] / ea[:, :, 2:3], (1, 1, zmax // 2))                    # FEATURE: the landmark seen from a window near the origin
    z = np.where((sched == FEATURE)[:, None, None], feat + rng.normal(size=(T, n, zmax)) * 0.01, z)
    x0, P0 = f.x.clone(), f.P.clone()
    z0 = t(z)
    zs = z0.clone()
    d = dict(tab=t(tab), sched=t(sched, torch.int32), aug=t(aug, torch.int32), dts=t(np.full(T, 0.05)), Rt=t(Rt), kd=t(kd, torch.int32), ag=t(ag, torch.int32),
             dts_pf=t(np.full((T, n), 0.05)), ea=t(ea))
    m8 = {k: t(kd == k, torch.uint8) for k in f.kinds}
    g8 = t(ag != 0, torch.uint8)
    shifts = ag.any(axis=1)
    Rk = {k: t(np.asarray(M.obs_noise[k], dtype=np.float64)) for k in f.kinds}
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    zk = {k: torch.empty((n, f.zdims[k]), dtype=torch.float64, device=dev) for k in f.kinds}

    def reset():
      f.x.copy_(x0)
      f.P.copy_(P0)
      zs.copy_(z0)

    def shared():
      f._call("batch_run", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["sched"]), f._p(d["dts"]), T, f._p(zs), f._p(d["Rt"]), n, f.norm_quats, None, None, None,
              f._p(d["ea"]), f._p(d["aug"]), f._stream())

    def fused():
      f._call("batch_run_pf_ea", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["kd"]), f._p(d["dts_pf"]), T, f._p(zs), f._p(d["tab"]), n, f.norm_quats, None, None, None,
              f._p(d["ea"]), f._p(d["ag"]), f._stream())

    def walk():
      for s in range(T):
        for k in f.kinds:
          if k != sched[s]:
            continue
          zk[k].copy_(zs[s, :, :f.zdims[k]])
          f._call(f"batch_predict_update_{k}_masked", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(d["dts_pf"][s]), 0.0, f._p(zk[k]), f._p(Rk[k]), 0,
                  f._p(d["ea"][s]) if f.eadims[k] else None, n, f.norm_quats, f._p(fl), f._p(m8[k][s]), f._stream())
          zs[s, :, :f.zdims[k]].copy_(zk[k])
        if shifts[s]:
          f._call("batch_augment_masked", f._p(f.x), f._p(f.P), f._p(g8[s]), n, f._stream())

    alts = [("a", shared), ("c", walk)] + ([("b", fused)] if has else [])
    rows = {key: [] for key in "abc"}
    for it in range(args.reps + 2):
      for key, fn in alts:
        reset()
        torch.cuda.synchronize()
        ms = timed(fn)
        if it >= 2:
          rows[key].append(ms)
    lines.append(f"\n== {name}, {n} filters x {T} entries, pattern POSITION + shift, FEATURE, FEATURE" + ("" if has else f"  (lib{name}.so has no batch_run_pf_ea kernel)") + " ==")
    lines.append(f"(a)  batch_run, the pattern as a shared schedule                          {stat(rows['a'])}")
    lines.append(f"(b)  batch_run_pf_ea, one launch, per filter, 20 % idle                   {stat(rows['b'])}")
    lines.append(f"(c)  the schedule of (b) as {T} masked steps + {int(shifts.sum())} masked shifts               {stat(rows['c'])}")
    if has:
      a_, b_, c_ = (float(np.median(rows[k])) for k in "abc")
      lines.append(f"     (b)/(a) = {b_ / a_:.2f}   (c)/(b) = {c_ / b_:.1f}   (a): {n * T / a_ / 1e6:.3f} G filter-steps/s, (b): {n * T / b_ / 1e6:.3f} G entries/s")
  ref = os.path.join(REPO, "profiles", "run_pf_times.txt")
  if os.path.exists(ref):
    with open(ref, encoding="utf-8") as fh:
      text = fh.read()
    pairs = re.findall(r"^== (\w+),.*?\(c\)/\(a\) = ([\d.]+)", text, re.M | re.S)
    lines.append("\nk_run_pf's own ratio to batch_run, kinds per filter and 20 % idle (profiles/run_pf_times.txt, (c)/(a)): " + ", ".join(f"{m} {r}" for m, r in pairs))
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)


if __name__ == "__main__":
  main()
