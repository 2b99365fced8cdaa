"""What a tick costs at which the filters of a batch bring different observation kinds: the per-kind `_masked` launches against the one
mixed-kind launch ({name}_batch_predict_update_kinds), and the same through BatchedEKF with a ring of 8.

  python tools/step_kinds_time.py [--launches 300] [--out profiles/step_kinds_times.txt]

One process, device warmed, HIP events around every single launch (or group of launches), the alternatives interleaved round by
round, medians with min / p5 / p95 / max -- p5 .. p95 is the spread that one outlier does not decide -- (A/B numbers are compared within one run only).  Rows per workload:
  1  one single-kind launch batch_predict_update_{k} per kind (what one trip of the state through HBM costs)
  2  the k `_masked` launches of a mixed tick, summed -- the yardstick
  3  the one k_kinds launch, kinds drawn uniformly per filter (every tile / pass mixed) and the same kinds sorted (uniform tiles)
  4  per call through BatchedEKF(per_filter=True, rewind_to_keep=8): predict_and_update_kinds against the k per-kind calls
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = (("kinematic9", 65536, (1, 2, 3)), ("live", 16384, (3, 4, 9, 10, 12, 13, 14, 19)))


def stat(v):
  v = np.asarray(v) * 1e3
  return f"median {np.median(v):8.2f} us   min {v.min():8.2f}   p5 {np.percentile(v, 5):8.2f}   p95 {np.percentile(v, 95):8.2f}   max {v.max():8.2f}"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--launches", type=int, default=300)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  import torch
  import bench
  from examples import ensure_generated
  from rednose_amd.helpers.ekf_sym import BatchedEKF
  lines = [f"# tools/step_kinds_time.py --launches {args.launches}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  for name, n, kinds in WORKLOADS:
    M = bench.model_class(name)
    gen = ensure_generated([name])
    D, E = M.initial_x.shape[0], M.initial_P_diag.shape[0]
    quat = list(getattr(M, "quaternion_idxs", []))
    Rs = {k: np.atleast_2d(M.obs_noise.get(k, np.eye(1 if (name == "live" and k == 3) else 3) * 0.1)) for k in kinds}
    mk = lambda **kw: BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat, **kw)      # noqa: E731
    f = mk()
    dev, zmax = f.device, max(f.zdims.values())
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    x0, P0 = f.x.clone(), f.P.clone()
    kd_rand = rng.choice(np.array(kinds, dtype=np.int32), size=n).astype(np.int32)
    kd_sort = np.sort(kd_rand)
    tab = np.zeros((len(f.kinds), zmax * zmax))
    for i, k in enumerate(f.kinds):
      if k in Rs:
        tab[i, :Rs[k].size] = Rs[k].reshape(-1)
    tab = t(tab)
    dt = t(np.full(n, 0.01))
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    zs = {k: t(np.zeros((n, Rs[k].shape[0]))) for k in kinds}
    Rd = {k: t(Rs[k]) for k in kinds}
    zm = t(np.zeros((n, zmax)))
    masks = {tag: {k: t(kd == k, torch.uint8) for k in kinds} for tag, kd in (("random", kd_rand), ("sorted", kd_sort))}
    kdd = {"random": t(kd_rand, torch.int32), "sorted": t(kd_sort, torch.int32)}

    def reset():      # every timed launch starts from the same state (an update shrinks P: a stream of them would drift)
      f.x.copy_(x0)
      f.P.copy_(P0)

    def single(k):
      f._call(f"batch_predict_update_{k}", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(dt), 0.0, f._p(zs[k]), f._p(Rd[k]), 0, None, n, f.norm_quats, f._p(fl), f._stream())

    def masked(tag):
      for k in kinds:
        f._call(f"batch_predict_update_{k}_masked", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(dt), 0.0, f._p(zs[k]), f._p(Rd[k]), 0, None, n, f.norm_quats, f._p(fl),
                f._p(masks[tag][k]), f._stream())

    def mixed(tag):
      f._call("batch_predict_update_kinds", f._p(f.x), f._p(f.P), f._p(f.Q), f._p(dt), 0.0, f._p(kdd[tag]), f._p(zm), f._p(tab), 0, n, f.norm_quats, f._p(fl), None, f._stream())

    rows = {("1", k): [] for k in kinds}
    rows.update({(r, tag): [] for r in ("2", "3") for tag in ("random", "sorted")})
    for it in range(args.launches + 20):
      for key in rows:
        reset()
        ms = timed((lambda k=key[1]: single(k)) if key[0] == "1" else ((lambda g=key[1]: masked(g)) if key[0] == "2" else (lambda g=key[1]: mixed(g))))
        if it >= 20:
          rows[key].append(ms)
    lines.append(f"\n== {name}, {n} filters, {len(kinds)} kinds {list(kinds)} ==")
    for k in kinds:
      lines.append(f"row 1  single-kind launch, kind {k:<3d}                         {stat(rows[('1', k)])}")
    one = float(np.median([np.median(rows[("1", k)]) for k in kinds]))
    for tag in ("random", "sorted"):
      lines.append(f"row 2  {len(kinds)} masked launches, kinds {tag:<7s} (yardstick)      {stat(rows[('2', tag)])}")
    for tag in ("random", "sorted"):
      r3, r2 = float(np.median(rows[("3", tag)])), float(np.median(rows[("2", tag)]))
      lines.append(f"row 3  one k_kinds launch, kinds {tag:<7s}                   {stat(rows[('3', tag)])}   = {r3 / r2:.2f} x row 2, {r3 / one:.2f} x a single-kind launch")
    # ---- row 4: through the orchestrator, a ring of 8 ----
    a, b = mk(per_filter=True, rewind_to_keep=8, device_timeline=True), mk(per_filter=True, rewind_to_keep=8, device_timeline=True)
    ta, tb = [], []
    for it in range(args.launches // 2 + 10):
      tt = t(np.full(n, 0.01 * (it + 1)))
      for obj, acc, call in ((a, ta, "mixed"), (b, tb, "per kind")):
        if it % 10 == 0:
          obj.x.copy_(x0)
          obj.P.copy_(P0)
        if call == "mixed":
          ms = timed(lambda: obj.predict_and_update_kinds(tt, kd_rand, zm, Rs))      # (kinds as the host has them: no read back to find which are present)
        else:
          def per_kind():
            for k in kinds:
              obj.predict_and_update_batch(tt, k, zs[k], Rd[k], active=masks["random"][k])
          ms = timed(per_kind)
        if it >= 10:
          acc.append(ms)
    assert a.pf_stats["legacy"] == 0, a.pf_stats
    lines.append(f"row 4  BatchedEKF, ring of 8: {len(kinds)} per-kind calls (yardstick)     {stat(tb)}")
    lines.append(f"row 4  BatchedEKF, ring of 8: one predict_and_update_kinds      {stat(ta)}   = {np.median(ta) / np.median(tb):.2f} x the per-kind calls")
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)


if __name__ == "__main__":
  main()
