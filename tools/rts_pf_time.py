"""What smoothing N recorded logs costs: the smoother with a schedule per filter ({name}_batch_rts_pf) against batch_rts on a shared schedule
and against what a user does without it, one batch_rts call per log.

  python tools/rts_pf_time.py [--reps 9] [--out profiles/rts_pf_times.txt]

One process, device warmed (two untimed rounds of every shape), HIP events around each alternative, the alternatives interleaved round by
round, separate output buffers (every timed call reads the same trace); median with [min, max] over the rounds.  The traces are synthetic:
states around the model's initial one, random SPD covariances around its initial one (tools/rts4_time.py's).  Rows per workload:
  (a)   batch_rts on a shared schedule
  (b)   batch_rts_pf with that schedule replicated per filter
  (c)   batch_rts_pf with ragged logs (every filter's log ends somewhere in the second half) and 20 % idle entries
  (d)   what a user does today: 64 of the logs of (c), each compacted to its real entries and smoothed by its own batch_rts call on a batch of one
  (d')  those same 64 logs in one batch_rts_pf launch
The tool exits non-zero unless the median of (d') lies below the minimum sample of (d).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = (("live", 8192, 300), ("kinematic6", 65536, 200), ("kinematic9", 65536, 100))      # (kinematic9: a library whose batch_rts_pf is k_rts4_pf)
LOGS = 64


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
  lines = [f"# tools/rts_pf_time.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, one process, HIP events, alternatives interleaved"]

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  failed = []
  for name, n, T in WORKLOADS:
    M = bench.model_class(name)
    gen = ensure_generated([name])
    D, E = M.initial_x.shape[0], M.initial_P_diag.shape[0]
    quat = [3] if name == "live" else []
    f = BatchedEKF(gen, name, M.Q, M.initial_x, np.diag(M.initial_P_diag), D, E, batch=n, quaternion_idxs=quat, per_filter=True)
    assert f._has_batch_rts_pf(), f"lib{name}.so has no batch_rts_pf kernel"
    dev = f.device
    g = torch.Generator(device=dev).manual_seed(0)
    tx = torch.as_tensor(M.initial_x, device=dev).repeat(T, n, 1).contiguous()
    if quat:
      tx[:, :, 3:7] += 0.01 * torch.randn((T, n, 4), dtype=torch.float64, device=dev, generator=g)
    A = torch.randn((n, E, E), dtype=torch.float64, device=dev, generator=g) * 0.01
    P = torch.diag(torch.as_tensor(M.initial_P_diag, device=dev)) * 1e-2 + A @ A.transpose(1, 2)
    tP = P.repeat(T, 1, 1, 1).contiguous()
    del A, P
    xs, Ps = torch.empty_like(tx), torch.empty_like(tP)
    rng = np.random.default_rng(0)
    t = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)      # noqa: E731
    ts = t(np.arange(T) * 0.01)
    act_c = rng.random((T, n)) >= 0.2
    act_c &= np.arange(T)[:, None] < rng.integers(T // 2, T + 1, size=n)[None, :]
    act_c[0] = True
    d = dict(dts=t(np.full((T, n), 0.01)), act_b=t(np.ones((T, n)), torch.uint8), act_c=t(act_c, torch.uint8))
    nq = f.norm_quats | (f.norm_quats << 1)
    # the 64 logs of (d) / (d'): dense for the one launch; compacted to their real entries, each with its own times, for the 64 calls
    sub = dict(tx=tx[:, :LOGS].contiguous(), tP=tP[:, :LOGS].contiguous(), act=d["act_c"][:, :LOGS].contiguous(), dts=d["dts"][:, :LOGS].contiguous())
    sub["xs"], sub["Ps"] = torch.empty_like(sub["tx"]), torch.empty_like(sub["tP"])
    one = []
    for i in range(LOGS):
      rows = torch.as_tensor(np.nonzero(act_c[:, i])[0], device=dev)
      one.append(dict(tx=tx[rows, i:i + 1].contiguous(), tP=tP[rows, i:i + 1].contiguous(), ts=t(np.arange(len(rows)) * 0.01), T=len(rows)))
      one[-1]["xs"], one[-1]["Ps"] = torch.empty_like(one[-1]["tx"]), torch.empty_like(one[-1]["tP"])

    def shared():
      f._call("batch_rts", f._p(tx), f._p(tP), f._p(ts), T, f._p(f.Q), n, nq, f._p(xs), f._p(Ps), None, None, f._stream())

    def fused(act):
      f._call("batch_rts_pf", f._p(tx), f._p(tP), f._p(d["dts"]), f._p(d[act]), T, f._p(f.Q), n, nq, f._p(xs), f._p(Ps), None, None, f._stream())

    def per_log():
      for o in one:
        f._call("batch_rts", f._p(o["tx"]), f._p(o["tP"]), f._p(o["ts"]), o["T"], f._p(f.Q), 1, nq, f._p(o["xs"]), f._p(o["Ps"]), None, None, f._stream())

    def one_launch():
      f._call("batch_rts_pf", f._p(sub["tx"]), f._p(sub["tP"]), f._p(sub["dts"]), f._p(sub["act"]), T, f._p(f.Q), LOGS, nq, f._p(sub["xs"]), f._p(sub["Ps"]),
              None, None, f._stream())

    alts = [("a", shared), ("b", lambda: fused("act_b")), ("c", lambda: fused("act_c")), ("d", per_log), ("d'", one_launch)]
    rows = {key: [] for key, _ in alts}
    for it in range(args.reps + 2):
      for key, fn in alts:
        torch.cuda.synchronize()
        ms = timed(fn)
        if it >= 2:
          rows[key].append(ms)
    assert bool(torch.isfinite(xs).all() and torch.isfinite(Ps).all() and torch.isfinite(sub["Ps"]).all())
    one_key = "d'"
    lines.append(f"\n== {name}, {n} filters x {T} steps ==")
    lines.append(f"(a)   batch_rts, shared schedule                               {stat(rows['a'])}")
    lines.append(f"(b)   batch_rts_pf, that schedule per filter                   {stat(rows['b'])}")
    lines.append(f"(c)   batch_rts_pf, ragged logs, 20 % idle                     {stat(rows['c'])}")
    lines.append(f"(d)   {LOGS} of the logs of (c), one batch_rts call each            {stat(rows['d'])}")
    lines.append(f"(d')  those {LOGS} logs in one batch_rts_pf launch                 {stat(rows[one_key])}")
    a_, b_, c_, d_, e_ = (float(np.median(rows[k])) for k in ("a", "b", "c", "d", "d'"))
    ok = e_ < min(rows["d"])
    if not ok:
      failed.append(name)
      lines.append(f"     FAILED: median (d') {e_:.3f} ms is not below the minimum sample of (d) {min(rows['d']):.3f} ms -- one launch loses to {LOGS} calls")
    lines.append(f"     (b)/(a) = {b_ / a_:.2f}   (c)/(a) = {c_ / a_:.2f}   (d)/(d') = {d_ / e_:.1f}   median (d') {'<' if ok else '>='} min (d) = {min(rows['d']):.3f} ms"
                 f"   (a): {n * (T - 1) / a_ / 1e3:.1f} M steps/s, (c): {int(act_c.sum()) / c_ / 1e3:.1f} M real entries/s")
    del tx, tP, xs, Ps, sub, one, d
    torch.cuda.empty_cache()
  text = "\n".join(lines) + "\n"
  print(text)
  if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
      fh.write(text)
  if failed:
    sys.exit(f"median (d') >= min (d) for {failed}")


if __name__ == "__main__":
  main()
