"""Per-call wall time of per-filter timelines (BatchedEKF(per_filter=True)) on kinematic6 with the in-order bookkeeping on the device (the
default where the library has {name}_batch_timeline_plan / _push) against the torch bookkeeping (device_timeline=False), in ONE process:
4 096 and 65 536 filters, every filter on its own clock, without a ring and with a ring of 8; in order, and with 1 % of the filters late
in every call.  Such a call takes the torch path on either object; the 1 % late rows time a third object, device_rewind=True, which serves it
on the device (batch_rewind_locate / _fetch, one mixed-kind step and one push per replay position).  The objects are fed the same calls in
alternating blocks of CALLS calls; a block is timed with the host clock around calls that end in a device synchronise.  Per row: min / median /
max over REPS blocks and the verdict against the spread (max - min) of the torch rows.

  python tools/pf_device_timeline_time.py [--out FILE] [--late-only]

--late-only: the 1 % late rows alone (profiles/pf_device_rewind_call_times.txt).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from examples import ensure_generated
from examples.kinematic6_kf import Kinematic6Kalman as K6
from rednose_amd.helpers.ekf_sym import BatchedEKF

CALLS, REPS, WARM = 200, 7, 50

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--late-only", action="store_true")
args = ap.parse_args()
lines = []


def say(s=""):
  print(s, flush=True)
  lines.append(s)


gen = ensure_generated(["kinematic6"])
dev = torch.device("cuda:0")
R = np.ascontiguousarray(K6.obs_noise[1], dtype=np.float64)


class Stream:
  """One object and its own clock: blocks of calls, each filter at its own time t + off[i]."""

  def __init__(self, n, ring, **kw):
    self.f = BatchedEKF(gen, "kinematic6", K6.Q, K6.initial_x, np.diag(K6.initial_P_diag), 6, 6, batch=n, device=dev, per_filter=True,
                        **({"rewind_to_keep": ring} if ring else {}), **kw)
    self.z = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    self.off = np.linspace(0.0, 0.005, n)
    self.t = 0.0
    self.k = 0

  def block(self, calls, late):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
      self.t += 0.01
      tt = self.t + self.off
      if late:
        # 1 % of the filters, another hundredth in every other call, are behind their own previous call: rewind two checkpoints, apply,
        # replay one.  (The same filters shifted in EVERY call would be late once and in order ever after.)
        self.k += 1
        tt[(self.k % 2)::100] -= 0.015
      self.f.predict_and_update_batch(tt, 1, self.z, R)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def stats(v):
  return min(v), float(np.median(v)), max(v)


say(f"# per-filter timelines, kinematic6, us per call: min / median / max of {REPS} blocks of {CALLS} calls after {WARM} warm-up calls,")
say("# the objects alternating block by block in one process.  torch = device_timeline=False (the bookkeeping in torch operations),")
say("# device = the default (batch_timeline_plan, the step, batch_timeline_push; a call with a late filter: the torch path),")
say("# device rewind = device_rewind=True (a call with a late filter: batch_rewind_locate / _fetch, mixed-kind replay).  spread = max - min of the torch row.")
say("# verdict, in-order rows: LOWER when median(device) < median(torch) - spread.  1 % late rows: NOT SLOWER when median(device) <= median(torch) + spread;")
say("# device rewind: LOWER when median(device rewind) < median(torch) - spread.")
say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
for n in (4096, 65536):
  for ring in (0, 8):
    for late in ((False, True) if ring else (False,)):
      if args.late_only and not late:
        continue
      variants = [("torch", dict(device_timeline=False), {}), ("device", {}, {})]
      if late:
        variants.append(("device rewind", dict(device_rewind=True), {}))
      if ring and not late:
        variants.append(("device, z cloned", {}, dict(timeline_plan_copies_z=False)))      # the observation kept by a clone() instead of by the plan kernel
      runs = []
      for label, kw, attrs in variants:
        s = Stream(n, ring, **kw)
        for k, v in attrs.items():
          setattr(s.f, k, v)
        s.block(WARM, False)
        if late:
          s.block(WARM, True)
        runs.append((label, s, []))
      for _ in range(REPS):
        for label, s, v in runs:
          v.append(s.block(CALLS, late))
      what = f"{n:6d} filters, ring {ring}, {'1 % late' if late else 'in order'}"
      (lo0, med0, hi0) = stats(runs[0][2])
      for label, s, v in runs:
        lo, med, hi = stats(v)
        verdict = ""
        if label != "torch":
          if label == "device rewind":
            verdict = "LOWER" if med < med0 - (hi0 - lo0) else "NOT LOWER"
          elif late:
            verdict = "NOT SLOWER" if med <= med0 + (hi0 - lo0) else "SLOWER"
          else:
            verdict = "LOWER" if med < med0 - (hi0 - lo0) else "NOT LOWER"
          verdict = f"   {verdict} ({med0 / med:.2f} x, spread {hi0 - lo0:.1f})"
        st, rw = s.f.pf_stats, s.f.rewind_stats
        served = f"   late calls: device {rw['device']:5d} torch {rw['torch']:5d}" if late else ""
        say(f"{what:42s} {label:18s} {lo:8.1f} / {med:8.1f} / {hi:8.1f}   fast {st['fast']:5d} torch {st['legacy']:5d}{served}{verdict}")
if args.out:
  with open(args.out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
