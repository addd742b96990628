#!/usr/bin/env python3
"""What one Adam step of the PPO update pays outside K7, from a rocprofv3 kernel trace.
python scripts/step_distance.py <kernel_trace.csv>
For every pair of consecutive launches of an Adam step's first kernel (rs_ppo_grad2_pair_kernel, or rs_ppo_grad2_kernel<8> where
the networks have a launch each) that belong to one update (start-to-start under 5 ms): the start-to-start distance, the duration
of the K7 kernel(s), and the rest (the kernels behind K7 and every gap).  Steps after a KL
early stop (K7 returns at once) are left out.  Medians."""
import csv
import sys

rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(sys.argv[1])))
FIRST = ("rs_ppo_grad2_kernel<8>", "rs_ppo_grad2_pair_kernel")
act = [i for i, r in enumerate(rows) if any(f in r[2] for f in FIRST)]
dist, k7, rest, tail = [], [], [], []
for a, b in zip(act, act[1:]):
    d = rows[b][0] - rows[a][0]
    mid = rows[a:b]
    t_k7 = sum(e - s for s, e, n in mid if "rs_ppo_grad2_" in n)
    if d > 5_000_000 or t_k7 < 200_000:
        continue
    dist.append(d / 1e3); k7.append(t_k7 / 1e3); rest.append((d - t_k7) / 1e3)
    tail.append(sum(e - s for s, e, n in mid if "rs_ppo_grad2_" not in n) / 1e3)
med = lambda v: sorted(v)[len(v) // 2]
print(f"{len(dist)} Adam steps: start-to-start {med(dist):.1f} us, K7 actor + critic {med(k7):.1f} us, outside K7 {med(rest):.1f} us "
      f"(of which kernels {med(tail):.1f} us, gaps {med(rest) - med(tail):.1f} us; min {min(rest):.1f}, max {max(rest):.1f})")
names = {}
for a, b in zip(act, act[1:]):
    for s, e, n in rows[a + 1:b]:
        if not any(f in n for f in FIRST) and rows[b][0] - rows[a][0] < 5_000_000:
            names.setdefault(n.split("(")[0][:60], []).append((e - s) / 1e3)
for n, v in names.items():
    print(f"   {n:60s} {len(v):6d} launches, median {med(v):8.1f} us")
