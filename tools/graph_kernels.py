"""The per-position table of ONE graph replayed by itself under rocprofv3 --kernel-trace (tools/graph_replay.py): per position of the graph
the median over replays [skip, n) of the kernel's start (us from the replay's first kernel), its own time, the distance to the next kernel's
start and the spread of its own time; then kernel, grid, workgroup.  A replay starts at the kernel named by --first (default k_merge_ticks,
the lidar graph's first launch).

    rocprofv3 --kernel-trace --output-format csv -d /tmp/gt -- python tools/graph_replay.py lidar 12
    python tools/graph_kernels.py /tmp/gt [--last 12] [--skip 3] [--first k_merge_ticks]"""
import argparse
import csv
import glob
import os
import re
import statistics

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--last", type=int, default=12, help="the table covers the last LAST replays of the trace (the ones graph_replay.py made)")
ap.add_argument("--skip", type=int, default=3, help="of those, the first SKIP are left out")
ap.add_argument("--first", default="k_merge_ticks")
a = ap.parse_args()
rows = []
for f in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
sh = lambda n: re.sub(r"\((anonymous namespace)::", "(", n.replace("(anonymous namespace)::", "").replace("void ", ""))[:110]
starts = [i for i, r in enumerate(rows) if a.first in r["Kernel_Name"]]
bounds = starts[-a.last:] + [len(rows)]
replays = [rows[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:])][a.skip:]
n = min(len(r) for r in replays)
if any(len(r) != n or [x["Kernel_Name"] for x in r] != [x["Kernel_Name"] for x in replays[0]] for r in replays):
    print(f"# replays differ in their launches: {[len(r) for r in replays]} (the first {n} positions are tabulated)")
S, E = (lambda r: int(r["Start_Timestamp"])), (lambda r: int(r["End_Timestamp"]))
tot = [(E(r[n - 1]) - S(r[0])) / 1e3 for r in replays]
print(f"== {n} launches, first start to last end median {statistics.median(tot):.1f} us (min {min(tot):.1f}, max {max(tot):.1f}) over {len(replays)} replays")
print("start_us  kernel_us  to_next_start_us  spread(kernel_us)  kernel  grid  wg")
k = rows[0].keys()
get = lambda r, *names: next((r[x] for x in names if x in k), "")
for p in range(n):
    st = statistics.median((S(r[p]) - S(r[0])) / 1e3 for r in replays)
    own = [(E(r[p]) - S(r[p])) / 1e3 for r in replays]
    nxt = statistics.median((S(r[p + 1]) - S(r[p])) / 1e3 for r in replays) if p + 1 < n else float("nan")
    r0 = replays[0][p]
    print(f"{st:8.1f}  {statistics.median(own):8.1f}  {nxt:8.1f}  {min(own):6.1f}-{max(own):<6.1f}  {sh(r0['Kernel_Name'])}  {get(r0, 'Grid_Size_X', 'Grid_Size')}  {get(r0, 'Workgroup_Size_X', 'Workgroup_Size')}")
