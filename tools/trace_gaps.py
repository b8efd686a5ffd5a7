"""Joints of the pipelined encode from a rocprofv3 kernel trace of bench.py:
python tools/trace_gaps.py run_kernel_trace.csv [launches per call]

Groups the k_lz4_encode launches into calls (a k_idx_exits launch ends one) and
prints, per call and as medians: the summed idle time between the end of one
parse and the start of the next (negative parts, i.e. overlap, are reported
apart), the time from the last parse's end to k_idx_exits' start, whether launch
i+1 starts before launch i ends, whether launches 0 and 1 start together, and
the queues the kernels ran on."""
import csv
import statistics
import sys

rows = []
with open(sys.argv[1], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"]))
rows.sort()
print("kernel launches in the run: %d" % len(rows))

queues = {}
for s, e, name, q in rows:
    short = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("bshuf::", "")
    short = short.split("(")[0].split("<")[0]
    queues.setdefault(short, set()).add(q)
for k in sorted(queues):
    print("queue(s) of %-28s %s" % (k, " ".join(sorted(queues[k]))))

calls, cur = [], []
for s, e, name, q in rows:
    if "k_lz4_encode" in name:
        cur.append((s, e))
    elif "k_idx_exits" in name and cur:
        calls.append((cur, s))
        cur = []
want = int(sys.argv[2]) if len(sys.argv) > 2 else 0
idle, over, tail, span, par, dur = [], [], [], [], [], []
for i, (p, idx) in enumerate(calls):
    if want and len(p) != want:
        continue
    end = p[0][1]
    gi = go = 0.0
    started_early = 0
    for s, e in p[1:]:
        g = (s - end) / 1e3
        if g >= 0:
            gi += g
        else:
            go -= g
            started_early += 1
        end = max(end, e)
    idle.append(gi)
    over.append(go)
    tail.append((idx - end) / 1e3)
    span.append((end - p[0][0]) / 1e3)
    par.append(started_early)
    dur.append(sum(e - s for s, e in p) / 1e3 / len(p))
    first = (p[1][0] - p[0][0]) / 1e3 if len(p) > 1 else 0.0
    print("call %3d: %2d parses, idle between %7.1f us, overlapped %8.1f us, launches starting before "
          "the previous ended %d, launch 1 starts %7.1f us after launch 0, first start to last end "
          "%8.1f us, last parse end to k_idx_exits %6.1f us" % (i, len(p), gi, go, started_early, first,
                                                             span[-1], tail[-1]))
if idle:
    med = statistics.median
    print("medians over %d calls: idle between parses %.1f us, overlapped %.1f us, early starts %g, "
          "parse span %.1f us, mean parse duration %.1f us, last parse end to k_idx_exits %.1f us" % (
              len(idle), med(idle), med(over), med(par), med(span), med(dur), med(tail)))
