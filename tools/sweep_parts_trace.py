"""What the tiles_* kernels of a bench run did in time, from a rocprofv3 kernel trace (profiles/r10_kernel_trace_sweep_parts.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python bench.py --gpus 1 --steps K --warmup W --replicas R
    python tools/sweep_parts_trace.py DIR K

Per queue (= sweep part) the launches are cut into sweeps at tiles_stats_kernel.  Printed: the time from the first to the last kernel
of the last K sweeps; for the middle one of them, per queue, launches, kernel time, span, summed gaps, launches under 10 us, time per
kernel; and, with several queues, how much of a part's tree-pass and reduction kernel time (and of its branch kernel) lies inside the
intervals of the other parts' tiles_branch_kernel, by timestamps."""
import csv, glob, sys, collections
d, K = sys.argv[1], int(sys.argv[2])
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
rows = []
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"]
    if "tiles_" not in n:
        continue
    short = n.split("tiles_")[1].split("<")[0].split("(")[0]
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short, r.get("Queue_Id", "0")))
rows.sort()
queues = sorted({q for *_, q in rows})
print("file", f, "tiles launches", len(rows), "queues", queues)
byq = {q: [x for x in rows if x[3] == q] for q in queues}
# sweeps of a queue end with its stats kernel
sweeps = {}
for q, rs in byq.items():
    cur, out = [], []
    for x in rs:
        cur.append(x)
        if x[2].startswith("stats"):
            out.append(cur); cur = []
    sweeps[q] = out
    print("queue", q, "sweeps", len(out), "launches per sweep", len(out[-1]) if out else 0)
nsw = min(len(v) for v in sweeps.values())
first = min(sweeps[q][nsw - K][0][0] for q in queues)
last = max(sweeps[q][nsw - 1][-1][1] for q in queues)
print("wall of the last %d sweeps, first kernel start to last kernel end: %.3f ms = %.3f ms per sweep" % (K, (last - first) / 1e6, (last - first) / 1e6 / K))
mid = nsw - K // 2
for q in queues:
    sw = sweeps[q][mid]
    dur = [e - s for s, e, *_ in sw]
    gaps = [sw[i + 1][0] - sw[i][1] for i in range(len(sw) - 1)]
    small = [x for x in dur if x < 10000]
    per = collections.defaultdict(float)
    for (s, e, n, _) in sw:
        per[n] += (e - s) / 1e6
    print("queue %s sweep %d: %d launches, busy %.3f ms, span %.3f ms, summed gaps %.3f ms (max %.1f us), launches under 10 us: %d taking %.3f ms"
          % (q, mid, len(sw), sum(dur) / 1e6, (sw[-1][1] - sw[0][0]) / 1e6, sum(gaps) / 1e6, max(gaps) / 1e3, len(small), sum(small) / 1e6))
    print("   per kernel ms:", {k: round(v, 3) for k, v in per.items()})
    others = [(s, e) for qq in queues if qq != q for (s, e, n, _) in byq[qq] if n.startswith("branch")]
    if others:
        def ov(s, e):
            return sum(max(0, min(e, b) - max(s, a)) for a, b in others)
        tree = [(s, e, n) for (s, e, n, _) in sw if not n.startswith("branch")]
        tt = sum(e - s for s, e, _ in tree); to = sum(ov(s, e) for s, e, _ in tree)
        nar = [(s, e) for s, e, _ in tree if e - s < 10000]
        print("   tree passes + reductions: %.3f ms of kernel time, %.3f ms of it while another part's branch kernel runs; launches under 10 us: %.3f of %.3f ms"
              % (tt / 1e6, to / 1e6, sum(ov(s, e) for s, e in nar) / 1e6, sum(e - s for s, e in nar) / 1e6))
        b = [(s, e) for (s, e, n, _) in sw if n.startswith("branch")][0]
        print("   this part's branch kernel: %.3f ms, %.3f ms of it beside another part's branch kernel" % ((b[1] - b[0]) / 1e6, ov(*b) / 1e6))
