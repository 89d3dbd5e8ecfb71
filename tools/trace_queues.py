"""Which hardware queue every role of every pipeline ran on, from a rocprofv3 kernel trace of a bench run (tools/trace_overlap.sh leaves one):
    python tools/trace_queues.py <kernel_trace.csv>
A pipeline is a submitting host thread (bench.py drives every detector from a thread of its own), a role is the stream of the sweep a
kernel belongs to -- known from its name.  Prints, over the busiest contiguous stretch of the trace (the timed region), the queue(s) per
(pipeline, role), per queue the roles that share it, and per kernel of the main chain how long it waited behind its predecessor of the
same batch (start - predecessor's end: the queueing delay of a launch under load) beside its duration."""
import csv
import sys
from collections import defaultdict

ROLE = {"candidate_compact_kernel": "corners", "line_setup_listed_kernel": "crowded", "gather_ranges_kernel": "ties", "gather_corners_kernel": "ties",
        "gather_columns_kernel": "ties"}
CHAIN = ["multi_copy_kernel", "line_classify_kernel", "line_setup_small_kernel", "vp3_support_kernel", "vp_support_kernel", "score_kernel", "rank_wave_kernel",
         "record_kernel"]


def short(name):
    n = name.split("(")[0].split("<")[0]
    return n.split("::")[-1].replace("void ", "").strip()


rows = []
rd = csv.DictReader(open(sys.argv[1]))
have_stream = "Stream_Id" in (rd.fieldnames or [])
for r in rd:
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r["Queue_Id"], r.get("Thread_Id", "?"), r.get("Stream_Id", "?"),
                 int(r.get("Dispatch_Id", 0))))
if not rows:
    sys.exit("%s: no kernel launches in this trace" % sys.argv[1])
rows.sort()
groups, cur = [], [rows[0]]
for a in rows[1:]:
    if a[0] - max(x[1] for x in cur[-50:]) > 5_000_000:
        groups.append(cur); cur = []
    cur.append(a)
groups.append(cur)
g = max(groups, key=len)
threads = sorted({r[4] for r in g if r[2] == "score_kernel"})
tname = {t: "P%d" % i for i, t in enumerate(threads)}
print("timed region: %d launches, %d pipelines (submitting threads), queues seen: %s%s" % (len(g), len(threads), " ".join(sorted({r[3] for r in g})),
                                                                                         "" if have_stream else "  (no Stream_Id column in this trace)"))
where = defaultdict(lambda: defaultdict(int))      # (pipeline, role) -> queue -> launches
streams = defaultdict(set)
per_queue = defaultdict(lambda: defaultdict(int))
for s, e, n, q, t, sid, _ in g:
    role = ROLE.get(n, "main" if n in CHAIN else "other:" + n)
    where[(tname.get(t, "T" + t), role)][q] += 1
    streams[(tname.get(t, "T" + t), role)].add(sid)
    per_queue[q][(tname.get(t, "T" + t), role)] += 1
print("pipeline role      -> queue (launches)   [stream ids]")
for k in sorted(where):
    print("  %-4s %-10s -> %s   [%s]" % (k[0], k[1], "  ".join("q%s (%d)" % (q, c) for q, c in sorted(where[k].items())), " ".join(sorted(streams[k]))))
print("queue -> what shares it")
for q in sorted(per_queue):
    print("  q%-3s %s" % (q, "  ".join("%s/%s" % k for k in sorted(per_queue[q]))))
# queueing delay along a batch's main chain: the launches of one thread in dispatch order, a chain starts at a line_classify_kernel
wait, dur = defaultdict(list), defaultdict(list)
for t in threads:
    mine = sorted((r for r in g if r[4] == t and r[2] in CHAIN and r[2] != "multi_copy_kernel"), key=lambda r: r[6])
    prev = None
    for r in mine:
        if r[2] == "line_classify_kernel":
            prev = None
        if prev is not None:
            wait[r[2]].append(max(0, r[0] - prev[1]) / 1e3)
        dur[r[2]].append((r[1] - r[0]) / 1e3)
        prev = r
print("main chain under load: mean wait behind the batch's previous kernel / mean duration (us)")
for n in CHAIN:
    if dur[n]:
        w = wait[n]
        print("  %-26s wait %7.1f   dur %7.1f   (%d)" % (n, sum(w) / len(w) if w else 0.0, sum(dur[n]) / len(dur[n]), len(dur[n])))
