#!/usr/bin/env python3
"""How full the timed steps of a bench.py run keep the GPU, from a rocprofv3 --kernel-trace CSV (bench.py --steps K --no-verify --no-extras: the timed steps are the last
thing the run does): over the window from the first to the last G1 accumulation of the last K steps, per step (a step of 1 024 proofs is 16 passes, so 16 G1 accumulation launches) the time during which no accumulation kernel (zkc_msm_accumulate29*, G1 or
G2) is resident, the same for the G1 accumulation alone, the time with no kernel resident at all, the mean number of resident kernels (kernel time summed over the window
/ the window), and per stream (the trace's Stream_Id, or Queue_Id where it has none) the kernels and kernel time inside the window with the stream's three most frequent kernels and its
launches of a millisecond and more that are witness kernels -- which is how one sees whether a lane's stream stands still while the next step's witness chunks run.  usage: lane_streams_timeline.py <kernel_trace.csv> [timed steps K, default 3] [passes per step, default 16]"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
per_step = int(sys.argv[3]) if len(sys.argv) > 3 else 16
qcol = 'Stream_Id' if rows and 'Stream_Id' in rows[0] else 'Queue_Id'
kq = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].split('(')[0].replace('void ', '').replace('zkc::', ''), r.get(qcol, '?')) for r in rows if 'zkc' in r['Kernel_Name'])
ks = [k[:3] for k in kq]
g1 = [k for k in ks if k[2].startswith('zkc_msm_accumulate29<')]
big = sorted(g1, key=lambda k: k[1] - k[0])[len(g1) // 2]                  # a full pass' launch: key load, lone proofs and the verifier's sample launch short ones
full = [k for k in g1 if k[1] - k[0] > (big[1] - big[0]) / 4]
assert len(full) >= steps * per_step, 'fewer than %d timed steps in the trace (%d full G1 accumulations)' % (steps, len(full))
first, last = full[-steps * per_step], full[-1]
t0, t1 = first[0], last[1]


def union(iv):
    tot, cur = 0, None
    for s, e in sorted(iv):
        s, e = max(s, t0), min(e, t1)
        if e <= s:
            continue
        if cur is None or s > cur[1]:
            if cur:
                tot += cur[1] - cur[0]
            cur = [s, e]
        else:
            cur[1] = max(cur[1], e)
    return tot + (cur[1] - cur[0] if cur else 0)


win = t1 - t0
acc_all = union([(s, e) for s, e, n in ks if n.startswith('zkc_msm_accumulate29')])
acc_g1 = union([(s, e) for s, e, n in ks if n.startswith('zkc_msm_accumulate29<')])
anyk = union([(s, e) for s, e, n in ks])
busy = sum(max(0, min(e, t1) - max(s, t0)) for s, e, n in ks)
ms = lambda x: x / 1e6
print('window: %d steps of %d passes, %.3f ms (%.3f ms per step, from the first G1 accumulation of the first of them to the end of the last; %d full G1 accumulations in the trace)' % (steps, per_step, ms(win), ms(win) / steps, len(full)))
print('no accumulation kernel (G1 or G2) resident: %.3f ms per step (%.1f %% of the window)' % (ms(win - acc_all) / steps, 100.0 * (win - acc_all) / win))
print('no G1 accumulation resident:                %.3f ms per step (%.1f %%)' % (ms(win - acc_g1) / steps, 100.0 * (win - acc_g1) / win))
print('no kernel resident at all:                  %.3f ms per step (%.1f %%)' % (ms(win - anyk) / steps, 100.0 * (win - anyk) / win))
print('mean number of resident kernels:            %.2f' % (busy / win))
import collections
by = collections.defaultdict(list)
for s, e, n, q in kq:
    if e > t0 and s < t1:
        by[q].append((s, e, n))
print('per stream (%s) inside the window:' % qcol)
for q, l in sorted(by.items(), key=lambda kv: -sum(e - s for s, e, n in kv[1])):
    top = ', '.join('%s x %d' % (n[:28], c) for n, c in collections.Counter(n for s, e, n in l).most_common(3))
    print('  stream %-4s %5d kernels  %8.1f ms of kernels  (%s)' % (q, len(l), ms(sum(min(e, t1) - max(s, t0) for s, e, n in l)), top))
    for s, e, n in l:
        if 'witness' in n and e - s >= 1e6:
            print('      %9.2f ms  +%6.2f ms  %s' % (ms(s - t0), ms(e - s), n[:40]))
