"""Where the run-ahead temporal stack sits relative to the persistent perception launches, step by step, from a kernel trace of
tools/faithful_only.py:
  ADX_RESNET_STREAMS=1 rocprofv3 --kernel-trace --output-format csv -d profile_out/walk_trace -- python3 tools/faithful_only.py
  python3 tools/walk_trace.py profile_out/walk_trace
A step runs from one stem launch to the next.  Launches are `persistent` (conv2d_hs3x3q_kernel), other perception launches
(conv2d / pool / fc kernels) and `other` (the temporal stack, the embedding, the scheduler step).  Per step: its length, the span
from the first to the last `other` launch, their summed run time, how many of them STARTED while a persistent launch was in flight
and how long they waited behind their predecessor on average (gap), and the tail: time from the last perception launch's end to
the step's end.  Then the same averaged over the faster and the slower half of the steps."""
import csv
import glob
import os
import sys


def rows(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not f:
        sys.exit(f"no *kernel_trace.csv under {d}")
    out = []
    for r in csv.DictReader(open(f[-1])):
        out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    return sorted(out)


def kind(name):
    if "conv2d_hs3x3q_kernel" in name:
        return "persistent"
    if any(k in name for k in ("conv2d", "maxpool", "avgpool", "stem")):
        return "perception"
    return "other"


def main(d):
    ks = rows(d)
    stems = [i for i, k in enumerate(ks) if "stem" in k[2]]
    steps = []
    for a, b in zip(stems[:-1], stems[1:]):
        seg = ks[a:b]
        t0, t1 = seg[0][0], ks[b][0]
        pers = [(s, e) for s, e, n in seg if kind(n) == "persistent"]
        perc_end = max(e for s, e, n in seg if kind(n) != "other")
        oth = [(s, e) for s, e, n in seg if kind(n) == "other"]
        if not oth or not pers:
            continue
        inflight = sum(1 for s, _ in oth if any(ps <= s < pe for ps, pe in pers))
        gaps = [max(0, oth[i + 1][0] - oth[i][1]) for i in range(len(oth) - 1)]
        steps.append(dict(len=(t1 - t0) / 1e3, span=(oth[-1][1] - oth[0][0]) / 1e3, run=sum(e - s for s, e in oth) / 1e3, n=len(oth),
                          inflight=inflight, gap=sum(gaps) / max(1, len(gaps)) / 1e3, tail=(t1 - perc_end) / 1e3,
                          pers=sum(e - s for s, e in pers) / 1e3, last_other_after=(oth[-1][1] - perc_end) / 1e3))
    steps = steps[3:]          # warm-up
    cols = ("len", "pers", "span", "run", "n", "inflight", "gap", "tail", "last_other_after")
    print("step " + " ".join(f"{c:>16s}" for c in cols) + "   (us)")
    for i, s in enumerate(steps):
        print(f"{i:4d} " + " ".join(f"{s[c]:16.1f}" for c in cols))
    order = sorted(steps, key=lambda s: s["len"])
    half = len(order) // 2
    for name, grp in (("faster half", order[:half]), ("slower half", order[half:])):
        if grp:
            print(f"{name:11s} " + " ".join(f"{c}={sum(s[c] for s in grp) / len(grp):.1f}" for c in cols))


if __name__ == "__main__":
    main(sys.argv[1])
