#!/usr/bin/env python3
"""Timeline of a rocprofv3 --kernel-trace CSV: for a window of dispatches in the steady state, each kernel's start and
end relative to the first one, its stream/queue, and how much of it overlapped the covariance downdate (P-GEMM); then, over everything after the skipped part, the duration
statistics per kernel and the P-GEMM's start-to-start period.
A trace without a P-GEMM (the particle filter's) names the kernel its window starts at and whose start-to-start period is
the step: e.g. `pf_resample_plan` -- the copy command of a step shows as its blit kernel, or as the gap it leaves.
Usage: python tools/trace_timeline.py <kernel_trace.csv> [skip_fraction=0.5] [count=40] [anchor=downdate]
       python tools/trace_timeline.py <kernel_trace.csv> --sequence
--sequence prints the whole trace as its launch sequence alone -- kernel name, grid (in threads) and queue (numbered
by first appearance) in start order, no times -- so that two runs of the same program can be compared line for line
(profiles/r07_launch_sequence_*.txt, profiles/r10_pf_launch_sequence_*.txt)."""
import csv
import sys


def short(name):
    n = name.split("(")[0]
    for pre in ("void cslam::", "cslam::", "void "):
        if n.startswith(pre):
            n = n[len(pre):]
    return n[:44]


def sequence(rows):
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    queues = {}
    print(f"{'kernel':70s} {'grid':>18s} queue")
    for r in rows:
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        q = queues.setdefault(r.get("Queue_Id", ""), len(queues) + 1)
        print(f"{r['Kernel_Name'][:70]:70s} {grid:>18s} {q}")


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    if "--sequence" in sys.argv[2:]:
        return sequence(rows)
    skip = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    anchor = sys.argv[4] if len(sys.argv) > 4 else "downdate"
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    i0 = int(len(rows) * skip)
    # start the window at a P-GEMM (or at the named kernel)
    while i0 < len(rows) and anchor not in rows[i0]["Kernel_Name"]:
        i0 += 1
    win = rows[i0:i0 + count]
    if not win:
        print("no rows")
        return
    t0 = int(win[0]["Start_Timestamp"])
    dd = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in win if "downdate" in r["Kernel_Name"]]
    qkey = "Queue_Id" if "Queue_Id" in win[0] else ("Stream_Id" if "Stream_Id" in win[0] else None)
    print(f"{'kernel':44s} {'queue':>6s} {'start_us':>9s} {'end_us':>9s} {'dur_us':>8s} {'under P-GEMM':>12s}")
    for r in win:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        ov = 0
        if "downdate" not in r["Kernel_Name"]:
            for a, b in dd:
                ov += max(0, min(e, b) - max(s, a))
        q = r.get(qkey, "") if qkey else ""
        print(f"{short(r['Kernel_Name']):44s} {q:>6s} {(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f} "
              f"{(100.0 * ov / max(e - s, 1)):11.0f}%")
    if len(dd) >= 2:
        per = (dd[-1][0] - dd[0][0]) / (len(dd) - 1) / 1e3
        busy = sum(b - a for a, b in dd[:-1]) / (len(dd) - 1) / 1e3
        print(f"P-GEMM period {per:.1f} us, P-GEMM busy {busy:.1f} us per period ({100 * busy / per:.0f} %)")
    stats(rows, int(len(rows) * skip), skip)
    if anchor != "downdate":
        st = [int(r["Start_Timestamp"]) for r in rows[int(len(rows) * skip):] if anchor in r["Kernel_Name"]]
        per = [(b - a) / 1e3 for a, b in zip(st, st[1:])]
        if per:
            print(f"  {anchor} start to start: n={len(per)} median {quantile(per, 0.5):.1f} us, quartiles "
                  f"[{quantile(per, 0.25):.1f}, {quantile(per, 0.5):.1f}, {quantile(per, 0.75):.1f}]")


def quantile(v, q):
    """linear interpolation between order statistics (numpy's default)"""
    v = sorted(v)
    x = q * (len(v) - 1)
    lo = int(x)
    hi = min(lo + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (x - lo)


def stats(rows, i0, skip):
    rest = rows[i0:]
    print(f"\nafter the first {skip:g} of the trace: {len(rest)} dispatches")
    dur = {}
    for r in rest:
        dur.setdefault(short(r["Kernel_Name"])[:40], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        print(f"  {k:40s} n={len(v):5d} median {quantile(v, 0.5):7.1f} min {min(v):7.1f} max {max(v):7.1f} us")
    # (the k = 128 flushes of the steady state: the dominant instantiation of the downdate kernel)
    names = [r["Kernel_Name"] for r in rest if "downdate" in r["Kernel_Name"]]
    if names:
        main_name = max(set(names), key=names.count)
        st = [int(r["Start_Timestamp"]) for r in rest if r["Kernel_Name"] == main_name]
        per = [(b - a) / 1e3 for a, b in zip(st, st[1:])]
        if per:
            print(f"  P-GEMM start to start: n={len(per)} median {quantile(per, 0.5):.1f} us, quartiles "
                  f"[{quantile(per, 0.25):.1f}, {quantile(per, 0.5):.1f}, {quantile(per, 0.75):.1f}]")
    count = lambda key: sum(1 for r in rows if key in r["Kernel_Name"])
    print(f"  in the whole trace: rows kernels {count('ekf_la_rows_kernel')}, blocks kernels {count('ekf_la_blocks')}, "
          f"wide kernels {count('ekf_la_wide')}, stage kernels {count('ekf_stage_obs')}")


if __name__ == "__main__":
    main()
