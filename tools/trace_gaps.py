"""Device idle time between the kernels of back-to-back builds, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o run -- python tools/build_only.py 10 31 20
    python tools/trace_gaps.py <dir> [builds]

Reads every *kernel_trace.csv under <dir>, takes the last `builds` (default 20) builds (a build
starts at a k_v2_hist0* kernel) and prints, per pair of consecutive kernel names, the median / min
/ max gap between one kernel's end and the next one's start, the kernels' summed medians and the
build period.  The gap after k_v2_stats is the tail between two builds.
"""
import csv
import glob
import os
import statistics
import sys


def main():
    d = sys.argv[1]
    builds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].split("(")[0].split("<")[0].split("::")[-1].strip()
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2].startswith("k_v2_hist0")]
    starts = starts[-(builds + 1):]
    gaps, durs, periods = {}, {}, []
    for a, b in zip(starts, starts[1:]):
        periods.append((rows[b][0] - rows[a][0]) / 1e3)
        for i in range(a, b):
            key = (i - a, rows[i][2], rows[i + 1][2])
            gaps.setdefault(key, []).append(max(0.0, (rows[i + 1][0] - rows[i][1]) / 1e3))
            durs.setdefault((i - a, rows[i][2]), []).append((rows[i][1] - rows[i][0]) / 1e3)
    print(f"{len(periods)} builds, {len(durs)} kernels per build")
    for (i, x, y), v in sorted(gaps.items()):
        print(f"  gap {i} {x} -> {y:<24} median {statistics.median(v):7.2f} us  "
              f"min {min(v):7.2f}  max {max(v):7.2f}")
    ksum = sum(statistics.median(v) for v in durs.values())
    gsum = sum(statistics.median(v) for v in gaps.values())
    print(f"  kernels {ksum:.2f} us  gap medians {gsum:.2f} us  period median "
          f"{statistics.median(periods):.2f} us  min {min(periods):.2f}  max {max(periods):.2f}")


if __name__ == "__main__":
    main()
