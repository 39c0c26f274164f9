"""The diagonal-segment pass (kmhg_rows_segments) timed on ONE GPU (tools, not product).

config2      config 2's self query (10 Mbp i.i.d., k = 31): ~10 M rows, one segment.  The pass
             beside kmhg_rows_runs (count + emit into a buffer) on the same rows, alternating in
             one process.  Expectation: parity within the baseline's own interquartile spread.
repeat_rich  a 2 Mbp sequence of config 4's generator (synth.config4), k = 31, self query: no
             baseline.  Rows, segments, ms per pass, the split between the pass's kernels (the
             library's per-kernel event timing, in a separate set of passes), the share of rows
             whose classification went past the neighbour row into the search, and the time of
             the query that made the rows.
Every leg is timed with HIP events on the stream it runs on and ends in the entry's own
synchronize; medians and interquartile spreads (q3 - q1) over the steps after a warm-up.

    python tools/segments_step.py [out.json] [steps] [warmup]

With KMHG_LIB_VARIANT naming a build that predates the segments entries (the parent commit's
library), only the kmhg_rows_runs leg runs: the baseline at that commit, in the same harness.
"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return {"median": round(q[1], 4), "iqr": round(q[2] - q[0], 4), "min": round(min(v), 4)}


def main():
    import torch
    from kmer_hasher_amd import _lib, device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "segments_step.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    have_segs = hasattr(L, "kmhg_rows_segments")
    k = 31

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def runs_leg(rows, buf):
        n = C.c_int64()
        _lib.check(L.kmhg_rows_runs(C.c_void_p(rows.data_ptr()), rows.shape[0],
                                    C.c_void_p(buf.data_ptr()), buf.shape[0], C.byref(n),
                                    device._stream_ptr()))
        return n.value

    report = {"k": k, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "library": os.environ.get("KMHG_LIB_VARIANT", "this commit"),
              "note": "ms; HIP-event timing per leg; legs alternated step by step in one process; "
                      "median, interquartile spread (q3 - q1) and minimum over the steps"}

    # ---------------------------------------------------------------- config 2, self
    A = torch.from_numpy(synth.iid(10_000_000, 1)).to(dev)
    idx = DeviceIndex.build(A, k).wait()
    tq, q = timed(lambda: idx.query(A, k))
    rows = q.rows_view()
    buf = torch.empty((max(rows.shape[0] // 16, 1), 3), dtype=torch.int32, device=dev)
    n_runs = runs_leg(rows, buf)
    c2 = {"rows": int(rows.shape[0]), "runs": int(n_runs), "query_ms_once": round(tq, 4)}
    tr, ts = [], []
    for it in range(warmup + steps):
        t, _ = timed(lambda: runs_leg(rows, buf))
        if it >= warmup:
            tr.append(t)
        if have_segs:
            t, g = timed(lambda: device.rows_segments(rows))
            if it >= warmup:
                ts.append(t)
            c2["segments"] = int(g.shape[0])
            del g
    c2["rows_runs_ms"] = stats(tr)
    if have_segs:
        c2["rows_segments_ms"] = stats(ts)
        ratio = c2["rows_segments_ms"]["median"] / c2["rows_runs_ms"]["median"]
        c2["ratio_segments_to_runs"] = round(ratio, 4)
        c2["within_baseline_spread"] = bool(
            abs(c2["rows_segments_ms"]["median"] - c2["rows_runs_ms"]["median"])
            <= c2["rows_runs_ms"]["iqr"])
        device.timing_enable(True)
        device.timing_reset()
        for _ in range(steps):
            device.rows_segments(rows)
        c2["kernel_ms_per_pass"] = {
            kn: round(v[1] / steps, 4) for kn, v in device.timing_report().items() if v[0]}
        device.timing_enable(False)
    print("config2", json.dumps(c2), flush=True)
    report["config2_self"] = c2
    del rows, buf
    q.free()
    idx.free()
    del A

    # ---------------------------------------------------------------- repeat-rich, self
    if have_segs:
        B = torch.from_numpy(synth.config4(2_000_000, 3)).to(dev)
        idx = DeviceIndex.build(B, k).wait()
        for _ in range(2):
            idx.query(B, k).free()
        tqs = []
        for _ in range(5):
            t, q = timed(lambda: idx.query(B, k))
            tqs.append(t)
            q.free()
        q = idx.query(B, k)
        rows = q.rows_view()
        H = rows.shape[0]
        # rows whose start (end) lookup went past the neighbour row: the wanted row exists in
        # principle (no zero coordinate) and the row before (after) lies above (below) it
        key = (rows[:, 0].to(torch.int64) << 32) | rows[:, 1].to(torch.int64)
        back = torch.zeros(H, dtype=torch.bool, device=dev)
        back[1:] = (key[:-1] > key[1:] - ((1 << 32) + 1)) & (rows[1:, 0] > 1) & (rows[1:, 1] > 1)
        fwd = torch.zeros(H, dtype=torch.bool, device=dev)
        fwd[:-1] = key[1:] < key[:-1] + ((1 << 32) + 1)
        rr = {"L": int(B.numel()), "rows": int(H), "query_ms": stats(tqs),
              "searched_rows_share": {"start": round(float(back.float().mean()), 4),
                                      "end": round(float(fwd.float().mean()), 4),
                                      "either": round(float((back | fwd).float().mean()), 4)}}
        del key, back, fwd
        ts = []
        for it in range(warmup + steps):
            t, g = timed(lambda: device.rows_segments(rows))
            if it >= warmup:
                ts.append(t)
            rr["segments"] = int(g.shape[0])
            rr["longest"] = int(g[:, 2].max())
            del g
        rr["rows_segments_ms"] = stats(ts)
        device.timing_enable(True)
        device.timing_reset()
        for _ in range(steps):
            device.rows_segments(rows)
        rr["kernel_ms_per_pass"] = {
            kn: round(v[1] / steps, 4) for kn, v in device.timing_report().items() if v[0]}
        device.timing_enable(False)
        t16, g16 = timed(lambda: device.rows_segments(rows, 16))
        rr["min_len_16"] = {"segments": int(g16.shape[0]), "ms_once": round(t16, 4)}
        print("repeat_rich", json.dumps(rr), flush=True)
        report["repeat_rich_self"] = rr
        del rows
        q.free()
        idx.free()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
