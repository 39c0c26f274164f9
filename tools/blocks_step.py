"""The block pass (kmhg_rows_blocks) timed beside the segment pass it extends (kmhg_rows_segments)
on ONE GPU (tools, not product).

snv_diverged  config 5 at 10 Mbp: the index holds A (i.i.d.), the query is B = synth.derived(A)
              -- A with 1 % SNVs plus inversions and translocations -- at k = 31.  Many segments,
              few blocks: every isolated substitution cuts a diagonal for k windows, which
              max_gap = k bridges.
repeat_rich   the 2 Mbp sequence of config 4's generator (synth.config4), k = 31, self query, as
              tools/segments_step.py times it.
Per case: the rows, the segments and the blocks at max_gap = k (and at min_len = 2), the two
entries' ms -- alternated step by step in one process on the same rows, each timed with HIP
events on the stream it runs on and ending in its own synchronize; medians, interquartile
spreads (q3 - q1) and minima over the steps after a warm-up -- their ratio, and the split between
the kernels of the block pass (the library's per-kernel event timing, in a separate set of
passes).

    python tools/blocks_step.py [out.json] [steps] [warmup]
"""
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
    from kmer_hasher_amd import device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "blocks_step.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    k = 31

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def kernel_split(fn):
        device.timing_enable(True)
        device.timing_reset()
        for _ in range(steps):
            fn()
        split = {kn: round(v[1] / steps, 4) for kn, v in device.timing_report().items() if v[0]}
        device.timing_enable(False)
        return split

    def case(index_seq, query_seq):
        idx = DeviceIndex.build(index_seq, k).wait()
        q = idx.query(query_seq, k)
        rows = q.rows_view()
        c = {"index_L": int(index_seq.numel()), "query_L": int(query_seq.numel()),
             "rows": int(rows.shape[0])}
        ts, tb, tb2 = [], [], []
        for it in range(warmup + steps):
            t, g = timed(lambda: device.rows_segments(rows))
            c["segments"] = int(g.shape[0])
            del g
            u, b = timed(lambda: device.rows_blocks(rows, k))
            c["blocks"] = int(b.shape[0])
            c["longest_span"] = int(b[:, 2].max())
            del b
            v, b = timed(lambda: device.rows_blocks(rows, k, 2))
            c["blocks_min_len_2"] = int(b.shape[0])
            del b
            if it >= warmup:
                ts.append(t)
                tb.append(u)
                tb2.append(v)
        c["rows_segments_ms"] = stats(ts)
        c["rows_blocks_ms"] = stats(tb)
        c["rows_blocks_min_len_2_ms"] = stats(tb2)
        c["ratio_blocks_to_segments"] = round(
            c["rows_blocks_ms"]["median"] / c["rows_segments_ms"]["median"], 4)
        c["ratio_blocks_min_len_2_to_segments"] = round(
            c["rows_blocks_min_len_2_ms"]["median"] / c["rows_segments_ms"]["median"], 4)
        c["segments_kernel_ms_per_pass"] = kernel_split(lambda: device.rows_segments(rows))
        c["blocks_kernel_ms_per_pass"] = kernel_split(lambda: device.rows_blocks(rows, k))
        c["blocks_min_len_2_kernel_ms_per_pass"] = kernel_split(
            lambda: device.rows_blocks(rows, k, 2))
        del rows
        q.free()
        idx.free()
        return c

    report = {"k": k, "max_gap": k, "steps": steps, "warmup": warmup,
              "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per entry; entries alternated step by step in one "
                      "process; median, interquartile spread (q3 - q1) and minimum over the steps"}
    A = synth.iid(10_000_000, 1)
    B = synth.derived(A, 5)
    report["snv_diverged"] = case(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev))
    print("snv_diverged", json.dumps(report["snv_diverged"]), flush=True)
    del A, B
    R = torch.from_numpy(synth.config4(2_000_000, 3)).to(dev)
    report["repeat_rich_self"] = case(R, R)
    print("repeat_rich", json.dumps(report["repeat_rich_self"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
