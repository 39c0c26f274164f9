"""The chain pass (kmhg_blocks_chains) timed beside the block pass it follows (kmhg_rows_blocks) on
ONE GPU (tools, not product).

snv_diverged  config 5 at 10 Mbp: the index holds A (i.i.d.), the query is B = synth.derived(A)
              -- A with 1 % SNVs plus inversions and translocations -- at k = 31.  Few blocks
              (about ten thousand): the chain passes are launch-bound.
repeat_rich   the 2 Mbp sequence of config 4's generator (synth.config4), k = 31, self query:
              about half a million blocks, whose candidate windows hold hundreds of blocks.
Both are tools/blocks_step.py's inputs.  Per case: the rows, the blocks at max_gap = k and the
chains at the default parameters (max_dist = 5000, max_drift = 500, min_hits = 1), the two
entries' ms -- alternated step by step in one process on the same rows and blocks, each timed with
HIP events on the stream it runs on and ending in its own synchronize; medians, interquartile
spreads (q3 - q1) and minima over the steps after a warm-up -- their ratio, and the split between
the kernels of each (the library's per-kernel event timing, in a separate set of passes).

    python tools/chains_step.py [out.json] [steps] [warmup]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_DIST, MAX_DRIFT = 5000, 500


def stats(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return {"median": round(q[1], 4), "iqr": round(q[2] - q[0], 4), "min": round(min(v), 4)}


def main():
    import torch
    from kmer_hasher_amd import device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "chains_step.json")
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
        blocks = device.rows_blocks(rows, k)
        c = {"index_L": int(index_seq.numel()), "query_L": int(query_seq.numel()),
             "rows": int(rows.shape[0]), "blocks": int(blocks.shape[0])}
        tb, tc = [], []
        for it in range(warmup + steps):
            u, b = timed(lambda: device.rows_blocks(rows, k))
            del b
            v, (chains, member) = timed(
                lambda: device.blocks_chains(blocks, MAX_DIST, MAX_DRIFT))
            c["chains"] = int(chains.shape[0])
            c["longest_chain_blocks"] = int(chains[:, 5].max())
            c["largest_chain_hits"] = int(chains[:, 4].max())
            c["chains_of_one_block"] = int((chains[:, 5] == 1).sum())
            del chains, member
            if it >= warmup:
                tb.append(u)
                tc.append(v)
        c["rows_blocks_ms"] = stats(tb)
        c["blocks_chains_ms"] = stats(tc)
        c["ratio_chains_to_blocks"] = round(
            c["blocks_chains_ms"]["median"] / c["rows_blocks_ms"]["median"], 4)
        c["blocks_kernel_ms_per_pass"] = kernel_split(lambda: device.rows_blocks(rows, k))
        c["chains_kernel_ms_per_pass"] = kernel_split(
            lambda: device.blocks_chains(blocks, MAX_DIST, MAX_DRIFT))
        del rows, blocks
        q.free()
        idx.free()
        return c

    report = {"k": k, "max_gap": k, "max_dist": MAX_DIST, "max_drift": MAX_DRIFT, "steps": steps,
              "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per entry; entries alternated step by step in one "
                      "process; median, interquartile spread (q3 - q1) and minimum over the steps; "
                      "blocks_chains includes the copy of its result into new tensors"}
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
