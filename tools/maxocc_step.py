"""kmer.max.occ (kmhg_set_max_occ, k_qrec_mask) timed on ONE GPU (tools, not product).

repeat_rich   the 2 Mbp sequence of config 4's generator (synth.config4), k = 31, self query --
              tools/chains_step.py's input, about 30 rows per window.  DeviceIndex.query at
              max_occ 0, 1, 8 and 64, and the row-free blocks and chains at 0 and 8.
iid_overhead  config 2's sequence (10 Mbp i.i.d., seed 1, k = 31), self query at max_occ 0 and
              2^31-1: nothing is masked there, so the difference is the pass's own cost over
              10 M windows.
The settings of one group alternate step by step in one process on one index; each call is timed
with HIP events on the stream it runs on and ends in its own synchronize; medians, interquartile
spreads (q3 - q1) and minima over the steps after a warm-up.  The split between the kernels of a
query (the library's per-kernel event timing) comes from a separate set of passes per setting.

    python tools/maxocc_step.py [out.json] [steps] [warmup]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 2**31 - 1


def stats(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return {"median": round(q[1], 4), "iqr": round(q[2] - q[0], 4), "min": round(min(v), 4)}


def main():
    import torch
    from kmer_hasher_amd import device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "maxocc_step.json")
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

    def alternate(idx, caps, fn, size):
        """fn() under every cap in turn, step by step: {cap: {size..., ms}}."""
        t = {c: [] for c in caps}
        out = {c: {} for c in caps}
        for it in range(warmup + steps):
            for c in caps:
                idx.set_max_occ(c)
                u, r = timed(fn)
                out[c].update(size(r))
                del r
                if it >= warmup:
                    t[c].append(u)
        for c in caps:
            out[c]["ms"] = stats(t[c])
        idx.set_max_occ(0)
        return {str(c): out[c] for c in caps}

    def query_case(seq, caps):
        idx = DeviceIndex.build(seq, k).wait()

        def run():
            q = idx.query(seq, k)
            n = q.n_rows
            q.free()
            return n

        c = {"L": int(seq.numel()), "windows": int(seq.numel()) - k + 1,
             "query": alternate(idx, caps, run, lambda n: {"rows": int(n)})}
        for cap in caps:
            idx.set_max_occ(cap)
            split = kernel_split(run)
            c["query"][str(cap)]["kernel_ms_per_query"] = {
                kn: split.get(kn, 0.0) for kn in ("k_query_probe", "k_qrec_mask",
                                                  "k_scan_tiles_u64", "k_query_emit")}
        idx.set_max_occ(0)
        return idx, c

    report = {"k": k, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per call; the caps of one group alternate step by "
                      "step in one process on one index; median, interquartile spread (q3 - q1) "
                      "and minimum over the steps; a query's ms include freeing its result; "
                      "kernel_ms_per_query from separate passes with the library's per-kernel "
                      "events on (k_query_emit: both emit kernels)"}
    R = torch.from_numpy(synth.config4(2_000_000, 3)).to(dev)
    idx, c = query_case(R, (0, 1, 8, 64))
    c["blocks_row_free"] = alternate(
        idx, (0, 8), lambda: idx.blocks(R, k, k),
        lambda r: {"blocks": int(r[0].shape[0]), "rows": int(r[1])})
    c["chains_row_free"] = alternate(
        idx, (0, 8), lambda: idx.chains(R, k, row_free=True),
        lambda r: {"chains": int(r[0].shape[0]), "blocks": int(r[1].shape[0]), "rows": int(r[3])})
    idx.free()
    report["repeat_rich_self"] = c
    print("repeat_rich", json.dumps(c), flush=True)
    del R
    A = torch.from_numpy(synth.iid(10_000_000, 1)).to(dev)
    idx, c = query_case(A, (0, M))
    idx.free()
    q = c["query"]
    c["pass_overhead_ms"] = round(q[str(M)]["ms"]["median"] - q["0"]["ms"]["median"], 4)
    report["iid_overhead"] = c
    print("iid_overhead", json.dumps(c), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
