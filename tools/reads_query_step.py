"""reads.kmer.pos / reads.kmer.vote (kmhg_readsq.hip) timed on ONE GPU (tools, not product).

Input: 1 M reads of 150 bp from synth.reads over config 2's sequence (10 Mbp i.i.d., seed 1),
against config 2's index at k = 31.  Every figure stands beside a baseline from the same run that
uses only entries the batched query does not touch:

forward        DeviceIndex.query_reads(strands=1) beside DeviceIndex.query on the same bases
               joined with N (151 chars per read: not the same rows, the same table lookups),
               alternating step by step; each with its per-kernel split (the library's event
               timing, separate passes), so the probe legs and the emit legs stand side by side
both           strands=3 beside the forward figure
loop           the batched call over the first 2,000 reads beside a loop of per-read query +
               query_rc over the same reads (launch-bound: it would not finish for 1 M reads)
votes          .votes(64) beside the batched query that made its rows

Each call is timed with HIP events on the stream it runs on and ends in its own synchronize;
medians, interquartile spreads (q3 - q1) and minima over the steps after a warm-up.

    python tools/reads_query_step.py [out.json] [steps] [warmup] [n_reads]
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
    import numpy as np
    import torch
    from kmer_hasher_amd import device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "reads_query_step.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    n_reads = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
    rl, k, n_loop = 150, 31, 2000
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def alternate(fns, n_steps=None, n_warm=None):
        """Every fn in turn, step by step: {name: {"ms": stats, **what fn returned}}."""
        n_steps, n_warm = n_steps or steps, warmup if n_warm is None else n_warm
        t = {name: [] for name in fns}
        out = {name: {} for name in fns}
        for it in range(n_warm + n_steps):
            for name, fn in fns.items():
                u, r = timed(fn)
                out[name].update(r)
                if it >= n_warm:
                    t[name].append(u)
        for name in fns:
            out[name]["ms"] = stats(t[name])
        return out

    def kernel_split(fn, n=5):
        fn()
        device.timing_enable(True)
        device.timing_reset()
        for _ in range(n):
            fn()
        split = {kn: round(v[1] / n, 4) for kn, v in device.timing_report().items() if v[0]}
        device.timing_enable(False)
        return split

    genome = synth.iid(10_000_000, 1)
    rs, _ = synth.reads(genome, n_reads, rl)
    A = torch.from_numpy(genome).to(dev)
    idx = DeviceIndex.build(A, k).wait()
    seq = torch.from_numpy(np.ascontiguousarray(rs.reshape(-1))).to(dev)
    off = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * rl
    joined_h = np.full((n_reads, rl + 1), ord("N"), np.uint8)
    joined_h[:, :rl] = rs
    joined = torch.from_numpy(joined_h.reshape(-1)).to(dev)
    del joined_h

    def batched(strands, s=seq, o=off):
        def run():
            q = idx.query_reads((s, o), k, strands)
            n = q.n_rows
            q.free()
            return {"rows": int(n)}
        return run

    def joined_query():
        q = idx.query(joined, k)
        n = q.n_rows
        q.free()
        return {"rows": int(n)}

    report = {"k": k, "reads": n_reads, "read_len": rl, "bases": n_reads * rl, "steps": steps,
              "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per call, each call ending in its own synchronize and "
                      "freeing its result; the entries of one group alternate step by step in "
                      "one process on one index; median, interquartile spread (q3 - q1) and "
                      "minimum over the steps; kernel_ms from separate passes with the library's "
                      "per-kernel events on"}

    g = alternate({"batched_forward": batched(1), "joined_query": joined_query,
                   "batched_both": batched(3)})
    g["batched_forward"]["kernel_ms"] = kernel_split(batched(1))
    g["joined_query"]["kernel_ms"] = kernel_split(joined_query)
    g["batched_both"]["kernel_ms"] = kernel_split(batched(3))
    fw, jq, bo = (g[n]["ms"]["median"] for n in ("batched_forward", "joined_query", "batched_both"))
    g["forward_over_joined"] = round(fw / jq, 3)
    g["both_over_forward"] = round(bo / fw, 3)
    report["million_reads"] = g
    print("million_reads", json.dumps(g), flush=True)

    # the first 2,000 reads: one batched call beside a loop of per-read calls
    s2, o2 = seq[:n_loop * rl].clone(), off[:n_loop + 1].clone()
    each = [seq[r * rl:(r + 1) * rl].clone() for r in range(n_loop)]

    def loop():
        n = 0
        for t in each:
            for q in (idx.query(t, k), idx.query_rc(t, k)):
                n += q.n_rows
                q.free()
        return {"rows": int(n)}

    g = alternate({"batched_both": batched(3, s2, o2), "per_read_loop": loop}, n_steps=5, n_warm=1)
    g["loop_over_batched"] = round(g["per_read_loop"]["ms"]["median"] /
                                   g["batched_both"]["ms"]["median"], 1)
    report["first_2000_reads"] = g
    print("first_2000_reads", json.dumps(g), flush=True)

    # the vote beside the query that made its rows
    q = idx.query_reads((seq, off), k, 3)

    def votes():
        q.votes(64)
        return {}

    g = alternate({"votes_64": votes})
    g["votes_64"]["kernel_ms"] = kernel_split(votes)
    g["rows"] = int(q.n_rows)
    g["reads_with_hits"] = int((q.votes(64)[:, 3] > 0).sum().item())
    g["votes_over_query"] = round(g["votes_64"]["ms"]["median"] / bo, 3)
    q.free()
    report["votes"] = g
    print("votes", json.dumps(g), flush=True)
    idx.free()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
