"""Minimizer-sampled indexes (kmhg_build_sampled_device, k_minimizer_mask) timed on ONE GPU (tools,
not product).

iid          config 2's sequence (10 Mbp i.i.d., seed 1, k = 31) at w = 1 (unsampled), 5, 10 and
             19, alternating step by step in one process: build time, index bytes
             (kmhg_image_sizes_get), the self query and an unrelated query (seed 2), the selected
             fraction.
repeat_rich  the 2 Mbp repeat-rich self query (synth.config4) at w = 1 and 10: rows, row-free
             blocks and chains, counts and times.

    python tools/minimizer_step.py [out.json] [steps] [warmup]
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
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "minimizer_step.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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

    def sizes(idx):
        sz = _lib.ImageSizes()
        hdr = (C.c_int64 * 8)()
        _lib.check(_lib.lib().kmhg_image_sizes_get(idx.handle, C.byref(sz), hdr))
        return {"table_bytes": sz.table_bytes, "positions_bytes": sz.positions_bytes,
                "codes_bytes": sz.codes_bytes,
                "index_bytes": sz.table_bytes + sz.positions_bytes + sz.codes_bytes}

    def alternate(ws, fns):
        """fns[w]() for every w in turn, step by step: {w: ms stats}, and the last results."""
        t = {w: [] for w in ws}
        last = {}
        for it in range(warmup + steps):
            for w in ws:
                u, r = timed(fns[w])
                last[w] = r
                if it >= warmup:
                    t[w].append(u)
        return {w: stats(t[w]) for w in ws}, last

    def n_rows(q):
        n = q.n_rows
        q.free()
        return n

    report = {"k": k, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per call; the values of w alternate step by step in "
                      "one process; median, interquartile spread and minimum over the steps; "
                      "w = 1 is the unsampled index (kmhg_build_device); a build's ms include "
                      "waiting for it and freeing the index; a query's include freeing its result"}

    def case(seq, other, ws, products):
        nw = int(seq.numel()) - k + 1
        c = {"L": int(seq.numel()), "windows": nw, "w": {}}

        def build(w):
            def f():
                idx = DeviceIndex.build(seq, k, w=w).wait()
                idx.free()
            return f

        bt, _ = alternate(ws, {w: build(w) for w in ws})
        idxs = {w: DeviceIndex.build(seq, k, w=w).wait() for w in ws}
        qt, qn = alternate(ws, {w: (lambda w=w: n_rows(idxs[w].query(seq, k))) for w in ws})
        for w in ws:
            inf = idxs[w].info()
            c["w"][str(w)] = {"build_ms": bt[w], **sizes(idxs[w]),
                              "positions": int(inf["n_positions"]),
                              "selected_fraction": round(inf["n_positions"] / nw, 5),
                              "self_query_ms": qt[w], "self_rows": int(qn[w])}
        if other is not None:
            ut, un = alternate(ws, {w: (lambda w=w: n_rows(idxs[w].query(other, k))) for w in ws})
            for w in ws:
                c["w"][str(w)].update(unrelated_query_ms=ut[w], unrelated_rows=int(un[w]))
        if products:
            b, br = alternate(ws, {w: (lambda w=w: idxs[w].blocks(seq, k, k)) for w in ws})
            ch, cr = alternate(ws, {w: (lambda w=w: idxs[w].chains(seq, k, row_free=True))
                                    for w in ws})
            for w in ws:
                c["w"][str(w)].update(blocks_row_free_ms=b[w], blocks=int(br[w][0].shape[0]),
                                      chains_row_free_ms=ch[w], chains=int(cr[w][0].shape[0]))
        for i in idxs.values():
            i.free()
        return c

    A = torch.from_numpy(synth.iid(10_000_000, 1)).to(dev)
    B = torch.from_numpy(synth.iid(10_000_000, 2)).to(dev)
    report["iid"] = case(A, B, (1, 5, 10, 19), False)
    print("iid", json.dumps(report["iid"]), flush=True)
    del A, B
    R = torch.from_numpy(synth.config4(2_000_000, 3)).to(dev)
    report["repeat_rich_self"] = case(R, None, (1, 10), True)
    print("repeat_rich", json.dumps(report["repeat_rich_self"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
