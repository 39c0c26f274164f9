"""The reverse-strand query against the route it replaces, on ONE GPU (tools, not product).

Route A (what a device caller could do before): materialise rc(B) on the device with torch (a
flip and a 256-entry lookup), then DeviceIndex.query of that buffer -- the two legs timed
separately.  Route B: DeviceIndex.query_rc of B itself.  Config 2 (10 Mbp i.i.d., k = 31) as the
index A; three queries: B = synth.derived(A) (SNVs, inversions, translocations, N-runs),
B = rc(A) (every window hits, one long diagonal on the reverse strand), and an unrelated B.
The routes alternate inside one process; every leg is timed with HIP events on the stream the
query runs on (the query entry returns after its own synchronize, so a leg covers launch to
rows-in-HBM); medians and interquartile spreads over the steps after a warm-up of both routes.

    python tools/rc_query_step.py [out.json] [steps] [warmup]

requirement recorded per input: median(B) <= median(A materialise + query) + the larger of the
two routes' interquartile spreads.  `ratio_to_A_query` compares B with A's query leg alone (the
probes are the same; only the stage fill differs).  `torch_peak_bytes` is the peak of the
caller-side allocations a route adds (route A's rc buffer and its temporaries; route B makes
none); the library's own per-query buffers are the same on both routes.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return q[0], q[1], q[2]


def main():
    import numpy as np
    import torch
    from kmer_hasher_amd import synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "rc_query_step.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    assert steps >= 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    k, L = 31, 10_000_000
    # rc of the definition: N / n stay N, every other byte "ACTG"[code ^ 2]
    lut_np = np.array([ord("N") if (c | 0x20) == ord("n") else b"ACTG"[((c >> 1) & 3) ^ 2]
                       for c in range(256)], np.uint8)
    lut = torch.from_numpy(lut_np).to(dev)

    def materialise(b):
        return torch.index_select(lut, 0, b.flip(0).to(torch.int32))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        r = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base, r

    A = synth.iid(L, 1)
    tA = torch.from_numpy(A).to(dev)
    idx = DeviceIndex.build(tA, k).wait()
    inputs = {"derived": synth.derived(A, 5),
              "rc_of_A": lut_np[A[::-1]],
              "unrelated": synth.iid(L, 2)}
    report = {"k": k, "L": L, "steps": steps, "warmup": warmup,
              "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per leg; routes alternated step by step in one "
                      "process; median and interquartile spread (q3 - q1) over the steps",
              "inputs": {}}
    ok_all = True
    for name, b_np in inputs.items():
        b = torch.from_numpy(np.ascontiguousarray(b_np)).to(dev)

        def route_a():
            tm, rcb = timed(lambda: materialise(b))
            tq, q = timed(lambda: idx.query(rcb, k))
            n = q.n_rows
            q.free()
            return tm, tq, n

        def route_b():
            t, q = timed(lambda: idx.query_rc(b, k))
            n = q.n_rows
            q.free()
            return t, n

        # same rows on both routes (checked once, outside the timing)
        qa, qb = idx.query(materialise(b), k), idx.query_rc(b, k)
        same = bool(torch.equal(qa.rows(), qb.rows()))
        rows = qb.n_rows
        qa.free()
        qb.free()
        for _ in range(warmup):
            route_a()
            route_b()
        am, aq, bt = [], [], []
        for _ in range(steps):
            tm, tq, _n = route_a()
            am.append(tm)
            aq.append(tq)
            t, _n = route_b()
            bt.append(t)
        pa, _ = peak(lambda: idx.query(materialise(b), k).free())
        pb, _ = peak(lambda: idx.query_rc(b, k).free())
        atot = [x + y for x, y in zip(am, aq)]
        qa1, qa2, qa3 = quartiles(atot)
        qq1, qq2, qq3 = quartiles(aq)
        qm1, qm2, qm3 = quartiles(am)
        qb1, qb2, qb3 = quartiles(bt)
        margin = max(qa3 - qa1, qb3 - qb1)
        meets = qb2 <= qa2 + margin
        ok_all &= meets and same
        report["inputs"][name] = {
            "rows": int(rows), "identical_rows": same,
            "A_materialise_ms": {"median": round(qm2, 4), "iqr": round(qm3 - qm1, 4)},
            "A_query_ms": {"median": round(qq2, 4), "iqr": round(qq3 - qq1, 4)},
            "A_total_ms": {"median": round(qa2, 4), "iqr": round(qa3 - qa1, 4)},
            "B_query_rc_ms": {"median": round(qb2, 4), "iqr": round(qb3 - qb1, 4)},
            "margin_ms": round(margin, 4), "meets_requirement": bool(meets),
            "ratio_to_A_total": round(qb2 / qa2, 4), "ratio_to_A_query": round(qb2 / qq2, 4),
            "B_slower_than_A_query_beyond_spread": bool(qb2 > qq2 + max(qq3 - qq1, qb3 - qb1)),
            "torch_peak_bytes": {"A": int(pa), "B": int(pb)},
            "gbp_per_s": {"A_total": round(L / qa2 / 1e6, 2), "B": round(L / qb2 / 1e6, 2)}}
        print(name, json.dumps(report["inputs"][name]), flush=True)
        del b
    report["all_meet"] = bool(ok_all)
    idx.free()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
