"""Host side of the headline step: wall time of the kmhg_build_device + kmhg_free call pair.

    python tools/build_host_probe.py <Mbp> <k> [steps]

Two settings in one run, one JSON line:
  back_to_back  the calls as bench.py's headline makes them (unwaited builds, freed at once): the
                median call pair, which holds whatever the host waits for inside the calls, and
                the step (wall time of the loop / steps, synchronized at its end);
  drained       the stream synchronized before every call pair, so no block is pending and the
                pool waits for nothing: the pure enqueue cost of one build + free.
The library is the product, or KMHG_LIB_VARIANT's (`test` with KMHG_POOL_STREAM=0 is the pool
without same-stream reuse).  If `drained` is not clearly below the kernels' sum of one build, the
host's enqueue is the limit of back-to-back builds, not the device.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from kmer_hasher_amd import device as D
    from kmer_hasher_amd import synth
    mbp, k = int(sys.argv[1]), int(sys.argv[2])
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    L = mbp * 1_000_000
    seed = {10: 1, 100: 2, 500: 4}.get(mbp, 1)
    torch.cuda.set_device(0)
    seq = torch.from_numpy(synth.iid(L, seed)).cuda()
    stream = torch.cuda.current_stream()
    for _ in range(3):
        D.DeviceIndex.build(seq, k, stream).wait().free()
    torch.cuda.synchronize()

    def pairs(drain):
        out = []
        for _ in range(steps):
            if drain:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            D.DeviceIndex.build(seq, k, stream).free()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    pairs(False)                                   # warm: the steady state of the pool
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b2b = pairs(False)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / steps * 1e3
    drained = pairs(True)
    torch.cuda.synchronize()

    def q(v):
        v = sorted(v)
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4),
                "p90_ms": round(v[int(0.9 * (len(v) - 1))], 4)}

    print(json.dumps({"mbp": mbp, "k": k, "steps": steps, "step_ms": round(step, 4),
                      "back_to_back": q(b2b), "drained": q(drained),
                      "lib": os.environ.get("KMHG_LIB_VARIANT", "product"),
                      "same_stream": os.environ.get("KMHG_POOL_STREAM", "1")}), flush=True)


if __name__ == "__main__":
    main()
