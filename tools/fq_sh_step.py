"""Step timings of count.kmers.fq.sh / kmer.spec.sh on one GPU (tools, not product), HIP events
around each call, the two entries of a comparison alternated inside one run:

(a) reads     kmhg_sh1_count_reads_device on bench.py's reads leg (400 K x 150 bp sampled from
              the config-2 sequence, k = 31, min quality 10) beside the existing .rp entry
(b) fasta     one 10 Mbp record without qualities (the config-2 sequence) through the
              position-parallel kernel, beside the same record through the .rp entry, whose
              lane-per-read walk gives it to one lane
(c) spectrum  kmhg_sh1_spectrum at max_count = 10000 on (a)'s suffix hash

    python tools/fq_sh_step.py [out.json] [reps]
"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, MINQ = 31, 10
READS_N, READS_LEN = 400_000, 150


def main():
    import numpy as np
    import torch
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd import device as D
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "fq_sh_step.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    prm1 = (C.c_int32 * 6)(K, 1, 30, 100, MINQ, -1)
    prm_rp = (C.c_int32 * 8)(K, 28, MINQ, 47, -1, 200, 1, 0)

    def count(reads, sh1):
        h = C.c_void_p()
        f = L.kmhg_sh1_count_reads_device if sh1 else L.kmhg_sh_count_reads_device
        _lib.check(f(C.byref(h), reads.seq.data_ptr(), reads.qual.data_ptr(), reads.off.data_ptr(),
                     reads.hasq.data_ptr(), reads.n, prm1 if sh1 else prm_rp, None))
        return h

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def n_kmers(h):
        inf = _lib.Info()
        _lib.check(L.kmhg_index_info(h, C.byref(inf)))
        return int(inf.n_kmers)

    def compare(reads, warm, n):
        """ms of the new entry and of the .rp entry, alternated"""
        t = {True: [], False: []}
        u = {}
        for i in range(warm + n):
            for sh1 in (True, False):
                ms, h = timed(lambda: count(reads, sh1))
                u[sh1] = n_kmers(h)
                L.kmhg_free(h)
                if i >= warm:
                    t[sh1].append(ms)
        return t, u

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}

    g = synth.iid(10_000_000, 1)
    rs, rq = synth.reads(g, READS_N, READS_LEN, 51)
    reads = D.DeviceReads.from_arrays(rs, rq, dev)
    rec = {"device": torch.cuda.get_device_name(0), "k": K, "min_quality": MINQ, "reps": reps,
           "clock": "HIP events around each call, entries alternated, warm-up calls dropped"}
    t, u = compare(reads, 3, reps)
    rec["reads"] = {"input": f"{READS_N} reads x {READS_LEN} bp of the config-2 sequence",
                    "bases": READS_N * READS_LEN, "sh1": stats(t[True]), "rp": stats(t[False]),
                    "distinct_sh1": u[True], "distinct_rp": u[False]}
    one = D.DeviceReads.from_arrays(g.reshape(1, -1), np.zeros((1, len(g)), np.uint8), dev,
                                    has_qual=np.zeros(1, np.uint8))
    t, u = compare(one, 1, min(reps, 3))
    rec["fasta"] = {"input": "one 10 Mbp record without qualities (config-2 sequence)",
                    "bases": len(g), "sh1_position_parallel": stats(t[True]),
                    "rp_lane_per_read": stats(t[False]),
                    "ratio_rp_over_sh1": statistics.median(t[False]) / statistics.median(t[True]),
                    "distinct_sh1": u[True], "distinct_rp": u[False]}
    h = count(reads, True)
    out = np.zeros(10001, np.float64)
    sp = []
    for i in range(3 + reps):
        ms, _ = timed(lambda: _lib.check(L.kmhg_sh1_spectrum(h, 10000, out.ctypes.data)))
        if i >= 3:
            sp.append(ms)
    rec["spectrum"] = {"max_count": 10000, "distinct": n_kmers(h), "bins_sum": float(out.sum()),
                       **stats(sp)}
    L.kmhg_free(h)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
