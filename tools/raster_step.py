"""seq.kmer.raster timed beside the query it replaces and the one-pass row reader it resembles, on
ONE GPU (tools, not product).

self       config 2: 10 Mbp i.i.d., k = 31, self query -- 10 M rows on one diagonal, the worst
           same-cell contention
unrelated  config 2's index, an unrelated 10 Mbp query: no hits, the probe alone
repeat     the 2 Mbp sequence of config 4's generator (synth.config4), k = 31, self query
Per case and frame (1024 x 1024 bins over the full ranges; width-1 bins in a 4096 x 4096 crop):
  query_ms        DeviceIndex.query -- probe, scan, row emit: the baseline, the same code as
                  before this entry existed
  raster_ms       kmhg_raster_run_device, the row-free route, and its ratio to query_ms
  rows_runs_ms    kmhg_rows_runs over the query's rows, the existing one-pass reader of rows
  rows_raster_ms  kmhg_rows_raster over the same rows, and its ratio to rows_runs_ms
(the two raster entries are timed as C calls into a u32 buffer; the int64 view device.py returns
is checked once, outside the timing)
alternated step by step in one process, each timed with HIP events on the stream it runs on;
medians, interquartile spreads (q3 - q1) and minima over the steps after a warm-up; then the
per-kernel split of the row-free route (the library's per-kernel event timing, separate passes).
host_api: seq_kmer_raster against seq_kmer_pos into a host matrix on the self case, wall clock.

    python tools/raster_step.py [out.json] [steps] [warmup]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return {"median": round(q[1], 4), "iqr": round(q[2] - q[0], 4), "min": round(min(v), 4)}


def main():
    import torch
    from kmer_hasher_amd import _lib, api, device, synth
    from kmer_hasher_amd.device import DeviceIndex
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "raster_step.json")
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

    # the C entries themselves, into `out` (u32 bits): the int64 view the device.py wrappers
    # return is three more torch kernels over the matrix and stays outside the timing
    L = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw_free(idx, seq, fc, out):
        h = C.c_int64()
        _lib.check(L.kmhg_raster_run_device(idx.handle, C.c_void_p(seq.data_ptr()), seq.numel(), k,
                                            0, fc, C.c_void_p(out.data_ptr()), sp, C.byref(h)))
        return h.value

    def raw_rows(rows, fc, out):
        _lib.check(L.kmhg_rows_raster(C.c_void_p(rows.data_ptr() if rows.shape[0] else None),
                                      rows.shape[0], fc, C.c_void_p(out.data_ptr()), sp))

    def frames(Lq, Li):
        bi, ni = api.raster_axis(1, Lq, 1024)
        bj, nj = api.raster_axis(1, Li, 1024)
        return {"bins_1024": (1, 1, bi, bj, ni, nj),
                "width_1_crop_4096": (Lq // 2, Li // 2, 1, 1, 4096, 4096)}

    def case(idx, index_L, query_seq):
        c = {"index_L": int(index_L), "query_L": int(query_seq.numel())}
        for name, f in frames(int(query_seq.numel()), int(index_L)).items():
            out = torch.empty(f[4] * f[5], dtype=torch.int32, device=dev)
            out2 = torch.empty_like(out)
            fc = (C.c_int64 * 6)(*f)
            tq, tr, tu, tw = [], [], [], []
            for it in range(warmup + steps):
                a, q = timed(lambda: idx.query(query_seq, k))
                b, h = timed(lambda: raw_free(idx, query_seq, fc, out))
                assert h == q.n_rows
                rows = q.rows_view()
                u, _ = timed(lambda: device.rows_to_runs(rows)) if q.n_rows else (0.0, None)
                w, _ = timed(lambda: raw_rows(rows, fc, out2))
                if it == 0:
                    assert torch.equal(out, out2)
                    m, h2 = idx.raster(query_seq, k, f)
                    assert h2 == h and torch.equal(m, device.rows_raster(rows, f))
                    c["rows"] = int(h)
                    c.setdefault("in_frame", {})[name] = int(m.sum())
                    del m
                del rows
                q.free()
                if it >= warmup:
                    tq.append(a)
                    tr.append(b)
                    tu.append(u)
                    tw.append(w)
            r = {"frame": list(f), "query_ms": stats(tq), "raster_ms": stats(tr),
                 "rows_runs_ms": stats(tu), "rows_raster_ms": stats(tw)}
            r["ratio_raster_to_query"] = round(r["raster_ms"]["median"] / r["query_ms"]["median"], 4)
            if r["rows_runs_ms"]["median"]:
                r["ratio_rows_raster_to_rows_runs"] = round(
                    r["rows_raster_ms"]["median"] / r["rows_runs_ms"]["median"], 4)
            r["raster_kernel_ms_per_pass"] = kernel_split(
                lambda: raw_free(idx, query_seq, fc, out))
            c[name] = r
        c["query_kernel_ms_per_pass"] = kernel_split(lambda: idx.query(query_seq, k).free())
        return c

    report = {"k": k, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "note": "ms; HIP-event timing per entry; entries alternated step by step in one "
                      "process; median, interquartile spread (q3 - q1) and minimum over the steps"}
    A = synth.iid(10_000_000, 1)
    At = torch.from_numpy(A).to(dev)
    idx = DeviceIndex.build(At, k).wait()
    report["self"] = case(idx, At.numel(), At)
    print("self", json.dumps(report["self"]), flush=True)
    Bt = torch.from_numpy(synth.iid(10_000_000, 2)).to(dev)
    report["unrelated"] = case(idx, At.numel(), Bt)
    print("unrelated", json.dumps(report["unrelated"]), flush=True)
    del Bt, idx

    # through the host API: a host string in, a host matrix out (wall clock, ms)
    s = A.tobytes().decode("latin-1")
    ptr = api.make_kmer_hash(s, k)
    tp, tr = [], []
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        rows = api.seq_kmer_pos(ptr, s, k)
        t1 = time.perf_counter()
        del rows
        t2 = time.perf_counter()
        r = api.seq_kmer_raster(ptr, s, k, bins=1024)
        t3 = time.perf_counter()
        if it >= warmup:
            tp.append((t1 - t0) * 1e3)
            tr.append((t3 - t2) * 1e3)
    report["host_api_self"] = {"seq_kmer_pos_ms": stats(tp), "seq_kmer_raster_ms": stats(tr),
                               "rows": int(r["n_rows"]), "counts_bytes": int(r["counts"].nbytes),
                               "ratio_raster_to_pos": round(stats(tr)["median"] / stats(tp)["median"], 4)}
    print("host_api", json.dumps(report["host_api_self"]), flush=True)
    ptr.free()
    del A, At, s

    R = torch.from_numpy(synth.config4(2_000_000, 3)).to(dev)
    idx = DeviceIndex.build(R, k).wait()
    report["repeat_rich_self"] = case(idx, R.numel(), R)
    print("repeat_rich", json.dumps(report["repeat_rich_self"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
