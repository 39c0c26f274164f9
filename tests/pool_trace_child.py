"""Child process of test_gpu_pool.py: two rounds of build + self-query + free against the device
pool of the test build (KMHG_LIB_VARIANT=test, KMHG_POOL_TRACE=1: one stderr line per device
allocation), a marker line on stderr between them, then kmhg_pool_trim.  Prints each round's
(U, N, P) and the bytes the pool still caches after the trim."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

MARKER = "pool_trace_child: second round"


def main():
    assert os.environ.get("KMHG_LIB_VARIANT"), "run with KMHG_LIB_VARIANT=test"
    import torch
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    torch.cuda.set_device(0)
    seq = torch.from_numpy(synth.iid(4096, 5)).cuda()
    for rnd in (1, 2):
        idx = DeviceIndex.build(seq, 15).wait()
        info = idx.info()
        q = idx.query(seq, 15)
        torch.cuda.synchronize()
        q.free()
        idx.free()
        print("round", rnd, info["n_kmers"], info["n_positions"], info["n_pairs"], flush=True)
        if rnd == 1:
            sys.stderr.write(MARKER + "\n")
            sys.stderr.flush()
    _lib.check(_lib.lib().kmhg_pool_trim())
    print("cached", _lib.lib().kmhg_pool_cached_bytes(), flush=True)


if __name__ == "__main__":
    main()
