"""Child process of test_gpu_stream_reuse.py: two rounds of build chains on one stream (A kept, B
and C freed unwaited, D; one chain per shape and one of alternating shapes) against the device
pool of the test build (KMHG_LIB_VARIANT=test, KMHG_POOL_TRACE=1: one stderr line per device
allocation), a marker line on stderr between the rounds.  Prints each round's (U, N, P) of the
kept indices."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

MARKER = "stream_reuse_child: second round"
SHAPES = [(5_000, 31), (70_000, 31), (300, 5)]


def main():
    assert os.environ.get("KMHG_LIB_VARIANT"), "run with KMHG_LIB_VARIANT=test"
    import torch
    from kmer_hasher_amd import synth
    from kmer_hasher_amd.device import DeviceIndex
    torch.cuda.set_device(0)
    seqs = {L: [torch.from_numpy(synth.iid(L, 31 + i)).cuda() for i in range(4)]
            for L, _ in SHAPES}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    chains = [[sh] * 4 for sh in SHAPES] + [[SHAPES[0], SHAPES[1]] * 2]
    for rnd in (1, 2):
        totals = []
        for ch in chains:
            idx = [None] * 4
            for i, (L, k) in enumerate(ch):
                idx[i] = DeviceIndex.build(seqs[L][i], k, stream)
                if i in (1, 2):
                    idx[i].free()
            for i in (3, 0):
                inf = idx[i].wait().info()
                totals += [inf["n_kmers"], inf["n_positions"], inf["n_pairs"]]
                idx[i].free()
        stream.synchronize()
        print("round", rnd, *totals, flush=True)
        if rnd == 1:
            sys.stderr.write(MARKER + "\n")
            sys.stderr.flush()


if __name__ == "__main__":
    main()
