"""dist.owner_kmer_pos (kmer.pos over owner-computes parts, no assembly) over gloo on CPU: the
collective layer -- status round, mask all-reduce, size all-gather, segments to the root, merge
-- with a numpy part engine cut from the oracle's index.  The HIP kernels behind the product
engine are tested on the GPU (test_gpu_parts_pos.py, test_gpu_dist_parts_pos.py)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from kmer_hasher_amd import dist as kd

K = 21


def _rendezvous(tmp_path) -> str:
    """A file rendezvous for the spawned ranks: no port is picked ahead of its use, so nothing
    else on the host can take it between the pick and the bind."""
    return "file://" + os.path.join(str(tmp_path), "store")


def _sequence() -> bytes:
    from kmer_hasher_amd import synth
    return synth.add_n_runs(synth.repeat_rich(30_000, 12, n_gap_every=3_001), 0.004, 13).tobytes()


class NumpyPartEngine:
    """Rank r's share of the oracle's index: the k-mers whose key hashes into its range.  At
    world 5 rank 3's range is empty (a part that owns no bucket).  Labels are counted from the
    all-reduced mask, not taken from the oracle's ids, so a wrong union shows."""

    def __init__(self, seq_bytes, k, rank, world):
        from oracle import oracle as O
        self.oi = oi = O.OracleIndex(seq_bytes, k)
        self.k, self.L, self.device = k, len(seq_bytes), torch.device("cpu")
        live = [r for r in range(world) if not (world == 5 and r == 3)]
        h = (oi.keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)        # 24 bits
        owner = np.asarray(live)[((h * np.uint64(len(live))) >> np.uint64(24)).astype(np.int64)]
        self.mine = np.nonzero(owner == rank)[0]          # canonical ids: ascending first position
        self.first = oi.positions[oi.offsets[:-1]].astype(np.int64)   # 1-based first positions

    def part_info(self):
        return {}

    def first_mask(self):
        bits = np.zeros((self.L + 31) // 32 * 32, np.uint8)
        bits[self.first[self.mine] - 1] = 1
        return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy())

    def positions_part(self, mask, opt):
        oi, mine = self.oi, self.mine
        bits = np.unpackbits(mask.numpy().view(np.uint8), bitorder="little")
        rank_at = np.cumsum(bits, dtype=np.int64)         # set bits at or before each position
        label_of = rank_at[self.first - 1].astype(np.int32)      # by canonical id
        own = np.zeros(oi.U + 1, bool)
        own[mine + 1] = True
        out = {"labels": torch.from_numpy(label_of[mine].copy())}
        if opt & 8:
            out["count"] = torch.from_numpy(oi.counts[mine].copy())
        if opt & 1:
            strs = oi.kmer_strings()
            a = np.zeros((mine.size, self.k + 1), np.uint8)
            for j, i in enumerate(mine):
                a[j, :self.k] = np.frombuffer(strs[i].encode(), np.uint8)
            out["kmer"] = torch.from_numpy(a)
        for f, rows, w in (("pos", oi.pos_rows, 2), ("pair.pos", oi.pair_rows, 3)):
            if opt & (2 if w == 2 else 4):
                r = rows().reshape(-1, w)
                r = r[own[r[:, 0]]].copy()
                r[:, 0] = label_of[r[:, 0] - 1]
                out[f] = torch.from_numpy(r)
        return out

    def merge(self, segs, opt):
        lab = np.concatenate([s["labels"].numpy() for s in segs])
        order = np.argsort(lab, kind="stable")
        assert np.array_equal(lab[order], np.arange(1, lab.size + 1))
        out = {"kmer": None, "pos": None, "pair.pos": None, "count": None}
        if opt & 8:
            out["count"] = np.concatenate([s["count"].numpy() for s in segs])[order]
        if opt & 1:
            out["kmer"] = np.concatenate([s["kmer"].numpy() for s in segs])[order]
        for f, bit in (("pos", 2), ("pair.pos", 4)):
            if opt & bit:
                r = np.concatenate([s[f].numpy() for s in segs])
                out[f] = r[np.argsort(r[:, 0], kind="stable")]
        return out


def _worker(rank, world, rdv, seq_bytes, opt, out_q):
    dist.init_process_group("gloo", init_method=rdv, rank=rank, world_size=world)
    try:
        eng = NumpyPartEngine(seq_bytes, K, rank, world)
        ph = {}
        dst = world - 1
        res = kd.owner_kmer_pos(eng, opt, dst=dst, timings=ph)
        assert (res is None) == (rank != dst)
        if rank == dst:
            oi = eng.oi
            ok = {"phases": sorted(ph) == ["gather", "mask", "merge", "readout"],
                  "count": np.array_equal(res["count"], oi.counts),
                  "pos": np.array_equal(res["pos"].reshape(-1), oi.pos_rows()),
                  "pair.pos": np.array_equal(res["pair.pos"].reshape(-1), oi.pair_rows()),
                  "kmer": [bytes(r[:K]).decode() for r in res["kmer"]] == oi.kmer_strings(),
                  "empty part": world != 5 or NumpyPartEngine(seq_bytes, K, 3, 5).mine.size == 0}
            out_q.put(ok)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 5])
def test_owner_kmer_pos_equals_the_oracle(tmp_path, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    rdv = _rendezvous(tmp_path)
    procs = [ctx.Process(target=_worker, args=(r, world, rdv, _sequence(), 15, q))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        ok = q.get(timeout=120)
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert all(ok.values()), ok


class FailingEngine(NumpyPartEngine):
    """A part whose build failed on its own rank (kmhg_part_info raising KMHG_EOVERFLOW)."""

    def part_info(self):
        from kmer_hasher_amd import _lib
        raise _lib.KmhgError(_lib.KMHG_EOVERFLOW, "a bucket of a part build overflowed its LDS table")


def _failing_worker(rank, world, rdv, bad, seq_bytes, out_q):
    dist.init_process_group("gloo", init_method=rdv, rank=rank, world_size=world)
    try:
        eng = (FailingEngine if rank == bad else NumpyPartEngine)(seq_bytes, K, rank, world)
        try:
            kd.owner_kmer_pos(eng, 15)
            out_q.put((rank, "read"))
        except Exception as e:                       # every rank must land here, none may hang
            out_q.put((rank, type(e).__name__ + ": " + str(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,bad", [(2, 1), (3, 0)])
def test_owner_kmer_pos_failure_reaches_every_rank(tmp_path, world, bad):
    """A part build that failed on one rank makes every rank raise before the mask all-reduce
    (dist.part_info_all goes first), instead of the others blocking in it forever."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    rdv = _rendezvous(tmp_path)
    procs = [ctx.Process(target=_failing_worker, args=(r, world, rdv, bad, _sequence(), q))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in range(world))
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert "overflowed" in res[bad], res
    for r in range(world):
        if r != bad:
            assert "another rank's part build failed" in res[r], res
