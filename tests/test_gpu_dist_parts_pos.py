"""dist.owner_kmer_pos over spawned ranks sharing cuda:0: an owner-computes build whose parts
stay resident, read as kmer.pos with no assembly (mask all-reduce, labelled part readouts,
segments to rank 0, kmhg_merge_part_positions there) -- equal to the oracle's kmer.pos."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rendezvous(tmp_path) -> str:
    """A file rendezvous for the spawned ranks: no port is picked ahead of its use, so nothing
    else on the host can take it between the pick and the bind."""
    return "file://" + os.path.join(str(tmp_path), "store")


def _worker(rank, world, rdv, seq_bytes, k, backend, out_q):
    import torch
    import torch.distributed as dist
    from kmer_hasher_amd import dist as kd
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if backend == "nccl":
        dist.init_process_group("nccl", init_method=rdv, rank=rank, world_size=world,
                                device_id=dev)
    else:
        dist.init_process_group("gloo", init_method=rdv, rank=rank, world_size=world)
    try:
        seq = torch.from_numpy(np.frombuffer(seq_bytes, np.uint8).copy()).to(dev) \
            if rank == 0 else None
        part, _ = kd.owner_build(seq, k, dev, src=0)
        ph = {}
        res = kd.owner_kmer_pos(part, 15, dst=0, timings=ph)
        torch.cuda.synchronize()
        assert (res is None) == (rank != 0)
        if rank == 0:
            out_q.put(({f: v.cpu().numpy() for f, v in res.items()}, sorted(ph)))
        dist.barrier()
        part.free()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,k,backend", [(2, 31, "gloo"), (3, 21, "gloo"), (1, 21, "nccl")])
def test_owner_kmer_pos_over_resident_parts(gpu, tmp_path, world, k, backend):
    import torch.multiprocessing as mp
    from kmer_hasher_amd import synth
    from oracle import oracle as O
    s = synth.add_n_runs(synth.repeat_rich(160_000, 12, n_gap_every=10_009), 0.004, 13)
    s[-k - 2] = ord("N")
    seq_bytes = s.tobytes()
    oi = O.OracleIndex(seq_bytes, k)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    rdv = _rendezvous(tmp_path)
    procs = [ctx.Process(target=_worker, args=(r, world, rdv, seq_bytes, k, backend, q))
             for r in range(world)]                  # at most 3 processes hold the GPU
    for p in procs:
        p.start()
    try:
        res, phases = q.get(timeout=100)
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert oi.U > 0 and oi.P > 0
    assert np.array_equal(res["count"], oi.counts)
    assert np.array_equal(res["pos"].reshape(-1), oi.pos_rows())
    assert np.array_equal(res["pair.pos"].reshape(-1), oi.pair_rows())
    assert [bytes(r[:k]).decode() for r in res["kmer"]] == oi.kmer_strings()
    assert phases == ["gather", "mask", "merge", "readout"]
