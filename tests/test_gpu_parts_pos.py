"""kmer.pos over the parts of an owner-computes build with no index assembly (kmhg_part_first_mask,
kmhg_part_positions_fill_device, kmhg_merge_part_positions; reference reader src/kmer_hash.c:
1054-1147 over the partition of src/kmer_reader.c:28-39), parts built on one device: the merged
result must be byte for byte the single-device index's kmer.pos and the oracle's.  Cases as
test_gpu_parts.py: long position lists and pair rows over many scan tiles, the k = 32 side slot
(one part owns it), and more parts than buckets (parts with an empty mask and no rows)."""
import numpy as np
import pytest

from kmh_canon import oracle_index

pytestmark = pytest.mark.gpu

CASES = ["iid31", "rr21", "rr9", "side32", "tiny31"]
_REF = {}


def _case(name):
    """(sequence, k, the single-device index's kmer.pos(15) as numpy, n_kmers): once per session."""
    if name not in _REF:
        import torch
        from kmer_hasher_amd import synth
        from kmer_hasher_amd.device import DeviceIndex
        if name in ("rr21", "rr9"):
            seq = synth.add_n_runs(synth.repeat_rich(400_000, 31, n_gap_every=70_000), 0.001, 32)
        else:
            seq = {"iid31": lambda: synth.iid(300_000, 33),
                   "side32": lambda: np.frombuffer(b"G" * 40 + b"ACGT" * 800 + b"G" * 35, np.uint8),
                   "tiny31": lambda: synth.iid(3_000, 34)}[name]()     # 3 buckets
        k = {"iid31": 31, "rr21": 21, "rr9": 9, "side32": 32, "tiny31": 31}[name]
        whole = DeviceIndex.build(torch.from_numpy(seq.copy()).cuda(), k)
        res = {f: v.cpu().numpy() for f, v in whole.positions(15).items()}
        n_kmers = whole.info()["n_kmers"]
        whole.free()
        _REF[name] = (seq, k, res, n_kmers)
    return _REF[name]


def _bits(mask) -> np.ndarray:
    return np.unpackbits(mask.cpu().numpy().view(np.uint8), bitorder="little")


def _np(d):
    return {f: None if v is None else v.cpu().numpy() for f, v in d.items()}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n_parts", [1, 2, 3, 5, 8])
def test_parts_kmer_pos_equals_the_single_build(gpu, n_parts, case):
    torch = gpu
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex, merge_part_positions
    seq_np, k, want, n_kmers = _case(case)
    seq = torch.from_numpy(seq_np.copy()).cuda()
    parts = [DeviceIndex.build_part(seq, k, p, n_parts) for p in range(n_parts)]
    masks = [p.first_mask() for p in parts]
    union = np.zeros_like(_bits(masks[0]))
    for m in masks:
        b = _bits(m)
        assert not (union & b).any(), "masks overlap"
        union |= b
    assert int(union.sum()) == n_kmers
    if case == "tiny31" and n_parts > 3:
        assert any(not _bits(m).any() for m in masks)          # parts that own no bucket
    gmask = torch.stack(masks).sum(0, dtype=torch.int32)       # disjoint bits: the sum is the OR
    assert np.array_equal(_bits(gmask), union)

    segs = [p.positions_part(gmask, 15) for p in parts]
    labs = [s["labels"].cpu().numpy() for s in segs]
    for lab, p in zip(labs, parts):
        assert lab.size == p.part_info()["n_kmers"]
        assert (np.diff(lab) > 0).all()
    assert np.array_equal(np.sort(np.concatenate(labs)), np.arange(1, n_kmers + 1))

    got = _np(merge_part_positions(segs, 15, k))
    for f in ("count", "pos", "pair.pos", "kmer"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert got[f].tobytes() == want[f].tobytes(), (case, n_parts, f)
    oi = oracle_index(seq_np.tobytes(), k)
    assert np.array_equal(got["count"], oi.counts)
    assert np.array_equal(got["pos"].reshape(-1), oi.pos_rows())
    assert np.array_equal(got["pair.pos"].reshape(-1), oi.pair_rows())
    assert [bytes(r[:k]).decode() for r in got["kmer"]] == oi.kmer_strings()
    assert not got["kmer"][:, k].any()

    # each opt bit alone: the other pointers NULL, the same bytes as in the full readout
    for opt, f in ((2, "pos"), (4, "pair.pos"), (8, "count"), (1, "kmer")):
        sub = [p.positions_part(gmask, opt) for p in parts]
        for s, full in zip(sub, segs):
            assert [g for g in ("kmer", "pos", "pair.pos", "count") if s[g] is not None] == [f]
            assert torch.equal(s["labels"], full["labels"]) and torch.equal(s[f], full[f])
        if opt & 6:                     # the merge's row offsets come from the parts' counts
            sub = [dict(s, count=full["count"]) for s, full in zip(sub, segs)]
        m = _np(merge_part_positions(sub, opt, k))
        assert [g for g in m if m[g] is not None] == [f]
        assert m[f].tobytes() == want[f].tobytes(), (case, n_parts, opt)

    # the whole-index readers still refuse a part; so does the khash order
    with pytest.raises(_lib.KmhgError, match="assembled"):
        parts[0].positions(8)
    _lib.check(_lib.lib().kmhg_set_row_order(parts[0].handle, _lib.KMHG_ORDER_KHASH))
    with pytest.raises(_lib.KmhgError, match="first-occurrence order only"):
        parts[0].positions_part(gmask, 8)
    for p in parts:
        p.free()


def test_part_entries_refuse_a_whole_index(gpu):
    torch = gpu
    import ctypes as C
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    seq = torch.from_numpy(synth.iid(20_000, 36)).cuda()
    whole = DeviceIndex.build(seq, 21)
    mask = torch.zeros((20_000 + 31) // 32, dtype=torch.int32, device="cuda")
    n = C.c_int64()
    L = _lib.lib()
    for rc in (L.kmhg_part_first_mask(whole.handle, C.c_void_p(mask.data_ptr()), None),
               L.kmhg_part_positions_size(whole.handle, 15, C.byref(n), None, None),
               L.kmhg_part_positions_fill_device(whole.handle, C.c_void_p(mask.data_ptr()), 8,
                                                 None, None, None, None, None, None)):
        assert rc == _lib.KMHG_EINVAL and L.kmhg_last_error() == b"not a part index"
    whole.free()
