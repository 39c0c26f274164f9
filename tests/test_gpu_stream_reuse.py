"""Same-stream block reuse on the GPU: builds queued back to back on one stream take over the
blocks of builds freed unwaited before them, with no host wait in between (kmhg_pool.h), so a
kept index (A) and the last of the chain (D) are the ones a wrong reuse would damage: a later
build writing into blocks an earlier one still reads, or into A's.  kmer.pos of both against the
oracle.  Shapes: L = 5,000 (one tile) and L = 70,000 (many tiles, two radix passes) at k = 31,
L = 300 at k = 5 (a tiny build)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(5_000, 31), (70_000, 31), (300, 5)]
_CACHE = {}


def case(L, k, seed):
    """(sequence, its oracle index), made once per (L, k, seed) and never changed."""
    key = (L, k, seed)
    if key not in _CACHE:
        from kmer_hasher_amd import synth
        s = synth.iid(L, seed).copy()
        if L >= 1000:                   # repeated k-mers (pair.pos rows) and a few N runs
            r = np.random.default_rng(seed)
            for _ in range(8):
                n = int(r.integers(k, L // 10))
                a, b = (int(x) for x in r.integers(0, L - n, 2))
                s[b:b + n] = s[a:a + n].copy()
            s = synth.add_n_runs(s, 0.002, seed + 1, max_run=20)
        s.setflags(write=False)
        _CACHE[key] = (s, O.OracleIndex(s.tobytes(), k))
    return _CACHE[key]


def check(idx, oi, stream):
    res = idx.positions(15, stream)
    stream.synchronize()
    inf = idx.info()
    assert (inf["n_kmers"], inf["n_positions"], inf["n_pairs"]) == (oi.U, oi.N, oi.P)
    assert inf["fallback"] == 0
    assert np.array_equal(res["count"].cpu().numpy(), oi.counts)
    assert np.array_equal(res["pos"].cpu().numpy().reshape(-1), oi.pos_rows())
    assert np.array_equal(res["pair.pos"].cpu().numpy().reshape(-1), oi.pair_rows())
    k = inf["k"]
    assert [bytes(r[:k]).decode() for r in res["kmer"].cpu().numpy()] == oi.kmer_strings()


def chain(torch, shapes, stream):
    """Build A (kept), B and C (freed unwaited), D on `stream`, shapes[i % len] each from a
    sequence of its own; A and D against the oracle."""
    from kmer_hasher_amd.device import DeviceIndex
    cs = [case(*shapes[i % len(shapes)], seed=11 + i) for i in range(4)]
    ks = [shapes[i % len(shapes)][1] for i in range(4)]
    ts = [torch.from_numpy(c[0].copy()).cuda() for c in cs]
    torch.cuda.synchronize()
    a = DeviceIndex.build(ts[0], ks[0], stream)
    DeviceIndex.build(ts[1], ks[1], stream).free()
    DeviceIndex.build(ts[2], ks[2], stream).free()
    d = DeviceIndex.build(ts[3], ks[3], stream)
    check(d, cs[3][1], stream)
    check(a, cs[0][1], stream)
    a.free()
    d.free()
    stream.synchronize()


@pytest.mark.parametrize("L,k", SHAPES)
def test_a_chain_of_builds_on_one_stream(gpu, L, k):
    chain(gpu, [(L, k)], gpu.cuda.Stream())


@pytest.mark.parametrize("L,k", SHAPES)
def test_a_chain_of_builds_on_the_null_stream(gpu, L, k):
    chain(gpu, [(L, k)], gpu.cuda.default_stream())


@pytest.mark.parametrize("shapes", [[SHAPES[0], SHAPES[1]], [SHAPES[1], SHAPES[2]],
                                    [SHAPES[2], SHAPES[0]]])
def test_a_chain_of_alternating_lengths(gpu, shapes):
    chain(gpu, shapes, gpu.cuda.Stream())


@pytest.mark.parametrize("L,k", SHAPES)
def test_a_build_behind_another_streams_freed_build_waits(gpu, L, k):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    (s1, _), (s2, o2) = case(L, k, seed=21), case(L, k, seed=22)
    t1, t2 = torch.from_numpy(s1.copy()).cuda(), torch.from_numpy(s2.copy()).cuda()
    torch.cuda.synchronize()
    st1, st2 = torch.cuda.Stream(), torch.cuda.Stream()
    DeviceIndex.build(t1, k, st1).free()
    b = DeviceIndex.build(t2, k, st2)
    check(b, o2, st2)
    b.free()
    torch.cuda.synchronize()


def test_a_second_round_of_chains_makes_no_device_allocation(gpu):
    """One child process with the test build and KMHG_POOL_TRACE=1 (tests/stream_reuse_child.py):
    the chains above, twice; after the marker no allocation is traced."""
    sys.path.insert(0, HERE)
    from stream_reuse_child import MARKER
    env = dict(os.environ, KMHG_LIB_VARIANT="test", KMHG_POOL_TRACE="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable,
                        os.path.join(HERE, "stream_reuse_child.py")], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [l.split() for l in r.stdout.split("\n") if l]
    assert [l[0] for l in out] == ["round", "round"], r.stdout
    assert out[0][2:] == out[1][2:], r.stdout             # (U, N, P) of every kept index
    err = r.stderr.split("\n")
    assert err.count(MARKER) == 1, r.stderr[-4000:]
    at = err.index(MARKER)
    first = sum("kmhg pool: hipMalloc" in l for l in err[:at])
    second = sum("kmhg pool: hipMalloc" in l for l in err[at:])
    print("hipMalloc lines: first round", first, "second round", second)
    assert first > 0                                      # the trace is on
    assert second == 0
