"""The partitioned build's plan (kmer_hasher_amd/csrc/kmhg_plan.h: plan_build) on the CPU: the
sanitized stand-alone tools/asan/host_check prints the plan of a request (`host_check plan`), and
this file checks the three benchmark workloads' plans against values derived by hand from the
rules, every forced path at the sizes the GPU suites force it at (test_gpu_stream_formats.py,
test_gpu_bid_pack.py, test_gpu_parts.py), and the plan's invariants over a sweep of requests."""
import time

from test_asan_host import exe, run  # noqa: F401  (exe: the fixture that builds host_check)

MAXR_IL = 320       # kmhg_plan.h V2_MAXR_IL
ROUND = 2048        # one round of the bucket kernel on a 256-CU device: 256 x 8 workgroups
# a stream's first-array bytes per element and whether it keeps a position array (StreamFmt)
FMT = {"Keys": (8, False), "KeyPos": (8, True), "Packed12": (12, False), "Packed8": (8, False),
       "Bids": (4, False), "BidPos": (4, True), "DigitPos": (4, False), "Pos": (0, True)}
BUCKET_INPUT = {"Pos", "Packed12", "KeyPos", "Keys"}      # what launch_v2_bucket_wg accepts


def parse(line):
    if line.startswith("err=") and not line.startswith("err=0"):
        code, msg = line.split(" ", 1)
        return {"err": int(code[4:]), "msg": msg[4:]}
    d = {}
    for tok in line.split():
        name, v = tok.split("=", 1)
        if name == "fmt":
            d[name] = v.split(",")
        elif "," in v or name in ("side", "fused", "ds_out"):
            d[name] = [int(x) for x in v.split(",")]
        else:
            d[name] = int(v)
    return d


def plan(exe, *args):
    return parse(run(exe, "plan", *args)[0])


def test_workload_plans(exe):
    """bench.py's three sizes at a device round of 2,048."""
    p = plan(exe, "seq", "L=10000000", "k=31", f"round={ROUND}")
    assert (p["Nw"], p["nb"], p["passes"], p["R"]) == (9_999_970, 10_240, 2, 102)
    assert -(-9_999_970 // 1024) == 9_766 and 10_240 == 5 * ROUND
    assert p["fmt"] == ["Bids", "DigitPos", "Pos"]
    assert p["bid"] == 1 and p["bid_pack"] == 1 and p["tags"] == 0
    assert p["key_bytes"] == [4, 4] and p["pos_array"] == [0, 1]

    p = plan(exe, "seq", "L=100000000", "k=21", f"round={ROUND}")
    assert (p["Nw"], p["nb"], p["passes"], p["R"]) == (99_999_980, 97_657, 2, 313)
    assert 97_657 > 16 * ROUND
    assert p["fmt"] == ["Keys", "Packed8", "Packed12"]
    assert (p["bid"], p["pack8"], p["sh8"], p["nseg8"], p["ds"], p["tags"]) == (0, 1, 22, 24, 0, 1)

    p = plan(exe, "seq", "L=500000000", "k=31", f"round={ROUND}")
    assert (p["Nw"], p["nb"], p["passes"], p["R"]) == (499_999_970, 488_282, 3, 79)
    assert p["fmt"] == ["Keys", "Packed12", "Packed12", "Packed12"]
    assert (p["bid"], p["ds"], p["ds8"], p["pack8"], p["sh8"], p["tags"]) == (0, 1, 1, 0, 2, 1)


def test_forced_paths(exe):
    bid = ["seq", "L=60000", "k=31", "KMHG_BUILD_BID=1"]
    keys = ["seq", "L=60000", "k=31", "KMHG_BUILD_BID=0"]
    # 59 buckets at radix 8: the digit-pos word, or the two arrays under KMHG_BID_PACK=0
    p = plan(exe, *bid, "KMHG_MAXR=8")
    assert (p["nb"], p["passes"], p["R"], p["fmt"]) == (59, 2, 8, ["Bids", "DigitPos", "Pos"])
    p = plan(exe, *bid, "KMHG_MAXR=8", "KMHG_BID_PACK=0")
    assert p["fmt"] == ["Bids", "BidPos", "Pos"] and p["bid_pack"] == 0
    # three passes keep the two arrays
    p = plan(exe, *bid, "KMHG_MAXR=4")
    assert (p["passes"], p["R"], p["bid_pack"]) == (3, 4, 0)
    assert p["fmt"] == ["Bids", "BidPos", "BidPos", "Pos"]
    # digit streams on key streams, u8 and u16, packed and KeyPos middle streams
    p = plan(exe, *keys, "KMHG_MAXR=4", "KMHG_DIGIT_STREAM=1")
    assert (p["ds"], p["ds8"], p["ds_out"]) == (1, 1, [0, 1, 1, 0])
    assert p["fmt"] == ["Keys", "Packed12", "Packed12", "Packed12"]
    p = plan(exe, *keys, "KMHG_MAXR=4", "KMHG_DIGIT_STREAM=1", "KMHG_DS_U8=0", "KMHG_DS_PACK=0")
    assert (p["ds"], p["ds8"]) == (1, 0)
    assert p["fmt"] == ["Keys", "KeyPos", "KeyPos", "Packed12"]
    assert p["key_bytes"] == [12, 8] and p["pos_array"] == [1, 1]
    # Pack8 at k = 21 (391 buckets, two passes) and KMHG_PACK8=0
    k21 = ["seq", "L=400000", "k=21", "KMHG_BUILD_BID=0"]
    p = plan(exe, *k21)
    assert (p["nb"], p["passes"], p["pack8"], p["sh8"]) == (391, 2, 1, 22)
    assert p["fmt"][1] == "Packed8"
    p = plan(exe, *k21, "KMHG_PACK8=0")
    assert p["pack8"] == 0 and p["fmt"] == ["Keys", "KeyPos", "Packed12"]
    # a compacting part: the dense stream on side 0, pass 0's output on side 1
    pc = ["part=0", "n_parts=2", "KMHG_BUILD_BID=0", "KMHG_PART_COMPACT=1"]
    p = plan(exe, "seq", "L=300000", "k=31", *pc)
    assert (p["partc"], p["first"], p["nbh"], p["nb"], p["passes"]) == (1, 0, 293, 146, 1)
    assert p["fmt"] == ["KeyPos", "Packed12"] and p["side"] == [0, 1]
    p = plan(exe, "seq", "L=400000", "k=21", *pc)
    assert p["R"] == 195 and p["fmt"] == ["Packed12", "Packed12"] and p["side"] == [0, 1]
    assert p["key_bytes"] == [12, 12] and p["pos_array"] == [0, 1]    # side 1: compacted tiles
    p = plan(exe, "seq", "L=300000", "k=31", "part=0", "n_parts=2", "KMHG_BUILD_BID=0",
             "KMHG_PART_COMPACT=0")
    assert p["partc"] == 0 and p["first"] == 1 and p["side"] == [1, 0]
    # more parts than buckets: 3 buckets over 8 parts
    p = plan(exe, "seq", "L=3000", "k=31", "part=0", "n_parts=8")
    assert (p["empty"], p["nb"], p["b0"], p["nbh"]) == (1, 0, 0, 3)
    # count-only with the spread chosen after the passes
    p = plan(exe, "count", "n=100000", "k=21", "spread=0")
    assert p["co_auto"] == 1 and p["nb"] % 12 == 0 and p["nb"] == 12 * -(-100000 // (12 * 1024))
    assert set(p["fmt"]) == {"Keys"} and p["fused"][-1] == 0
    # no plan of four passes
    p = plan(exe, *keys, "KMHG_MAXR=2")
    assert p == {"err": 4, "msg": "sequence too long for the partitioned build"}
    p = plan(exe, "keys", "n=1000", "k=21", "KMHG_MAXR=2")
    assert p["passes"] == 1 and p["side"] == [0, 1] and p["fmt"] == ["Keys", "KeyPos"]


def test_invariants_over_a_sweep(exe, tmp_path):
    windows = [1, 2, 1000, 1024, 1025, 2048, 2049, 4097, 60_000, 340_000, 1 << 20, 3_000_000,
               12 << 20, (12 << 20) + 1, (1 << 24) - 1, 1 << 24, 25_000_000, 66_000_000,
               100_000_000, 200_000_000, 300_000_000]
    reqs = []
    for nw in windows:
        for k in (8, 15, 21, 26, 31, 32):
            for rnd in (0, ROUND):
                for n_parts in (0, 2, 4, 8):
                    for part in range(max(1, n_parts)):
                        reqs.append((nw, k, rnd, n_parts, part,
                                     f"seq L={nw + k - 1} k={k} round={rnd}" +
                                     (f" part={part} n_parts={n_parts}" if n_parts else "")))
        for rnd in (0, ROUND):
            reqs.append((nw, 21, rnd, 0, 0, f"keys n={nw} k=21 round={rnd}"))
            for spread in (0, 1, 4):
                reqs.append((nw, 21, rnd, 0, 0, f"count n={nw} k=21 spread={spread} round={rnd}"))
    path = tmp_path / "requests.txt"
    path.write_text("".join(r[-1] + "\n" for r in reqs))
    t0 = time.perf_counter()
    lines = run(exe, "plan", "@" + str(path))
    took = time.perf_counter() - t0
    plans = [parse(l) for l in lines if l]
    assert len(plans) == len(reqs)
    print(f"{len(plans)} plans in {took:.3f} s")
    assert took < 1.0
    builds = {}
    for (nw, k, rnd, n_parts, part, text), p in zip(reqs, plans):
        assert p.get("err") == 0, (text, p)
        if text.startswith("seq"):
            builds.setdefault((nw, k, rnd), {}).setdefault(n_parts, []).append(p)
        if p["empty"]:
            continue
        assert p["Nw"] == nw
        assert p["R"] ** p["passes"] >= p["nb"] and p["R"] <= MAXR_IL, text
        fmt, side = p["fmt"], p["side"]
        assert len(fmt) == p["passes"] + 1
        stored = range(0 if p["bid"] or p["partc"] else 1, len(fmt))   # index 0 is F(-1)
        for i in stored:
            nbytes, pos = FMT[fmt[i]]
            assert p["key_bytes"][side[i]] >= nbytes, (text, i)
            assert p["pos_array"][side[i]] or not pos, (text, i)
        assert fmt[-1] in BUCKET_INPUT, text
        if "DigitPos" in fmt:
            assert p["passes"] == 2 and p["R"] <= 256 and nw < 1 << 24, text
    for key, by_parts in builds.items():
        whole = by_parts[0][0]
        for n_parts, ps in by_parts.items():
            if not n_parts:
                continue
            end = 0
            for p in ps:                             # in part order
                assert p["nbh"] == whole["nb"] and p["b0"] == end, (key, n_parts)
                end += p["nb"]
            assert end == whole["nb"], (key, n_parts)
