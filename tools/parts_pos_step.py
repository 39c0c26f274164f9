"""Rehearsal of kmer.pos over resident owner-computes parts on ONE GPU (tools, not product): the
n parts of one index built in one process, read with no assembly -- every part's first-occurrence
mask, their sum, every part's labelled readout, the root's merge -- and, in the same run, the
route it replaces: the parts exported into one image (what dist.assemble_parts all-gathers),
kmhg_image_import, and DeviceIndex.positions.  10 Mbp i.i.d. and the 40 Mbp repeat-rich config 4,
k = 31, opt 14 (pos + pair.pos + count), n = 2, 4, 8.  One GPU does every part's work in turn
here, so the phase times are sums over the parts, not a rank's share, and no link is crossed.

    python tools/parts_pos_step.py [out.json] [reps]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPT = 14


def assemble(parts, torch):
    """The parts as one imported index (the single-process form of dist.assemble_parts)."""
    from kmer_hasher_amd import dist as kd
    from kmer_hasher_amd.device import SLOT_BYTES, DeviceIndex
    infos = [p.part_info() for p in parts]
    lay = kd.part_layout(infos)
    dev, capb = parts[0].device, lay["capb"]
    table = torch.empty(lay["slots"] * SLOT_BYTES, dtype=torch.uint8, device=dev)
    positions = torch.empty(max(1, lay["N"] * 4), dtype=torch.uint8, device=dev)
    codes = torch.empty(max(1, lay["codes_bytes"]), dtype=torch.uint8, device=dev)
    code_src = next((r for r, inf in enumerate(infos) if inf["nb"] and inf["codes_bytes"]), 0)
    for r, (p, inf) in enumerate(zip(parts, infos)):
        a, b = inf["b0"] * capb * SLOT_BYTES, lay["pos_base"][r] * 4
        p.export_into(lay["pos_base"][r], table[a:a + inf["nb"] * capb * SLOT_BYTES],
                      table[-SLOT_BYTES:] if r == lay["side_owner"] else None,
                      positions[b:b + inf["n_positions"] * 4], codes if r == code_src else None)
    header = [parts[0].k, parts[0].L, (lay["nb_total"] << 32) | capb, lay["U"], lay["N"],
              lay["P"], lay["max_n"], kd.IMAGE_MAGIC]
    meta = torch.tensor(header + [table.numel(), lay["N"] * 4, lay["codes_bytes"]],
                        dtype=torch.int64)
    torch.cuda.synchronize()
    return DeviceIndex.import_image(meta, [table, positions, codes])


def main():
    import torch
    from kmer_hasher_amd import device as D
    from kmer_hasher_amd import synth
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "parts_pos_step.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    k = 31

    def now():
        torch.cuda.synchronize()
        return time.perf_counter()

    def parts_route(parts, ph):
        t0 = now()
        gmask = torch.stack([p.first_mask() for p in parts]).sum(0, dtype=torch.int32)
        t1 = now()
        segs = [p.positions_part(gmask, OPT) for p in parts]
        t2 = now()
        res = D.merge_part_positions(segs, OPT, k)
        t3 = now()
        for name, dt in (("mask", t1 - t0), ("readout", t2 - t1), ("merge", t3 - t2),
                         ("total", t3 - t0)):
            ph.setdefault(name, []).append(dt * 1e3)
        return res

    def assemble_route(parts, ph):
        t0 = now()
        idx = assemble(parts, torch)
        t1 = now()
        res = idx.positions(OPT)
        t2 = now()
        idx.free()
        for name, dt in (("assemble", t1 - t0), ("positions", t2 - t1), ("total", t2 - t0)):
            ph.setdefault(name, []).append(dt * 1e3)
        return res

    report = {"k": k, "opt": OPT, "reps": reps, "device": torch.cuda.get_device_name(0),
              "note": "one GPU runs every part in turn; ms are medians over reps after one "
                      "warm-up of each route, routes alternated; no run on more than one GPU",
              "configs": {}}
    for name, make in (("iid_10Mbp", lambda: synth.iid(10_000_000, 1)),
                       ("config4_40Mbp", lambda: synth.config4(40_000_000, 3))):
        seq = torch.from_numpy(make()).to(dev)
        rows = {}
        for n in (2, 4, 8):
            parts = [D.DeviceIndex.build_part(seq, k, p, n) for p in range(n)]
            a, b = parts_route(parts, {}), assemble_route(parts, {})      # warm-up + check
            same = all(torch.equal(a[f], b[f]) for f in ("pos", "pair.pos", "count"))
            sizes = {f: int(a[f].shape[0]) for f in ("pos", "pair.pos", "count")}
            del a, b
            pa, pb = {}, {}
            for _ in range(reps):
                parts_route(parts, pa)
                assemble_route(parts, pb)
            med = lambda d: {f: round(statistics.median(v), 3) for f, v in d.items()}  # noqa: E731
            rows[n] = {"identical": same, "rows": sizes, "parts_ms": med(pa),
                       "assemble_ms": med(pb),
                       "parts_total_min_max_ms": [round(min(pa["total"]), 3),
                                                  round(max(pa["total"]), 3)],
                       "assemble_total_min_max_ms": [round(min(pb["total"]), 3),
                                                     round(max(pb["total"]), 3)],
                       "ratio_parts_over_assemble": round(
                           statistics.median(pa["total"]) / statistics.median(pb["total"]), 3)}
            print(name, n, json.dumps(rows[n]), flush=True)
            for p in parts:
                p.free()
        report["configs"][name] = {"L": int(seq.numel()), "parts": rows}
        del seq
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
