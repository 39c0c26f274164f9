"""Generate tests/golden/fq_sh_golden.json (count.kmers.fq.sh / kmer.spec.sh) from the compiled
reference, through tests/ref_fq_sh.py (needs oracle/_ref/libkmh_ref_sh.so: ``make -C oracle``):

    python tests/golden/make_fq_sh_golden.py

Recorded per case: U, sha256 of the sorted keys and of their counts, the spectra (digest, and
the list when short), and the full key / count lists for cases under 400 keys.  Cases: the
reference's own fixtures with test.R's parameter shapes, and the seeded edge records of
tests/fq_sh_inputs.py.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from kmh_canon import sha  # noqa: E402
import fq_sh_inputs as I  # noqa: E402
import ref_fq_sh as R  # noqa: E402


def record(name, ref):
    keys, cnt = ref.arrays()
    rec = {"name": name, "U": int(len(keys)), "keys_sha": sha(keys), "counts_sha": sha(cnt),
           "spectra": {}}
    for mc in I.SPECTRA:
        sp = ref.spectrum(mc)
        rec["spectra"][str(mc)] = {"sha": sha(sp)}
        if mc <= 10:
            rec["spectra"][str(mc)]["counts"] = sp.tolist()
    if len(keys) < 400:
        rec["keys"] = [int(x) for x in keys]
        rec["counts"] = [int(x) for x in cnt]
    ref.close()
    return rec


def file_case(name):
    calls = I.FILE_CASES[name]
    k = calls[0][1][0]
    ref = R.RefSH1(k, calls[0][1][2], calls[0][1][3])
    for f, prm in calls:
        ref.add_fastx(os.path.join(I.GOLDEN, f), prm)
    return record(name, ref)


def seeded_case(name, k, records, min_quality):
    ref = R.RefSH1(k, I.prefix_bits_for(k))
    ref.add_records(records, min_quality)
    return record(name, ref)


def all_cases():
    out = [file_case(n) for n in I.FILE_CASES]
    for k in I.LANE_KS:
        for n, (recs, mq) in I.lane_cases(k).items():
            out.append(seeded_case(f"lane_k{k}_{n}", k, recs, mq))
    for k in I.FA_KS:
        for n, recs in I.fa_cases(k).items():
            out.append(seeded_case(f"fa_k{k}_{n}", k, recs, I.MQ))
    return out


def main():
    out = {"source": "oracle/_ref/libkmh_ref_sh.so (the reference's init_kmer_qual_2, "
                     "init_suffix_hash_p, sh_add_kmer, sh_kmer_count, sh_count_spectrum) driven by "
                     "tests/ref_fq_sh.py",
           "cases": all_cases()}
    with open(I.golden_path(), "w") as fh:
        json.dump(out, fh, indent=0)
    print(len(out["cases"]), "cases", file=sys.stderr)


if __name__ == "__main__":
    main()
