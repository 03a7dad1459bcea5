"""Generates tests/golden/ksw_edge_pairs.json: what the REFERENCE's getAlignmentCigarKsw returns
(oracle/_ref/ref_dumper --ksw-pairs, as for ksw_pairs.json) for the crafted pairs of tests/ksw_craft.py -- class
edges of the device dispatcher, ring wraps, stage flushes, look-ahead and tile edges, tie rules, band-edge paths.
Per case: name, tlen, qlen, the error rate's bit pattern and a sha256 of the CIGAR text; the strings themselves
are rebuilt by ksw_craft.cases().

    python tests/golden/make_ksw_edge_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ksw_craft  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    cs = ksw_craft.cases()
    ksw_craft.assert_claims(cs)
    ref = O.ref_ksw_cigars([(t, q) for _, t, q in cs])
    assert len(ref) == len(cs)
    rows = [json.dumps([name, int(len(t)), int(len(q)), bits, hashlib.sha256(cig.encode()).hexdigest()],
                       separators=(",", ":"))
            for (name, t, q), (bits, cig) in zip(cs, ref)]
    with open(os.path.join(HERE, "ksw_edge_pairs.json"), "w") as f:
        f.write("[\n" + ",\n".join(rows) + "\n]\n")
    print(len(rows), "pairs")


if __name__ == "__main__":
    main()
