"""Generates tests/golden/edlib_edge_pairs.json: what the REFERENCE's edlib returns (oracle/_ref/ref_dumper
--edlib-pairs = edlibAlign(NW, TASK_DISTANCE, k = -1), as for edlib_pairs.json) for the crafted pairs of
tests/edit_craft.py -- route, band and strip edges of the device's edit-distance kernels, the branches of the
homopolymer compression.  Per case: its tag, switches, form and seeded spec (edit_craft.build regenerates the
strings) and six integers: both lengths and the distance, plain and homopolymer-compressed.

    python tests/golden/make_edlib_edge_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edit_craft  # noqa: E402
from helpers import hpc  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    cs = edit_craft.cases()
    pairs = [edit_craft.build(c["spec"]) for c in cs]
    comp = [(hpc(a), hpc(b)) for a, b in pairs]
    plain = O.ref_edlib_distances(pairs)
    hdist = O.ref_edlib_distances(comp)
    assert len(plain) == len(hdist) == len(cs)
    rows = [json.dumps(dict(tag=c["tag"], env=c["env"], use_hpc=c["use_hpc"], spec=c["spec"], n=int(len(a)), m=int(len(b)),
                            dist=int(d), hpc_n=int(len(ha)), hpc_m=int(len(hb)), hpc_dist=int(h)), separators=(",", ":"))
            for c, (a, b), (ha, hb), d, h in zip(cs, pairs, comp, plain, hdist)]
    with open(os.path.join(HERE, "edlib_edge_pairs.json"), "w") as f:
        f.write("[\n" + ",\n".join(rows) + "\n]\n")
    print(len(rows), "pairs; max distance", max(plain))


if __name__ == "__main__":
    main()
