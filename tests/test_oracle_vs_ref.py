"""Live check of the oracle against the compiled reference (only where build()
could compile oracle/_ref, i.e. where the reference sources are).  Minimizer
configs only: the reference's raw-read build spends ~90 s in its 8 GiB flat
counter, the raw path is covered by the golden vectors."""
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="reference build not available")

# the reference's shipped config files, stored as settings fixtures (tests/test_config.py)
REF_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bin_cfg")


# with the golden vectors at k = 15, 18 and 31 (tests/test_oracle_golden.py) this pins the oracle to the reference at
# k = 11, 13, 15, 17, 18, 25 and 31; below 11, at 16 and at 32 nobody has compared them (32: the reference's own
# k-mer mask is undefined there)
@pytest.mark.parametrize("preset,kind,opts", [
    ("hifi", "hifi", dict()),
    ("corrected", "hifi03", dict(rc_queries=True, max_overlaps=15)),
    ("subasm", "hifi", dict()),
    ("hifi", "hifi", dict(kmer_size=25)),
    ("corrected", "hifi03", dict(kmer_size=11, coverage=8)),      # short k-mers: many seed hits per read pair
    ("raw", "pb_raw", dict(kmer_size=13)),                        # solid build; the flat counter is small below 17
])
def test_oracle_equals_reference(built, tmp_path, preset, kind, opts):
    from flye_amd import config, synth
    fa = str(tmp_path / "r.fasta")
    rs = synth.simulate(seed=4242, genome_len=30_000, coverage=opts.get("coverage", 20), kind=kind, fasta_path=fa).filter_min_len(1000)
    cfg = config.preset(preset)
    k = int(opts.get("kmer_size", cfg["kmer_size"]))
    info = O.run_ref(fa, config=os.path.join(REF_CFG, config.CFG_FILES[preset]), threads=4,
                     params_string=f"kmer_size={k}" if "kmer_size" in opts else None,
                     min_read_len=1000, index_out=str(tmp_path / "i.txt"), ovlp_out=str(tmp_path / "o.txt"),
                     rc_queries=opts.get("rc_queries", False), max_overlaps=opts.get("max_overlaps", 0))
    o = O.Oracle(k, threads=4)
    o.set_reads(rs)
    st = o.build_index(cfg)
    hdr, refidx = O.parse_ref_index(str(tmp_path / "i.txt"), rs)
    assert o.export_index().same_as(refidx)
    assert np.float32(st["sample_rate"]).view(np.uint32) == int(hdr["sampleRateBits"], 16)
    q = np.arange(1 if opts.get("rc_queries") else 0, 2 * rs.n, 2)
    res = o.overlaps(O.detector_params(cfg), q, max_overlaps=opts.get("max_overlaps", 0))
    ref = [l.strip() for l in open(tmp_path / "o.txt") if not l.startswith("#")]
    assert res.lines() == ref and len(ref) == info["overlaps"] > 0
