"""bench.py's setup without a device: the chunks made by its process pool are the generator's own, in seed order, and the
legs beside the headline run only when asked for."""
import numpy as np

import bench
from margin_amd import capi, synth


def test_make_chunks_matches_the_generator():
    seeds = [3, 1, 7, 2, 9, 4, 5]
    kw = dict(region_bp=60_000, n_sites=120, coverage=12.0)
    got = bench.make_chunks(seeds, 3, **kw)
    assert len(got) == len(seeds)
    for s, g in zip(seeds, got):
        want = synth.make_ont_chunk(seed=s, **kw)
        for k in ("allele_number", "allele_offset", "sub", "prior", "pool", "hap1", "hap2"):
            a, b = getattr(g, k), getattr(want, k)
            assert a.dtype == b.dtype and np.array_equal(a, b), k
        assert g.reads == want.reads and g.units == want.units
        assert getattr(g, "_mrp_records", None) is not None  # built by make_chunks as the chunk arrived
        recs, names = capi.read_records(g)
        assert recs is g._mrp_records[0] and names == [r.name.encode() for r in want.reads]
        assert [recs[i].pool_offset for i in range(len(g.reads))] == [r.pool_off for r in want.reads]


def test_plain_run_is_the_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True
