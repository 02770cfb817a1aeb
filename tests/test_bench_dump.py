"""bench.py --dump-outputs without a device: the chunk sample is fixed by the inputs and stays under the size bound, and the
files hold the result fields as float64 / float32, concatenated over the sampled chunks in order."""
import os
from types import SimpleNamespace

import numpy as np

import bench


def _fake_chunks(n, sites, reads):
    return [SimpleNamespace(allele_number=np.zeros(sites, np.uint32), reads=[None] * reads) for _ in range(n)]


def _fake_result(i, sites, reads):
    r = np.random.default_rng(i)
    d = dict(ref_start=100 * i, length=sites, reads1=list(range(0, reads, 2)), reads2=list(range(1, reads, 2)),
             hmm_forward=-float(i), hmm_backward=-float(i) - 0.5, n_sweeps=i + 3)
    for k in ("hap1", "hap2", "genotype", "ancestor", "support1", "support2"):
        d[k] = r.integers(0, 40, sites).astype(np.uint64)
    for k in ("genotype_probs", "hap_probs1", "hap_probs2"):
        d[k] = -r.random(sites).astype(np.float32)
    return d


def test_dump_sample_is_fixed_and_bounded():
    chunks = _fake_chunks(1152, 2000, 1700)
    a, b = bench.dump_sample(chunks), bench.dump_sample(chunks)
    assert a == b == sorted(set(a)) and 0 < len(a) <= bench.DUMP_MAX_CHUNKS and max(a) < len(chunks)
    big = bench.dump_sample(_fake_chunks(1152, 200_000, 30_000))
    assert 0 < len(big) < bench.DUMP_MAX_CHUNKS
    assert sum(60 * 200_000 + 8 * 30_000 + 64 for _ in big) <= bench.DUMP_MAX_BYTES


def test_write_dump_round_trip(tmp_path):
    idx = [3, 7, 11]
    res = [_fake_result(i, 50 + i, 20 + i) for i in idx]
    info = bench.write_dump(str(tmp_path / "d"), idx, res)
    files = {f[:-4]: np.load(os.path.join(tmp_path, "d", f)) for f in os.listdir(tmp_path / "d")}
    assert set(files) == set(info["files"]) and info["chunks"] == 3
    assert sum(a.nbytes for a in files.values()) == info["bytes"] <= bench.DUMP_MAX_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert files["chunk_index"].tolist() == idx and files["length"].tolist() == [r["length"] for r in res]
    off = np.concatenate([[0], np.cumsum(files["length"])]).astype(int)
    for j, r in enumerate(res):
        for k, dt in bench.DUMP_SITE_KEYS.items():
            assert files[k].dtype == dt and (files[k][off[j]:off[j + 1]] == r[k]).all(), k
    n1 = np.concatenate([[0], np.cumsum(files["n_reads1"])]).astype(int)
    assert files["reads1"][n1[1]:n1[2]].tolist() == res[1]["reads1"]
    assert files["hmm_forward"].tolist() == [r["hmm_forward"] for r in res]
