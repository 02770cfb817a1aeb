"""mrp_equal_substring_classes (the classes of equal substrings of every site, found on the device) against a grouping made on the
host: one call holding every shape, then every site alone, then the call again."""
import numpy as np
import pytest

from margin_amd import capi

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 200)  # around the wave's 64 lanes; 200: several strides of the lanes


def kernel_key(strings: np.ndarray) -> np.ndarray:
    """the kernel's key of n strings of one length (uint8 [n, length]): length << 32 | FNV-1a (32 bit) of the symbols"""
    h = np.full(len(strings), 2166136261, np.uint64)
    for i in range(strings.shape[1]):
        h = ((h ^ strings[:, i].astype(np.uint64)) * np.uint64(16777619)) & np.uint64(0xFFFFFFFF)
    return (np.uint64(strings.shape[1]) << np.uint64(32)) | h


def same_key_pair():
    """two distinct strings of one length with one key: a birthday search over every string of 8 symbols from the 5-symbol alphabet
    (5^8 = 390 625 strings against 2^32 hashes: about 18 pairs are expected)"""
    n, length = 5 ** 8, 8
    idx = np.arange(n)
    strings = np.stack([(idx // 5 ** k) % 5 for k in range(length)], axis=1).astype(np.uint8)
    key = kernel_key(strings)
    order = np.argsort(key, kind="stable")
    hit = np.flatnonzero(key[order][1:] == key[order][:-1])
    assert len(hit) > 0, "no two strings with one key: the search space is too small"
    a, b = strings[order[hit[0]]], strings[order[hit[0] + 1]]
    assert (a != b).any() and kernel_key(a[None])[0] == kernel_key(b[None])[0]
    return a, b


def host_classes(sites):
    """per site a list of uint8 arrays -> rep per entry, as indices within the call"""
    rep, base = [], 0
    for subs in sites:
        first = {}
        for k, s in enumerate(subs):
            rep.append(base + first.setdefault(bytes(s), k))
        base += len(subs)
    return np.array(rep, np.int32)


def arrays(sites):
    first = np.zeros(len(sites) + 1, np.int64)
    np.cumsum([len(s) for s in sites], out=first[1:])
    flat = [s for subs in sites for s in subs]
    length = np.array([len(s) for s in flat], np.int32)
    rng = np.random.default_rng(5)
    # the substrings lie in the pool in a shuffled order, with gaps: offsets carry no meaning
    order = rng.permutation(len(flat))
    off = np.zeros(len(flat), np.int64)
    parts, at = [], 3
    parts.append(np.full(3, 9, np.uint8))
    for k in order:
        off[k] = at
        parts.append(flat[k])
        parts.append(np.full(int(rng.integers(0, 3)), 9, np.uint8))
        at += len(flat[k]) + len(parts[-1])
    return first, np.concatenate(parts).astype(np.uint8), off, length


@pytest.fixture(scope="module")
def sites():
    rng = np.random.default_rng(17)
    sym = lambda n: rng.integers(0, 5, size=n).astype(np.uint8)
    out = []
    for n in SIZES:  # a few distinct strings, each many times over, and a few singletons
        base = [sym(int(rng.integers(1, 40))) for _ in range(max(1, n // 6))]
        out.append([base[int(rng.integers(0, len(base)))].copy() if rng.random() < 0.8 else sym(int(rng.integers(0, 40))) for _ in range(n)])
    one = sym(25)
    out.append([one.copy() for _ in range(70)])                               # all equal
    out.append([np.concatenate([sym(12), np.array([k % 5, k // 5 % 5, k // 25], np.uint8)]) for k in range(70)])  # none equal
    a = sym(30)
    b = a.copy()
    b[29] = (b[29] + 1) % 5
    c = a.copy()
    c[0] = (c[0] + 1) % 5
    out.append([a, b, c, a.copy(), b.copy()])                                 # equal length, different bytes (first and last symbol)
    out.append([a, a[:29].copy(), a[:1].copy(), a.copy(), a[:29].copy()])     # equal prefix, different length
    out.append([np.zeros(0, np.uint8), np.array([0], np.uint8), np.zeros(0, np.uint8), np.array([1], np.uint8), np.array([0], np.uint8)])  # length 0 beside length 1
    p, q = same_key_pair()
    out.append([p, q, p.copy(), sym(8), q.copy()])                            # one key, different bytes: decided by the symbols
    out.append([sym(20), sym(20)] + [out[1][0].copy()])                       # the last site of the call; a string of another site is no match
    return out


def test_classes_equal_the_host_grouping(sites):
    want = host_classes(sites)
    first, pool, off, length = arrays(sites)
    assert want[first[8]:first[9]].tolist() == list(range(int(first[8]), int(first[9])))  # the site where none are equal
    assert (want[first[7]:first[8]] == first[7]).all()                                    # the site where all are
    with capi.Context(0) as ctx:
        got = capi.equal_substring_classes(ctx, first, pool, off, length)
        assert got.dtype == np.int32 and (got == want).all(), np.flatnonzero(got != want)[:10]
        again = capi.equal_substring_classes(ctx, first, pool, off, length)
        assert (again == got).all()
        # every site alone: its classes do not depend on its neighbours
        for v, subs in enumerate(sites):
            f1, p1, o1, l1 = arrays([subs])
            alone = capi.equal_substring_classes(ctx, f1, p1, o1, l1)
            assert (alone == want[first[v]:first[v + 1]] - first[v]).all(), v
        # no site, and sites without entries only
        assert capi.equal_substring_classes(ctx, np.zeros(1, np.int64), pool, [], []).size == 0
        assert capi.equal_substring_classes(ctx, np.zeros(4, np.int64), pool, [], []).size == 0
