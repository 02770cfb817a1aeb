"""mrp_allele_read_supports_rle, mrp_rle_lane_caps and mrp_context_set_rle_lane_pairs without a device: the exports, the caps'
arithmetic, every MRP_ERR_ARG of the supports entry with a NULL context (raised before the context is looked at, nothing written), and
the C example's build."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import posterior_cases as pc
from tests import rle_lane_cases as lc


def test_exports_and_abi():
    L = capi.load()
    assert capi.ABI_VERSION == L.mrp_abi_version() == 6  # additions only
    for name in ("mrp_context_set_rle_lane_pairs", "mrp_rle_lane_caps", "mrp_allele_read_supports_rle"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    assert L.mrp_context_set_rle_lane_pairs(None, 1) == capi.MRP_ERR_ARG


# ---- mrp_rle_lane_caps -------------------------------------------------------------------------------------------------------------

LDS_BYTES = 160 * 1024
BYTES_PER_X = 3 * 64 * 8 + 64  # three states per lane and the lane's symbol, per wave and x position


@pytest.mark.parametrize("n_models", [1, 2, 3, 8, 13])
def test_lane_caps(n_models):
    caps, bound = capi.rle_lane_caps(n_models)
    assert bound >= 2
    assert all(caps[c] <= caps[c + 1] for c in range(3)) and caps[3] <= 100 and caps[0] >= 0
    # the arithmetic, stated a second time: coef, etab, em and the compact repeat table, then rows of 1 600 B per wave and x position
    left = LDS_BYTES - 8 * (16 + n_models * (150 + 25 + 5 * bound * bound))
    assert caps == [min(100, left // BYTES_PER_X, left // ((4 - c) * BYTES_PER_X)) for c in range(4)]


def test_lane_caps_of_two_models_keep_four_waves_up_to_21_symbols():
    assert capi.rle_lane_caps(2) == ([21, 29, 43, 87], 16)


@pytest.mark.parametrize("n_models", [14, 100, 256])
def test_lane_caps_without_room_for_a_row(n_models):
    assert capi.rle_lane_caps(n_models)[0] == [-1, -1, -1, -1]


def test_lane_caps_arguments():
    L = capi.load()
    assert L.mrp_rle_lane_caps(0, None, None) == capi.MRP_ERR_ARG and L.mrp_rle_lane_caps(-1, None, None) == capi.MRP_ERR_ARG
    assert L.mrp_rle_lane_caps(2, None, None) == capi.MRP_OK  # either output may be NULL
    bound = C.c_int32(0)
    assert L.mrp_rle_lane_caps(2, None, C.byref(bound)) == capi.MRP_OK and bound.value == 16


# ---- the argument errors ------------------------------------------------------------------------------------------------------------

WHO = "mrp_allele_read_supports_rle"
R = 4


class Call:
    """one bubble of two alleles and three reads as the C entry takes it; every field can be replaced (None: a NULL pointer)"""

    def __init__(self):
        self.m = pc.model()
        self.fr = capi.RepeatModel(np.zeros((4, R, R)), 1)
        self.rr = capi.RepeatModel(np.zeros((4, R, R)), 0)
        self.pool = np.array([0, 1, 2, 3, 0, 1, 3, 0, 1, 2, 1, 1, 2, 0, 1, 2], np.uint8)
        self.counts = np.array([1, 2, 0, 3, 1, 1, 3, 1, 2, 3, 0, 2, 1, 1, 2, 3], np.uint8)
        self.allele_first = np.array([0, 2], np.int64)
        self.read_first = np.array([0, 3], np.int64)
        self.allele_off, self.allele_len = np.array([0, 4], np.int64), np.array([4, 3], np.int32)
        self.read_off, self.read_len = np.array([7, 10, 13], np.int64), np.array([3, 3, 3], np.int32)
        self.strand = np.array([1, 0, 1], np.uint8)
        self.support = np.full(6, 7.0, np.float32)
        self.forward_model = self.reverse_model = self.m
        self.forward_repeat, self.reverse_repeat = self.fr, self.rr
        self.n_bubbles, self.expansion = 1, 4

    def run(self, ctx=None):
        p = lambda a: None if a is None else a.ctypes.data
        s = lambda r: None if r is None else C.byref(r)
        keep = [None if r is None else r.struct() for r in (self.forward_repeat, self.reverse_repeat)]
        rc = capi.load().mrp_allele_read_supports_rle(
            ctx, s(self.forward_model), s(self.reverse_model), s(keep[0]), s(keep[1]), self.n_bubbles, p(self.allele_first), p(self.read_first), p(self.pool),
            p(self.counts), self.pool.size if self.pool is not None else 16, p(self.allele_off), p(self.allele_len), p(self.read_off), p(self.read_len),
            p(self.strand), self.expansion, p(self.support), None)
        return rc, capi.load().mrp_last_error().decode()


def expect(code, text, **fields):
    c = Call()
    support = c.support
    for k, v in fields.items():
        setattr(c, k, v)
    rc, msg = c.run()
    assert rc == code, msg
    assert text in msg and WHO in msg, msg
    assert (support == 7.0).all()  # nothing written


@pytest.mark.parametrize("field", ["forward_model", "reverse_model", "forward_repeat", "reverse_repeat", "allele_first", "read_first", "pool", "allele_off",
                                   "allele_len", "read_off", "read_len", "strand", "support"])
def test_every_null_is_an_argument_error(field):
    expect(capi.MRP_ERR_ARG, "null argument", **{field: None})


def test_null_counts():
    expect(capi.MRP_ERR_ARG, "counts is NULL", counts=None)


def test_arg_errors_come_before_the_context():
    i64, i32 = (lambda *v: np.array(v, np.int64)), (lambda *v: np.array(v, np.int32))
    expect(capi.MRP_ERR_ARG, "bad sizes", n_bubbles=-1)
    expect(capi.MRP_ERR_ARG, "read substring 2 lies outside the pool", read_off=i64(7, 10, 14))
    expect(capi.MRP_ERR_ARG, "read substring 0 lies outside the pool", read_len=i32(-1, 3, 3))
    expect(capi.MRP_ERR_ARG, "allele 1 lies outside the pool", allele_off=i64(0, 15))
    expect(capi.MRP_ERR_ARG, "allele 0 lies outside the pool", allele_off=i64(-1, 4))
    expect(capi.MRP_ERR_ARG, "offsets not ascending at bubble 1", n_bubbles=2, read_first=i64(0, 3, 2), allele_first=i64(0, 1, 2))
    expect(capi.MRP_ERR_ARG, "offsets not ascending at bubble 1", n_bubbles=2, read_first=i64(0, 3, 3), allele_first=i64(0, 2, 1))
    expect(capi.MRP_ERR_ARG, "offsets not ascending at bubble 0", n_bubbles=2, read_first=i64(0, -1, 3), allele_first=i64(0, 1, 2))
    expect(capi.MRP_ERR_ARG, "offsets must start at 0", read_first=i64(1, 3))
    expect(capi.MRP_ERR_ARG, "offsets must start at 0", allele_first=i64(2, 2))
    for bad in (1, 0, -3, 257):
        expect(capi.MRP_ERR_ARG, f"repeat model 0: max_repeat {bad} outside [2, 256]", forward_repeat=capi.RepeatModel(np.zeros((4, R, R)), 1, max_repeat=bad))
        expect(capi.MRP_ERR_ARG, f"repeat model 1: max_repeat {bad} outside [2, 256]", reverse_repeat=capi.RepeatModel(np.zeros((4, R, R)), 0, max_repeat=bad))
    expect(capi.MRP_ERR_ARG, "repeat model 1: strand must be 0 or 1", reverse_repeat=capi.RepeatModel(np.zeros((4, R, R)), 2))
    expect(capi.MRP_ERR_ARG, "repeat model 0 has no log_prob", forward_repeat=capi.RepeatModel(None, 1, max_repeat=R))
    expect(capi.MRP_ERR_ARG, "diagonalExpansion must be even", expansion=3)
    # a count equal to R; the message names where
    counts = Call().counts
    bad = counts.copy(); bad[11] = R
    expect(capi.MRP_ERR_ARG, "bubble 0: the count 4 of symbol 1 of read 1 is not below max_repeat 4", counts=bad)
    bad = counts.copy(); bad[5] = R
    expect(capi.MRP_ERR_ARG, "bubble 0: the count 4 of symbol 1 of allele 1 is not below max_repeat 4", counts=bad)
    # against the max_repeat of the strand that scores it: the reverse strand's model has R = 3, read 1 (reverse) holds a 3 ...
    small = capi.RepeatModel(np.zeros((4, 3, 3)), 0)
    bad = counts.copy(); bad[[3, 6, 9, 15]] = 2; bad[10] = 3
    expect(capi.MRP_ERR_ARG, "the count 3 of symbol 0 of read 1 is not below max_repeat 3", counts=bad, reverse_repeat=small)
    # ... and with only forward reads owning scores the alleles' counts of 3 pass
    ok = counts.copy(); ok[10:13] = ok[7:10]  # read 1 repeats read 0: it copies, its strand's model scores nothing
    pool = Call().pool
    pool[10:13] = pool[7:10]
    expect(capi.MRP_ERR_NO_DEVICE, "no context", counts=ok, pool=pool, reverse_repeat=small)


def test_a_valid_call_without_a_context_has_no_device():
    expect(capi.MRP_ERR_NO_DEVICE, "no context")
    expect(capi.MRP_ERR_NO_DEVICE, "no context", n_bubbles=0, allele_first=None, read_first=None, allele_off=None, allele_len=None, read_off=None, read_len=None,
           strand=None, support=None)
    with pytest.raises(capi.MrpError) as e:
        capi.allele_read_supports_rle(None, pc.model(), pc.model(), capi.RepeatModel(lc.example_table(), 1), capi.RepeatModel(lc.example_table(), 0),
                                      [lc.example_bubble()], expansion=lc.EXAMPLE_EXPANSION)
    assert e.value.code == capi.MRP_ERR_NO_DEVICE


# ---- the C example ----------------------------------------------------------------------------------------------------------------

def test_c_example_builds_and_compresses_without_a_device(tmp_path):
    exe = lc.build_example(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is tests/test_gpu_rle_lane.py's)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "mrp_context_create" in r.stderr
    assert r.stdout.splitlines() == lc.example_compressed_lines()  # the compression needs no device
