"""The host halves of mrp_poa_augment and mrp_poa_consensus, no device: the restatement (tests/poa_oracle.py) on the reference's only
vector, every argument error of mrp_poa_augment in the header's order with the outputs untouched and then the NULL context,
mrp_poa_consensus against the restatement, and the stand-alone host check under the sanitizers."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from margin_amd import capi
from tests import poa_cases as cases
from tests import poa_edge_cases as edge
from tests import poa_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "mrp_poa_augment"


def test_symbols_exported_and_transcribed():
    lib = capi.load()
    for name in ("mrp_poa_augment", "mrp_poa_free", "mrp_poa_consensus"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert capi.ABI_VERSION == lib.mrp_abi_version() == 6  # additions only
    assert C.sizeof(capi.PoaOptions) == 32 and C.sizeof(capi.Poa) == 24 * 8 and C.sizeof(capi.PoaStats) == 18 * 8
    with open(os.path.join(ROOT, "include", "margin_rphmm.h")) as f:
        header = f.read()
    assert header.index("int64_t mrp_rle_expand(") < header.index("int mrp_poa_augment(") < header.index("int mrp_poa_consensus(")


# ---- the reference's vector -----------------------------------------------------------------------------------------------------------

def vector_call():
    with open(os.path.join(ROOT, "tests", "golden", "poa", "augment_example.json")) as f:
        v = json.load(f)
    swap = lambda l: [(x, y, w) for w, x, y in l]
    rd = cases.read(cases.SYM(v["read"]), [1] * len(v["read"]), 1, swap(v["matches"]), swap(v["deletes"]), swap(v["inserts"]))
    return v, [cases.consensus(cases.SYM(v["reference"]), None, [rd])]


def test_the_restatement_reproduces_the_references_vector():
    v, call = vector_call()
    _, (poa,), st = cases.want(call, 51, merge=False)
    assert len(poa["nodes"]) == len(v["nodes"]) == 8 and (st["complete_inserts"], st["complete_deletes"]) == (4, 2)
    for node, want in zip(poa["nodes"], v["nodes"]):
        assert "ACGTN"[node["base"]] == want["base"] and node["base_weights"] == want["base_weights"]
        assert [["".join("ACGTN"[b] for b in e["symbols"]), e["forward"]] for e in node["inserts"]] == want["inserts"]
        assert [[e["length"], e["forward"]] for e in node["deletes"]] == want["deletes"]
        assert all(e["reverse"] == 0.0 for e in node["inserts"] + node["deletes"])
    # the order of a read's entries does not matter
    rng = np.random.default_rng(3)
    rd = call[0]["reads"][0]
    mixed = [dict(call[0], reads=[dict(rd, **{k: [rd[k][i] for i in rng.permutation(len(rd[k]))] for k in ("matches", "deletes", "inserts")})])]
    w0, w1 = cases.want(call, 51, merge=False)[0], cases.want(mixed, 51, merge=False)[0]
    cases.assert_equal(dict(w1, stats=None), w0)


def test_the_edge_call_holds_what_it_claims():
    edge.assert_claims()


# ---- the argument errors, in the header's order ------------------------------------------------------------------------------------------

def small():
    """two consensus strings: 3 positions under 2 reads (the second cropped by 1), 2 positions under 1 read"""
    a = cases.consensus([0, 1, 4], [1, 2, 3], [
        cases.read([0, 1, 2], [1, 2, 3], 1, [(0, 0, 5), (1, 1, 7), (2, 2, 1)], [(1, 0, 4)], [(0, 1, 3), (-1, 0, 2)]),
        cases.read([1, 3], [2, 9], 0, [(0, 0, 3), (1, 1, 4)], [(0, -1, 6)], [(1, 1, 2)], x_shift=1)])
    b = cases.consensus([2, 3], [1, 1], [cases.read([2, 3], [1, 1], 1, [(0, 0, 9), (1, 1, 9)], [], [])])
    return [a, b]


NAMES = ("node_first", "symbols", "ref_counts", "read_first", "read_symbols", "read_counts", "y_off", "y_len", "read_forward_strand", "matches",
         "deletes", "inserts")


def call(call_=None, ctx=None, R=12, **kw):
    args, x_shift = cases.pack(small() if call_ is None else call_)
    p = dict(zip(NAMES, args), x_shift=x_shift)
    p.update({k: kw.pop(k) for k in list(kw) if k in p})
    return capi.poa_augment(ctx, R, **p, **kw)  # (asserts that the outputs came back untouched from an error)


def expect(code, text, **kw):
    with pytest.raises(capi.MrpError) as e:
        call(**kw)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value) and WHO in str(e.value), str(e.value)


def changed(which, key, at, value):
    args, _ = cases.pack(small())
    l = {k: v.copy() for k, v in dict(zip(NAMES, args))[which].items()}
    l[key][at] = value
    return {which: l}


def test_null_context_comes_after_the_checks():
    expect(capi.MRP_ERR_NO_DEVICE, "no context")
    expect(capi.MRP_ERR_NO_DEVICE, "no context", call_=[])
    expect(capi.MRP_ERR_NO_DEVICE, "no context", x_shift=None, **changed("matches", "x", 3, 1), **changed("deletes", "x", 1, 1), **changed("inserts", "x", 2, 2))
    expect(capi.MRP_ERR_NO_DEVICE, "no context", R=255, reference_base_penalty=0.0, compare_repeat_counts=False, merge_ends=False, want_repeat_count_weight=True)
    expect(capi.MRP_ERR_NO_DEVICE, "no context", read_counts=np.array([255, 0, 200, 0, 9, 1, 1], np.uint8))  # read counts of 0 and of R and more are accepted
    expect(capi.MRP_ERR_NO_DEVICE, "no context", **changed("matches", "weight", 1, 0))


@pytest.mark.parametrize("name", ["node_first", "read_first", "matches", "deletes", "inserts", "opt", "out", "symbols", "ref_counts", "y_off", "y_len",
                                  "read_forward_strand", "read_symbols", "read_counts", "matches.first", "deletes.first", "inserts.first", "matches.x",
                                  "deletes.y", "inserts.weight"])
def test_null_arguments(name):
    expect(capi.MRP_ERR_ARG, "NULL" if name.endswith(".first") else "null", nulls=(name,))


def test_sizes_and_options():
    expect(capi.MRP_ERR_ARG, "bad sizes", pool_bytes=-1)
    for R in (1, 0, -2, 256):
        expect(capi.MRP_ERR_ARG, f"max_repeat {R} outside [2, 255]", R=R)
    for k in ("compare_repeat_counts", "merge_ends", "want_repeat_count_weight"):
        expect(capi.MRP_ERR_ARG, "must be 0 or 1", **{k: 2})
    expect(capi.MRP_ERR_ARG, "reference_base_penalty is NaN or negative", reference_base_penalty=math.nan)
    expect(capi.MRP_ERR_ARG, "reference_base_penalty is NaN or negative", reference_base_penalty=-0.5)
    expect(capi.MRP_ERR_ARG, "reserved", reserved=1)
    expect(capi.MRP_ERR_ARG, "reserved", reserved2=-1)
    # the order: the scalar checks come before the arrays are read
    expect(capi.MRP_ERR_ARG, "max_repeat", R=1, reserved=1, node_first=np.array([1, 3, 5], np.int64))
    expect(capi.MRP_ERR_ARG, "reserved", reserved=1, node_first=np.array([1, 3, 5], np.int64))


def test_offsets_symbols_counts_and_reads():
    expect(capi.MRP_ERR_ARG, "begin at 0", node_first=np.array([1, 3, 5], np.int64))
    expect(capi.MRP_ERR_ARG, "begin at 0", read_first=np.array([1, 2, 3], np.int64))
    expect(capi.MRP_ERR_ARG, "consensus 1: node_first or read_first descends", node_first=np.array([0, 3, 2], np.int64))
    expect(capi.MRP_ERR_ARG, "consensus 0: node_first or read_first descends", read_first=np.array([0, -1, 3], np.int64))
    expect(capi.MRP_ERR_ARG, "reference position 1: symbol 5 above 4", symbols=np.array([0, 5, 4, 2, 3], np.uint8))
    expect(capi.MRP_ERR_ARG, "reference position 3: count 0 outside [1, 11]", ref_counts=np.array([1, 2, 3, 0, 1], np.uint8))
    expect(capi.MRP_ERR_ARG, "reference position 2: count 12 outside [1, 11]", ref_counts=np.array([1, 2, 12, 1, 1], np.uint8))
    expect(capi.MRP_ERR_ARG, "symbol 5 above 4", symbols=np.array([0, 5, 4, 2, 3], np.uint8), ref_counts=np.array([0, 2, 3, 1, 1], np.uint8))  # the order
    expect(capi.MRP_ERR_ARG, "read 2 lies outside the pools", y_off=np.array([0, 3, 6], np.int64))
    expect(capi.MRP_ERR_ARG, "read 1 lies outside the pools", y_len=np.array([3, -1, 2], np.int32))
    expect(capi.MRP_ERR_ARG, "read 1, position 1: symbol 7 above 4", read_symbols=np.array([0, 1, 2, 1, 7, 2, 3], np.uint8))


def test_lists_are_checked_and_named():
    args, _ = cases.pack(small())
    p = dict(zip(NAMES, args))
    for which in ("matches", "deletes", "inserts"):
        l = dict(p[which])
        l["first"] = p[which]["first"] + 1
        expect(capi.MRP_ERR_ARG, f"{which}->first must begin at 0", **{which: l})
        l["first"] = np.array([0, 3, 2, 7], np.int64)
        expect(capi.MRP_ERR_ARG, f"read 1: {which}->first descends", **{which: l})
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, matches entry 4: y 2 outside [0, 2)", **changed("matches", "y", 4, 2))
    expect(capi.MRP_ERR_ARG, "consensus 1, read 2, matches entry 5: y -1 outside [0, 2)", **changed("matches", "y", 5, -1))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, matches entry 4: x 2 + x_shift 1 outside [0, 3)", **changed("matches", "x", 4, 2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, matches entry 0: x -1 + x_shift 0 outside [0, 3)", **changed("matches", "x", 0, -1))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, matches entry 3: x -2 + x_shift 1 outside", **changed("matches", "x", 3, -2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, deletes entry 0: x -1 + x_shift 0 outside [0, 3)", **changed("deletes", "x", 0, -1))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, deletes entry 0: x 3 + x_shift 0 outside [0, 3)", **changed("deletes", "x", 0, 3))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, deletes entry 1: y -2 outside [-1, 2)", **changed("deletes", "y", 1, -2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, deletes entry 1: y 2 outside [-1, 2)", **changed("deletes", "y", 1, 2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, inserts entry 1: x -2 + x_shift 0 outside [-1, 3)", **changed("inserts", "x", 1, -2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 1, inserts entry 2: x 2 + x_shift 1 outside [-1, 3)", **changed("inserts", "x", 2, 2))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, inserts entry 0: y -1 outside [0, 3)", **changed("inserts", "y", 0, -1))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, inserts entry 0: y 3 outside [0, 3)", **changed("inserts", "y", 0, 3))
    for which, at in (("matches", 1), ("deletes", 1), ("inserts", 2)):
        expect(capi.MRP_ERR_ARG, f"{which} entry {at}: negative weight -7", **changed(which, "weight", at, -7))
    expect(capi.MRP_ERR_ARG, "consensus 0, read 0, matches entry 2: x 2 + x_shift 1 outside", x_shift=np.array([1, 1, 0], np.int32))


# ---- mrp_poa_consensus ----------------------------------------------------------------------------------------------------------------

def graph_arrays(poas):
    """the restatement's graphs as mrp_poa's arrays (what the device returns, made on the host)"""
    return cases.flatten(poas, [[0.0] * 4] * len(poas), poas[0]["R"])


def assert_consensus(call_, R=12, **kw):
    w, poas, _ = cases.want(call_, R, **kw)
    for use_rle in (True, False):
        cases.assert_consensus(w, poas, call_, use_rle)
    return poas


def test_consensus_of_the_vector_and_of_a_zero_length_reference():
    _, vc = vector_call()
    poas = assert_consensus(vc, 51, merge=False)
    s, c, cmap = po.consensus(poas[0], True)
    assert "".join("ACGTN"[b] * n for b, n in zip(s, c)) == "GATACGGT" and cmap == [0, 1, -1, 2, 3, 4, 5]
    assert_consensus([cases.consensus([])])
    s, c, cmap = capi.poa_consensus(graph_arrays(cases.want([cases.consensus([])], 12)[1]), 0, 0)
    assert len(s) == len(c) == len(cmap) == 0
    assert_consensus([cases.consensus([]), cases.consensus([0, 1, 2, 3], [1, 2, 3, 4]), vc[0]])  # offsets into a call's arrays; a reference without a read


def one_node_call(reads_of):
    """reference G C T A G; reads_of(x0) gives the reads"""
    return [cases.consensus([2, 1, 3, 0, 2], [1, 2, 1, 3, 1], reads_of)]


def path(ops, ref=((2, 1), (1, 2), (3, 1), (0, 3), (2, 1)), strand=1, weight=1000):
    ch = edge.Chain(1)
    ch.s, ch.c = [b for b, _ in ref], [c for _, c in ref]
    ch.aligned("r", 0, ops, strand, weight)
    return ch.reads[0]


def test_consensus_where_an_insert_or_a_delete_of_length_3_wins_and_ties():
    full = ["m"] * 5
    # the insert wins: three of four reads carry it
    ins = ["m", "m", ("I", 0, 2), "m", "m", "m"]
    poas = assert_consensus(one_node_call([path(ins), path(ins, strand=0), path(ins), path(full)]))
    assert po.consensus(poas[0], True)[0] == [2, 1, 0, 3, 0, 2]
    # a delete of length 3 wins
    dele = ["m", "D", "D", "D", "m"]
    poas = assert_consensus(one_node_call([path(dele), path(dele, strand=0), path(dele), path(full)]))
    s, c, cmap = po.consensus(poas[0], True)
    assert s == [2] and c == [2] and cmap == [-1, -1, -1, -1, 0]  # G G: the two ends merge, the first maps nowhere
    # a tie between two inserts: the first in the node's order wins (>)
    a, b = ["m", "m", ("I", 0, 2), "m", "m", "m"], ["m", "m", ("I", 2, 5), "m", "m", "m"]
    for first, second, sym in ((a, b, 0), (b, a, 2)):
        poas = assert_consensus(one_node_call([path(first), path(second), path(first), path(second)]))
        assert [e["forward"] for e in poas[0]["nodes"][2]["inserts"]] == [2000.0, 2000.0]
        assert po.consensus(poas[0], True)[0][2] == sym
    # a pick of repeat count 0 is stored as it is and becomes 1 in the consensus
    zero = ["m", ("M", 1, 0), "m", "m", "m"]
    poas = assert_consensus(one_node_call([path(zero), path(zero), path(zero)]))
    assert poas[0]["nodes"][2]["repeat_count_pick"] == 0 and po.consensus(poas[0], True)[1][1] == 1


def test_consensus_on_the_edge_and_random_calls():
    assert_consensus(edge.edge_call(), edge.EDGE_R)
    assert_consensus(cases.random_call(), 12)


def test_consensus_refuses_where_the_reference_dereferences_null():
    ins = ["m", "m", ("I", 0, 2), "m", "m", "m"]
    w, poas, _ = cases.want(one_node_call([path(ins), path(ins)]), 12)
    w["insert_weight_forward"] = w["insert_weight_forward"].copy()
    w["insert_weight_forward"][0] = math.nan  # p is NaN: never the maximum, and the totals are NaN, so neither test of :1542-1546 holds
    poas[0]["nodes"][2]["inserts"][0]["forward"] = math.nan
    with pytest.raises(ValueError, match="node [0-9]+: no maximal (insert|delete)") as v:
        po.consensus(poas[0], True)
    with pytest.raises(capi.MrpError) as e:
        capi.poa_consensus(w, 0, 5)  # (asserts that the outputs came back untouched)
    assert e.value.code == capi.MRP_ERR_ARG and str(v.value) in str(e.value)  # the same node, the same NULL


def test_consensus_argument_errors():
    w, _, _ = cases.want(cases.random_call(), 12)

    def refused(text, L=300, nulls=(), **kw):
        with pytest.raises(capi.MrpError) as e:
            capi.poa_consensus(dict(w, **kw), 0, L, nulls=nulls)
        assert e.value.code == capi.MRP_ERR_ARG and text in str(e.value), str(e.value)

    for name in ("base_weight", "base_pick", "repeat_count_pick", "insert_first", "delete_first", "insert_str_off", "delete_length"):
        refused("null", nulls=(name,))
    refused("bad sizes", L=-1)
    first = w["insert_first"].copy()
    first[4] = first[3] - 1
    refused("node 3: insert_first or delete_first descends", insert_first=first)
    off = w["insert_str_off"].copy()
    off[2] = len(w["pool_symbols"])
    refused("insert 2: its string lies outside the pool", insert_str_off=off)
    length = w["delete_length"].copy()
    length[0] = 0
    refused("delete 0: length 0 below 1", delete_length=length)
    length[0] = 400
    refused("delete 0: length 400 below 1 or beyond the last node", delete_length=length)
    pick = w["base_pick"].copy()
    pick[7] = 5
    refused("node 7: a pick outside its range", base_pick=pick)


# ---- the stand-alone host check under the sanitizers ----------------------------------------------------------------------------------------

def test_the_host_check_is_clean_under_the_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clang = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    assert shutil.which(hipcc) and os.path.exists(clang)
    csrc, lib = os.path.join(ROOT, "margin_amd", "csrc"), os.path.dirname(capi.LIB_PATH)
    flags = ["-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=all", "-I" + csrc]
    objs = [str(tmp_path / n) for n in ("check_main.o", "check_poa.o", "check_poa_consensus.o")]
    subprocess.check_call([hipcc, *flags, "-x", "hip", "-c", os.path.join(ROOT, "tools", "hostcheck", "poa_host_check.cpp"), "-o", objs[0]])
    subprocess.check_call([hipcc, *flags, "-c", os.path.join(csrc, "mrp_poa.hip"), "-o", objs[1]])
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-c",
                           os.path.join(csrc, "mrp_poa_consensus.cpp"), "-o", objs[2]])
    exe = str(tmp_path / "poa_host_check")
    subprocess.check_call([clang, "-fsanitize=address,undefined", *objs, "-L" + lib, "-lmargin_rphmm", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
