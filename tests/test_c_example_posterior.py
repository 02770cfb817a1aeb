"""examples/posterior_aligned_pairs.c: mrp_posterior_tracebacks and mrp_posterior_aligned_pairs from plain C.  It must compile against
include/ and link against the in-tree library; on a GPU the lists it prints must be the sequential restatement's, exactly."""
import os
import subprocess

import pytest

from margin_amd import capi
from tests import posterior_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS = ("AGCG", "ACGTTGCATGCCATTGACGGATCCGTAATG")
YS = ("AGTTCG", "ACGTTGCATGCCTGACGGATCCGTAATG")
KW = dict(expansion=8, min_diags=12, traceback_diagonals=3)


def _build(tmp_path):
    exe = str(tmp_path / "posterior_aligned_pairs")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "posterior_aligned_pairs.c"),
                           "-L" + libdir, "-lmargin_rphmm", "-lm", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def _plan_lines():
    out = []
    for i, (x, y) in enumerate(zip(XS, YS)):
        t = po.tracebacks(len(x), len(y), [], KW["expansion"], KW["min_diags"], KW["traceback_diagonals"])
        out.append(f"tracebacks {i} {len(t)}:" + "".join(f" {d},{a},{b}" for d, a, b in t))
    return out


def test_c_example_builds_plans_and_refuses_to_run_without_a_device(tmp_path):
    exe = _build(tmp_path)
    if capi.load().mrp_device_count() > 0:
        return  # (its run on a device is the test below)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "mrp_context_create" in r.stderr
    assert r.stdout.splitlines() == _plan_lines()  # the planner needs no device
    assert len(po.tracebacks(len(XS[1]), len(YS[1]), [], **KW)) > 2


@pytest.mark.gpu
def test_c_example_equals_the_restatement(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:2] == _plan_lines()
    m = capi.PairHmm.default_nucleotide()
    want = []
    for i, (x, y) in enumerate(zip(XS, YS)):
        lists, _ = po.posterior(m, capi.symbols_from_chars(x), capi.symbols_from_chars(y), [], threshold=0.2, with_gaps=True, **KW)
        assert all(len(l) > 0 for l in lists[:2]) or i == 0
        for name, l in zip(("match", "gap_x", "gap_y"), lists):
            want += [f"{name} {i} {px} {py} {w} {float(v).hex()}" for w, px, py, v in l]
    got = [ln for ln in lines if ln.split()[0] in ("match", "gap_x", "gap_y")]
    norm = lambda ln: " ".join(ln.split()[:5] + [float.fromhex(ln.split()[5]).hex()])
    assert [norm(ln) for ln in got] == [norm(ln) for ln in want]
    assert {(int(ln.split()[2]), int(ln.split()[3])) for ln in got if ln.startswith("match 0 ")} == {(0, 0), (1, 1), (2, 4), (3, 5)}
    assert "aligned pairs" in lines[-1]
