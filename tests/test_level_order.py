"""The host arithmetic of staging a resident level (margin_amd/csrc/mrp_level_order.h) without a device: tests/level_order_check.cpp,
a stand-alone program built with the address and undefined-behaviour sanitizers.  It checks the order of a level's hmms and their
launch classes on seeded random levels (n in {0, 1, 2, 63, 4 096, 4 097, 6 000}; few distinct column counts and bounds, so ties are
common; bounds on both sides of every threshold; unit and cell levels) against a plain restatement; the prune kernel's class from (chain mode, largest column) on both sides of every threshold
(256/257, 4 096/4 097, 5 120/5 121, 10 240/10 241, the end of the range at 13 824/13 825; cell levels and unit levels) and at every size
up to there against a table of what each class holds; the prune kernel's LDS request within the budget at every size the selector
accepts (89 424 bytes at 116 x 116 cells, its largest reachable level) and the layout behind it (mrp_prune_lds.h: regions in order, disjoint,
aligned as the kernel reads them; the request is their end plus the tail slack, and the hand-written sum of before minus the flag words); the cross product + emission plan at 64/65 and 128/129 cells with the level mostly
single-wave or not; the census slots (named, distinct, class-major); and the block carver's sizing
pass against its pointer pass (64-byte aligned, inside the block, disjoint regions; a zero count takes nothing), and the chunk block of
a work queue's batch (chunks of 0, 1 and 5 sites with slot totals not divisible by 4, profile pools of 0, 1, 255, 256 and 257 bytes, with
and without the pools in the block): sizing pass equal to pointer pass, every slice 256-byte aligned, inside the block and disjoint,
a zero-length slice takes nothing, and every pool -- the last one too -- ends MRP_POOL_TAIL_PAD bytes or more before the reserved size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_order_classes_and_block_carver(tmp_path):
    exe = str(tmp_path / "level_order_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "level_order_check.cpp")])
    out = subprocess.check_output([exe], text=True)
    assert out.strip() == "level order ok", out
