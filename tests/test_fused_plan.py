"""The launch plan of the one-pass stage-B kernels (csrc/sc_fused_plan.h): which 32-channel blocks each launch stages and
which block products it owns.  Pure integer logic in a header with no HIP in it, so it is checked here on the CPU for every
block count the library accepts (1 ... 32 blocks = up to 1024 signals): tests/fused_plan_dump.cpp, built with the host
compiler, prints the plan and this module checks it.  A product written twice or never would otherwise only show in GPU
tests at the handful of channel counts they run."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "spectral_connectivity_amd", "csrc")

# (nb, col_lo, row_hi): the kernel instantiations that exist.  The last one only in sc_fused2.hip (more than 8 blocks).
COMMON_SHAPES = {(1, 0, 1), (2, 0, 2), (3, 0, 3), (4, 0, 4), (4, 2, 2), (3, 1, 3), (4, 2, 4), (4, 1, 4), (4, 1, 1)}
PLANES_SHAPES = COMMON_SHAPES | {(3, 2, 2)}

# The plans of up to eight blocks as they stood in launch_fused_all / fused2_launch_all before the plan had one home:
# (blocks, col_lo, row_hi) per launch, in launch order.
TABLES = {
    1: [((0,), 0, 1)],
    2: [((0, 1), 0, 2)],
    3: [((0, 1, 2), 0, 3)],
    4: [((0, 1, 2, 3), 0, 4)],
    5: [((0, 1, 2), 0, 3), ((0, 1, 3, 4), 2, 2), ((2, 3, 4), 1, 3)],
    6: [((0, 1, 2, 3), 0, 4), ((0, 1, 4, 5), 2, 4), ((2, 3, 4, 5), 2, 2)],
    7: [((0, 1, 2, 3), 0, 4), ((0, 4, 5, 6), 1, 4), ((1, 4, 5, 6), 1, 1), ((2, 4, 5, 6), 1, 1), ((3, 4, 5, 6), 1, 1)],
    8: [((0, 1, 2, 3), 0, 4), ((4, 5, 6, 7), 0, 4), ((0, 1, 4, 5), 2, 2), ((0, 1, 6, 7), 2, 2), ((2, 3, 4, 5), 2, 2),
        ((2, 3, 6, 7), 2, 2)],
}

# n: (launches, staged blocks) of the plan before the move
COUNTS = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (1, 4), 5: (3, 10), 6: (3, 12), 7: (5, 20), 8: (6, 24),
          9: (11, 37), 10: (11, 42), 11: (15, 55), 12: (15, 60), 13: (22, 79), 14: (22, 86), 15: (28, 105), 16: (28, 112),
          17: (37, 137), 18: (37, 146), 19: (45, 171), 20: (45, 180), 21: (56, 211), 22: (56, 222), 23: (66, 253), 24: (66, 264),
          25: (79, 301), 26: (79, 314), 27: (91, 351), 28: (91, 364), 29: (106, 407), 30: (106, 422), 31: (120, 465), 32: (120, 480)}


def general_plan(n):
    """More than eight blocks, transliterated from fused2_launch_all as it stood: the triangles of the groups of four, the
    64 x 64 rectangles between pairs of blocks of different groups, the lone odd block against every pair outside its group."""
    out = [(tuple(range(g0, min(g0 + 4, n))), 0, min(4, n - g0)) for g0 in range(0, n, 4)]
    n_pairs, lone = n // 2, (n - 1 if n & 1 else -1)
    for hi in range(n_pairs):
        for hj in range(hi + 1, n_pairs):
            if hi // 2 != hj // 2:
                out.append(((2 * hi, 2 * hi + 1, 2 * hj, 2 * hj + 1), 2, 2))
        if lone >= 0 and hi // 2 != lone // 4:
            out.append(((2 * hi, 2 * hi + 1, lone), 2, 2))
    return out


def owned(launch):
    """The block products (bi <= bj, record block numbers) a launch owns: i < row_hi, j >= max(i, col_lo) of its staged blocks."""
    blocks, col_lo, row_hi = launch
    return [(blocks[i], blocks[j]) for i in range(min(row_hi, len(blocks))) for j in range(max(i, col_lo), len(blocks))]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{n: [(blocks, col_lo, row_hi), ...]} for n = 0 ... 33 as the header computes them, plus its two capacity constants."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("fused_plan") / "fused_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "fused_plan_dump.cpp"), "-o", exe],
                   check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got, counts, capacity = {}, {}, None
    for line in filter(None, lines):
        w = line.split()
        if w[0] == "capacity":
            capacity = (int(w[1]), int(w[2]))
        elif w[0] == "count":
            counts[int(w[1])] = int(w[2])
            got[int(w[1])] = []
        else:
            n, nb, b0, b1, b2, b3, col_lo, row_hi = map(int, w)
            assert 1 <= nb <= 4, line
            got[n].append((tuple((b0, b1, b2, b3)[:nb]), col_lo, row_hi))
    assert {n: len(v) for n, v in got.items()} == counts
    return got, capacity


def test_capacity_and_range(plans):
    got, (max_blocks, max_launches) = plans
    assert max_blocks == 32
    assert max_launches == max(len(got[n]) for n in range(1, 33)) == 120
    assert got[0] == [] and got[33] == [], "a block count out of range gets no launches"


@pytest.mark.parametrize("n", range(1, 33))
def test_every_block_product_is_owned_once(plans, n):
    products = sorted(p for launch in plans[0][n] for p in owned(launch))
    assert products == [(bi, bj) for bi in range(n) for bj in range(bi, n)]


@pytest.mark.parametrize("n", range(1, 33))
def test_launches_stage_ascending_blocks_in_a_shape_that_exists(plans, n):
    for blocks, col_lo, row_hi in plans[0][n]:
        assert 1 <= len(blocks) <= 4 and list(blocks) == sorted(set(blocks)) and 0 <= blocks[0] and blocks[-1] < n
        assert (len(blocks), col_lo, row_hi) in (COMMON_SHAPES if n <= 8 else PLANES_SHAPES)


@pytest.mark.parametrize("n", range(1, 33))
def test_plan_is_the_one_before_the_move(plans, n):
    """Launch by launch, in order: the tables up to eight blocks, the transliterated general plan beyond -- and with them the
    number of launches and of staged blocks (each staging reads its channels from HBM again)."""
    before = TABLES[n] if n <= 8 else general_plan(n)
    assert (len(before), sum(len(b) for b, _, _ in before)) == COUNTS[n], "the transliteration itself"
    assert plans[0][n] == before
    assert (len(plans[0][n]), sum(len(b) for b, _, _ in plans[0][n])) == COUNTS[n]


@pytest.mark.parametrize("n", range(1, 33))
def test_the_transliteration_has_the_properties_too(n):
    before = TABLES[n] if n <= 8 else general_plan(n)
    assert sorted(p for launch in before for p in owned(launch)) == [(bi, bj) for bi in range(n) for bj in range(bi, n)]
    assert all((len(b), lo, hi) in (COMMON_SHAPES if n <= 8 else PLANES_SHAPES) for b, lo, hi in before)
