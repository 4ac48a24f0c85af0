"""The split plan of the one-pass stage-B kernels (csrc/sc_fused_split.h): into which parts the observation chunks of a bin are
cut -- equal parts, or equal big parts and one short tail part that is dispatched after the big parts of every bin.  Pure integer
logic in a header with no HIP in it, so it is checked here on the CPU over a grid of shapes: tests/fused_split_dump.cpp, built
with the host compiler, prints the plans and this module checks them -- the parts tile the chunks, the closed-form makespan of
the header is what a list-scheduling simulation of the plan gives, and no plan is worse under that simulation than the equal
parts of the rule before."""
import heapq
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "spectral_connectivity_amd", "csrc")

N_BINS = (1, 2, 3, 7, 33, 64, 100, 128, 129, 200, 255, 256, 257, 304, 305, 513, 600, 903, 1000, 1500, 2049, 2709, 3000)
N_CHUNKS = (1, 2, 15, 16, 17, 20, 28, 31, 32, 33, 40, 47, 48, 55, 64, 73, 79, 100, 110, 150, 219, 250, 333, 400, 499, 500)
N_CU = (64, 256, 304)
FIXED, MIN_BIG, MAX_PARTS, TAPER_ROUNDS = 3, 16, 24, 7


def factor(n_parts):
    return 1.0 + 0.02 * (n_parts - 1)


def parent_parts(n_bins, nc, n_cu):
    """sc_internal_fused_pick_split as it stood before the plans had a header: the number of EQUAL parts."""
    best, best_cost = 1, 1e30
    for s in range(1, 25):
        if s > 1 and nc // s < 16:
            break
        rounds = float((n_bins * s + n_cu - 1) // n_cu)
        cost = rounds * (nc / s + 3.0) * (1.0 + 0.02 * (s - 1))
        if cost < best_cost - 1e-9:
            best_cost, best = cost, s
    return best


def equal_bounds(nc, s):
    return [k * nc // s for k in range(s)] + [nc]


def block_sizes(n_bins, bounds, tail):
    """Chunks of every workgroup in dispatch order: (bin, part) for equal parts; the big parts of all bins, then the tails."""
    sizes = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
    if not tail:
        return sizes * n_bins
    return sizes[:-1] * n_bins + sizes[-1:] * n_bins


def simulate(n_bins, bounds, tail, n_cu):
    """List scheduling: every workgroup, in dispatch order, goes to the compute unit that is free first."""
    f = factor(len(bounds) - 1)
    free = [0.0] * n_cu
    for c in block_sizes(n_bins, bounds, tail):
        heapq.heapreplace(free, free[0] + (c + FIXED) * f)
    return max(free)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("fused_split") / "fused_split_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "fused_split_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        return subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def plans(dump):
    """{(n_bins, n_chunks, n_cu): (n_parts, tail, makespan, bounds)} over the grid, as the header computes them."""
    grid = [(b, c, p) for p in N_CU for b in N_BINS for c in N_CHUNKS]
    out = dump([f"{b} {c} {p}" for b, c, p in grid])
    assert out[0].split() == ["capacity", str(MAX_PARTS), str(MIN_BIG), str(FIXED), str(TAPER_ROUNDS)]
    got = {}
    for line in filter(None, out[1:]):
        w = line.split()
        key, n_parts, tail, makespan = tuple(map(int, w[:3])), int(w[3]), int(w[4]), float(w[5])
        bounds = list(map(int, w[6:]))
        assert len(bounds) == n_parts + 1, line
        got[key] = (n_parts, tail, makespan, bounds)
    assert sorted(got) == sorted(grid)
    return got


def test_grid_has_the_shapes_that_matter():
    assert {129, 513, 903, 2049} <= set(N_BINS) and min(N_BINS) == 1 and max(N_BINS) == 3000
    assert min(N_CHUNKS) == 1 and max(N_CHUNKS) == 500 and {28, 55, 110, 219} <= set(N_CHUNKS)      # cfg3 at 125 ... 1000 trials


@pytest.mark.parametrize("n_cu", N_CU)
def test_parts_tile_the_chunks(plans, n_cu):
    for (n_bins, nc, p), (n_parts, tail, _, bounds) in plans.items():
        if p != n_cu:
            continue
        where = (n_bins, nc, p, n_parts, tail, bounds)
        assert 1 <= n_parts <= MAX_PARTS, where
        assert bounds[0] == 0 and bounds[-1] == nc, where
        sizes = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
        assert all(s >= 1 for s in sizes), where                       # in order, no gap, no overlap, nothing empty
        if n_parts > 1:
            big = sizes[:-1] if tail else sizes
            assert min(big) >= MIN_BIG, where
        if tail:
            assert sizes[-1] == tail and tail <= min(sizes[:-1]), where
            assert len(set(sizes[:-1])) == 1, where                    # one size of big parts: the closed form counts on it
        else:
            assert bounds == equal_bounds(nc, n_parts), where


@pytest.mark.parametrize("n_cu", N_CU)
def test_makespan_is_the_simulated_one_and_never_above_the_parents(plans, n_cu):
    """The closed form against the simulation, to within one tail workgroup (exact for tapered plans; equal parts that differ by
    a chunk are priced at their mean by the rounds formula).  And the plan against the rule before, both simulated."""
    n_tapered = 0
    for (n_bins, nc, p), (n_parts, tail, makespan, bounds) in plans.items():
        if p != n_cu:
            continue
        where = (n_bins, nc, p, n_parts, tail)
        sim = simulate(n_bins, bounds, tail, p)
        one_tail = (bounds[-1] - bounds[-2] + FIXED) * factor(n_parts)
        assert abs(sim - makespan) <= one_tail + 1e-6, (where, sim, makespan)
        s_parent = parent_parts(n_bins, nc, p)
        if tail:
            n_tapered += 1
            assert abs(sim - makespan) <= 1e-6 * makespan, (where, sim, makespan)
            sim_parent = simulate(n_bins, equal_bounds(nc, s_parent), 0, p)
            assert sim <= sim_parent + 1e-9, (where, sim, s_parent, sim_parent)
        else:
            assert n_parts == s_parent, where                          # no tapered plan wins: the equal parts of before
    assert n_tapered > 0


def test_measured_shapes(plans):
    """On 256 compute units: cfg3 at 500 trials (903 bins of 110 chunks) and cfg5 (513 bins of 79) take a tail; cfg3 itself (219
    chunks), whose three equal parts run in 11 rounds, keeps them -- the guard of fu_split_plan: equal parts in more than
    TAPER_ROUNDS rounds stay, because the model's gain did not show there on the device."""
    n_parts, tail, makespan, bounds = plans[(903, 110, 256)]
    assert (n_parts, tail, bounds) == (2, 10, [0, 100, 110]) and makespan == pytest.approx(421.26)
    n_parts, tail, makespan, bounds = plans[(513, 79, 256)]
    assert (n_parts, tail, bounds) == (2, 19, [0, 60, 79]) and makespan == pytest.approx(195.84)
    n_parts, tail, makespan, bounds = plans[(903, 219, 256)]
    assert (n_parts, tail, bounds) == (3, 0, [0, 73, 146, 219]) and makespan == pytest.approx(11 * 76 * 1.04)
    assert simulate(903, bounds, 0, 256) == pytest.approx(11 * 76 * 1.04)


def test_no_tapered_plan_beyond_the_guarded_rounds(plans):
    for (n_bins, nc, p), (n_parts, tail, _, _) in plans.items():
        s_parent = parent_parts(n_bins, nc, p)
        if (n_bins * s_parent + p - 1) // p > TAPER_ROUNDS:
            assert tail == 0 and n_parts == s_parent, (n_bins, nc, p, n_parts, tail)


def test_forced_plans(dump):
    """The diagnostic switches: n equal parts exactly as before; n parts with a tail of t chunks, big parts sharing the rest."""
    out = dump(["forced 20 3 0", "forced 20 2 2", "forced 20 3 1", "forced 2 2 1", "forced 2 3 0", "forced 20 1 5", "forced 3 3 2",
                "forced 20 25 0"])[1:]
    assert [list(map(int, l.split()[1:])) for l in filter(None, out)] == [
        [20, 3, 0, 3, 0, 6, 13, 20], [20, 2, 2, 2, 0, 18, 20], [20, 3, 1, 3, 0, 9, 19, 20], [2, 2, 1, 2, 0, 1, 2], [2, 3, 0, -1],
        [20, 1, 5, 1, 0, 20], [3, 3, 2, -1], [20, 25, 0, -1]]
