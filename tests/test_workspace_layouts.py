"""The caller workspaces of the Wilson-family entry points (csrc/sc_workspace.h): one layout function per entry point, run on
a counting carver by the sc_*_workspace_bytes query and on d_work by the entry point.  Integer logic in a header with no HIP in
it, so it is checked here on the CPU over a grid of problems: tests/workspace_dump.cpp, built with the host compiler, prints
every layout's total and items, and this module holds the queries and the carves AS THEY STOOD before the layouts had one
home, transliterated, and checks totals, offsets, bounds, overlaps and the unions against them."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "spectral_connectivity_amd", "csrc")

CS = (1, 2, 5, 16, 47, 48, 49, 64, 65, 96, 128, 129, 256, 257, 512)
NS = (2, 4, 8, 32, 256, 4096)
RESIDENT_NS = (256, 512, 1024, 2048, 4096, 250, 1000, 4000)        # lengths of the resident pairwise form that the dump prints
PS = (1, 2, 7)
DS = (1, 2, 28)
SMALLS = (48, 64)                # mv_small_max(): the default, and SC_MVAR_INVERSE=small64
HIST, CMID, BW_LDS_NULLSPACE = 1024, 128, 64
LIMIT = 1 << 62


def align256(b):
    return (b + 255) & ~255


# ---- the queries and carves before the move: {name: (offset, bytes)} in bytes, total from the query's own formula ----------
def old_wilson(G, D, N):
    """sc_granger_workspace_bytes and wilson_carve (sc_wilson.hip)."""
    P = G * D
    total = P * N * (4 * 8 + 4 * 16 + 4 * 16) + P * (8 + 4 + 4 + 4 * 8 * 3) + 256 + HIST * 4
    items, w = {}, 0
    for name, size in (("S", P * N * 4 * 8), ("G", P * N * 4 * 16), ("A", P * N * 4 * 16), ("err", P * 8), ("h0", P * 32),
                       ("hinv", P * 32), ("rot", P * 32), ("n_fallback", 256), ("n_running", HIST * 4)):
        items[name] = (w, size)
        w += size
    return total, items


def old_pair(G, D, N):
    """pair_workspace_bytes and the carve of sc_internal_granger_resident (sc_wilson_pair.hip)."""
    P, F = G * D, N // 2 + 1
    total = P * F * 4 * 16 + P * 4 * 8 * 4 + D * 4 + 256
    items, w = {}, 0
    for name, size in (("Ghalf", P * F * 4 * 16), ("chol", P * 32), ("h0", P * 32), ("hinv", P * 32), ("rot", P * 32),
                       ("batch_bad", D * 4), ("summary", 256)):
        items[name] = (w, size)
        w += size
    return total, items


def old_mvar_total(P, C, N, small_max):
    """sc_mvar_workspace_bytes (sc_mvar.hip)."""
    E, F = C * C, N // 2 + 1
    n_big = 5 if C > small_max else 3
    factor = n_big * P * E * N * 16 + P * 16 + P * E * 8 + 128 + HIST * 4
    n_sq = max(max(F, 16), (E + 255) // 256)
    meas = (3 if C > CMID else 2) * P * F * E * 16 + P * E * 8 * 3 + P * n_sq * 8 + P * C * 8 + P * 8 + 256
    return max(factor, meas) + 256, factor + 256, meas + 256


def old_mvar_factor(P, C, N, small_max):
    """The carve of sc_mvar_factor_f64.  T doubles as the scratch of the blocked inverse beyond 128 signals."""
    E = C * C
    big = C > small_max
    items, w = {}, 0
    names = ["S", "G", "A"] + (["Ginv", "T"] if big else [])
    for name in names:
        items[name] = (w, P * E * N * 16)
        w += P * E * N * 16
    if C > CMID:
        items["T.inverse_scratch"] = items["T"]
    for name, size in (("err", P * 8), ("g0", P * E * 8), ("n_fallback", 64), ("n_running", HIST * 4)):
        items[name] = (w, size)
        w += size
    return old_mvar_total(P, C, N, small_max)[1], items


def old_mvar_measure(P, C, N):
    """The carve of sc_mvar_measure_f64: h0c / hinvc parked in A_mvar, the scratch behind lam rounded up to 16 bytes."""
    E, F = C * C, N // 2 + 1
    n_sq = max(max(F, 16), (E + 255) // 256)
    items, w = {}, 0
    for name, size in (("H", P * F * E * 16), ("Amv", P * F * E * 16), ("h0", P * E * 8), ("hinv", P * E * 8), ("sigma", P * E * 8),
                       ("sq", P * n_sq * 8), ("tot", P * C * 8), ("lam", 64)):
        items[name] = (w, size)
        w += size
    items["Amv.h0c"] = (items["Amv"][0], P * E * 16)
    items["Amv.hinvc"] = (items["Amv"][0] + P * E * 16, P * E * 16)
    if C > CMID:                 # (below, the rounded pointer was never used)
        w += (16 - (w & 15)) & 15
        items["scratch"] = (w, P * F * E * 16)
    return old_mvar_total(P, C, N, 48)[2], items


def old_conditional(G, C, N, D, small_max):
    """sc_conditional_granger_workspace_bytes and the carve of sc_conditional_granger_f64 (sc_conditional.hip)."""
    P, E, Er, F = G * D, C * C, (C - 1) * (C - 1), N // 2 + 1
    mvar = old_mvar_total(P, C - 1, N, small_max)[0]
    epi = align256(P * Er * 16) + 2 * align256(P * N * Er * 16)
    total = align256(G * E * 16) + align256(G * F * E * 16) + 256 + 2 * align256(P * N * Er * 16) + align256(max(mvar, epi))
    items, w = {}, 0
    for name, size in (("Psi0T", G * E * 16), ("M", G * F * E * 16), ("zero", 256), ("Sred", P * N * Er * 16), ("Phi", P * N * Er * 16)):
        items[name] = (w, size)
        w += align256(size)
    tail = w
    items["tail.mvar"] = (tail, mvar)
    items["tail.Phi0"] = (tail, P * Er * 16)
    k = tail + align256(P * Er * 16)
    items["tail.K"] = (k, P * N * Er * 16)
    items["tail.scratch"] = (k + P * N * Er * 16, P * N * Er * 16)          # cd* scratch = K + P N Er
    return total, items, (tail, align256(max(mvar, epi)))


def old_blockwise(G, m, N, D, small_max):
    """sc_blockwise_granger_workspace_bytes and the carve of sc_blockwise_granger_f64 (sc_blockwise.hip)."""
    P, E, F = G * D, m * m, N // 2 + 1
    mvar = old_mvar_total(P, m, N, small_max)[0]
    epi = align256(P * E * 16) + align256(P * F * E * 16) + align256(P * E * 8)
    total = 2 * align256(P * N * E * 16) + align256(max(mvar, epi))
    tail = 2 * align256(P * N * E * 16)
    y = tail + align256(P * E * 16)
    items = {"S2": (0, P * N * E * 16), "Psi": (align256(P * N * E * 16), P * N * E * 16), "tail.mvar": (tail, mvar),
             "tail.R": (tail, P * E * 16), "tail.Y": (y, P * F * E * 16), "tail.psi0": (y + align256(P * F * E * 16), P * E * 8)}
    return total, items, (tail, align256(max(mvar, epi)))


# ---- the header's layouts ---------------------------------------------------------------------------------------------------
def build_dump(tmp, extra=()):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / "workspace_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", *extra, "-I", CSRC, os.path.join(HERE, "workspace_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{(layout, small_max, a, b, c, d): (total, {name: (offset, bytes)})} as the header computes them."""
    exe = build_dump(tmp_path_factory.mktemp("workspace"))
    got, items = {}, None
    for line in filter(None, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")):
        w = line.split()
        if w[0] == "L":
            items = {}
            got[(w[1],) + tuple(map(int, w[2:7]))] = (int(w[7]), items)
        else:
            assert w[0] == "I" and w[1] not in items, line
            items[w[1]] = (int(w[2]), int(w[3]))
    return got


def pair_grid(ns=NS):
    return [(G, D, N) for G in PS for D in DS for N in ns]


def mvar_grid():
    return [(sm, P, C, N) for sm in SMALLS for P in PS for C in CS for N in NS]


def group_grid():
    return [(sm, G, C, N, D) for sm, G, C, N in mvar_grid() if C >= 2 for D in DS]


def check(got, total, old_items, alive_sets, ignore=("reserved", "tail.reserved", "end")):
    """Total and offsets as before; every item inside [0, total); the items alive at the same time (one list of names per
    alternative, the fixed part included) do not overlap."""
    new_total, items = got
    assert new_total == total
    named = {n: v for n, v in items.items() if n not in ignore}
    assert named == old_items
    for name, (off, size) in items.items():
        assert 0 <= off and off + size <= total, name
    for alive in alive_sets:
        spans = sorted(items[n] for n in alive if n in items and items[n][1] > 0)
        for (o0, s0), (o1, _) in zip(spans, spans[1:]):
            assert o0 + s0 <= o1, alive


def test_grid_stays_below_the_limit():
    """(nothing of the grid is dropped: the largest workspace is far below 2^62 bytes)"""
    assert max(old_conditional(7, 512, 4096, 28, 48)[0], old_blockwise(7, 512, 4096, 28, 48)[0]) < LIMIT


def test_batched_pairwise(layouts):
    fixed = ["S", "G", "A", "err", "h0", "hinv", "rot", "n_fallback", "n_running", "reserved"]
    for G, D, N in pair_grid(NS + RESIDENT_NS[1:4] + RESIDENT_NS[5:]):
        total, items = old_wilson(G, D, N)
        check(layouts[("wilson", 0, G, D, N, 0)], total, items, [fixed])


def test_resident_pairwise(layouts):
    fixed = ["Ghalf", "chol", "h0", "hinv", "rot", "batch_bad", "summary"]
    for G, D, N in pair_grid(NS + RESIDENT_NS[1:4] + RESIDENT_NS[5:]):
        total, items = old_pair(G, D, N)
        check(layouts[("pair", 0, G, D, N, 0)], total, items, [fixed])


def test_resident_pairwise_fits_the_batched_query(layouts):
    """sc_granger_pairwise_f64 checks the batched query's size and then hands the workspace to the resident form."""
    for G, D, N in pair_grid(RESIDENT_NS):
        assert layouts[("pair", 0, G, D, N, 0)][0] <= layouts[("wilson", 0, G, D, N, 0)][0] == old_wilson(G, D, N)[0]


def test_mvar_factor(layouts):
    rest = ["S", "G", "A", "Ginv", "err", "g0", "n_fallback", "n_running", "reserved"]
    for sm, P, C, N in mvar_grid():
        total, items = old_mvar_factor(P, C, N, sm)
        got = layouts[("mvar_factor", sm, P, C, N, 0)]
        check(got, total, items, [rest + ["T"], rest + ["T.inverse_scratch"]], ignore=("reserved",) + (() if C > CMID else ("T.inverse_scratch",)))
        assert ("Ginv" in got[1]) == ("T" in got[1]) == (C > sm)
        assert got[1]["reserved"][1] == P * 8 + 64 + 256, "the query's P * 16 + 128 (+ 256) against the carve's P * 8 + 64"
        if C > CMID:
            assert got[1]["T.inverse_scratch"] == got[1]["T"]


def test_mvar_measure(layouts):
    rest = ["H", "h0", "hinv", "sigma", "sq", "tot", "lam", "scratch", "reserved"]
    for sm, P, C, N in mvar_grid():
        total, items = old_mvar_measure(P, C, N)
        got = layouts[("mvar_measure", sm, P, C, N, 0)]
        check(got, total, items, [rest + ["Amv"], rest + ["Amv.h0c", "Amv.hinvc"]])
        amv, h0c, hinvc = (got[1][n] for n in ("Amv", "Amv.h0c", "Amv.hinvc"))
        assert amv[0] == h0c[0] and hinvc[0] + hinvc[1] <= amv[0] + amv[1], "2 P C^2 parked elements fit A_mvar"
        assert ("scratch" in got[1]) == (C > CMID) and got[1].get("scratch", (0, 0))[0] % 16 == 0
    assert layouts[("mvar_measure", 48, 7, 512, 2, 0)][1]["Amv"][1] == 2 * 7 * 512 * 512 * 16, "N = 2: exactly the parked matrices"


def test_mvar_query_is_the_larger_layout(layouts):
    for sm, P, C, N in mvar_grid():
        assert layouts[("mvar", sm, P, C, N, 0)][0] == old_mvar_total(P, C, N, sm)[0] == max(
            layouts[("mvar_factor", sm, P, C, N, 0)][0], layouts[("mvar_measure", sm, P, C, N, 0)][0])


def check_tail(got, tail, members):
    """Every member of the tail union lies within the tail."""
    t0, size = tail
    assert got[0] == t0 + size
    for name in members:
        off, b = got[1][name]
        assert t0 <= off and off + b <= t0 + size, name


def test_conditional(layouts):
    fixed = ["Psi0T", "M", "zero", "Sred", "Phi"]
    for sm, G, C, N, D in group_grid():
        total, items, tail = old_conditional(G, C, N, D, sm)
        got = layouts[("conditional", sm, G, C, N, D)]
        check(got, total, items, [fixed + ["tail.mvar"], fixed + ["tail.Phi0", "tail.K", "tail.scratch", "tail.reserved"]])
        check_tail(got, tail, ["tail.mvar", "tail.Phi0", "tail.K", "tail.scratch", "tail.reserved"])
        assert all(off % 256 == 0 for name, (off, _) in got[1].items() if name not in ("tail.scratch", "tail.reserved"))
        # the blocked inverse (beyond 128 reduced signals) writes one matrix per (problem, bin < F) into the scratch
        assert G * D * (N // 2 + 1) * (C - 1) ** 2 * 16 <= got[1]["tail.scratch"][1]


def test_blockwise(layouts):
    fixed = ["S2", "Psi"]
    for sm, G, m, N, D in group_grid():
        total, items, tail = old_blockwise(G, m, N, D, sm)
        got = layouts[("blockwise", sm, G, m, N, D)]
        check(got, total, items, [fixed + ["tail.mvar"], fixed + ["tail.R", "tail.Y", "tail.psi0"]])
        check_tail(got, tail, ["tail.mvar", "tail.R", "tail.Y", "tail.psi0"])
        assert all(off % 256 == 0 for off, _ in got[1].values())
        assert got[1]["tail.psi0"][1] == G * D * m * m * 8, "bw_nullspace's Psi0 beyond BW_LDS_NULLSPACE signals"
    assert any(m > BW_LDS_NULLSPACE for _, _, m, _, _ in group_grid())


def test_the_transliteration_agrees_with_itself():
    """The old carves end within the old queries (what the slack items of the layouts stand for)."""
    olds = itertools.chain((f(G, D, N) for G, D, N in pair_grid(NS + RESIDENT_NS) for f in (old_wilson, old_pair)),
                           (old_mvar_factor(P, C, N, sm) for sm, P, C, N in mvar_grid()),
                           (old_mvar_measure(P, C, N) for _, P, C, N in mvar_grid()),
                           (f(G, C, N, D, sm)[:2] for sm, G, C, N, D in group_grid() for f in (old_conditional, old_blockwise)))
    for total, items in olds:
        assert max(off + b for off, b in items.values()) <= total
