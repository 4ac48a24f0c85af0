"""The value kernels of canonical coherence and of the imaginary interaction (sc_canonical_coherence_f64, sc_imaginary_interaction_f64,
csrc/sc_canonical.hip) on records built by hand: no stage A, no stage B, no Multitaper.  tests/canonical_values_ref.py builds joint
matrices of channel groups whose canonical coherences are known without rounding (``exact``) and Wishart matrices with a truth in
extended precision (``free``), packs n_obs x matrix into a record with SC_PLANE_CSM, and measures rho_1^2, MIC and MIM in units of
2^-52 (MIM: 2^-52 min(na, nb)).  The bars are 8 x what the plain NumPy reference (cholesky, two solves, svd) reaches on the cases of
(a), rounded up to a power of two (profiles/canonical_values_accuracy.txt); no device number enters them.  The kernels are chosen by
the largest group of a launch:

  1 ... 16     canonical_factor_kernel + canonical_pair_hh_kernel: a wave per (bin, pair), B in registers, Householder + Sturm multisection
  17 ... 64    canonical_big_hh_kernel, every pair in LDS (row length max group | 1), up to 1024 persistent workgroups
  65 ... 128   canonical_big_hh_kernel with a global scratch: pairs up to 64 channels in LDS, B in LDS up to 96, beyond in the scratch
  SC_CANON_EIG=jacobi (canonical coherence only): canonical_pair_kernel up to 16, canonical_kernel<32> up to 32, canonical_big_kernel beyond

(a) every tier at its edges, both families, both label orders; three groups; ten pairs on eight waves; LDS and scratch pairs in one launch.
(b) the record: float32 records, n_obs = 12, every other plane beside SC_PLANE_CSM, two runs -- the same bits.
(c) a workgroup takes a second item (more (bin, pair) items than slots), diagonal B before dense B and the reverse; the vectors kernels too.
(d) structure of the whitened spectrum: equal, rho_1 = 1, rho_1 = rho_2, rank one, zero, graded, clusters 0.75 + k 2^-p.
(e) the conditioning series.
(f) tesla^2 and count^2 amplitudes: the same bits.
(g) a group that cannot be whitened: NaN in its pairs, the third pair under the bars, fail = 2.
(h) the diagnostic Jacobi kernels against their stopping rule and against the default kernels.
(i) nothing is stored outside the outputs and ``fail``; the argument checks return their codes and write nothing.

What the suite found when it first ran on the MI355X (fixed in csrc/sc_canonical.hip); errors in units of 2^-52:
  (d) the cluster 0.75 + k 2^-p at 16 x 16 channels: rho_1^2 off by 10 332 at p = 40 and 1 106 at p = 44, as a NumPy emulation of
      cb_top_eigenvalue had predicted (8 166 at p = 40): ``p2 * p1 < 0`` of the unscaled Sturm recurrence underflowed to 0 in every
      lane and the multisection left with the Gershgorin bracket open.  The signs are compared now; at most 3.5 after the fix.
  (a) MIC x MIC one unit above MIM where a group has one channel ((1, 2), (1, 17), a group of 1 among five): lambda_max = trace(B), and
      the rounded square of the rounded root exceeded it.  MIC steps down one unit there.
  (d) rho_1^2 = -2.2e-308 for a zero cross block from 17 channels on (the midpoint of the last bracket, +- pivmin); clamped at 0.
  (h) SC_CANON_EIG=jacobi up to 16 channels (canonical_pair_kernel): rho_1^2 off by up to 6.8e7 (1.5e-8) from 4 x 4 channels on, where
      the stopping rule allows 2.5e4 -- the rotation angle is good to f32 only, and the diagonal block stored 0 for the pivot instead
      of the 1e-7 of it the rotation leaves.  It stores that remainder now and (c, s) are normalised to second order; at most 34 after.
Nothing in the whitening of any tier, the item loops of the value and the vectors kernels, the stores, or sc_jacobi.h.

Worst device ratios after the fixes (bars 128 / 128 / 8): (a) 2.0 / 1.5 / 1.26, (c) 2.0 / 1.0 / 0.98 and 2.98 between the vectors and the
value kernels, (d) 6.5 / 5.5 / 3.5, (e) 0.025 of a bar of 1, (g) under 1, (h) 34 against bars of 128 ... 25 476.

What each part is there to catch -- expectations from reading the kernels, not mutations that were run:
  a multisection cut short (fewer rounds, a bracket that does not close): the ratios of (a) and the clusters of (d);
  ``if (tid == 0) bad = 0`` or the e2 / dg arrays not rewritten at the top of an item: the bit-equality of (c) and fail of (g);
  the swap to the smaller group's side dropped or applied to one of the two member pointers only: (a) with the smaller group last;
  a row length of the LDS blocks that does not match the launch (small_ld): (a) at 17, 33 and 64, (i) at 33 and 65.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canonical_values_ref as vref                                           # noqa: E402
import epilogue_ref as eref                                                   # noqa: E402
import global_coherence_ref as gref                                           # noqa: E402
from guarded_buffers import BAND, FILL, guarded, guarded_memory, intact       # noqa: E402
from spectral_connectivity_amd import _lib, _stage_d, engine                  # noqa: E402

K_CANONICAL, K_MIC, K_MIM, K_CONDITIONING = vref.K_CANONICAL, vref.K_MIC, vref.K_MIM, vref.K_CONDITIONING
assert (K_CANONICAL, K_MIC, K_MIM, K_CONDITIONING) == (128.0, 128.0, 8.0, 1.0)
SC_EINVAL, SC_EUNSUPPORTED = -1, -5
CSM = eref.PLANE_CSM
N_OBS = vref.N_OBS
VIEWS = vref.VIEWS
KINDS = {"canonical": ("canonical",), "interaction": ("mic", "mim")}


def upload(rec):
    _lib.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(rec)).to("cuda:0")


def pack(mats, n_obs=N_OBS, dtype=np.float64):
    """(record [F, floats_per_bin], what a consumer must see [F, C, C]) of the matrices ``mats`` [F, C, C]: a bin each"""
    rec, stack = gref.record(np.asarray(mats)[None], n_obs, dtype, True)
    return rec, stack[0]


def run(view, accum, C, groups, n_obs=N_OBS, planes=CSM):
    """({kind: [F, G, G] float64}, fail) of one entry point on the records ``accum``"""
    groups = [np.asarray(g) for g in groups]
    G = len(groups)
    if view == "canonical":
        out, fail = engine.canonical_coherence(accum, C, planes, n_obs, groups)
        outs = {"canonical": out}
    else:
        members, sizes, _ = _lib.member_table(groups)
        mic, mim, fail = engine.imaginary_interaction(accum, C, planes, n_obs, members, sizes)
        outs = {"mic": mic, "mim": mim}
    for o in outs.values():
        assert tuple(o.shape) == (accum.shape[0], G, G) and o.dtype == torch.float64
    return {k: o.cpu().numpy() for k, o in outs.items()}, int(fail)


def well_formed(outs, what=""):
    """symmetric, NaN on the diagonal; MIC^2 <= MIM to the last bit"""
    for kind, o in outs.items():
        G = o.shape[-1]
        assert np.array_equal(o, o.swapaxes(-1, -2), equal_nan=True), (what, kind, "not symmetric")
        assert np.isnan(o[:, np.arange(G), np.arange(G)]).all(), (what, kind, "diagonal")
    if "mic" in outs:
        ok = ~np.isnan(outs["mic"])
        assert np.array_equal(ok, ~np.isnan(outs["mim"]))
        assert (outs["mic"][ok] * outs["mic"][ok] <= outs["mim"][ok]).all(), (what, "MIC^2 > MIM")


def ratios(outs, f, a, b, truth, n_min, kappa=1.0):
    """{kind: ratio} of the pair (a, b) of bin f"""
    return {kind: vref.check(kind, o[f, a, b], truth[kind], n_min, kappa) for kind, o in outs.items()}


def judge(worst, bad, what, bars=None):
    print(f"\n  {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, (what, bad)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_outputs(x, y):
    return x.keys() == y.keys() and all(same_bits(x[k], y[k]) for k in x)


# ---- (a) every tier at its edges ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def record_a(family, sizes, view):
    """(device record, groups, truths per bin) of a case of (a): uploaded once per case"""
    mats, groups, truths = vref.case_a(family, sizes, view)
    rec, seen = pack(mats)
    assert np.array_equal(seen, mats)
    return upload(rec), groups, truths


def pair_ratios(family, sizes, view, swapped, allowance=None):
    """(worst {kind: ratio}, [(bin, kind, ratio, bar)] above the bars, outputs) of a case of (a); ``swapped``: the groups change labels"""
    accum, groups, truths = record_a(family, sizes, view)
    order = [groups[1], groups[0]] if swapped else list(groups)
    outs, fail = run(view, accum, sum(sizes), order)
    assert fail == 0, f"fail = {fail}"
    well_formed(outs, (family, sizes, view))
    worst, bad = {}, []
    for f in range(accum.shape[0]):
        for kind, r in ratios(outs, f, 0, 1, truths[f], min(sizes)).items():
            bar = max(vref.BARS[kind], allowance or 0.0)
            worst[kind] = max(r, worst.get(kind, 0.0))
            if not r <= bar:
                bad.append((f, kind, r, bar))
    return worst, bad, outs


def device_ratios(family, sizes):
    """the worst ratios of a case of (a), both label orders (tools/canonical_values_accuracy.py)"""
    worst = {}
    for view in VIEWS:
        for swapped in (False, True):
            for k, v in pair_ratios(family, sizes, view, swapped)[0].items():
                worst[k] = max(v, worst.get(k, 0.0))
    return worst


@pytest.mark.parametrize("swapped", [False, True], ids=["smaller_first", "smaller_last"])
@pytest.mark.parametrize("family", vref.FAMILIES)
@pytest.mark.parametrize("sizes", vref.PAIR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_tier_at_its_edges(sizes, family, swapped):
    """``swapped``: the smaller group has the higher label (the swap at the top of canonical_big_hh_kernel; up to 16 channels B is
    then of the larger group's order, with zero eigenvalues)."""
    for view in VIEWS:
        worst, bad, _ = pair_ratios(family, sizes, view, swapped)
        judge(worst, bad, f"{family} {sizes} {view} swapped = {swapped}")


def several_groups(sizes, family, view, seed):
    """(mats [2, C, C], groups, {(a, b): truths per bin}) of a launch of several groups, every pair coupled"""
    G = len(sizes)
    pairs = [(a, b) for a in range(G) for b in range(a + 1, G)]
    if family == "exact":
        made = [vref.exact_groups(sizes, {(a, b): vref.distinct_coherences(min(sizes[a], sizes[b]), seed + 10 * f + 3 * a + b)
                                          for a, b in pairs}, seed + f, view) for f in range(2)]
        mats, groups = vref.stack_bins(made)
        truths = {p: [{k: vref.truth_exact(m.rho[p])[k] for k in KINDS[view]} for m in made] for p in pairs}
    else:
        made = [vref.free(sizes, 2 * sum(sizes), seed + f) for f in range(2)]
        mats, groups = vref.stack_bins(made)
        truths = {(a, b): [vref.truth_free(mats[f], groups[a], groups[b], view) for f in range(2)] for a, b in pairs}
    return mats, groups, truths


@pytest.mark.parametrize("family", vref.FAMILIES)
@pytest.mark.parametrize("sizes", [(5, 16, 9), (3, 16, 7, 12, 1), (8, 40, 100)], ids=lambda s: "x".join(map(str, s)))
def test_several_groups_in_one_launch(sizes, family):
    """Three groups of 5, 16 and 9 channels; five groups of at most 16 (ten pairs on workgroups of CB_WAVES = 8 waves: the last
    workgroup of a bin has idle waves); groups of 8, 40 and 100 (the pair (8, 40) stays in LDS, the pairs with the group of 100 use
    the scratch of the same launch)."""
    for view in VIEWS:
        mats, groups, truths = several_groups(sizes, family, view, 2000 + sum(sizes))
        outs, fail = run(view, upload(pack(mats)[0]), sum(sizes), groups)
        assert fail == 0
        well_formed(outs, sizes)
        worst, bad = {}, []
        for (a, b), per_bin in truths.items():
            for f, truth in enumerate(per_bin):
                for kind, r in ratios(outs, f, a, b, truth, min(sizes[a], sizes[b])).items():
                    worst[kind] = max(r, worst.get(kind, 0.0))
                    if not r <= vref.BARS[kind]:
                        bad.append((a, b, f, kind, r))
        judge(worst, bad, f"{family} groups {sizes} {view}")


# ---- (b) the record ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(16, 16), (17, 33), (65, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_record_variants_give_the_same_bits(sizes):
    """The ``exact`` family in float32 records (its entries have at most 19 bits), with n_obs = 12 (12 S / 12 = S: the kernels divide,
    and an IEEE quotient that is representable is exact), in a record that carries every other plane around SC_PLANE_CSM, and run
    twice: the matrix the kernels see is the same, so the outputs are the same bits."""
    C = sum(sizes)
    rng = np.random.default_rng(5)
    for view in VIEWS:
        mats, groups, _ = vref.case_a("exact", sizes, view)
        rec, seen = pack(mats)
        want, fail = run(view, upload(rec), C, groups)
        assert fail == 0
        assert same_outputs(run(view, upload(rec), C, groups)[0], want), "two runs differ"
        rec32, seen32 = pack(mats, dtype=np.float32)
        assert np.array_equal(seen32, seen), "float32 does not hold an entry"
        assert same_outputs(run(view, upload(rec32), C, groups)[0], want), "float32 records differ from float64 records of the same numbers"
        rec12, seen12 = pack(mats, n_obs=12)
        assert np.array_equal(seen12, seen) and not np.array_equal(rec12, rec)
        assert same_outputs(run(view, upload(rec12), C, groups, n_obs=12)[0], want), "n_obs = 12 differs from n_obs = 8"
        junk = {k: rng.standard_normal(mats.shape) for k in ("abs_im", "im_sq", "sign_im")}
        junk["unit"] = rng.standard_normal(mats.shape) + 1j * rng.standard_normal(mats.shape)
        full = eref.pack_record(dict(junk, s=mats * N_OBS), C, eref.PLANES_ALL, np.float64)
        assert full.shape[1] == 7 * rec.shape[1] // 2
        assert same_outputs(run(view, upload(full), C, groups, planes=eref.PLANES_ALL)[0], want), "the other planes of a record change the result"


# ---- (c) a workgroup takes a second item -------------------------------------------------------------------------------------------
def value_slots(items, max_group):
    """The persistent workgroups canonical_launch starts for groups of 17 ... 128 channels, from its code: up to 64 channels 256 x
    (workgroups a compute unit holds by LDS, at most 4), beyond 256."""
    if max_group > 64:
        return min(items, 256)
    lds = 2 * max_group * (max_group | 1) * 16
    per_cu = min(max((160 * 1024 - 8 * 1024) // (lds + 7 * 1024), 1), 4)
    return min(items, 256 * per_cu)


def diagonal_groups(sizes, seed, view):
    """``exact_groups`` with diagonal mixers (gains 1 and 2): S_gg and M are diagonal, every reflection of the reduction is the
    identity; every pair coupled"""
    G = len(sizes)
    rng = np.random.default_rng(seed)
    C = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    gains = [2.0 ** rng.integers(0, 2, n) for n in sizes]
    S = np.zeros((C, C), dtype=np.complex128)
    rho = {}
    for a in range(G):
        S[off[a]:off[a + 1], off[a]:off[a + 1]] = np.diag(gains[a] ** 2)
        for b in range(a + 1, G):
            n = min(sizes[a], sizes[b])
            r = vref.distinct_coherences(n, seed + 7 * a + b)
            X = np.zeros((sizes[a], sizes[b]), dtype=np.complex128)
            X[np.arange(n), np.arange(n)] = gains[a][:n] * r * gains[b][:n] * (1j if view == "interaction" else 1.0)
            S[off[a]:off[a + 1], off[b]:off[b + 1]] = X
            S[off[b]:off[b + 1], off[a]:off[a + 1]] = X.conj().T
            rho[(a, b)] = r
    return S + 0.0, rho


@pytest.mark.parametrize("sizes,F", [((17, 17, 17, 17), 180), ((65, 65, 65), 90)], ids=["4x17", "3x65"])
def test_a_workgroup_takes_a_second_item(sizes, F):
    """More (bin, pair) items than slots: 1080 against 1024 (768 in the canonical vectors kernel), 270 against 256.  Even bins hold a
    dense ``exact`` matrix, odd bins one whose group blocks and whitened cross blocks are diagonal (B diagonal: every reflection is
    the identity, e^2 = 0 throughout).  Items of the second pass follow items of both kinds on the d, e^2, v, w arrays and the LDS or
    scratch blocks of their workgroup.  Each of the two matrices is checked once against its exact coherences, and every bin that
    repeats it must repeat its bits.  The vectors kernels (sc_canonical_coherence_vectors_f64, sc_imaginary_interaction_vectors_f64:
    persistent loops with a rotation log per slot) run on the same records: their rho_1 agrees with the value kernels within the sum
    of the bars, and their vectors pass the identities of the vector suites on the first bin of each kind and repeat their bits."""
    from test_gpu_canonical_vectors import check_identities as canonical_identities
    from test_gpu_interaction_vectors import check_identities as interaction_identities
    G, C = len(sizes), sum(sizes)
    n_pairs = G * (G - 1) // 2
    items = F * n_pairs
    slots = value_slots(items, max(sizes))
    assert slots + 4 <= items <= 2 * slots, (items, slots)          # the formula above changed: this test would run one pass only
    assert slots == {17: 1024, 65: 256}[max(sizes)]
    pairs = [(a, b) for a in range(G) for b in range(a + 1, G)]
    kind_of_bin = np.arange(F) % 2
    for view in VIEWS:
        dense = vref.exact_groups(sizes, {p: vref.distinct_coherences(sizes[0], 3000 + 10 * p[0] + p[1]) for p in pairs}, 3100 + C, view)
        order = np.concatenate(dense.groups)
        diag, diag_rho = diagonal_groups(sizes, 3200 + C, view)
        moved = np.zeros_like(diag)
        moved[np.ix_(order, order)] = diag                          # the diagonal matrix on the dense one's member lists
        unique = np.array([dense.S, moved])
        rec_u, seen_u = pack(unique)
        assert np.array_equal(seen_u, unique)
        accum = upload(rec_u[kind_of_bin])
        outs, fail = run(view, accum, C, dense.groups)
        assert fail == 0
        well_formed(outs, (sizes, view))
        worst, bad = {}, []
        for k, rho in enumerate((dense.rho, diag_rho)):
            where = np.flatnonzero(kind_of_bin == k)
            for kind, o in outs.items():
                for f in where[1:]:
                    assert same_bits(o[f], o[where[0]]), f"{view} {kind}: bin {f} differs from bin {where[0]} holding the same matrix"
            for a, b in pairs:
                truth = vref.truth_exact(rho[(a, b)])
                for kind, r in ratios(outs, where[0], a, b, truth, sizes[0]).items():
                    worst[kind] = max(r, worst.get(kind, 0.0))
                    if not r <= vref.BARS[kind]:
                        bad.append((k, a, b, kind, r))
        judge(worst, bad, f"second item, groups {sizes}, {view}")
        # the vectors kernels on the same record
        members, msizes, _ = _lib.member_table([np.asarray(g) for g in dense.groups])
        firsts = [0, 1]
        if view == "canonical":
            coh, cohs, filt, patt, vfail = engine.canonical_coherence_vectors(accum, C, CSM, N_OBS, members, msizes)
            coh, cohs, filt, patt = (t.cpu().numpy() for t in (coh, cohs, filt, patt))
            filt, patt = filt[..., 0] + 1j * filt[..., 1], patt[..., 0] + 1j * patt[..., 1]
            got = (coh, cohs, filt, patt)
            canonical_identities(unique, tuple(x[firsts] for x in got) + (dense.groups,), 1e-9, 1e-9, f"second item {sizes}")
            ok = ~np.isnan(coh)
            err = np.abs(coh[ok].astype(vref.LD) ** 2 - outs["canonical"][ok].astype(vref.LD)).max() / vref.EPS
            bar = 2 * K_CANONICAL
        else:
            mic, filt, patt, vfail = engine.imaginary_interaction_vectors(accum, C, CSM, N_OBS, members, msizes)
            mic, filt, patt = (t.cpu().numpy() for t in (mic, filt, patt))
            got = (mic, filt, patt)
            interaction_identities(unique, tuple(x[firsts] for x in got) + (dense.groups,), 1e-9, 1e-9, f"second item {sizes}", interior=range(2))
            ok = ~np.isnan(mic)
            err = np.abs(mic[ok] - outs["mic"][ok]).max() / vref.EPS
            bar = 2 * K_MIC
        assert vfail == 0
        print(f"  vectors kernel against the value kernel, {view}: {err:.2f} (bar {bar:.0f})")
        assert err <= bar, (view, err, bar)
        for x in got:
            for k in (0, 1):
                where = np.flatnonzero(kind_of_bin == k)
                for f in where[1:]:
                    assert same_bits(x[f], x[where[0]]), f"vectors kernel, {view}: bin {f} differs from bin {where[0]} holding the same matrix"


# ---- (d) structure of the whitened spectrum ----------------------------------------------------------------------------------------
SIZES_D = (16, 17, 64, 65, 128)


def exact_bins(made, view, n, what, expect_zero=False):
    """the bins ``made`` (``exact`` results of one size) in one launch: every ratio under its bar; returns the outputs"""
    mats, groups = vref.stack_bins(made)
    outs, fail = run(view, upload(pack(mats)[0]), 2 * n, groups)
    assert fail == 0, (what, fail)
    well_formed(outs, what)
    worst, bad = {}, []
    for f, m in enumerate(made):
        truth = vref.truth_exact(m.rho.get((0, 1), np.zeros(1)))
        for kind, r in ratios(outs, f, 0, 1, truth, n).items():
            worst[kind] = max(r, worst.get(kind, 0.0))
            if not r <= vref.BARS[kind]:
                bad.append((f, kind, r))
    judge(worst, bad, what)
    return outs


@pytest.mark.parametrize("n", SIZES_D)
@pytest.mark.parametrize("name", list(vref.SPECTRA))
def test_structure_of_the_whitened_spectrum(name, n):
    """All coherences equal (B = c I behind unitary mixers: one cluster of n), rho_1 = 1 (the joint matrix is singular, both groups
    are positive definite), rho_1 = rho_2, a single non-zero coherence (B of rank one), all zero (rho_1^2 = 0, MIC exactly 0, MIM 0)
    and a graded spectrum 2^0 ... 2^-20; each as bin 1 behind a dense bin 0."""
    for view in VIEWS:
        made = [vref.exact(n, n, vref.distinct_coherences(n, 4000 + n), 4100 + n, view),
                vref.exact(n, n, vref.SPECTRA[name](n), 4200 + n, view)]
        outs = exact_bins(made, view, n, f"{name} n = {n} {view}")
        if name == "all_zero":
            for kind, o in outs.items():            # (rho_1^2: the midpoint of the last bracket around 0, under the bar and not negative)
                assert o[1, 0, 1] == 0.0 if kind != "canonical" else o[1, 0, 1] >= 0.0, (kind, o[1, 0, 1])


@pytest.mark.parametrize("n", SIZES_D)
@pytest.mark.parametrize("p", vref.CLUSTER_P)
def test_clusters(p, n):
    """Coherences 0.75 + k 2^-p, k = 0 ... n - 1.  At n = 16, p = 40 the unscaled three-term Sturm recurrence of cb_top_eigenvalue
    was predicted to lose every sign change to underflow of the product of consecutive minors (a NumPy emulation of its arithmetic:
    rho_1^2 off by 8166 x 2^-52)."""
    for view in VIEWS:
        exact_bins([vref.cluster_case(n, p, 4300 + n + p, view)], view, n, f"cluster p = {p} n = {n} {view}")


@pytest.mark.parametrize("n", SIZES_D)
def test_real_cross_block_has_no_interaction(n):
    """A cross block with an arbitrary real part and no imaginary part: MIC and MIM are exactly 0"""
    m = vref.exact(n, n, vref.distinct_coherences(n, 4400 + n), 4500 + n, "canonical")
    a, b = m.groups
    S = m.S.copy()
    S[np.ix_(a, b)] = S[np.ix_(a, b)].real + np.abs(S[np.ix_(a, b)].imag)       # (dense, real)
    S[np.ix_(b, a)] = S[np.ix_(a, b)].T
    assert np.array_equal(S, S.conj().T) and np.count_nonzero(S[np.ix_(a, b)]) > n
    outs, fail = run("interaction", upload(pack(S[None])[0]), 2 * n, m.groups)
    assert fail == 0
    well_formed(outs)
    assert outs["mic"][0, 0, 1] == 0.0 and outs["mim"][0, 0, 1] == 0.0, (outs["mic"][0, 0, 1], outs["mim"][0, 0, 1])


# ---- (e) the conditioning series ---------------------------------------------------------------------------------------------------
def device_conditioning_ratio(sizes, p):
    """the worst ratio of the three values on a case of the conditioning series, unit 2^-52 (kappa_a + kappa_b)"""
    worst = 0.0
    for view in VIEWS:
        S, groups, truth, kappa = vref.conditioning_case(sizes, p, view)
        outs, fail = run(view, upload(pack(S[None])[0]), sum(sizes), groups)
        assert fail == 0
        well_formed(outs)
        worst = max([worst] + list(ratios(outs, 0, 0, 1, truth, min(sizes), kappa).values()))
    return worst


@pytest.mark.parametrize("p", vref.CONDITIONING)
@pytest.mark.parametrize("sizes", vref.CONDITIONING_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conditioning_series(sizes, p):
    """Family ``exact`` with gains 2^0 ... 2^(p / 2): cond(S_gg) = 2^p ... 2^(p + 1); the error in units of 2^-52 (kappa_a + kappa_b)"""
    r = device_conditioning_ratio(sizes, p)
    print(f"\n  conditioning p = {p} {sizes}: {r:.4f}")
    assert r <= K_CONDITIONING, r


# ---- (f) amplitudes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0 ** -90, 2.0 ** 44])
@pytest.mark.parametrize("sizes", [(16, 16), (64, 65), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_amplitudes_of_real_recordings(sizes, scale):
    """The records of (a) times 2^-90 (tesla^2) and 2^44 (squares of 24-bit counts).  Both are even powers of two: the Cholesky factors
    are the unscaled ones times 2^-45 / 2^22 exactly (sqrt of an even power of two is exact), every quotient and product of the
    whitening scales by a power of two without rounding, M and B are the unscaled ones, and no threshold of the kernels (pivot > 0,
    pivmin relative to max e^2 of B) sees the scale: the outputs are identical in every bit, which is what is asserted."""
    for family in vref.FAMILIES:
        for view in VIEWS:
            mats, groups, _ = vref.case_a(family, sizes, view)
            want, fail = run(view, record_a(family, sizes, view)[0], sum(sizes), groups)
            assert fail == 0
            rec, seen = pack(mats * scale)
            assert np.array_equal(seen, mats * scale)
            got, fail = run(view, upload(rec), sum(sizes), groups)
            assert fail == 0
            assert same_outputs(got, want), f"{family} {view}: x 2^{int(np.log2(scale))} changes the result"


# ---- (g) groups that cannot be whitened --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(8, 8, 8), (40, 40, 40), (100, 100, 56)], ids=lambda s: "x".join(map(str, s)))
def test_group_that_cannot_be_whitened(sizes):
    """X^H X of Gaussian integers; the first two members of group 1 are the same channel, of power 25: l_00 = 5, l_10 = 25 / 5 = 5 and
    the second pivot is 25 - 5 x 5 = 0 without rounding, in the complex blocks and in their real parts.  Both pairs of group 1 are
    NaN in every output, the pair (0, 2) is under the bars, and ``fail`` counts the two pairs (include/sc_hip.h)."""
    C = sum(sizes)
    rng = np.random.default_rng(5000 + C)
    X = rng.integers(-3, 4, (2 * C, C)) + 1j * rng.integers(-3, 4, (2 * C, C))
    perm = rng.permutation(C)
    off = np.concatenate([[0], np.cumsum(sizes)])
    groups = [perm[off[g]:off[g + 1]].astype(np.int64) for g in range(3)]
    first, second = groups[1][:2]
    X[:, first] = 0
    X[0, first], X[1, first] = 3, 4j
    X[:, second] = X[:, first]
    S = X.conj().T @ X
    assert np.array_equal(S, S.conj().T) and S[first, first] == S[second, second] == S[first, second] == 25
    rec, seen = pack(S[None])
    assert np.array_equal(seen[0], S)
    for view in VIEWS:
        outs, fail = run(view, upload(rec), C, groups)
        assert fail == 2, (view, fail)
        well_formed(outs, sizes)
        truth = vref.truth_free(S, groups[0], groups[2], view)
        bad = []
        for kind, o in outs.items():
            assert np.isnan(o[0, 0, 1]) and np.isnan(o[0, 1, 2]), (view, kind, o[0])
            r = vref.check(kind, o[0, 0, 2], truth[kind], min(sizes[0], sizes[2]))
            print(f"  {view} {kind} of the pair (0, 2), groups {sizes}: {r:.2f}")
            if not r <= vref.BARS[kind]:
                bad.append((kind, r))
        assert not bad, bad


# ---- (h) the diagnostic kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", vref.FAMILIES)
@pytest.mark.parametrize("sizes", [(16, 16), (17, 32), (33, 64), (65, 128), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_diagnostic_jacobi_kernels(sizes, family, debug_env):
    """SC_CANON_EIG=jacobi, canonical coherence: canonical_pair_kernel (16), canonical_kernel<32> (32), canonical_big_kernel with the
    Jacobi of csrc/sc_jacobi.h beyond.  Bar: the larger of K_CANONICAL and what their stopping rule allows
    (canonical_values_ref.jacobi_allowance); and they agree with the default kernels within the sum of both bars."""
    allowance = vref.jacobi_allowance(sizes[0], sizes[1], max(sizes))
    for swapped in (False, True):
        _, _, default = pair_ratios(family, sizes, "canonical", swapped)
        debug_env("SC_CANON_EIG", "jacobi")
        worst, bad, outs = pair_ratios(family, sizes, "canonical", swapped, allowance=allowance)
        debug_env("SC_CANON_EIG", None)
        judge(worst, bad, f"SC_CANON_EIG=jacobi {family} {sizes} swapped = {swapped} (allowance {allowance:.1f})")
        apart = np.abs(outs["canonical"][:, 0, 1] - default["canonical"][:, 0, 1]).max() / vref.EPS
        assert apart <= K_CANONICAL + max(K_CANONICAL, allowance), apart


# ---- (i) writes and argument checks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 33, 65, 128])
def test_nothing_is_stored_outside_the_outputs(n):
    """The outputs and ``fail`` between two 4 KB bands each: the bands survive, the outputs are the bits of the ordinary run, and no
    element is left at the fill pattern."""
    fill = np.frombuffer(bytes([FILL]) * 8, dtype=np.float64)[0]
    for view in VIEWS:
        mats, groups, _ = vref.case_a("exact", (n, n), view)
        accum = record_a("exact", (n, n), view)[0]
        want, _ = run(view, accum, 2 * n, groups)
        mem = guarded_memory()
        mem.zeros = lambda shape, dtype, mem=mem: mem.empty(shape, dtype).zero_()      # ``fail`` between two bands as well
        if view == "canonical":
            out, fail = _stage_d.canonical_coherence(mem, accum, 2 * n, CSM, N_OBS, [np.asarray(g) for g in groups])
            got = {"canonical": out}
        else:
            members, sizes, _ = _lib.member_table([np.asarray(g) for g in groups])
            mic, mim, fail = _stage_d.imaginary_interaction(mem, accum, 2 * n, CSM, N_OBS, members, sizes)
            got = {"mic": mic, "mim": mim}
        torch.cuda.synchronize()
        assert fail == 0
        assert mem.sizes() == [accum.shape[0] * 4 * 8] * len(got) + [4], mem.sizes()
        assert mem.intact(), f"n = {n} {view}: stored outside the outputs"
        got = {k: o.cpu().numpy() for k, o in got.items()}
        assert same_outputs(got, want)
        assert not any((o == fill).any() for o in got.values()), "an element was not written"


def call(view, accum, n_bins, C, planes, n_obs, members, sizes, G, max_group, outs, fail, null=None):
    """the status of an entry point called through ctypes on raw buffers; ``null``: the name of one pointer to pass as NULL"""
    stream = engine.TorchMemory(torch.device("cuda:0")).stream()
    ptr = {"accum": accum.data_ptr(), "members": members.data_ptr(), "sizes": sizes.data_ptr(), "fail": fail.data_ptr() + BAND}
    for k, o in enumerate(outs):
        ptr[f"out{k}"] = o.data_ptr() + BAND
    if null:
        ptr[null] = None
    p = {k: ctypes.c_void_p(v) for k, v in ptr.items()}
    lib = _lib._handle()
    fn = lib.sc_canonical_coherence_f64 if view == "canonical" else lib.sc_imaginary_interaction_f64
    return fn(p["accum"], n_bins, C, planes, n_obs, p["members"], p["sizes"], G, max_group, *[p[f"out{k}"] for k in range(len(outs))],
              p["fail"], stream)


@pytest.mark.parametrize("what,code,args", [
    ("NULL accum", SC_EINVAL, dict(null="accum")),
    ("NULL members", SC_EINVAL, dict(null="members")),
    ("NULL sizes", SC_EINVAL, dict(null="sizes")),
    ("NULL out", SC_EINVAL, dict(null="out0")),
    ("NULL second out", SC_EINVAL, dict(null="out1")),
    ("NULL fail", SC_EINVAL, dict(null="fail")),
    ("n_groups = 0", SC_EINVAL, dict(G=0)),
    ("n_bins = 0", SC_EINVAL, dict(n_bins=0)),
    ("max_group_size = 129", SC_EUNSUPPORTED, dict(max_group=129)),
    ("no SC_PLANE_CSM", SC_EINVAL, dict(planes=eref.PLANE_UNIT)),
])
def test_argument_checks(what, code, args):
    """include/sc_hip.h: SC_EINVAL for a NULL pointer, an empty problem or a record without SC_PLANE_CSM, SC_EUNSUPPORTED for a group
    of more than sc_canonical_max_group() channels; either before anything is launched or written"""
    _lib.require_gpu()
    assert _lib._handle().sc_canonical_max_group() == 128
    C, G, n_bins = 12, 2, 3
    kw = dict(n_bins=n_bins, planes=CSM, G=G, max_group=6, null=None)
    kw.update(args)
    lay = eref.layout(C, CSM)
    accum = torch.zeros((n_bins, lay.floats_per_bin), dtype=torch.float64, device="cuda:0")
    members_h, sizes_h, _ = _lib.member_table([np.arange(6), np.arange(6, 12)])
    members, sizes = torch.from_numpy(members_h).to("cuda:0"), torch.from_numpy(sizes_h).to("cuda:0")
    n_out = n_bins * G * G * 8
    for view in VIEWS:
        if kw["null"] == "out1" and view == "canonical":
            continue
        outs = [guarded(n_out) for _ in KINDS[view]]
        fail = guarded(4)
        status = call(view, accum, kw["n_bins"], C, kw["planes"] | _lib.RECORD_F64, N_OBS, members, sizes, kw["G"], kw["max_group"], outs, fail,
                      kw["null"])
        torch.cuda.synchronize()
        assert status == code, (view, status, _lib._handle().sc_last_error())
        for buf, n in [(o, n_out) for o in outs] + [(fail, 4)]:
            assert intact(buf, n) and bool((buf[BAND:BAND + n] == FILL).all()), f"{view}: a refused call wrote"
