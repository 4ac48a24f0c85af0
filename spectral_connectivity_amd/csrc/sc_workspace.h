// sc_workspace.h -- the caller workspaces of the Wilson-family entry points (sc_wilson.hip, sc_wilson_pair.hip, sc_mvar.hip,
// sc_conditional.hip, sc_blockwise.hip).  One layout function per entry point: its sc_*_workspace_bytes query runs it on a counting
// carver, the entry point on d_work, so the two cannot disagree.  Plain C++17 integer logic with no HIP in it: a host compiler
// builds it alone (tests/test_workspace_layouts.py does, over a grid of sizes).  Z: the caller's 16-byte complex type.  "reserved"
// items are bytes the queries have always counted and nothing uses: the hosts size their chunks from these totals.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct ScWsLog { int n; struct { const char* name; size_t offset, bytes; } item[24]; };     // the items in carving order (tests)
// Hands out consecutive items of a workspace, each at an offset rounded up to `align`.  base == nullptr: counts only.
struct ScCarver {
    char* base;
    size_t used = 0;
    ScWsLog* log = nullptr;
    explicit ScCarver(void* b) : base((char*)b) {}
    template <class T> T* take(const char* name, size_t count, size_t align = 1) {
        const size_t at = (used + align - 1) / align * align;
        if (log && log->n < 24) log->item[log->n++] = {name, at, count * sizeof(T)};
        used = at + count * sizeof(T);
        return base ? (T*)(base + at) : nullptr;
    }
    // the region from here on is either what `a` or, later, what `b` took (copies of *this made here): as long as the longer
    void either(const ScCarver& a, const ScCarver& b) { used = a.used > b.used ? a.used : b.used; }
};

// sc_granger_pairwise_f64 (batched form) and sc_wilson_factor_f64: P problems of N two-sided bins, series [P][4][N].  n_fallback:
// `fallback_bytes` for the count of problems started from the identity, the slots of WilsonCounters (sc_wilson_loop.h) behind them.
template <class Z> struct WsWilson { double* S; Z *G, *A; double *err, *h0, *hinv, *rot; int32_t* n_fallback; size_t fallback_bytes; };
template <class Z> WsWilson<Z> ws_wilson(ScCarver& w, size_t P, size_t N, size_t hist) {
    WsWilson<Z> k;
    k.S = w.take<double>("S", P * N * 4);            // (s00, s11, Re s01, Im s01)
    k.G = w.take<Z>("G", P * N * 4); k.A = w.take<Z>("A", P * N * 4); k.err = w.take<double>("err", P);
    k.h0 = w.take<double>("h0", P * 4); k.hinv = w.take<double>("hinv", P * 4); k.rot = w.take<double>("rot", P * 4);
    k.n_fallback = (int32_t*)w.take<char>("n_fallback", k.fallback_bytes = 256); w.take<int32_t>("n_running", hist);
    w.take<char>("reserved", P * 8);                 // (4 + 4 bytes per problem: n_iter and status are the caller's arrays)
    return k;
}
// the same request in the resident form (sc_wilson_pair.hip): half factors [P][4][N/2+1]; the summary behind the per-pair flags
template <class Z> struct WsPair { Z* Ghalf; double *chol, *h0, *hinv, *rot; int32_t *batch_bad, *summary; };
template <class Z> WsPair<Z> ws_pair(ScCarver& w, size_t P, size_t n_pairs, size_t N) {
    WsPair<Z> k;
    k.Ghalf = w.take<Z>("Ghalf", P * (N / 2 + 1) * 4);
    k.chol = w.take<double>("chol", P * 4); k.h0 = w.take<double>("h0", P * 4); k.hinv = w.take<double>("hinv", P * 4);
    k.rot = w.take<double>("rot", P * 4); k.batch_bad = w.take<int32_t>("batch_bad", n_pairs); k.summary = w.take<int32_t>("summary", 64);
    return k;
}

// sc_mvar_factor_f64: [P][N][C][C] series; beyond small_max signals also G^-1 and T = G^-1 S.  Beyond cmid signals T is first the
// scratch of the blocked inverse; the product after it writes T (G and T swap per iteration, so the entry point passes T itself).
template <class Z> struct WsMvarFactor { Z *S, *G, *A, *Ginv, *T; double *err, *g0; int32_t* n_fallback; size_t fallback_bytes; };
template <class Z> WsMvarFactor<Z> ws_mvar_factor(ScCarver& w, size_t P, size_t C, size_t N, size_t small_max, size_t cmid, size_t hist) {
    const size_t X = P * C * C * N, big = C > small_max;
    WsMvarFactor<Z> k;
    k.S = w.take<Z>("S", X); k.G = w.take<Z>("G", X); k.A = w.take<Z>("A", X);
    k.Ginv = big ? w.take<Z>("Ginv", X) : nullptr;
    ScCarver t = w, s = w;
    k.T = big ? t.take<Z>("T", X) : nullptr; s.take<Z>("T.inverse_scratch", C > cmid ? X : 0); w.either(t, s);
    k.err = w.take<double>("err", P); k.g0 = w.take<double>("g0", P * C * C);
    k.n_fallback = (int32_t*)w.take<char>("n_fallback", k.fallback_bytes = 64); w.take<int32_t>("n_running", hist);
    w.take<char>("reserved", P * 8 + 64 + 256);      // (the query counts P * 16 + 128 for err and n_fallback, and 256 on top)
    return k;
}
// sc_mvar_measure_f64: [P][N/2+1][C][C] natural layout.  Until A_mvar is written it parks H0 and (H0 + lam I)^-1 as complex matrices.
// sq: per (window, bin) and, before that, per (window, 256-element chunk); lam: [0] of H0, [1] of H; scratch (16-aligned, beyond
// cmid signals only): the blocked inverse's matrices, then m_measure's squared moduli.
template <class Z> struct WsMvarMeasure { Z *H, *Amv, *h0c, *hinvc, *scratch; double *h0, *hinv, *sigma, *sq, *tot, *lam; };
template <class Z> WsMvarMeasure<Z> ws_mvar_measure(ScCarver& w, size_t P, size_t C, size_t N, size_t cmid) {
    const size_t E = C * C, F = N / 2 + 1, f16 = F > 16 ? F : 16, chunks = (E + 255) / 256;
    WsMvarMeasure<Z> k;
    k.H = w.take<Z>("H", P * F * E);
    ScCarver a = w, parked = w;
    k.Amv = a.take<Z>("Amv", P * F * E);
    k.h0c = parked.take<Z>("Amv.h0c", P * E); k.hinvc = parked.take<Z>("Amv.hinvc", P * E); w.either(a, parked);
    k.h0 = w.take<double>("h0", P * E); k.hinv = w.take<double>("hinv", P * E); k.sigma = w.take<double>("sigma", P * E);
    k.sq = w.take<double>("sq", P * (f16 > chunks ? f16 : chunks));
    k.tot = w.take<double>("tot", P * C); k.lam = w.take<double>("lam", 8);
    const size_t pad = C > cmid ? (16 - w.used % 16) % 16 : 0;
    k.scratch = C > cmid ? w.take<Z>("scratch", P * F * E, 16) : nullptr;
    w.take<char>("reserved", P * 8 + 192 - pad + 256);      // (the query counts P * 8 + 256 for lam and the rounding, and 256 on top)
    return k;
}
struct ScWsZ { double x, y; };
inline size_t ws_mvar_bytes(size_t P, size_t C, size_t N, size_t small_max, size_t cmid, size_t hist) {      // sc_mvar_workspace_bytes:
    ScCarver f(nullptr), m(nullptr);                                                                          // one workspace for both
    ws_mvar_factor<ScWsZ>(f, P, C, N, small_max, cmid, hist);
    ws_mvar_measure<ScWsZ>(m, P, C, N, cmid);
    return f.used > m.used ? f.used : m.used;
}

// sc_conditional_granger_f64, G groups x D dropped signals of C, 256-aligned items: Psi0^T [G][C][C], M [G][F][C][C], one double 0
// (the Tikhonov term of the small inverse), S_red (later Phi^-1) and Phi [D G][N][C-1][C-1].  The tail is the workspace of the
// reduced factorisation (mvar_bytes: sc_mvar_workspace_bytes of D G problems of C - 1 signals) and, once that has returned, Phi0
// [D G][C-1][C-1], K and right behind it the blocked inverse's scratch (beyond 128 reduced signals) at the first F bins.
template <class Z> struct WsConditional { Z *Psi0T, *M, *Sred, *Phi, *Phi0, *K, *scratch; double* zero; void* mvar; size_t mvar_bytes; };
template <class Z> WsConditional<Z> ws_conditional(ScCarver& w, size_t G, size_t C, size_t N, size_t D, size_t mvar_bytes) {
    const size_t E = C * C, Er = (C - 1) * (C - 1), F = N / 2 + 1, X = G * D * N * Er, Xb = X * sizeof(Z);
    WsConditional<Z> k;
    k.Psi0T = w.take<Z>("Psi0T", G * E, 256); k.M = w.take<Z>("M", G * F * E, 256); k.zero = w.take<double>("zero", 32, 256);
    k.Sred = w.take<Z>("Sred", X, 256); k.Phi = w.take<Z>("Phi", X, 256);
    ScCarver f = w, e = w;
    k.mvar = f.take<char>("tail.mvar", k.mvar_bytes = mvar_bytes, 256);
    k.Phi0 = e.take<Z>("tail.Phi0", G * D * Er, 256); k.K = e.take<Z>("tail.K", X, 256); k.scratch = e.take<Z>("tail.scratch", X);
    e.take<char>("tail.reserved", 2 * (((Xb + 255) & ~(size_t)255) - Xb));      // (the query rounds K and the scratch up to 256 each)
    w.either(f, e); w.take<char>("end", 0, 256);
    return k;
}
// sc_blockwise_granger_f64, P = pairs x groups problems of m signals: S2 and Psi [P][N][m][m]; in the tail, after the factorisation,
// R [P][m][m], Y = Psi R [P][F][m][m] and bw_nullspace's Psi0 (double [P][m][m], read beyond BW_LDS_NULLSPACE signals only)
template <class Z> struct WsBlockwise { Z *S2, *Psi, *R, *Y; double* psi0; void* mvar; size_t mvar_bytes; };
template <class Z> WsBlockwise<Z> ws_blockwise(ScCarver& w, size_t P, size_t m, size_t N, size_t mvar_bytes) {
    const size_t E = m * m, F = N / 2 + 1;
    WsBlockwise<Z> k;
    k.S2 = w.take<Z>("S2", P * N * E, 256); k.Psi = w.take<Z>("Psi", P * N * E, 256);
    ScCarver f = w, e = w;
    k.mvar = f.take<char>("tail.mvar", k.mvar_bytes = mvar_bytes, 256);
    k.R = e.take<Z>("tail.R", P * E, 256); k.Y = e.take<Z>("tail.Y", P * F * E, 256);
    k.psi0 = e.take<double>("tail.psi0", P * E, 256);
    w.either(f, e); w.take<char>("end", 0, 256);
    return k;
}
