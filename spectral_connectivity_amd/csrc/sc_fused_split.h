// sc_fused_split.h -- into which parts the one-pass stage-B kernels (sc_fused.hip, sc_fused2.hip) cut the observation chunks of a
// bin.  Plain C++17 integer logic with no HIP in it: a host compiler builds it alone (tests/test_fused_split_plan.py does, over a
// grid of shapes).
//
// One workgroup fills a compute unit (LDS), so the n_bins x n_parts workgroups of a launch run in rounds of n_cu, handed out in
// block order as compute units fall free, and what is left of the last round is idle time: 903 bins in three EQUAL parts on 256
// compute units are 10.58 rounds of work that take 11.  A TAPERED plan cuts a bin into n_parts - 1 equal big parts and one short
// tail part, and the launch runs the big parts of all bins first, the tail parts last: the short workgroups fill the hole
// behind the last round of big ones (cfg3 at 500 trials: 100 + 10 chunks, 421 model units against 452 for one part of 110).
//
// Cost model (round 4's, fitted on 125 ... 1000 trials of cfg3): a workgroup costs its chunks + 3 chunks' worth of prologue,
// record write and drain; every part beyond the first adds 2 % (the partial records the epilogue / combine kernel reads); a big
// part has at least 16 chunks.
#pragma once
#include <stdint.h>

enum {
    FU_SPLIT_MAX = 24,           // parts per bin at most
    FU_SPLIT_MIN_BIG = 16,       // chunks of a big part at least (n_parts > 1)
    FU_SPLIT_FIXED = 3,          // chunks' worth of fixed cost per workgroup
    FU_SPLIT_CANDIDATES = 256,   // big-part sizes tried per part count
    FU_SPLIT_TAPER_ROUNDS = 7    // tapered plans only where the equal parts run in at most this many rounds (fu_split_plan)
};

// Part k sums the chunks [bound[k], bound[k + 1]).  tail = 0: n_parts equal parts, bound[k] = k n_chunks / n_parts, blocks in
// (bin, part) order.  tail > 0: the last part has `tail` chunks, the n_parts - 1 before it share the rest equally, and the big
// parts of every bin are dispatched ahead of the tail parts (fu_part_range in sc_fused_common.h).
struct FuSplitPlan {
    int n_parts, tail;
    int bound[FU_SPLIT_MAX + 1];
    double makespan;             // the model's, in chunks (0: a forced plan, not priced)
};

inline double fu_split_part_factor(int n_parts) { return 1.0 + 0.02 * (n_parts - 1); }

// bound[k] in closed form, as the kernels compute it (n_big = the parts ahead of the tail part: n_parts - 1, or n_parts without one)
#ifdef __HIPCC__
__host__ __device__
#endif
inline int fu_split_bound(int k, int n_big, int n_chunks, int tail) {
    return k < n_big ? (int)((int64_t)k * (n_chunks - tail) / n_big) : (k == n_big ? n_chunks - tail : n_chunks);
}
// bound[] of n_parts parts with a tail of `tail` chunks (0: equal parts)
inline void fu_split_fill(FuSplitPlan* p, int n_chunks, int n_parts, int tail) {
    p->n_parts = n_parts;
    p->tail = n_parts > 1 ? tail : 0;
    const int n_big = p->tail ? n_parts - 1 : n_parts, big_chunks = n_chunks - p->tail;
    for (int k = 0; k <= FU_SPLIT_MAX; ++k) p->bound[k] = n_chunks;
    for (int k = 0; k < n_big; ++k) p->bound[k] = (int)((int64_t)k * big_chunks / n_big);
    if (p->tail) p->bound[n_big] = big_chunks;
    p->makespan = 0.0;
}

// Equal parts: rounds of workgroups x (chunks of a part + fixed cost) x 2 % per extra part.
inline double fu_split_equal_cost(int n_bins, int n_chunks, int n_cu, int S) {
    const double rounds = (double)(((int64_t)n_bins * S + n_cu - 1) / n_cu);
    return rounds * ((double)n_chunks / S + FU_SPLIT_FIXED) * fu_split_part_factor(S);
}
// The number of equal parts with the least of that cost (the rule of the rounds before the tapered plans).
inline int fu_split_equal_parts(int n_bins, int n_chunks, int n_cu) {
    int best = 1;
    double best_cost = 1e30;
    for (int S = 1; S <= FU_SPLIT_MAX; ++S) {
        if (S > 1 && n_chunks / S < FU_SPLIT_MIN_BIG) break;
        const double cost = fu_split_equal_cost(n_bins, n_chunks, n_cu, S);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = S; }
    }
    return best;
}
// What S equal parts take at the least, however the dispatch deals them: the parts of a bin differ by one chunk when S does not
// divide n_chunks, the rounds formula prices them all at the mean, and a dispatch in order of arrival can come out below it.  Some
// compute unit runs ceil(n_bins S / n_cu) workgroups of at least the shortest part, and all of them together run all the work.
// (Equal to fu_split_equal_cost when S divides n_chunks and n_cu divides n_bins S.)
inline double fu_split_equal_floor(int n_bins, int n_chunks, int n_cu, int S) {
    const int64_t rounds = ((int64_t)n_bins * S + n_cu - 1) / n_cu;
    const double by_rounds = (double)(rounds * (n_chunks / S + FU_SPLIT_FIXED));
    const double by_work = (double)((int64_t)n_bins * (n_chunks + (int64_t)FU_SPLIT_FIXED * S)) / n_cu;
    return (by_rounds > by_work ? by_rounds : by_work) * fu_split_part_factor(S);
}

// Makespan of the tapered plan of S parts, S - 1 of `big` chunks and a tail of `tail`, closed form of a dispatch in block order
// to whichever compute unit is free first: the B = n_bins (S - 1) big workgroups run in R full rounds and leave r = B mod n_cu
// compute units one big workgroup ahead of the others.  The tail workgroups go to the n_cu - r units behind, q = ceil(big cost /
// tail cost) each until those have caught up (they end d < one tail workgroup ahead), and what is left of them is dealt over all
// units, the r that are behind by d first.
inline double fu_split_tapered_cost(int n_bins, int n_cu, int S, int big, int tail) {
    const int64_t cb = big + FU_SPLIT_FIXED, ct = tail + FU_SPLIT_FIXED;
    const int64_t B = (int64_t)n_bins * (S - 1), R = B / n_cu, r = B % n_cu, P = n_cu, nb = n_bins;
    int64_t U;
    if (r == 0) {
        U = R * cb + (nb + P - 1) / P * ct;
    } else {
        const int64_t low = P - r, q = (cb + ct - 1) / ct, hole = low * q, high = (R + 1) * cb;
        if (nb <= hole) {
            const int64_t filled = R * cb + (nb + low - 1) / low * ct;
            U = filled > high ? filled : high;
        } else {
            const int64_t d = R * cb + q * ct - high, left = nb - hole, m = left / P, rem = left % P;
            U = rem == 0 ? high + d + m * ct : rem <= r ? high + (m + 1) * ct : high + d + (m + 1) * ct;
        }
    }
    return (double)U * fu_split_part_factor(S);
}

// The plan of a launch of n_bins bins of n_chunks chunks on n_cu compute units: the best tapered plan under the model if it beats
// what the best number of equal parts can take at the least (fu_split_equal_floor: no tapered plan is chosen on the strength of
// the rounds formula's rounding) by more than 1 %, the equal parts otherwise.  Tapered candidates have big parts of one size
// (n_parts - 1 divides n_chunks - tail), which is what makes the closed form exact, and a tail shorter than a big part; per part
// count at most FU_SPLIT_CANDIDATES sizes, evenly spaced, are priced: the cost of a call is bounded whatever n_chunks is.
// A guard from measurement, not a term of the model (profiles/tapered_split_ab.txt): where the equal parts already run in many
// rounds the model's gain did not show on MI355X -- cfg3, 2709 workgroups in 11 rounds: fused2_kernel 3.51 ms with 3 x 73 chunks
// and with 197 + 22, for a predicted 6 % --, while it showed at 4 rounds (500 trials: -2.8 %) and at 7 (256 channels: -4.7 %).
// So shapes whose equal parts take more than FU_SPLIT_TAPER_ROUNDS rounds keep them.
inline void fu_split_plan(int n_bins, int n_chunks, int n_cu, FuSplitPlan* out) {
    if (n_bins < 1) n_bins = 1;
    if (n_chunks < 1) n_chunks = 1;
    if (n_cu < 1) n_cu = 1;
    const int S_eq = fu_split_equal_parts(n_bins, n_chunks, n_cu);
    const double floor_eq = fu_split_equal_floor(n_bins, n_chunks, n_cu, S_eq);
    const bool taper = ((int64_t)n_bins * S_eq + n_cu - 1) / n_cu <= FU_SPLIT_TAPER_ROUNDS;
    int best_S = 0, best_big = 0;
    double best = 0.99 * floor_eq;
    for (int S = 2; taper && S <= FU_SPLIT_MAX; ++S) {
        // big (S - 1) + tail = n_chunks with 1 <= tail < big: n_chunks / S < big <= (n_chunks - 1) / (S - 1)
        int lo = n_chunks / S + 1;
        if (lo < FU_SPLIT_MIN_BIG) lo = FU_SPLIT_MIN_BIG;
        const int hi = (n_chunks - 1) / (S - 1);
        if (hi < lo) continue;
        const int step = (hi - lo + FU_SPLIT_CANDIDATES) / FU_SPLIT_CANDIDATES;
        for (int big = lo; big <= hi; big += step) {
            const double cost = fu_split_tapered_cost(n_bins, n_cu, S, big, n_chunks - big * (S - 1));
            if (cost < best - 1e-9) { best = cost; best_S = S; best_big = big; }
        }
    }
    if (best_S) {
        fu_split_fill(out, n_chunks, best_S, n_chunks - best_big * (best_S - 1));
        out->makespan = best;
    } else {
        fu_split_fill(out, n_chunks, S_eq, 0);
        out->makespan = fu_split_equal_cost(n_bins, n_chunks, n_cu, S_eq);
    }
}

// A plan fixed from outside (the diagnostic switches): n_parts parts, a tail of `tail` chunks (0: equal parts, the split of
// SC_FUSED_SPLIT alone).  false: the parts would not all have a chunk.
inline bool fu_split_forced(int n_chunks, int n_parts, int tail, FuSplitPlan* out) {
    if (n_parts < 1 || n_parts > FU_SPLIT_MAX || tail < 0) return false;
    if (n_parts == 1) { fu_split_fill(out, n_chunks, 1, 0); return true; }
    const int n_big = tail ? n_parts - 1 : n_parts;
    if ((n_chunks - tail) / n_big < 1) return false;
    fu_split_fill(out, n_chunks, n_parts, tail);
    return true;
}
