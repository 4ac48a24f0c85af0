// sc_fused_plan.h -- which launches cover the record of the one-pass stage-B kernels (sc_fused.hip, sc_fused2.hip).  Plain
// C++17 integer logic with no HIP in it: a host compiler builds it alone (tests/test_fused_plan.py does, for every n).
#pragma once

// One launch: it stages the nb (<= 4) 32-channel blocks `blocks` (ascending block numbers of the record's channels) and
// owns the products (bi <= bj, bj >= col_lo, bi < row_hi) of them, bi / bj counting the staged blocks.
struct FuLaunch { int nb, blocks[4], col_lo, row_hi; };

enum {
    FU_PLAN_MAX_BLOCKS = 32,        // 1024 signals
    FU_PLAN_MAX_LAUNCHES = 120      // what 32 blocks take: 8 triangles + 112 rectangles (31 blocks: 8 + 98 + 14 with the lone one)
};

// Every tile of the record once: writes the launches for n 32-channel blocks to out[FU_PLAN_MAX_LAUNCHES], in launch
// order, and returns their count (0: n is out of range).  Up to 128 channels: one launch, the triangle of its 1 ... 4
// blocks.  Above, a launch can stage four of the n = 5 ... 8 blocks at a time, and the n (n + 1) / 2 block products are
// dealt over launches so that few blocks are staged twice (each staging reads its channels from HBM again):
//   n = 5   triangle {0,1,2};  {0,1} x {3,4};  {2} x {3,4} + triangle {3,4}                        15 products, 10 staged
//   n = 6   triangle {0,1,2,3};  {0,1} x {4,5} + triangle {4,5};  {2,3} x {4,5}                     21 products, 12 staged
//   n = 7   triangle {0,1,2,3};  {0} x {4,5,6} + triangle {4,5,6};  {1}, {2}, {3} x {4,5,6}         28 products, 20 staged
//   n = 8   triangle {0..3};  triangle {4..7};  {0,1}, {2,3} x {4,5}, {6,7}                         36 products, 24 staged
// (round 2 ran every count in 129 ... 255 as n = 8: 160 channels cost what 256 do).
// More than 256 signals (round 6; before: the host tiled the channels in blocks of 128 and paid a gathered 256-channel
// triangle per block pair, on the complex64 kernels).  Groups of four consecutive blocks take their triangle; two halves
// (pairs of blocks) of DIFFERENT groups take their 64 x 64 rectangle; with an odd block count the last block is a group (or
// the third block of one) of its own and meets every pair outside its group as a 64 x 32 rectangle, shape (3, 2, 2).  Every
// 32 x 32 block product exactly once.
inline int fu_plan(int n, FuLaunch* out) {
    static const FuLaunch tri[4] = {{1, {0}, 0, 1}, {2, {0, 1}, 0, 2}, {3, {0, 1, 2}, 0, 3}, {4, {0, 1, 2, 3}, 0, 4}};
    static const FuLaunch p5[] = {{3, {0, 1, 2}, 0, 3}, {4, {0, 1, 3, 4}, 2, 2}, {3, {2, 3, 4}, 1, 3}};
    static const FuLaunch p6[] = {{4, {0, 1, 2, 3}, 0, 4}, {4, {0, 1, 4, 5}, 2, 4}, {4, {2, 3, 4, 5}, 2, 2}};
    static const FuLaunch p7[] = {{4, {0, 1, 2, 3}, 0, 4}, {4, {0, 4, 5, 6}, 1, 4}, {4, {1, 4, 5, 6}, 1, 1},
                                  {4, {2, 4, 5, 6}, 1, 1}, {4, {3, 4, 5, 6}, 1, 1}};
    static const FuLaunch p8[] = {{4, {0, 1, 2, 3}, 0, 4}, {4, {4, 5, 6, 7}, 0, 4}, {4, {0, 1, 4, 5}, 2, 2},
                                  {4, {0, 1, 6, 7}, 2, 2}, {4, {2, 3, 4, 5}, 2, 2}, {4, {2, 3, 6, 7}, 2, 2}};
    if (n < 1 || n > FU_PLAN_MAX_BLOCKS) return 0;
    int k = 0;
    if (n <= 8) {
        const FuLaunch* plan = n <= 4 ? &tri[n - 1] : n == 5 ? p5 : n == 6 ? p6 : n == 7 ? p7 : p8;
        const int n_launch = n <= 4 ? 1 : n == 5 ? 3 : n == 6 ? 3 : n == 7 ? 5 : 6;
        for (int l = 0; l < n_launch; ++l) out[k++] = plan[l];
        return k;
    }
    const int n_pairs = n / 2, lone = (n & 1) ? n - 1 : -1;
    for (int g0 = 0; g0 < n; g0 += 4) {
        FuLaunch t = tri[(n - g0 < 4 ? n - g0 : 4) - 1];
        for (int b = 0; b < t.nb; ++b) t.blocks[b] += g0;
        out[k++] = t;
    }
    for (int hi = 0; hi < n_pairs; ++hi) {
        for (int hj = hi + 1; hj < n_pairs; ++hj) {
            if (hi / 2 == hj / 2) continue;                    // the two halves of one group: inside its triangle
            out[k++] = FuLaunch{4, {2 * hi, 2 * hi + 1, 2 * hj, 2 * hj + 1}, 2, 2};
        }
        if (lone >= 0 && hi / 2 != lone / 4) out[k++] = FuLaunch{3, {2 * hi, 2 * hi + 1, lone}, 2, 2};
    }
    return k;
}
