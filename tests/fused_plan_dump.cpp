// Prints the stage-B launch plan (spectral_connectivity_amd/csrc/sc_fused_plan.h, nothing else) for every block count:
// one line "n nb b0 b1 b2 b3 col_lo row_hi" per launch, in launch order; blocks past nb print as -1.
// tests/test_fused_plan.py builds this with the host compiler and checks the lines.
#include <cstdio>
#include "sc_fused_plan.h"

int main() {
    std::printf("capacity %d %d\n", (int)FU_PLAN_MAX_BLOCKS, (int)FU_PLAN_MAX_LAUNCHES);
    for (int n = 0; n <= FU_PLAN_MAX_BLOCKS + 1; ++n) {
        FuLaunch plan[FU_PLAN_MAX_LAUNCHES];
        const int count = fu_plan(n, plan);
        if (count < 0 || count > FU_PLAN_MAX_LAUNCHES) return 1;
        std::printf("count %d %d\n", n, count);
        for (int l = 0; l < count; ++l) {
            const FuLaunch& p = plan[l];
            std::printf("%d %d", n, p.nb);
            for (int b = 0; b < 4; ++b) std::printf(" %d", b < p.nb ? p.blocks[b] : -1);
            std::printf(" %d %d\n", p.col_lo, p.row_hi);
        }
    }
    return 0;
}
