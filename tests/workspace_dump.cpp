// Prints the workspace layouts of the Wilson-family entry points (spectral_connectivity_amd/csrc/sc_workspace.h, nothing else)
// over a grid of problems.  Per layout one line "L <layout> <small_max> <a> <b> <c> <d> <total bytes>" (a ... d: the layout's
// dimensions, see main) followed by one line "I <name> <offset> <bytes>" per item, in carving order.
// tests/test_workspace_layouts.py builds this with the host compiler and checks the lines.
#include <cstdio>
#include "sc_workspace.h"

static const size_t CMID = 128, HIST = 1024;        // MV_CMID, WILSON_HIST
static ScWsLog g_log;

template <class Layout>
static void dump(const char* name, size_t small_max, size_t a, size_t b, size_t c, size_t d, Layout layout) {
    ScCarver w(nullptr);
    g_log.n = 0;
    w.log = &g_log;
    layout(w);
    std::printf("L %s %zu %zu %zu %zu %zu %zu\n", name, small_max, a, b, c, d, w.used);
    for (int i = 0; i < g_log.n; ++i) std::printf("I %s %zu %zu\n", g_log.item[i].name, g_log.item[i].offset, g_log.item[i].bytes);
}

int main() {
    const size_t Cs[] = {1, 2, 5, 16, 47, 48, 49, 64, 65, 96, 128, 129, 256, 257, 512};
    const size_t Ns[] = {2, 4, 8, 32, 256, 4096, 250, 512, 1000, 1024, 2048, 4000};       // the grid, then more lengths of the resident form
    const size_t Ps[] = {1, 2, 7}, Ds[] = {1, 2, 28}, smalls[] = {48, 64};
    for (size_t G : Ps)
        for (size_t D : Ds)
            for (size_t N : Ns) {
                dump("wilson", 0, G, D, N, 0, [&](ScCarver& w) { ws_wilson<ScWsZ>(w, G * D, N, HIST); });
                dump("pair", 0, G, D, N, 0, [&](ScCarver& w) { ws_pair<ScWsZ>(w, G * D, D, N); });
            }
    for (size_t sm : smalls)
        for (size_t P : Ps)
            for (size_t C : Cs)
                for (int n = 0; n < 6; ++n) {
                    const size_t N = Ns[n];
                    dump("mvar_factor", sm, P, C, N, 0, [&](ScCarver& w) { ws_mvar_factor<ScWsZ>(w, P, C, N, sm, CMID, HIST); });
                    dump("mvar_measure", sm, P, C, N, 0, [&](ScCarver& w) { ws_mvar_measure<ScWsZ>(w, P, C, N, CMID); });
                    std::printf("L mvar %zu %zu %zu %zu 0 %zu\n", sm, P, C, N, ws_mvar_bytes(P, C, N, sm, CMID, HIST));
                    if (C < 2) continue;
                    for (size_t D : Ds) {
                        dump("conditional", sm, P, C, N, D, [&](ScCarver& w) {
                            ws_conditional<ScWsZ>(w, P, C, N, D, ws_mvar_bytes(P * D, C - 1, N, sm, CMID, HIST));
                        });
                        dump("blockwise", sm, P, C, N, D, [&](ScCarver& w) {
                            ws_blockwise<ScWsZ>(w, P * D, C, N, ws_mvar_bytes(P * D, C, N, sm, CMID, HIST));
                        });
                    }
                }
    return 0;
}
