// sc_seed_layout.h -- the seed record (sc_seed.hip writes it, sc_seed_jackknife.hip writes and reads one): where its sums are and
// which counts and planes a call may ask for.  Host code only.
#pragma once
#include "sc_common.h"

namespace {

constexpr int SEED_TILE = 64;                       // targets of a wave: one per lane
constexpr int SEED_CHUNK = 4;                       // seeds of a workgroup
constexpr int SEED_MAX = 64;
constexpr uint32_t SEED_PLANES_ALL = SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ | SC_PLANE_SIGN_IM | SC_PLANE_UNIT | SC_SEED_PLANE_POWER;

// where the sums of a record are: planes (in [n_seeds][n_targets] blocks from the start of a bin) or -1, the powers (in doubles) or -1
struct SeedLayout {
    int p_csm, p_abs, p_sq, p_sign, p_unit;
    int64_t pow_off, per_bin;
};

inline SeedLayout seed_layout(int n_seeds, int n_targets, uint32_t planes) {
    SeedLayout l;
    const uint32_t acc = planes & ~SC_SEED_PLANE_POWER;
    l.p_csm = (planes & SC_PLANE_CSM) ? sc_plane_offset(acc, SC_PLANE_CSM) : -1;
    l.p_abs = (planes & SC_PLANE_ABS_IM) ? sc_plane_offset(acc, SC_PLANE_ABS_IM) : -1;
    l.p_sq = (planes & SC_PLANE_IM_SQ) ? sc_plane_offset(acc, SC_PLANE_IM_SQ) : -1;
    l.p_sign = (planes & SC_PLANE_SIGN_IM) ? sc_plane_offset(acc, SC_PLANE_SIGN_IM) : -1;
    l.p_unit = (planes & SC_PLANE_UNIT) ? sc_plane_offset(acc, SC_PLANE_UNIT) : -1;
    const int64_t cells = (int64_t)sc_plane_count(acc) * n_seeds * n_targets;
    l.pow_off = (planes & SC_SEED_PLANE_POWER) ? cells : -1;
    l.per_bin = cells + ((planes & SC_SEED_PLANE_POWER) ? n_seeds + n_targets : 0);
    return l;
}

inline int seed_check_counts(int64_t n_seeds, int64_t n_targets, uint32_t planes) {
    SC_REQUIRE(n_seeds >= 1 && n_seeds <= SEED_MAX, "n_seeds: 1 ... sc_seed_connectivity_max_seeds()");
    SC_REQUIRE(n_targets >= 1 && n_targets <= 32768, "n_targets: 1 ... 32768");
    SC_REQUIRE(planes && !(planes & ~SEED_PLANES_ALL) && (planes & ~SC_SEED_PLANE_POWER),
               "planes: a set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM, _UNIT with at least one of them, and SC_SEED_PLANE_POWER");
    return SC_OK;
}

}  // namespace
