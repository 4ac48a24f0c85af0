// sc_seed.hip -- seed-based connectivity: a few signals (seeds) against a list of signals (targets) in one pass over the spectra (gfx950).
//
// seed_accumulate_kernel.  For a kept index and bin the un-normalised sums over the observations of, per (seed, target) and only
// for the families asked for, with s = x_seed conj(x_target):
//     Re s, Im s | |Im s| | (Im s)^2 | sign(Im s) | Re, Im of (x_seed / |x_seed|) conj(x_target / |x_target|) | |x_seed|^2, |x_target|^2
// One workgroup of 256 threads owns (bin, tile of 64 targets, chunk of 4 seeds, share of the observations).  A lane owns one target:
// it reads its coefficient of every row straight from global memory by index, so a wave's load is 512 contiguous bytes of a row
// (1024 of complex128 spectra) when the targets are contiguous and ascending.  The rows are walked 32 at a time; wave w takes the
// rows w, w + 4, ... of a block and has its 8 loads in flight together with the block's seed coefficients, which 128 threads
// stage in LDS once per block (with their unit phasors and |x|^2), so that a seed's coefficient comes from HBM for one workgroup
// and from cache for the others -- the seed chunks and target tiles of a bin are consecutive workgroups.  Which families are summed
// is a wave-uniform mask (scalar branches, no divergent lanes).  Products are in the engine's precision; complex64 spectra sum a
// wave's (at most 8) rows of a block in float32 and add that to the fp64 sum after the block -- except Im s, |Im s| and (Im s)^2 where
// (Im s)^2 is asked for, which take every term in fp64 (the debiased wPLI cancels) --, complex128 spectra sum in fp64 directly.
// At the end the four waves' sums are added in wave order through LDS.  Where bins x tiles x chunks do not fill the chip the
// observations are split over gridDim.y workgroups that write partial records to the workspace, added in split order by
// seed_fold_kernel: no floating-point atomics, results are bit-identical from run to run.
//
// Record: double [bin][plane][n_seeds][n_targets] with the planes in the order of the accumulator records (sc_plane_offset), then
// (SC_SEED_PLANE_POWER) the power sums [n_seeds] and [n_targets] of the bin.  Records of trial shards add.
//
// seed_measure_kernel: record -> measures, one thread per (bin, seed, target), with measure_value of the measures epilogue
// (sc_measure_value.h): the formulas, the eps floors, the n_obs-dependent debiasing and -- where a seed is its own target -- what
// each measure puts on its diagonal.
#include "sc_measure_value.h"
#include "sc_seed_layout.h"
#include "sc_workspace.h"

namespace {

constexpr int SEED_ROWS = 32;                       // observation rows per staging block
constexpr int SEED_WAVES = 4;
constexpr int SEED_RPW = SEED_ROWS / SEED_WAVES;    // rows of a block a wave walks: its loads in flight
constexpr int SEED_MAX_SPLITS = 256;
constexpr int SEED_MAX_MEASURES = 10;

// (the record's layout and the checks of the counts and planes: sc_seed_layout.h; 7 sums per seed of a chunk in a thread's registers)
struct SeedArgs {
    ScAxes a;
    const int32_t* seeds;
    const int32_t* targets;      // nullptr: target t is signal t
    int n_seeds, n_targets, n_chunks, n_tiles;
    uint32_t planes;
    SeedLayout l;
    int n_obs, rows_per_split;
    int64_t record_doubles;
    double* out;                 // split y writes at out + y * record_doubles
};

template <typename T> __device__ __forceinline__ T seed_rsqrt(T x);
template <> __device__ __forceinline__ float seed_rsqrt<float>(float x) { return rsqrtf(x); }       // 0 -> inf -> 0 * inf = NaN, like x / abs(x)
template <> __device__ __forceinline__ double seed_rsqrt<double>(double x) { return 1.0 / sqrt(x); }

template <typename T, typename T2>
__global__ __launch_bounds__(256) void seed_accumulate_kernel(const T2* __restrict__ X, SeedArgs p) {
    constexpr bool F32 = sizeof(T) == 4;
    __shared__ T2 sx[SEED_ROWS][SEED_CHUNK];          // the seeds' coefficients of the block's rows
    __shared__ T2 su[SEED_ROWS][SEED_CHUNK];          // ... and their unit phasors
    __shared__ int64_t row_off[SEED_ROWS];            // element offset of every row of the block: one decode per row
    __shared__ double red[SEED_WAVES][SEED_CHUNK][SEED_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t wg = blockIdx.x;
    const int chunk = (int)(wg % p.n_chunks); wg /= p.n_chunks;
    const int tile = (int)(wg % p.n_tiles);
    const int64_t bin = wg / p.n_tiles;
    const int f = (int)(bin % p.a.F), grp = (int)(bin / p.a.F);
    const T2* Xb = X + (int64_t)f * p.a.sF + sc_group_offset(p.a, grp);
    const int C = p.a.C;
    const int s0 = chunk * SEED_CHUNK;
    const int ns = p.n_seeds - s0 < SEED_CHUNK ? p.n_seeds - s0 : SEED_CHUNK;
    const bool want_csm = p.planes & SC_PLANE_CSM, want_abs = p.planes & SC_PLANE_ABS_IM, want_sq = p.planes & SC_PLANE_IM_SQ,
               want_sign = p.planes & SC_PLANE_SIGN_IM, want_unit = p.planes & SC_PLANE_UNIT, want_pow = p.planes & SC_SEED_PLANE_POWER;

    // this lane's target; a lane past the list, or an index outside the signals, reads nothing and stores nothing
    const int t = tile * SEED_TILE + lane;
    int ct = -1;
    if (t < p.n_targets) ct = p.targets ? p.targets[t] : t;
    const bool t_ok = (unsigned)ct < (unsigned)C;
    // the (row, seed) this thread stages: threads 0 .. 127
    const int st_r = tid >> 2, st_s = tid & (SEED_CHUNK - 1);
    int cs = -1;
    if (tid < SEED_ROWS * SEED_CHUNK && st_s < ns) cs = p.seeds[s0 + st_s];
    const bool s_ok = (unsigned)cs < (unsigned)C;

    const int r_begin = (int)blockIdx.y * p.rows_per_split;
    const int r_end = r_begin + p.rows_per_split < p.n_obs ? r_begin + p.rows_per_split : p.n_obs;

    // q: 0 Re s, 1 Im s, 2 |Im s|, 3 (Im s)^2, 4 sign Im s, 5 / 6 Re / Im of the unit-phasor product
    double acc[7][SEED_CHUNK] = {};
    T part[7][SEED_CHUNK] = {};
    double pow_t = 0.0, pow_s = 0.0;
    T part_t = 0;
    auto add = [&](int q, int s, T v) {
        if constexpr (F32) part[q][s] += v;
        else acc[q][s] += v;
    };

    for (int r0 = r_begin; r0 < r_end; r0 += SEED_ROWS) {
        const int nr = r_end - r0 < SEED_ROWS ? r_end - r0 : SEED_ROWS;
        __syncthreads();
        if (tid < nr) row_off[tid] = sc_obs_offset(p.a, r0 + tid);
        __syncthreads();
        T2 xs;
        xs.x = 0; xs.y = 0;
        if (s_ok && st_r < nr) xs = Xb[row_off[st_r] + cs];
        T2 xt[SEED_RPW];
#pragma unroll
        for (int k = 0; k < SEED_RPW; ++k) {
            const int r = wave + SEED_WAVES * k;
            xt[k].x = 0; xt[k].y = 0;
            if (t_ok && r < nr) xt[k] = Xb[row_off[r] + ct];
        }
        if (tid < SEED_ROWS * SEED_CHUNK) {
            sx[st_r][st_s] = xs;
            T pw = xs.x * xs.x + xs.y * xs.y;
            if (want_unit) {
                const T ia = seed_rsqrt<T>(pw);
                T2 u;
                u.x = xs.x * ia; u.y = xs.y * ia;
                su[st_r][st_s] = u;
            }
            if (want_pow) {
                // the block's |x_seed|^2 over the 16 rows of this wave (waves 0 and 1): lanes 0 .. 3 end with the sum of their seed
#pragma unroll
                for (int off = SEED_CHUNK; off < 64; off <<= 1) pw += __shfl_xor(pw, off);
                pow_s += (double)pw;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SEED_RPW; ++k) {
            const int r = wave + SEED_WAVES * k;
            if (r >= nr) break;
            const T2 x = xt[k];
            if (want_pow) {
                if constexpr (F32) part_t += x.x * x.x + x.y * x.y;
                else pow_t += x.x * x.x + x.y * x.y;
            }
            T2 u;
            u.x = 0; u.y = 0;
            if (want_unit) {
                const T ia = seed_rsqrt<T>(x.x * x.x + x.y * x.y);
                u.x = x.x * ia; u.y = x.y * ia;
            }
#pragma unroll
            for (int s = 0; s < SEED_CHUNK; ++s) {
                if (s >= ns) break;
                const T2 y = sx[r][s];
                const T im = y.y * x.x - y.x * x.y;                  // Im of x_seed conj(x_target)
                if (want_csm) add(0, s, y.x * x.x + y.y * x.y);
                if (F32 && want_sq) {
                    // the debiased wPLI is (A^2 - Q) / (B^2 - Q) of A = sum Im s, B = sum |Im s|, Q = sum (Im s)^2, two differences that
                    // cancel when few observations dominate (two observations: +-1 exactly): its three sums take every term in fp64
                    // -- the square of a float is exact there -- so that they are the sums of ONE set of values Im s
                    const double d = (double)im;
                    if (want_csm) acc[1][s] += d;
                    if (want_abs) acc[2][s] += d < 0 ? -d : d;
                    acc[3][s] = fma(d, d, acc[3][s]);
                } else {
                    if (want_csm) add(1, s, im);
                    if (want_abs) add(2, s, im < 0 ? -im : im);
                    if (want_sq) add(3, s, im * im);
                }
                if (want_sign) add(4, s, (T)((im > 0) - (im < 0)));
                if (want_unit) {
                    const T2 v = su[r][s];
                    add(5, s, v.x * u.x + v.y * u.y);
                    add(6, s, v.y * u.x - v.x * u.y);
                }
            }
        }
        if constexpr (F32) {
#pragma unroll
            for (int q = 0; q < 7; ++q)
#pragma unroll
                for (int s = 0; s < SEED_CHUNK; ++s) {
                    acc[q][s] += (double)part[q][s];
                    part[q][s] = 0;
                }
            pow_t += (double)part_t;
            part_t = 0;
        }
    }

    // the four waves' sums, added in wave order; wave w then stores seed w of the chunk
    double* out = p.out + (int64_t)blockIdx.y * p.record_doubles + bin * p.l.per_bin;
    const int64_t cells = (int64_t)p.n_seeds * p.n_targets;
    auto fold_store = [&](int q, int plane) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SEED_CHUNK; ++s) red[wave][s][lane] = acc[q][s];
        __syncthreads();
        const double v = red[0][wave][lane] + red[1][wave][lane] + red[2][wave][lane] + red[3][wave][lane];
        if (wave < ns && t < p.n_targets) out[plane * cells + (int64_t)(s0 + wave) * p.n_targets + t] = t_ok ? v : 0.0;
    };
    if (want_csm) { fold_store(0, p.l.p_csm); fold_store(1, p.l.p_csm + 1); }
    if (want_abs) fold_store(2, p.l.p_abs);
    if (want_sq) fold_store(3, p.l.p_sq);
    if (want_sign) fold_store(4, p.l.p_sign);
    if (want_unit) { fold_store(5, p.l.p_unit); fold_store(6, p.l.p_unit + 1); }
    if (want_pow) {
        __syncthreads();
        red[wave][0][lane] = pow_t;
        red[wave][1][lane] = pow_s;          // (lanes 0 .. 3 of waves 0 and 1 hold the seeds' sums)
        __syncthreads();
        if (wave == 0) {
            if (chunk == 0 && t < p.n_targets)
                out[p.l.pow_off + p.n_seeds + t] = t_ok ? red[0][0][lane] + red[1][0][lane] + red[2][0][lane] + red[3][0][lane] : 0.0;
            if (tile == 0 && lane < ns) out[p.l.pow_off + s0 + lane] = red[0][1][lane] + red[1][1][lane];
        }
    }
}

// partial records of the observation splits -> the record, in split order
__global__ void seed_fold_kernel(const double* __restrict__ ws, int n_splits, int64_t record_doubles, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= record_doubles) return;
    double v = ws[e];
    for (int s = 1; s < n_splits; ++s) v += ws[(int64_t)s * record_doubles + e];
    out[e] = v;
}

// One description of a call: the query sizes the workspace from it and the launcher carves the workspace with it.
struct SeedPlan {
    ScAxes a;
    SeedLayout l;
    int n_seeds, n_targets, n_chunks, n_tiles;
    uint32_t planes;
    int64_t n_bins, record_doubles, rows_per_split, n_splits;
};

int seed_plan(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t planes, SeedPlan* pl) {
    SC_REQUIRE(desc, "NULL descriptor");
    if (sc_make_axes(desc, &pl->a) != SC_OK) return SC_EINVAL;
    const ScAxes& a = pl->a;
    SC_REQUIRE(a.F >= 1 && a.W >= 1 && a.R >= 1 && a.K >= 1 && a.C >= 1 && a.C <= 32768, "bad spectra sizes");
    const int rc = seed_check_counts(n_seeds, n_targets, planes);
    if (rc != SC_OK) return rc;
    pl->n_seeds = (int)n_seeds; pl->n_targets = (int)n_targets; pl->planes = planes;
    pl->l = seed_layout(pl->n_seeds, pl->n_targets, planes);
    pl->n_chunks = (pl->n_seeds + SEED_CHUNK - 1) / SEED_CHUNK;
    pl->n_tiles = (pl->n_targets + SEED_TILE - 1) / SEED_TILE;
    pl->n_bins = (int64_t)a.n_groups * a.F;
    pl->record_doubles = pl->n_bins * pl->l.per_bin;
    const int64_t base = pl->n_bins * pl->n_tiles * pl->n_chunks;
    SC_REQUIRE(base < (int64_t)1 << 31, "too many (bin, target tile, seed chunk) workgroups for one launch");
    // splits of the observations: only when the workgroups above leave compute units idle, and never less than a row block each
    int64_t want = base >= 1024 ? 1 : (2048 + base - 1) / base;
    const int64_t by_rows = a.n_obs / SEED_ROWS > 1 ? a.n_obs / SEED_ROWS : 1;
    if (want > by_rows) want = by_rows;
    if (want > SEED_MAX_SPLITS) want = SEED_MAX_SPLITS;
    int64_t per = (a.n_obs + want - 1) / want;
    per = (per + SEED_ROWS - 1) / SEED_ROWS * SEED_ROWS;
    pl->rows_per_split = per;
    pl->n_splits = (a.n_obs + per - 1) / per;
    return SC_OK;
}

struct SeedWorkspace { double* partial; };
SeedWorkspace seed_workspace(ScCarver& w, const SeedPlan& pl) {
    SeedWorkspace k;
    k.partial = w.take<double>("partial records", pl.n_splits > 1 ? (size_t)(pl.n_splits * pl.record_doubles) : 0, 16);
    return k;
}

template <typename T, typename T2>
int seed_accumulate_run(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                        const int32_t* d_targets, int64_t n_targets, uint32_t planes, double* d_record, void* d_workspace,
                        int64_t workspace_bytes, void* stream) {
    ScTimed timed_("seed_accumulate", stream);
    SeedPlan pl;
    const int rc = seed_plan(desc, n_seeds, n_targets, planes, &pl);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_X && d_seeds && d_record, "NULL argument");
    ScCarver need(nullptr);
    seed_workspace(need, pl);
    SC_REQUIRE(need.used == 0 || (d_workspace && workspace_bytes >= (int64_t)need.used), "workspace too small");
    SC_REQUIRE((uintptr_t)d_workspace % 16 == 0, "workspace must be 16-byte aligned");
    ScCarver carve(d_workspace);
    const SeedWorkspace ws = seed_workspace(carve, pl);
    SeedArgs p = {};
    p.a = pl.a;
    p.seeds = d_seeds; p.targets = d_targets;
    p.n_seeds = pl.n_seeds; p.n_targets = pl.n_targets; p.n_chunks = pl.n_chunks; p.n_tiles = pl.n_tiles;
    p.planes = planes;
    p.l = pl.l;
    p.n_obs = pl.a.n_obs; p.rows_per_split = (int)pl.rows_per_split;
    p.record_doubles = pl.record_doubles;
    p.out = pl.n_splits > 1 ? ws.partial : d_record;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(pl.n_bins * pl.n_tiles * pl.n_chunks), (unsigned)pl.n_splits);
    hipLaunchKernelGGL((seed_accumulate_kernel<T, T2>), grid, dim3(256), 0, st, (const T2*)d_X, p);
    SC_CHECK_HIP(hipGetLastError());
    if (pl.n_splits > 1) {
        hipLaunchKernelGGL(seed_fold_kernel, dim3((unsigned)((pl.record_doubles + 255) / 256)), dim3(256), 0, st,
                           (const double*)ws.partial, (int)pl.n_splits, pl.record_doubles, d_record);
        SC_CHECK_HIP(hipGetLastError());
    }
    return SC_OK;
}

// ---- record -> measures ------------------------------------------------------------------------------------------------------------
struct SeedMeasureArgs {
    const double* rec;
    const int32_t* seeds;
    const int32_t* targets;
    int n_seeds, n_targets;
    int64_t total;               // n_bins * n_seeds * n_targets
    SeedLayout l;
    double n_obs, rn_obs;
    int n_measures;
    int measure[SEED_MAX_MEASURES], wide[SEED_MAX_MEASURES];
    void* out[SEED_MAX_MEASURES];
};

__global__ __launch_bounds__(256) void seed_measure_kernel(SeedMeasureArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int64_t cells = (int64_t)a.n_seeds * a.n_targets;
    const int64_t bin = idx / cells, e = idx - bin * cells;
    const int s = (int)(e / a.n_targets), t = (int)(e - (int64_t)s * a.n_targets);
    const double* r = a.rec + bin * a.l.per_bin;
    MeasureIn v = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (a.l.p_csm >= 0) { v.s_re = r[a.l.p_csm * cells + e]; v.s_im = r[(a.l.p_csm + 1) * cells + e]; }
    if (a.l.pow_off >= 0) { v.p_i = r[a.l.pow_off + s]; v.p_j = r[a.l.pow_off + a.n_seeds + t]; }
    if (a.l.p_abs >= 0) v.sa = r[a.l.p_abs * cells + e];
    if (a.l.p_sq >= 0) v.sq = r[a.l.p_sq * cells + e];
    if (a.l.p_sign >= 0) v.sg = r[a.l.p_sign * cells + e];
    if (a.l.p_unit >= 0) { v.u_re = r[a.l.p_unit * cells + e]; v.u_im = r[(a.l.p_unit + 1) * cells + e]; }
    const int cs = a.seeds[s], ct = a.targets ? a.targets[t] : t;
    const bool diag = cs == ct;                                         // a seed that is its own target: the measure's diagonal
    // Below the diagonal the all-pairs epilogue negates the entry above it, whose sum starts at +0: a cross-spectrum that is real
    // in every observation (the zero and Nyquist bins of a real series) has Im S = -0 there and a coherence phase of -pi where it
    // is negative.  The same sign of zero here (nothing else changes: -(-x + 0) = x for x != 0).
    if (cs > ct) v.s_im = -(-v.s_im + 0.0);
    for (int m = 0; m < a.n_measures; ++m) {
        const double2 x = measure_value(a.measure[m], a.n_obs, a.rn_obs, v, diag);
        if (a.measure[m] == SC_M_COHERENCY) {
            if (a.wide[m]) ((double2*)a.out[m])[idx] = x;
            else ((float2*)a.out[m])[idx] = make_float2((float)x.x, (float)x.y);
        } else {
            if (a.wide[m]) ((double*)a.out[m])[idx] = x.x;
            else ((float*)a.out[m])[idx] = (float)x.x;
        }
    }
}

// planes of a record a measure reads, 0: not a measure of this kernel
uint32_t seed_measure_needs(int measure) {
    switch (measure) {
    case SC_M_COHERENCY: case SC_M_COHERENCE_MAGNITUDE: case SC_M_COHERENCE_PHASE: case SC_M_IMAGINARY_COHERENCE:
        return SC_PLANE_CSM | SC_SEED_PLANE_POWER;
    case SC_M_PLV: case SC_M_PPC: return SC_PLANE_UNIT;
    case SC_M_PLI: case SC_M_DEBIASED_PLI2: return SC_PLANE_SIGN_IM;
    case SC_M_WPLI: return SC_PLANE_CSM | SC_PLANE_ABS_IM;
    case SC_M_DEBIASED_WPLI2: return SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ;
    }
    return 0;
}

}  // namespace

extern "C" int sc_seed_connectivity_max_seeds(void) { return SEED_MAX; }

extern "C" int sc_seed_record_layout(int64_t n_seeds, int64_t n_targets, uint32_t planes, int64_t* doubles_per_bin) {
    const int rc = seed_check_counts(n_seeds, n_targets, planes);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(doubles_per_bin, "NULL argument");
    *doubles_per_bin = seed_layout((int)n_seeds, (int)n_targets, planes).per_bin;
    return SC_OK;
}

extern "C" int64_t sc_seed_accumulate_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t planes) {
    SeedPlan pl;
    if (seed_plan(desc, n_seeds, n_targets, planes, &pl) != SC_OK) return 0;
    ScCarver need(nullptr);
    seed_workspace(need, pl);
    return (int64_t)need.used;
}

extern "C" int sc_seed_accumulate_f32(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                      const int32_t* d_targets, int64_t n_targets, uint32_t planes, double* d_record,
                                      void* d_workspace, int64_t workspace_bytes, void* stream) {
    return seed_accumulate_run<float, float2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, planes, d_record, d_workspace,
                                              workspace_bytes, stream);
}

extern "C" int sc_seed_accumulate_f64(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                      const int32_t* d_targets, int64_t n_targets, uint32_t planes, double* d_record,
                                      void* d_workspace, int64_t workspace_bytes, void* stream) {
    return seed_accumulate_run<double, double2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, planes, d_record, d_workspace,
                                                workspace_bytes, stream);
}

extern "C" int sc_seed_measure_f64(const double* d_record, int64_t n_bins, const int32_t* d_seeds, int64_t n_seeds,
                                   const int32_t* d_targets, int64_t n_targets, uint32_t planes, int64_t n_observations,
                                   int n_measures, const int* measures, const int* wide, void* const* d_outs, void* stream) {
    ScTimed timed_("seed_measure", stream);
    const int rc = seed_check_counts(n_seeds, n_targets, planes);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_record && d_seeds && measures && wide && d_outs, "NULL argument");
    SC_REQUIRE(n_bins >= 1 && n_observations >= 1, "dimensions must be positive");
    SC_REQUIRE(n_measures >= 1 && n_measures <= SEED_MAX_MEASURES, "1 ... 10 measures per launch");
    SeedMeasureArgs a = {};
    a.rec = d_record; a.seeds = d_seeds; a.targets = d_targets;
    a.n_seeds = (int)n_seeds; a.n_targets = (int)n_targets;
    a.l = seed_layout(a.n_seeds, a.n_targets, planes);
    a.total = n_bins * n_seeds * n_targets;
    SC_REQUIRE((a.total + 255) / 256 < (int64_t)1 << 31, "output too large for one launch");
    a.n_obs = (double)n_observations;
    a.rn_obs = 1.0 / a.n_obs;
    a.n_measures = n_measures;
    for (int m = 0; m < n_measures; ++m) {
        const uint32_t need = seed_measure_needs(measures[m]);
        if (!need) {
            sc_set_error("sc_seed_measure_f64: measure %d is not one of the ten seed measures", measures[m]);
            return SC_EINVAL;
        }
        if ((planes & need) != need) {
            sc_set_error("measure %d needs the planes 0x%x, the seed record has 0x%x", measures[m], need, planes);
            return SC_EINVAL;
        }
        SC_REQUIRE(d_outs[m] != nullptr, "NULL output");
        a.measure[m] = measures[m]; a.wide[m] = wide[m] ? 1 : 0; a.out[m] = d_outs[m];
    }
    hipLaunchKernelGGL(seed_measure_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
