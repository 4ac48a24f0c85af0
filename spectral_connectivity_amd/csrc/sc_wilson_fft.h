// sc_wilson_fft.h -- the register-resident fp64 transform the Wilson kernels share (sc_wilson_fft.hip: one causal projection per
// launch over series in HBM; sc_wilson_pair.hip: the whole 2 x 2 iteration of a channel pair on one compute unit).
// N = 256 .. 4096 (powers of two): 16 points per thread, radix 16 x 16 x R3 with R3 = N / 256 in {1, 2, 4, 8, 16}; the first
// pass takes x[i + t N/16] and the last leaves X[i + t N/16] in the same thread's registers.  Twiddles W_N^m = lo[m & 63] *
// hi[m >> 6] from two small LDS tables.  The butterflies zdft2/4/8/16 and zmul are those of sc_complex.h.
#pragma once
#include "sc_common.h"

#define WF_PHYS(idx) ((idx) + ((idx) >> 4))

// One forward transform of the NF series of this workgroup: a[t] = x[i + t TPF] in, a[t] = X[i + t TPF] out.
template <int LOG2N>
__device__ __forceinline__ void wf_fft(cd (&a)[16], cd* zf, const cd* lo, const cd* hi, int i) {
    constexpr int N = 1 << LOG2N, TPF = N / 16, R3 = N / 256;
    cd o[16];
    auto W = [&](int m) -> cd { return zmul(lo[m & 63], hi[m >> 6]); };
    __syncthreads();                    // tables visible (first call); the previous transform's reads of z done
    zdft16(a, o);
#pragma unroll
    for (int u = 0; u < 16; ++u) zf[WF_PHYS(16 * i + u)] = o[u];
    __syncthreads();
    const int kk = i & 15;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const cd v = zf[WF_PHYS(i + t * TPF)];
        a[t] = (t == 0) ? v : zmul(v, W(t * kk * (N / 256)));
    }
    zdft16(a, o);
    if constexpr (R3 == 1) {
#pragma unroll
        for (int t = 0; t < 16; ++t) a[t] = o[t];         // X[i + 16 t]
        return;
    } else {
        __syncthreads();
        const int j = ((i - kk) << 4) + kk;
#pragma unroll
        for (int u = 0; u < 16; ++u) zf[WF_PHYS(j + 16 * u)] = o[u];
        __syncthreads();
        if constexpr (R3 == 16) {                          // one radix-16 butterfly per thread, ib = i
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const cd v = zf[WF_PHYS(i + t * 256)];
                a[t] = (t == 0) ? v : zmul(v, W(t * i));
            }
            zdft16(a, o);
#pragma unroll
            for (int t = 0; t < 16; ++t) a[t] = o[t];      // X[i + 256 t]
        } else {
            constexpr int NB3 = 16 / R3;
#pragma unroll
            for (int b = 0; b < NB3; ++b) {
                const int ib = i + b * TPF;                // 0..255
                cd r[R3];
#pragma unroll
                for (int t = 0; t < R3; ++t) {
                    const cd v = zf[WF_PHYS(ib + t * 256)];
                    r[t] = (t == 0) ? v : zmul(v, W(t * ib));
                }
                if constexpr (R3 == 2) zdft2(r[0], r[1]);
                if constexpr (R3 == 4) zdft4(r[0], r[1], r[2], r[3]);
                if constexpr (R3 == 8) zdft8(r);
#pragma unroll
                for (int u = 0; u < R3; ++u) a[b + NB3 * u] = r[u];     // X[ib + 256 u] = X[i + (b + NB3 u) TPF]
            }
        }
    }
}

