// sc_complex.h -- complex float64 arithmetic and the register-resident radix-2/4/8/16 butterflies of every fp64 device
// path: the Wilson kernels (sc_wilson*.hip, sc_mvar.hip), the group measures (sc_canonical.hip, sc_global.hip via
// sc_jacobi.h) and the float64 stage A (sc_mtfft_f64.hip).  One expression text per operation: a kernel's rounding is the
// same whichever file it lives in.
#pragma once
#include <hip/hip_runtime.h>

typedef double2 cd;

__device__ __forceinline__ cd zmul(cd a, cd b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cd zmul_conj(cd a, cd b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ cd zmul_cs(cd a, double c, double s) { return make_double2(a.x * c - a.y * s, a.x * s + a.y * c); }   // a (c + i s)
__device__ __forceinline__ cd zconj(cd a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ cd zadd(cd a, cd b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cd zsub(cd a, cd b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cd zdiv(cd a, cd b) {
    const double d = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
__device__ __forceinline__ cd zscale(cd a, double s) { return make_double2(a.x * s, a.y * s); }

__device__ __forceinline__ void zdft2(cd& a0, cd& a1) {
    const cd t = a0;
    a0 = make_double2(t.x + a1.x, t.y + a1.y);
    a1 = make_double2(t.x - a1.x, t.y - a1.y);
}
// forward 4-point DFT, natural order in and out
__device__ __forceinline__ void zdft4(cd& a0, cd& a1, cd& a2, cd& a3) {
    const cd b0 = make_double2(a0.x + a2.x, a0.y + a2.y), b1 = make_double2(a0.x - a2.x, a0.y - a2.y);
    const cd b2 = make_double2(a1.x + a3.x, a1.y + a3.y), b3 = make_double2(a1.y - a3.y, a3.x - a1.x);
    a0 = make_double2(b0.x + b2.x, b0.y + b2.y);
    a1 = make_double2(b1.x + b3.x, b1.y + b3.y);
    a2 = make_double2(b0.x - b2.x, b0.y - b2.y);
    a3 = make_double2(b1.x - b3.x, b1.y - b3.y);
}
// forward 8-point DFT, natural order in and out: even/odd 4-point DFTs, X[k] = E[k] + W8^k O[k]
__device__ __forceinline__ void zdft8(cd (&x)[8]) {
    constexpr double H = 0.70710678118654752440;
    cd e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6], o0 = x[1], o1 = x[3], o2 = x[5], o3 = x[7];
    zdft4(e0, e1, e2, e3);
    zdft4(o0, o1, o2, o3);
    o1 = zmul_cs(o1, H, -H);
    o2 = make_double2(o2.y, -o2.x);
    o3 = zmul_cs(o3, -H, -H);
    x[0] = make_double2(e0.x + o0.x, e0.y + o0.y); x[4] = make_double2(e0.x - o0.x, e0.y - o0.y);
    x[1] = make_double2(e1.x + o1.x, e1.y + o1.y); x[5] = make_double2(e1.x - o1.x, e1.y - o1.y);
    x[2] = make_double2(e2.x + o2.x, e2.y + o2.y); x[6] = make_double2(e2.x - o2.x, e2.y - o2.y);
    x[3] = make_double2(e3.x + o3.x, e3.y + o3.y); x[7] = make_double2(e3.x - o3.x, e3.y - o3.y);
}
// forward 16-point DFT: x[n], n = 4 n1 + n2 in; o[k], k = k1 + 4 k2 out (both natural order)
__device__ __forceinline__ void zdft16(cd (&x)[16], cd (&o)[16]) {
    constexpr double C1 = 0.92387953251128675613, S1 = 0.38268343236508977173, H = 0.70710678118654752440;
    // (the float64 stage A spelled cos / sin of pi / 8 with other trailing digits: the same doubles)
    static_assert(C1 == 0.92387953251128673848 && S1 == 0.38268343236508978178, "one double per constant");
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) zdft4(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);
    x[4 + 1] = zmul_cs(x[4 + 1], C1, -S1);  x[8 + 1] = zmul_cs(x[8 + 1], H, -H);    x[12 + 1] = zmul_cs(x[12 + 1], S1, -C1);
    x[4 + 2] = zmul_cs(x[4 + 2], H, -H);    x[8 + 2] = make_double2(x[8 + 2].y, -x[8 + 2].x);
    x[12 + 2] = zmul_cs(x[12 + 2], -H, -H);
    x[4 + 3] = zmul_cs(x[4 + 3], S1, -C1);  x[8 + 3] = zmul_cs(x[8 + 3], -H, -H);   x[12 + 3] = zmul_cs(x[12 + 3], -C1, S1);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
        cd a0 = x[4 * k1], a1 = x[4 * k1 + 1], a2 = x[4 * k1 + 2], a3 = x[4 * k1 + 3];
        zdft4(a0, a1, a2, a3);
        o[k1] = a0; o[k1 + 4] = a1; o[k1 + 8] = a2; o[k1 + 12] = a3;
    }
}
