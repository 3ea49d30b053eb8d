// Mixed-precision refinement: fp32 factors, fp64 residual and update
// (the scheme of the reference's psgsrfs_d2, SRC/psgsrfs_d2.c:400-555).
//
// An fp32 plan keeps the caller's fp64 values of A on the device
// (slu_plan_fill_a_d2 rounds them into L / U in the same pass).  Each step
// forms r = b - A x, s = |A||x| + |b|, berr = max |r_i| / s_i and
// rmax = max |r_i| in fp64, scales r by the power of two 2^-e that brings
// rmax into [0.5, 1), rounds it to fp32, sweeps with the fp32 factors and
// adds the correction back in fp64: x += 2^e dx.  The scaling is exact, so
// it changes nothing while r and dx are inside fp32's range and keeps the
// loop working where they are not (right-hand sides near 1e-45 or 1e38).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fill.h"
#include "solve.h"

namespace slu {

// k_fill_a for an fp32 storage fed from fp64 values: L / U get (float)a[e],
// round to nearest even; amap as in fill.h.
__global__ void __launch_bounds__(FILL_THREADS)
k_fill_a_d2(const int64_t *__restrict__ amap, const double *__restrict__ a, int64_t nnz,
            float *__restrict__ L, float *__restrict__ U) {
    const int64_t stride = (int64_t)gridDim.x * FILL_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x; e < nnz; e += stride) {
        const int64_t m = amap[e];
        if (m < 0) continue;
        const float v = (float)a[e];
        if (m & 1) U[m >> 1] = v;
        else L[m >> 1] = v;
    }
}

// The two maxima of a residual pass over the wave, then into out[0] (berr:
// a NaN wins, as in k_resid) and out[1] (rmax: fmax drops a NaN) as bit
// patterns of non-negative doubles.
__device__ __forceinline__ void d2_wave_max(double be, double rm, unsigned long long *out) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(be, off, 64);
        be = (be != be || o != o) ? __builtin_nan("") : fmax(be, o);
        rm = fmax(rm, __shfl_xor(rm, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (!(be <= 0.0)) atomicMax(out, (unsigned long long)__double_as_longlong(be));
        if (rm > 0.0) atomicMax(out + 1, (unsigned long long)__double_as_longlong(rm));
    }
}

__device__ __forceinline__ double d2_berr_row(double ra, double s, double safe1, double safe2) {
    if (s > safe2) return ra / s;
    if (s != 0.0) return (safe1 + ra) / s;
    return 0.0;
}

// k_resid in fp64 on the fp64 values of A, one row per thread; out[0] = berr,
// out[1] = max |r_i|.
__global__ void __launch_bounds__(256)
k_resid_d2(const int64_t *rp, const int *rc, const int64_t *re, const double *a, const double *x,
           const double *b, double *r, int n, double safe1, double safe2, unsigned long long *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double be = 0.0, rm = 0.0;
    if (i < n) {
        double acc = b[i], tmp = fabs(b[i]);
        for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
            const double av = a[re[e]], xv = x[rc[e]];
            acc = fma(-av, xv, acc);
            tmp = fma(fabs(av), fabs(xv), tmp);
        }
        r[i] = acc;
        rm = fabs(acc);
        be = d2_berr_row(rm, tmp, safe1, safe2);
    }
    d2_wave_max(be, rm, out);
}

// 2D grids: k_resid_part / k_resid_fin with fp64 partial rows and slots.
__global__ void __launch_bounds__(256)
k_resid_part_d2(const int64_t *rp, const int *rc, const int64_t *re, const double *a,
                const double *x, double *r, double *s, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0, tmp = 0.0;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        const double av = a[re[e]], xv = x[rc[e]];
        acc = fma(-av, xv, acc);
        tmp = fma(fabs(av), fabs(xv), tmp);
    }
    r[i] = acc;
    s[i] = tmp;
}

__global__ void __launch_bounds__(256)
k_resid_fin_d2(const RfRow *items, const double *b, double *r, const double *s,
               const double *slot_r, const double *slot_s, double safe1, double safe2,
               unsigned long long *out) {
    const RfRow it = items[blockIdx.x];
    double be = 0.0, rm = 0.0;
    for (int i = threadIdx.x; i < it.len; i += 256) {
        const int64_t row = it.fst + i;
        double rv = r[row] + b[row];
        double sv = s[row] + fabs(b[row]);
        for (int q = 0; q < it.nslot; ++q) {
            rv += slot_r[it.src + (int64_t)q * it.len + i];
            sv += slot_s[it.src + (int64_t)q * it.len + i];
        }
        r[row] = rv;
        const double ra = fabs(rv);
        const double e = d2_berr_row(ra, sv, safe1, safe2);
        be = (be != be || e != e) ? __builtin_nan("") : fmax(be, e);
        rm = fmax(rm, ra);
    }
    d2_wave_max(be, rm, out);
}

// r32 = (float)(r 2^-e): the right-hand side of the fp32 sweep.
__global__ void __launch_bounds__(256) k_scale_cvt_d2(const double *r, float *r32, int n, int e) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) r32[i] = (float)ldexp(r[i], -e);
}

// x += 2^e dx32 in fp64.
__global__ void __launch_bounds__(256) k_axpy_d2(double *x, const float *dx32, int n, int e) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] += ldexp((double)dx32[i], e);
}

} // namespace slu
