// Block iterative refinement for many right-hand sides (1x1 plans): the
// pdgsrfs loop of slu_plan_refine / slu_plan_refine_d2 on a pass of SVB_NR
// columns at once.  Per step: one residual kernel over all of the pass's
// columns, one block sweep (solve_block.h), one masked update.  Included by
// engine.hip.
//
// X, B and R live in working buffers of n rows of SVB_NR contiguous values
// (row-major, the layout of solve_block.h's X), in the plan's type (fp64 for
// the mixed-precision loop on an fp32 plan).  Dead columns of a partial pass
// are zeros from k_svb_in on: their residual and berr are zeros.
//
// Every column keeps its own stopping rule on the host.  A stopped column is
// frozen: the update skips it, and its column of R is zeroed before the
// sweep, so that a NaN or Inf it holds never enters an MFMA product.  The
// right-hand sides sit on the N index of solve_block.h's fragments, so the
// columns of a block never mix in the sweep.
#pragma once
#include "refine_d2.h"
#include "solve_block_t.h"

namespace slu {

constexpr int RFB_THREADS = 256;

// per-column power-of-two exponents of the mixed-precision step, by value
struct RfbExp {
    int e[32];
};

// The per-column maxima of a residual kernel's workgroup: s = this lane's berr
// term of column q = lane % NRB (a NaN wins), rm = its |r_i| (D2; a NaN
// dropped).  Shuffles between lanes of equal q, the waves through LDS, one
// atomicMax per column on the bit patterns of non-negative doubles:
// out[q] = berr of column q and, with D2, out[NRB + q] = max |r_i|.
template <int NRB, bool D2>
__device__ __forceinline__ void rfb_colmax(double s, double rm, unsigned long long *out) {
    constexpr int NW = RFB_THREADS / 64;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    // the rows of the wave: lanes of equal q are NRB apart
#pragma unroll
    for (int off = 32; off >= NRB; off >>= 1) {
        const double o = __shfl_xor(s, off, 64);
        s = (s != s || o != o) ? __builtin_nan("") : fmax(s, o);
        if constexpr (D2) rm = fmax(rm, __shfl_xor(rm, off, 64));
    }
    __shared__ double s_be[NW][NRB], s_rm[D2 ? NW : 1][NRB];
    if (lane < NRB) {
        s_be[wv][lane] = s;
        if constexpr (D2) s_rm[wv][lane] = rm;
    }
    __syncthreads();
    if (t < NRB) {
        s = s_be[0][t];
        if constexpr (D2) rm = s_rm[0][t];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const double o = s_be[w][t];
            s = (s != s || o != o) ? __builtin_nan("") : fmax(s, o);
            if constexpr (D2) rm = fmax(rm, s_rm[w][t]);
        }
        if (!(s <= 0.0)) atomicMax(out + t, (unsigned long long)__double_as_longlong(s));
        if constexpr (D2)
            if (rm > 0.0) atomicMax(out + NRB + t, (unsigned long long)__double_as_longlong(rm));
    }
}

// k_resid / k_resid_d2 for SVB_NR columns: NRB consecutive lanes own one row
// of A, lane q is column q.  A gathered row of X is one contiguous read of
// NRB values and a[re[e]] one address per lane group.  A lane visits its
// row's entries in k_resid's order with k_resid's expressions, so for an
// identical x the residual and berr are those of the per-column kernel, bit
// for bit.  The per-column maxima leave through rfb_colmax.
// D2: X, B, R and A in fp64 with k_resid_d2's fma forms (T = double).
template <typename T, bool D2>
__global__ void __launch_bounds__(RFB_THREADS)
k_rfb_resid(const int64_t *rp, const int *rc, const int64_t *re, const T *a, const T *xb, const T *bb,
            T *rb, int n, double safe1, double safe2, unsigned long long *out) {
    using Sx = S<T>;
    constexpr int NRB = SvbNr<T>::v, ROWS = RFB_THREADS / NRB;
    const int t = threadIdx.x, q = t % NRB;
    const int64_t i = (int64_t)blockIdx.x * ROWS + t / NRB;
    double s = 0.0, rm = 0.0;
    if (i < n) {
        const T bv = bb[i * NRB + q];
        T acc = bv;
        double tmp = Sx::abs1(bv);
        for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
            const T av = a[re[e]], xv = xb[(int64_t)rc[e] * NRB + q];
            if constexpr (D2) {
                acc = fma(-av, xv, acc);
                tmp = fma(fabs(av), fabs(xv), tmp);
            } else {
                acc = Sx::fms(acc, av, xv);
                tmp += Sx::abs1(av) * Sx::abs1(xv);
            }
        }
        rb[i * NRB + q] = acc;
        const double ra = Sx::abs1(acc);
        if constexpr (D2) {
            rm = ra;
            s = d2_berr_row(ra, tmp, safe1, safe2);
        } else {
            if (tmp > safe2) s = ra / tmp;
            else if (tmp != 0.0) s = (safe1 + ra) / tmp;
        }
    }
    rfb_colmax<NRB, D2>(s, rm, out);
}

// k_resid_t for SVB_NR columns, the residual of the transposed loop: NRB
// consecutive lanes own one column j of B over the CSC view of build_csc,
// lane q is right-hand side q.  A lane visits the column's entries in
// ascending order with k_resid_t's expressions, so for an identical x the
// residual and berr are those of the per-column kernel, bit for bit.
template <typename T>
__global__ void __launch_bounds__(RFB_THREADS)
k_rfb_resid_t(const unsigned long long *lo, const unsigned long long *hi, const int *ci, const T *a,
              const T *xb, const T *bb, T *rb, int n, double safe1, double safe2, unsigned long long *out,
              int conj) {
    using Sx = S<T>;
    constexpr int NRB = SvbNr<T>::v, ROWS = RFB_THREADS / NRB;
    const int t = threadIdx.x, q = t % NRB;
    const int64_t j = (int64_t)blockIdx.x * ROWS + t / NRB;
    double s = 0.0;
    if (j < n) {
        const T bv = bb[j * NRB + q];
        T acc = bv;
        double tmp = Sx::abs1(bv);
        for (unsigned long long e = lo[j]; e < hi[j]; ++e) {
            const T av = sv_cj(a[e], conj), xv = xb[(int64_t)ci[e] * NRB + q];
            acc = Sx::fms(acc, av, xv);
            tmp += Sx::abs1(av) * Sx::abs1(xv);
        }
        rb[j * NRB + q] = acc;
        const double ra = Sx::abs1(acc);
        if (tmp > safe2) s = ra / tmp;
        else if (tmp != 0.0) s = (safe1 + ra) / tmp;
    }
    rfb_colmax<NRB, false>(s, 0.0, out);
}

// zeros in the columns of R outside `keep` (bit q = column q)
template <typename T>
__global__ void __launch_bounds__(RFB_THREADS) k_rfb_mask(T *rb, int64_t total, unsigned keep) {
    constexpr int NRB = SvbNr<T>::v;
    const int64_t e = (int64_t)blockIdx.x * RFB_THREADS + threadIdx.x;
    if (e < total && !((keep >> (e % NRB)) & 1u)) rb[e] = S<T>::zero();
}

// k_axpy1 on the columns of `act`: x[:, q] += dx[:, q]
template <typename T>
__global__ void __launch_bounds__(RFB_THREADS) k_rfb_axpy(T *xb, const T *dx, int64_t total, unsigned act) {
    constexpr int NRB = SvbNr<T>::v;
    const int64_t e = (int64_t)blockIdx.x * RFB_THREADS + threadIdx.x;
    if (e < total && ((act >> (e % NRB)) & 1u)) xb[e] = S<T>::sub(xb[e], S<T>::neg(dx[e]));
}

// k_scale_cvt_d2 with one exponent per column: r32 = (float)(r 2^-e[q]) in
// the columns of `act`, zeros in the others
__global__ void __launch_bounds__(RFB_THREADS)
k_rfb_scale_cvt_d2(const double *rb, float *r32, int64_t total, RfbExp ex, unsigned act) {
    constexpr int NRB = SvbNr<float>::v;
    const int64_t e = (int64_t)blockIdx.x * RFB_THREADS + threadIdx.x;
    if (e >= total) return;
    const int q = (int)(e % NRB);
    r32[e] = ((act >> q) & 1u) ? (float)ldexp(rb[e], -ex.e[q]) : 0.0f;
}

// k_axpy_d2 with one exponent per column, on the columns of `act`:
// x[:, q] += 2^e[q] dx32[:, q] in fp64
__global__ void __launch_bounds__(RFB_THREADS)
k_rfb_axpy_d2(double *xb, const float *dx32, int64_t total, RfbExp ex, unsigned act) {
    constexpr int NRB = SvbNr<float>::v;
    const int64_t e = (int64_t)blockIdx.x * RFB_THREADS + threadIdx.x;
    if (e >= total) return;
    const int q = (int)(e % NRB);
    if ((act >> q) & 1u) xb[e] += ldexp((double)dx32[e], ex.e[q]);
}

} // namespace slu
