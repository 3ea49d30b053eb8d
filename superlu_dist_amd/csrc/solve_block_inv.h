// DiagInv for the block sweep (the reference's options->DiagInv,
// pdCompute_Diag_Inv in SRC/pdgstrs.c): every supernode's diagonal block is
// inverted once per factorization, and solve_block.h's diagonal solves
// become one w x w x SvbNr product per supernode on MFMA -- no substitution
// chain and no barrier per panel.  Included by engine.hip.
//
// The inverses sit in one buffer, one w x w column-major block (ld = w) per
// SvDiag item of build_solve's level order, at the offsets of an int64 table
// beside d_sv_lvl.  Like the block itself, an inverse block holds both
// triangles: L_kk^-1 strictly below the diagonal (its unit diagonal implied)
// and U_kk^-1 on and above it.
//
// Only the block sweep of solve_block.h dispatches to these kernels; the
// transposed block sweep (solve_block_t.h) keeps substituting with the mode on.
#pragma once
#include "solve_block.h"

namespace slu {

constexpr int SVB_ITHREADS = 512; // the inversion and the two products: 8 waves, one 16-row fragment each per round

// X[lo:hi, 0:ncol] <- (NEG ? -1 : 1) * Tri[lo:hi, lo:hi] * X[lo:hi, 0:ncol] in
// place, by one workgroup.  Tri is a triangle of the inverse block Mi (w x w,
// ld = w): UP ? the upper triangle with its diagonal : the strict lower
// triangle with a unit diagonal.  X(k, q) is X[k * sxk + q * sxq], k the row
// in the block; lo is a multiple of 16.  Fragments are Mma<T>'s with M = rows
// of Tri, N = the columns of X (SvbNr<T> = SvPanel<T> of them at most), K =
// columns of Tri; A streams from global memory (column-major: a fragment's 16
// rows are contiguous per column), B is read from X in L2.  A fragment's K
// range is the part of its rows where Tri is not structurally zero.
//
// In place: row fragment f of the lower product reads rows <= f of X, of the
// upper product rows >= f.  Fragments go in rounds of one per wave, from the
// last fragment up (lower) or from the first down (upper), with a barrier
// between a round's last read and its first write: the rows a round writes
// are rows no later round reads.  Nothing outside Mi's triangle and X's
// [lo, hi) x [0, ncol) is loaded.  No LDS.
template <typename T, bool UP, bool NEG>
__device__ __forceinline__ void svb_tri_mul(const T *Mi, int w, int lo, int hi, T *X, int64_t sxk, int64_t sxq,
                                            int ncol) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int NF = SvbNr<T>::v / 16, NW = SVB_ITHREADS / 64;
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int nfr = (hi - lo + 15) / 16;
    for (int g0 = 0; g0 < nfr; g0 += NW) { // uniform: every wave meets the round's barrier
        const int g = UP ? g0 + wv : nfr - 1 - g0 - wv;
        const bool live = g >= 0 && g < nfr;
        const int f0 = lo + g * 16, i = f0 + lr;
        typename M::acc_t acc[NF];
        svb_acc_zero<T>(acc);
        if (live) {
            const int kb = UP ? f0 : lo, ke = UP ? hi : min(hi, f0 + 16);
            for (int k1 = kb; k1 < ke; k1 += 16) { // 4 + 4 NF loads in flight per lane
#pragma unroll
                for (int k0 = k1; k0 < k1 + 16; k0 += 4) {
                    const int k = k0 + lk;
                    const bool in = (UP ? k >= i : k < i) && k < ke && i < hi;
                    T a = in ? gld(Mi + i + (int64_t)k * w) : Sx::zero();
                    if (!UP && k == i && i < hi) a = one_of(a);
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf) {
                        const int q = nf * 16 + lr;
                        const T b = (k < ke && q < ncol) ? gld(X + k * sxk + q * sxq) : Sx::zero();
                        M::step(acc[nf], a, b);
                    }
                }
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int r = f0 + M::row(lane, ii);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const int q = nf * 16 + lr;
                    const T v = M::get(acc[nf], ii);
                    if (r < hi && q < ncol) X[r * sxk + q * sxq] = NEG ? Sx::neg(v) : v;
                }
            }
        }
    }
}

// X_k <- L_kk^-1 X_k (UP = false) or U_kk^-1 X_k (UP = true) on the row-major
// X of solve_block.h: one workgroup per supernode of the level, in the place
// of k_svb_ldiag / k_svb_udiag (Lval is sv_diag's argument and is not read).
template <typename T, bool UP>
__global__ void __launch_bounds__(SVB_ITHREADS)
k_svb_minv(const SvDiag *items, const T *, const int64_t *ioff, const T *inv, T *xb) {
    constexpr int NRB = SvbNr<T>::v;
    const SvDiag it = items[blockIdx.x];
    svb_tri_mul<T, UP, false>(inv + ioff[blockIdx.x], it.w, 0, it.w, xb + (int64_t)it.fst * NRB, NRB, 1, NRB);
}

// The block column j0 .. j0 + nj of a triangle's inverse outside its diagonal
// panel, rows [lo, hi): M[R, J] = -M[R, R] (B[R, J] M_JJ), B the block at Lb
// (ld), M the inverse block Mo (ld = w) whose M_JJ and M[R, R] are finished.
// The inner product goes to M[R, J] (MFMA, A = B's rows from global memory,
// B = M_JJ from L2), then M[R, R] multiplies it in place (svb_tri_mul).
template <typename T, bool UP>
__device__ __forceinline__ void svb_inv_column(const T *Lb, int64_t ld, T *Mo, int w, int j0, int nj, int lo,
                                               int hi) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int SVP = SvPanel<T>::v, NF = SVP / 16, NW = SVB_ITHREADS / 64;
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int nfr = (hi - lo + 15) / 16;
    for (int g = wv; g < nfr; g += NW) {
        const int f0 = lo + g * 16, i = f0 + lr;
        typename M::acc_t acc[NF];
        svb_acc_zero<T>(acc);
#pragma unroll
        for (int k0 = 0; k0 < SVP; k0 += 4) {
            const int k = k0 + lk;
            const T a = (i < hi && k < nj) ? gld(Lb + i + (j0 + k) * ld) : Sx::zero();
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int q = nf * 16 + lr;
                const bool in = (UP ? k <= q : k > q) && k < nj && q < nj;
                T b = in ? gld(Mo + (j0 + k) + (int64_t)(j0 + q) * w) : Sx::zero();
                if (!UP && k == q && q < nj) b = one_of(b);
                M::step(acc[nf], a, b);
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int r = f0 + M::row(lane, ii);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int q = nf * 16 + lr;
                if (r < hi && q < nj) Mo[r + (int64_t)(j0 + q) * w] = M::get(acc[nf], ii);
            }
        }
    }
    __syncthreads();
    svb_tri_mul<T, UP, true>(Mo, w, lo, hi, Mo + (int64_t)j0 * w, 1, w, nj);
    __syncthreads();
}

// Both triangles of every diagonal block inverted, out of place from Lval
// into inv: one workgroup per supernode (no level dependency), blocked by
// SVP-column panels.
// (1) Each panel's own SVP x SVP triangles, by substitution on the identity:
//     the square goes to LDS, and lane q of one wave per triangle solves
//     column q in registers (the triangle's entries are LDS broadcasts, the
//     loops are unrolled over the whole panel and masked by q).  L_jj^-1
//     needs columns j >= q only and U_jj^-1 rows j <= q only, so a zero pivot
//     reaches exactly the entries that depend on it; U's diagonal is divided
//     (Sx::div), not multiplied by a reciprocal.  Rows and columns past a
//     partial last panel are never stored.
// (2) The rest of each block column by svb_inv_column, panels descending for
//     L (rows below) and ascending for U (rows above).  The finished part of
//     the inverse is read back from global memory behind a workgroup barrier,
//     as k_svb_ldiag reads X.
template <typename T>
__global__ void __launch_bounds__(SVB_ITHREADS)
k_svb_inv(const SvDiag *items, const T *Lval, const int64_t *ioff, T *inv) {
    using Sx = S<T>;
    constexpr int SVP = SvPanel<T>::v, NS = SVB_ITHREADS / 128; // panels in flight: two waves each
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    T *Mo = inv + ioff[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int w = it.w;
    const int64_t ld = it.ld;
    __shared__ T s_t[NS][SVP][SVP + 1]; // s_t[s][j][i] = block(j0 + i, j0 + j) of panel s, zeros past the block
    for (int p0 = 0; p0 < w; p0 += NS * SVP) {
        for (int e = t; e < NS * SVP * SVP; e += SVB_ITHREADS) {
            const int i = e % SVP, j = e / SVP % SVP, s = e / (SVP * SVP);
            const int j0 = p0 + s * SVP;
            s_t[s][j][i] = (j0 + i < w && j0 + j < w) ? gld(L + (j0 + i) + (j0 + j) * ld) : Sx::zero();
        }
        __syncthreads();
        const int s = wv >> 1, q = lane, j0 = p0 + s * SVP;
        if (q < SVP && j0 + q < w) {
            T y[SVP];
#pragma unroll
            for (int i = 0; i < SVP; ++i) y[i] = Sx::zero();
            if (wv & 1) { // column q of U_jj^-1: rows q .. 0
#pragma unroll
                for (int j = SVP - 1; j >= 0; --j) {
                    if (j == q) y[j] = one_of(y[j]);
                    const T yj = j <= q ? Sx::div(y[j], s_t[s][j][j]) : Sx::zero();
                    y[j] = yj;
#pragma unroll
                    for (int i = 0; i < j; ++i) y[i] = j <= q ? Sx::fms(y[i], s_t[s][j][i], yj) : y[i];
                }
#pragma unroll
                for (int i = 0; i < SVP; ++i)
                    if (i <= q) Mo[(j0 + i) + (int64_t)(j0 + q) * w] = y[i];
            } else { // column q of L_jj^-1 below its unit diagonal: rows q + 1 .. SVP - 1
#pragma unroll
                for (int j = 0; j < SVP - 1; ++j) {
                    const T yj = j == q ? one_of(y[j]) : y[j];
#pragma unroll
                    for (int i = j + 1; i < SVP; ++i) y[i] = j >= q ? Sx::fms(y[i], s_t[s][j][i], yj) : y[i];
                }
#pragma unroll
                for (int i = 1; i < SVP; ++i)
                    if (i > q && j0 + i < w) Mo[(j0 + i) + (int64_t)(j0 + q) * w] = y[i];
            }
        }
        __syncthreads();
    }
    for (int j0 = ((w - 1) / SVP - 1) * SVP; j0 >= 0; j0 -= SVP)
        svb_inv_column<T, false>(L, ld, Mo, w, j0, SVP, j0 + SVP, w);
    for (int j0 = SVP; j0 < w; j0 += SVP) svb_inv_column<T, true>(L, ld, Mo, w, j0, min(SVP, w - j0), 0, j0);
}

} // namespace slu
