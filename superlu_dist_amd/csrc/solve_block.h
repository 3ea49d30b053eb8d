// Block solve L U X = B for many right-hand sides on the device factors
// (1x1 plans): the level sweeps of solve.h with the panel products on MFMA,
// what pdgstrs does with GEMM / TRSM for nrhs > 1 (SRC/pdgstrs_lsum.c,
// dlsum_fmod / dlsum_bmod).  Included by engine.hip.
//
// X lives in a working buffer of n rows of SVB_NR contiguous values
// (row-major): a gathered or scattered row is one or two cache lines, and the
// atomics of a panel update run along the right-hand sides.  Every factor
// element is read once per sweep for SVB_NR columns; dead columns of a
// partial pass are zeros from k_svb_in on and stay zeros.
//
// Fragments are Mma<T>'s 16x16x4 with M = factor rows, N = right-hand sides,
// K = supernode columns.  The tables are those of solve.h (build_solve).
#pragma once
#include "solve.h"

namespace slu {

// right-hand sides per pass: 256 bytes per row of X in fp64 and complex
template <typename T> struct SvbNr { static constexpr int v = sizeof(T) == 16 ? 16 : 32; };

constexpr int SVB_TR_ROWS = 64;    // rows of X per workgroup of the transpositions
constexpr int SVB_LTHREADS = 512;  // k_svb_lpanel: 8 waves x 32 rows = a 256-row chunk of solve.h
constexpr int SVB_KS = 64;         // k_svb_lpanel: rows of Y_k staged in LDS at a time
constexpr int SVB_DTHREADS = 256;  // diagonal solves
constexpr int SVB_CH = 8;          // diagonal solves: rows of a panel column a lane updates per batch of LDS reads

// caller's column-major b (nr live columns, ld ldb) -> row-major X, zeros in
// the dead columns; through an LDS tile so that both sides are coalesced
template <typename T>
__global__ void __launch_bounds__(256) k_svb_in(const T *b, int64_t ldb, int n, int nr, T *xb) {
    using Sx = S<T>;
    constexpr int NRB = SvbNr<T>::v;
    __shared__ T s[SVB_TR_ROWS][NRB + 1];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SVB_TR_ROWS;
    for (int e = t; e < SVB_TR_ROWS * NRB; e += 256) {
        const int i = e % SVB_TR_ROWS, q = e / SVB_TR_ROWS;
        s[i][q] = (r0 + i < n && q < nr) ? b[r0 + i + q * ldb] : Sx::zero();
    }
    __syncthreads();
    for (int e = t; e < SVB_TR_ROWS * NRB; e += 256) {
        const int q = e % NRB, i = e / NRB;
        if (r0 + i < n) xb[(r0 + i) * NRB + q] = s[i][q];
    }
}

// row-major X -> the nr live columns of the caller's b; nothing else of b is written
template <typename T>
__global__ void __launch_bounds__(256) k_svb_out(const T *xb, int n, int nr, T *b, int64_t ldb) {
    using Sx = S<T>;
    constexpr int NRB = SvbNr<T>::v;
    __shared__ T s[SVB_TR_ROWS][NRB + 1];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SVB_TR_ROWS;
    for (int e = t; e < SVB_TR_ROWS * NRB; e += 256) {
        const int q = e % NRB, i = e / NRB;
        s[i][q] = r0 + i < n ? xb[(r0 + i) * NRB + q] : Sx::zero();
    }
    __syncthreads();
    for (int e = t; e < SVB_TR_ROWS * NRB; e += 256) {
        const int i = e % SVB_TR_ROWS, q = e / SVB_TR_ROWS;
        if (r0 + i < n && q < nr) b[r0 + i + q * ldb] = s[i][q];
    }
}

// L_kk Y = B_k (unit lower), blocked by SVP-column panels.  Per panel: the
// SVP x SVP triangle (column-major, zeros outside) and the panel's rows of X
// go to LDS, lane q < NRB of the first wave substitutes down column q of
// the panel in LDS (the triangle's entries are broadcasts; neighbouring
// lanes are neighbouring words of a row, and a lane touches its own column
// only), the solved panel goes back to X and stays in LDS as the B operand,
// and every 16-row fragment below the panel subtracts L(rows, panel) Y_panel
// on MFMA.  X is streamed: a fragment's rows are read and written in global
// memory (L2-resident, the workgroup owns them); the LDS window is one panel.
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_ldiag(const SvDiag *items, const T *Lval, T *xb) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int SVP = SvPanel<T>::v, NRB = SvbNr<T>::v, NF = NRB / 16, NW = SVB_DTHREADS / 64;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int w = it.w;
    const int64_t ld = it.ld;
    T *X = xb + (int64_t)it.fst * NRB;
    // (SVB_CH rows of padding: a batch may read past the panel's end; its
    // values are never used and never stored)
    __shared__ T s_t[SVP][SVP + SVB_CH]; // s_t[j][i] = L(j0 + i, j0 + j), i > j
    __shared__ T s_p[SVP + SVB_CH][NRB];
    for (int e = t; e < SVB_CH * NRB; e += SVB_DTHREADS) s_p[SVP + e / NRB][e % NRB] = Sx::zero();
    for (int e = t; e < SVP * SVB_CH; e += SVB_DTHREADS) s_t[e / SVB_CH][SVP + e % SVB_CH] = Sx::zero();
    for (int j0 = 0; j0 < w; j0 += SVP) {
        const int nj = min(SVP, w - j0);
        for (int e = t; e < SVP * SVP; e += SVB_DTHREADS) {
            const int i = e % SVP, j = e / SVP;
            s_t[j][i] = (i > j && i < nj) ? gld(L + (j0 + i) + (j0 + j) * ld) : Sx::zero();
        }
        for (int e = t; e < SVP * NRB; e += SVB_DTHREADS) {
            const int i = e / NRB, q = e % NRB;
            s_p[i][q] = i < nj ? X[(int64_t)(j0 + i) * NRB + q] : Sx::zero();
        }
        __syncthreads();
        if (t < NRB) {
            for (int j = 0; j + 1 < nj; ++j) {
                const T yj = s_p[j][t];
                for (int i = j + 1; i < nj; i += SVB_CH) { // SVB_CH LDS reads in flight, then the stores
                    T v[SVB_CH], l[SVB_CH];
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u) {
                        v[u] = s_p[i + u][t];
                        l[u] = s_t[j][i + u];
                    }
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u)
                        if (i + u < nj) s_p[i + u][t] = Sx::fms(v[u], l[u], yj);
                }
            }
        }
        __syncthreads();
        for (int e = t; e < nj * NRB; e += SVB_DTHREADS) X[(int64_t)j0 * NRB + e] = s_p[e / NRB][e % NRB];
        const int nfr = (w + 15) / 16;
        for (int mf = (j0 + SVP) / 16 + wv; mf < nfr; mf += NW) {
            const int i = mf * 16 + lr;
            typename M::acc_t acc[NF];
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) acc[nf] = M::zero();
#pragma unroll
            for (int k0 = 0; k0 < SVP; k0 += 4) {
                const int k = k0 + lk;
                const T a = (i < w && k < nj) ? gld(L + i + (j0 + k) * ld) : Sx::zero();
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) M::step(acc[nf], a, s_p[k][nf * 16 + lr]);
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int r = mf * 16 + M::row(lane, ii);
                if (r < w) {
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf) {
                        T *px = X + (int64_t)r * NRB + nf * 16 + lr;
                        *px = Sx::sub(*px, M::get(acc[nf], ii));
                    }
                }
            }
        }
        __syncthreads();
    }
}

// U_kk X = Y (upper, non-unit), k_svb_ldiag from the last panel up: back
// substitution in the panel (the diagonal divided as Sx::div does in
// k_sv_udiag, no reciprocal), then every fragment above the panel subtracts
// U(rows, panel) X_panel.  Panels start at multiples of SVP, so the rows
// above are whole fragments.
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_udiag(const SvDiag *items, const T *Lval, T *xb) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int SVP = SvPanel<T>::v, NRB = SvbNr<T>::v, NF = NRB / 16, NW = SVB_DTHREADS / 64;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int w = it.w;
    const int64_t ld = it.ld;
    T *X = xb + (int64_t)it.fst * NRB;
    __shared__ T s_t[SVP][SVP + SVB_CH]; // s_t[j][i] = U(j0 + i, j0 + j), i <= j; padded as in k_svb_ldiag
    __shared__ T s_p[SVP + SVB_CH][NRB];
    for (int e = t; e < SVB_CH * NRB; e += SVB_DTHREADS) s_p[SVP + e / NRB][e % NRB] = Sx::zero();
    for (int e = t; e < SVP * SVB_CH; e += SVB_DTHREADS) s_t[e / SVB_CH][SVP + e % SVB_CH] = Sx::zero();
    for (int j0 = ((w - 1) / SVP) * SVP; j0 >= 0; j0 -= SVP) {
        const int nj = min(SVP, w - j0);
        for (int e = t; e < SVP * SVP; e += SVB_DTHREADS) {
            const int i = e % SVP, j = e / SVP;
            s_t[j][i] = (i <= j && j < nj) ? gld(L + (j0 + i) + (j0 + j) * ld) : Sx::zero();
        }
        for (int e = t; e < SVP * NRB; e += SVB_DTHREADS) {
            const int i = e / NRB, q = e % NRB;
            s_p[i][q] = i < nj ? X[(int64_t)(j0 + i) * NRB + q] : Sx::zero();
        }
        __syncthreads();
        if (t < NRB) {
            for (int j = nj - 1; j >= 0; --j) {
                const T xj = Sx::div(s_p[j][t], s_t[j][j]);
                s_p[j][t] = xj;
                for (int i = 0; i < j; i += SVB_CH) {
                    T v[SVB_CH], u_[SVB_CH];
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u) {
                        v[u] = s_p[i + u][t];
                        u_[u] = s_t[j][i + u];
                    }
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u)
                        if (i + u < j) s_p[i + u][t] = Sx::fms(v[u], u_[u], xj);
                }
            }
        }
        __syncthreads();
        for (int e = t; e < nj * NRB; e += SVB_DTHREADS) X[(int64_t)j0 * NRB + e] = s_p[e / NRB][e % NRB];
        for (int mf = wv; mf < j0 / 16; mf += NW) {
            const int i = mf * 16 + lr; // < j0
            typename M::acc_t acc[NF];
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) acc[nf] = M::zero();
#pragma unroll
            for (int k0 = 0; k0 < SVP; k0 += 4) {
                const int k = k0 + lk;
                const T a = k < nj ? gld(L + i + (j0 + k) * ld) : Sx::zero();
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) M::step(acc[nf], a, s_p[k][nf * 16 + lr]);
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int r = mf * 16 + M::row(lane, ii);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    T *px = X + (int64_t)r * NRB + nf * 16 + lr;
                    *px = Sx::sub(*px, M::get(acc[nf], ii));
                }
            }
        }
        __syncthreads();
    }
}

// X[rows below] -= L_panel(256-row chunk of solve.h) * Y_k.  Each of the 8
// waves owns 32 panel rows (two fragments); Y_k is staged through LDS in
// strips of SVB_KS rows as the B operand, L streams from global memory as the
// A operand (column-major: a fragment's 16 rows are contiguous per column).
// K past w and rows past the panel's end are zeros that are never addressed.
// The scatter through `rows` is one atomic per element, 16 lanes along a row
// of X: 16 atomic instructions per wave.
template <typename T>
__global__ void __launch_bounds__(SVB_LTHREADS)
k_svb_lpanel(const SvChunk *chunks, const SvDiag *pan, const int64_t *roff, const int *rows,
             const T *Lval, T *xb) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int NRB = SvbNr<T>::v, NF = NRB / 16;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = pan[ch.sn];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int w = it.w, nb = it.pad;
    const int64_t ld = it.ld;
    const T *L = Lval + it.voff;
    const int rbase = ch.c0 + wv * 32;
    __shared__ T s_y[SVB_KS][NRB];
    typename M::acc_t acc[2][NF];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = M::zero();
    for (int ks = 0; ks < w; ks += SVB_KS) {
        if (ks) __syncthreads();
        for (int e = t; e < SVB_KS * NRB; e += SVB_LTHREADS) {
            const int k = e / NRB, q = e % NRB;
            s_y[k][q] = ks + k < w ? xb[(int64_t)(it.fst + ks + k) * NRB + q] : Sx::zero();
        }
        __syncthreads();
        const int kend = min(SVB_KS, w - ks);
        if (rbase < nb) {
            for (int k1 = 0; k1 < kend; k1 += 16) { // 8 loads in flight per lane
#pragma unroll
                for (int k0 = k1; k0 < k1 + 16; k0 += 4) {
                    const int k = ks + k0 + lk;
                    T a[2];
#pragma unroll
                    for (int mf = 0; mf < 2; ++mf) {
                        const int r = rbase + mf * 16 + lr;
                        a[mf] = (r < nb && k < w) ? gld(L + r + k * ld) : Sx::zero();
                    }
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf) {
                        const T b = s_y[k0 + lk][nf * 16 + lr];
#pragma unroll
                        for (int mf = 0; mf < 2; ++mf) M::step(acc[mf][nf], a[mf], b);
                    }
                }
            }
        }
    }
    const int *grow = rows + roff[ch.sn];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int r = rbase + mf * 16 + M::row(lane, ii);
            if (r < nb) {
                T *px = xb + (int64_t)grow[r] * NRB + lr;
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) Sx::atomic_sub(px + nf * 16, M::get(acc[mf][nf], ii));
            }
        }
}

// Y_k -= U(k, chunk of SVU_COLS columns) * X[gc]: the chunk's X rows are
// gathered into LDS as the B operand, A is the skyline segments (column c
// holds rows fst_c..w-1 contiguously; rows above fst_c are zeros that are not
// loaded, k_sv_upanel's guard).  A wave takes every fourth 16-row fragment of
// the supernode; atomics into Y_k's rows, 8 instructions per fragment.
template <typename T>
__global__ void __launch_bounds__(SV_THREADS)
k_svb_upanel(const SvChunk *chunks, const SvDiag *diag, const int64_t *coff, const int *ncol,
             const int64_t *ucol_voff, const int *ucol_fst, const int *ucol_gc, const T *Uval, T *xb) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int NRB = SvbNr<T>::v, NF = NRB / 16, NW = SV_THREADS / 64;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = diag[ch.sn];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int w = it.w;
    const int nc = min(SVU_COLS, ncol[ch.sn] - ch.c0);
    __shared__ int64_t s_v[SVU_COLS];
    __shared__ int s_f[SVU_COLS], s_gc[SVU_COLS];
    __shared__ T s_x[SVU_COLS][NRB];
    if (t < SVU_COLS) {
        const int64_t e = coff[ch.sn] + ch.c0 + t;
        s_v[t] = t < nc ? ucol_voff[e] : 0;
        s_f[t] = t < nc ? ucol_fst[e] - it.fst : w; // first row of the segment, relative
        s_gc[t] = t < nc ? ucol_gc[e] : -1;
    }
    __syncthreads();
    for (int e = t; e < SVU_COLS * NRB; e += SV_THREADS) {
        const int c = e / NRB, q = e % NRB;
        const int g = s_gc[c];
        s_x[c][q] = g >= 0 ? xb[(int64_t)g * NRB + q] : Sx::zero();
    }
    __syncthreads();
    const int nfr = (w + 15) / 16;
    T *Y = xb + (int64_t)it.fst * NRB;
    for (int mf = wv; mf < nfr; mf += NW) {
        const int i = mf * 16 + lr;
        typename M::acc_t acc[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[nf] = M::zero();
        for (int k1 = 0; k1 < nc; k1 += 16) { // 4 loads in flight per lane
#pragma unroll
            for (int k0 = k1; k0 < k1 + 16; k0 += 4) {
                const int c = k0 + lk;
                const int rf = s_f[c]; // w (no load) past the chunk's last column
                const T a = (i >= rf && i < w) ? gld(Uval + s_v[c] + i - rf) : Sx::zero();
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) M::step(acc[nf], a, s_x[c][nf * 16 + lr]);
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int r = mf * 16 + M::row(lane, ii);
            if (r < w) {
#pragma unroll
                for (int nf = 0; nf < NF; ++nf)
                    Sx::atomic_sub(Y + (int64_t)r * NRB + nf * 16 + lr, M::get(acc[nf], ii));
            }
        }
    }
}

} // namespace slu
