// Block solve with the transpose: U^T L^T X = C (or the conjugate transpose,
// conj != 0, complex plans) for SVB_NR right-hand sides per pass, on the
// factors, tables, levels and row-major X of solve_block.h.  The roles of L
// and U swap as in solve.h's transposed sweeps: U's row segments are pushed
// forward (k_svb_utpanel), L's panels are pulled backward (k_svb_ltpanel), and
// both diagonal solves are svb_diag on the transposed triangle.  Included by
// engine.hip.
//
// Fragments are Mma<T>'s 16x16x4 with N = right-hand sides.  In every product
// here the MFMA K index runs along the contiguous stored dimension of the
// factor, a lane owning a run of SvbRun consecutive K (svb_krun and
// svb_krun_step in solve_block.h).  A factor element is conjugated as it is
// loaded; X never is.  Dead columns of a partial pass are zeros throughout.
#pragma once
#include "solve_block.h"

namespace slu {

// U_kk^T Z = C_k: the transposed upper triangle with its diagonal, forward.
// This is svb_diag<T, false, true> written out: instantiated from the shared
// body the fp64 kernel compiled to a different block layout of the
// substitution loop and measured 8 % slower (216.8 against 200.8 ms over the
// 1000 launches of ten sweeps at lap3d 100^3), with no source difference to
// pin it on, so this one kernel keeps its own text.  The fragment helpers
// alone (svb_lane, svb_acc_zero, svb_krun_step, svb_row_sub in this text)
// change its fp64 code as well, 455 to 500 instructions, so it uses none of
// them; its complex arithmetic is S<zc>::fms as the compiler contracts it here
// (see svb_fms).  Row t of U_kk^T is
// column t of the block: the panel's triangle is read along the columns of
// the block under the triangle's mask, the rows below a panel exist only
// under full panels, and their fragments subtract U(panel, rows)^T Z_panel
// with K along the column of the block.
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_utdiag(const SvDiag *items, const T *Lval, T *xb, int conj) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int SVP = SvPanel<T>::v, NRB = SvbNr<T>::v, NF = NRB / 16, NW = SVB_DTHREADS / 64;
    constexpr int R = SvbRun<T>::v, KB = 4 * R;
    static_assert(SVP % KB == 0, "a panel is whole K blocks");
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int w = it.w;
    const int64_t ld = it.ld;
    T *X = xb + (int64_t)it.fst * NRB;
    __shared__ T s_t[SVP][SVP + SVB_CH]; // s_t[j][i] = op(U(j0 + j, j0 + i)), i >= j; padded as in k_svb_ldiag
    __shared__ T s_p[SVP + SVB_CH][NRB];
    for (int e = t; e < SVB_CH * NRB; e += SVB_DTHREADS) s_p[SVP + e / NRB][e % NRB] = Sx::zero();
    for (int e = t; e < SVP * SVB_CH; e += SVB_DTHREADS) s_t[e / SVB_CH][SVP + e % SVB_CH] = Sx::zero();
    for (int j0 = 0; j0 < w; j0 += SVP) {
        const int nj = min(SVP, w - j0);
        for (int e = t; e < SVP * SVP; e += SVB_DTHREADS) {
            const int j = e % SVP, i = e / SVP; // j runs down column j0 + i of the block
            s_t[j][i] = (j <= i && i < nj) ? sv_cj(gld(L + (j0 + j) + (j0 + i) * ld), conj) : Sx::zero();
        }
        for (int e = t; e < SVP * NRB; e += SVB_DTHREADS) {
            const int i = e / NRB, q = e % NRB;
            s_p[i][q] = i < nj ? X[(int64_t)(j0 + i) * NRB + q] : Sx::zero();
        }
        __syncthreads();
        if (t < NRB) {
            for (int j = 0; j < nj; ++j) {
                const T zj = Sx::div(s_p[j][t], s_t[j][j]);
                s_p[j][t] = zj;
                for (int i = j + 1; i < nj; i += SVB_CH) {
                    T v[SVB_CH], u_[SVB_CH];
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u) {
                        v[u] = s_p[i + u][t];
                        u_[u] = s_t[j][i + u];
                    }
#pragma unroll
                    for (int u = 0; u < SVB_CH; ++u)
                        if (i + u < nj) s_p[i + u][t] = Sx::fms(v[u], u_[u], zj);
                }
            }
        }
        __syncthreads();
        for (int e = t; e < nj * NRB; e += SVB_DTHREADS) X[(int64_t)j0 * NRB + e] = s_p[e / NRB][e % NRB];
        const int nfr = (w + 15) / 16;
        for (int mf = (j0 + SVP) / 16 + wv; mf < nfr; mf += NW) { // nj == SVP here
            const int i = mf * 16 + lr;
            typename M::acc_t acc[NF];
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) acc[nf] = M::zero();
            T a[SVP / KB][R];
#pragma unroll
            for (int b = 0; b < SVP / KB; ++b) // rows j0 .. j0 + SVP - 1 of column i lie above its diagonal
                svb_krun<T, R>(L + i * ld + j0 + b * KB + lk * R, i < w ? 0 : R, R, conj, a[b]);
#pragma unroll
            for (int b = 0; b < SVP / KB; ++b)
#pragma unroll
                for (int jj = 0; jj < R; ++jj)
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf)
                        M::step(acc[nf], a[b][jj], s_p[b * KB + lk * R + jj][nf * 16 + lr]);
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

// L_kk^T Y = Z: the transposed unit lower triangle, backward
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_ltdiag(const SvDiag *items, const T *Lval, T *xb, int conj) {
    svb_diag<T, true, true>(items, Lval, xb, conj);
}

// Forward push of U^T: X[gc_c, :] -= sum_i U(i, c) Z_k[i, :] for a chunk of
// SVU_COLS U columns of block row k (k_svb_upanel's chunks).  M = the chunk's
// columns, one 16-column fragment per wave; K = the supernode's rows, Z_k
// staged through LDS in strips of SVB_KS rows as the B operand.  Column c's
// segment holds rows fst_c .. w - 1 contiguously: a lane's K run is cut at
// fst_c (rows above are not stored) and at w.  A lane's output row is a row
// gc of X: 16 lanes along it, four rows per atomic instruction, 4 NF
// instructions per wave.
template <typename T>
__global__ void __launch_bounds__(SV_THREADS)
k_svb_utpanel(const SvChunk *chunks, const SvDiag *diag, const int64_t *coff, const int *ncol,
              const int64_t *ucol_voff, const int *ucol_fst, const int *ucol_gc, const T *Uval, T *xb,
              int conj) {
    using M = Mma<T>;
    constexpr int NRB = SvbNr<T>::v, NF = NRB / 16, R = SvbRun<T>::v, KB = 4 * R;
    static_assert(SVU_COLS == 16 * (SV_THREADS / 64) && SVB_KS % KB == 0, "one fragment per wave, whole K blocks");
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = diag[ch.sn];
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int w = it.w;
    const int nc = min(SVU_COLS, ncol[ch.sn] - ch.c0);
    __shared__ int s_gc[SVU_COLS];
    __shared__ T s_z[SVB_KS][NRB];
    if (t < SVU_COLS) s_gc[t] = t < nc ? ucol_gc[coff[ch.sn] + ch.c0 + t] : -1;
    const int c = wv * 16 + lr; // this lane's column of the chunk
    const int64_t e = coff[ch.sn] + ch.c0 + c;
    const int rf = c < nc ? ucol_fst[e] - it.fst : w; // first row of the segment, relative; w: nothing to load
    const T *seg = Uval + (c < nc ? ucol_voff[e] : 0);
    typename M::acc_t acc[NF];
    svb_acc_zero<T>(acc);
    for (int ks = 0; ks < w; ks += SVB_KS) {
        if (ks) __syncthreads();
        svb_stage_rows<T, SVB_KS, SV_THREADS, false>(s_z, xb + (int64_t)(it.fst + ks) * NRB, w - ks, t);
        __syncthreads();
        if (wv * 16 < nc) {
            const int kend = min(SVB_KS, w - ks);
            for (int kb = 0; kb < kend; kb += KB) {
                const int i0 = ks + kb + lk * R;
                T a[R];
                svb_krun<T, R>(seg + (i0 - rf), rf - i0, w - i0, conj, a);
                svb_krun_step<T>(acc, a, s_z, kb + lk * R, lr);
            }
        }
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
        const int g = s_gc[wv * 16 + M::row(lane, ii)];
        if (g >= 0) svb_row_sub<T, true>(xb + (int64_t)g * NRB + lr, acc, ii);
    }
}

// Backward pull of L^T: Y_k[j, :] -= sum_r L(r, j) X[rows[r], :] over a chunk
// of SV_THREADS rows below the diagonal block (k_svb_lpanel's chunks and
// panel descriptors).  M = the supernode's columns, K = the chunk's rows: a
// column of the panel is contiguous along K, a lane's run is cut at the
// panel's last row.  The gathered rows of X go through LDS in strips of
// SVB_KS as the B operand.  Each of the 8 waves owns two 16-column fragments;
// a supernode wider than 256 takes a second round over the strips.  Per
// round a wave's sums leave as atomics into Y_k's rows, 16 lanes along a row,
// 8 NF instructions: once per chunk.
template <typename T>
__global__ void __launch_bounds__(SVB_LTHREADS)
k_svb_ltpanel(const SvChunk *chunks, const SvDiag *pan, const int64_t *roff, const int *rows,
              const T *Lval, T *xb, int conj) {
    using M = Mma<T>;
    constexpr int NRB = SvbNr<T>::v, NF = NRB / 16, R = SvbRun<T>::v, KB = 4 * R, NW = SVB_LTHREADS / 64;
    static_assert(SVB_KS % KB == 0, "whole K blocks");
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = pan[ch.sn];
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int w = it.w;
    const int nr = min(SV_THREADS, it.pad - ch.c0); // rows of this chunk
    const int64_t ld = it.ld;
    const T *L = Lval + it.voff + ch.c0; // L[r + j * ld] = L(chunk row r, column j)
    const int *grow = rows + roff[ch.sn] + ch.c0;
    T *Y = xb + (int64_t)it.fst * NRB;
    __shared__ T s_x[SVB_KS][NRB];
    for (int m0 = 0; m0 < w; m0 += NW * 32) {
        const int jb = m0 + wv * 32;
        typename M::acc_t acc[2][NF];
        svb_acc_zero<T>(acc[0]);
        svb_acc_zero<T>(acc[1]);
        for (int ks = 0; ks < nr; ks += SVB_KS) {
            __syncthreads();
            svb_stage_rows<T, SVB_KS, SVB_LTHREADS, true>(s_x, xb, nr - ks, t, grow + ks);
            __syncthreads();
            if (jb < w) {
                const int kend = min(SVB_KS, nr - ks);
                for (int kb = 0; kb < kend; kb += KB) {
                    const int r0 = ks + kb + lk * R;
                    T a[2][R];
#pragma unroll
                    for (int mf = 0; mf < 2; ++mf) {
                        const int j = jb + mf * 16 + lr;
                        svb_krun<T, R>(L + r0 + j * ld, 0, j < w ? nr - r0 : 0, conj, a[mf]);
                    }
#pragma unroll
                    for (int jj = 0; jj < R; ++jj)
#pragma unroll
                        for (int nf = 0; nf < NF; ++nf) {
                            const T b = s_x[kb + lk * R + jj][nf * 16 + lr];
#pragma unroll
                            for (int mf = 0; mf < 2; ++mf) M::step(acc[mf][nf], a[mf][jj], b);
                        }
                }
            }
        }
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int j = jb + mf * 16 + M::row(lane, ii);
                if (j < w) svb_row_sub<T, true>(Y + (int64_t)j * NRB + lr, acc[mf], ii);
            }
    }
}

} // namespace slu
