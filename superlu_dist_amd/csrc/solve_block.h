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
//
// This file also holds what the transposed sweep (solve_block_t.h) and the
// inverted diagonal blocks (solve_block_inv.h) share with it: the fragment
// helpers below and svb_diag, the one body of the four substituting diagonal
// kernels.
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

// elements of a lane's K run in the transposed products: 32 bytes
template <typename T> struct SvbRun { static constexpr int v = 32 / (int)sizeof(T); };

// ---- fragment helpers of the block sweeps ----

// A thread's place in its wave's fragments: wave wv of the workgroup; lr is
// the lane's row of A and its column of B and C, lk its K index of a step (or
// its K run, svb_krun_step).
struct SvbLane { int t, lane, wv, lr, lk; };
__device__ __forceinline__ SvbLane svb_lane() {
    const int t = threadIdx.x, lane = t & 63;
    return {t, lane, t >> 6, lane & 15, lane >> 4};
}

template <typename T, int NF>
__device__ __forceinline__ void svb_acc_zero(typename Mma<T>::acc_t (&acc)[NF]) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[nf] = Mma<T>::zero();
}

// A lane's accumulator row ii (Mma<T>::row(lane, ii) of the fragment) leaves
// along one row of X: px[nf * 16] -= acc[nf](ii), px the row's address + lr.
// Atomically where other workgroups update the row in the same launch (the
// panel kernels), plainly where the workgroup owns it (the diagonal kernels).
template <typename T, bool ATOMIC, int NF>
__device__ __forceinline__ void svb_row_sub(T *px, const typename Mma<T>::acc_t (&acc)[NF], int ii) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        if constexpr (ATOMIC)
            S<T>::atomic_sub(px + nf * 16, Mma<T>::get(acc[nf], ii));
        else
            px[nf * 16] = S<T>::sub(px[nf * 16], Mma<T>::get(acc[nf], ii));
    }
}

// The B operand's LDS tile: s[k][:] = row k of X (GATHER: row idx[k] of X)
// for k < cnt, zeros for the rest of the ROWS rows; by all THREADS threads.
template <typename T, int ROWS, int THREADS, bool GATHER>
__device__ __forceinline__ void svb_stage_rows(T (*s)[SvbNr<T>::v], const T *X, int cnt, int t,
                                               const int *idx = nullptr) {
    constexpr int NRB = SvbNr<T>::v;
    for (int e = t; e < ROWS * NRB; e += THREADS) {
        const int k = e / NRB, q = e % NRB;
        if constexpr (GATHER)
            s[k][q] = k < cnt ? X[(int64_t)idx[k] * NRB + q] : S<T>::zero();
        else
            s[k][q] = k < cnt ? X[(int64_t)k * NRB + q] : S<T>::zero();
    }
}

// The transposed products run the MFMA K index along the contiguous stored
// dimension of the factor.  With the plain lane map A(m = lr, k = lk) a
// wave's load would touch 16 columns x 32 bytes; the MFMA sum does not care in
// which order K is visited as long as A and B agree, so a lane owns a run of
// R = SvbRun consecutive K (32 bytes, two 16-byte loads; the four lanes of a
// column cover 128 contiguous bytes) and reads B's LDS rows by the same
// permutation: step jj of a K block of 4 R multiplies A(m, kb + lk R + jj)
// with B(kb + lk R + jj, n).
//
// svb_krun loads a run: v[j] = op(p[j]) for the j in [lo, hi) and zero
// elsewhere, j < R; elements outside [lo, hi) are not loaded.  A run that lies
// inside goes by 16-byte loads (sv_run; p is element-aligned only), one that
// crosses an end element by element.  A factor element is conjugated as it is
// loaded (sv_cj); X never is.
template <typename T, int R>
__device__ __forceinline__ void svb_krun(const T *p, int lo, int hi, int conj, T (&v)[R]) {
    if (lo <= 0 && hi >= R) {
        sv_run<R>(p, v);
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = (j >= lo && j < hi) ? gld(p + j) : S<T>::zero();
    }
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = sv_cj(v[j], conj);
}

// ... and svb_krun_step multiplies it: the R steps of one K block, the run a
// against the rows k0 + jj of the LDS tile s, k0 = kb + lk R.  (k_svb_ltpanel
// has this loop for two row fragments that share each read of B.  Going
// through this helper, per fragment or with a fragment count, costs it 6 to
// 12 VGPRs and a wave per SIMD in fp32 or complex, so it keeps its own.)
template <typename T, int R, int NF>
__device__ __forceinline__ void svb_krun_step(typename Mma<T>::acc_t (&acc)[NF], const T (&a)[R],
                                              const T (*s)[SvbNr<T>::v], int k0, int lr) {
#pragma unroll
    for (int jj = 0; jj < R; ++jj)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) Mma<T>::step(acc[nf], a[jj], s[k0 + jj][nf * 16 + lr]);
}

// ---- the transpositions ----

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

// ---- the diagonal solves by substitution ----

// c - a b of the substitution.  The complex form spells out S<zc>::fms's
// multiply-adds: the build contracts them anyway (-ffp-contract=fast), and
// which product of a sum of two is rounded before the other is fused into it
// is then the instruction selector's choice, which moved with nothing more
// than the kernel's text being inlined from a device function.  This is the
// selection the four kernels had before they shared a body.  k_svb_utdiag
// (solve_block_t.h) is still that text and calls S<zc>::fms: it equals this
// only as long as the compiler goes on choosing the same way there, so the two
// can drift apart by a rounding with another compiler.
template <typename T> __device__ __forceinline__ T svb_fms(T c, T a, T b) { return S<T>::fms(c, a, b); }
template <> __device__ __forceinline__ zc svb_fms<zc>(zc c, zc a, zc b) {
    return {c.r - fma(a.r, b.r, -(a.i * b.i)), c.i - fma(a.r, b.i, a.i * b.r)};
}

// One step of a lane's substitution in LDS, column q of the panel: x_j is
// final (divided by the diagonal as Sx::div does in k_sv_udiag, no reciprocal,
// unless the diagonal is the unit one) and leaves rows [lo, hi) of the column,
// tj[i] = T(i, j).  SVB_CH LDS reads are in flight, then the stores; a batch
// may read past hi into the pads, whose values are never stored.
template <typename T, bool UNIT>
__device__ __forceinline__ void svb_subst_col(T (*s_p)[SvbNr<T>::v], const T *tj, int q, int j, int lo, int hi) {
    T xj = s_p[j][q];
    if constexpr (!UNIT) {
        xj = S<T>::div(xj, tj[j]);
        s_p[j][q] = xj;
    }
    for (int i = lo; i < hi; i += SVB_CH) {
        T v[SVB_CH], l[SVB_CH];
#pragma unroll
        for (int u = 0; u < SVB_CH; ++u) {
            v[u] = s_p[i + u][q];
            l[u] = tj[i + u];
        }
#pragma unroll
        for (int u = 0; u < SVB_CH; ++u)
            if (i + u < hi) s_p[i + u][q] = svb_fms(v[u], l[u], xj);
    }
}

// T X_k = X_k in place for one supernode per workgroup, T a triangle of the
// diagonal block (w x w at L, column-major, ld) or of its transpose, blocked
// by SVP-column panels.  Per panel: the SVP x SVP triangle (s_t[j][i] =
// T(j0 + i, j0 + j), zeros outside) and the panel's rows of X go to LDS, lane
// q < NRB of the first wave substitutes along column q of the panel in LDS
// (the triangle's entries are broadcasts; neighbouring lanes are neighbouring
// words of a row, and a lane touches its own column only), the solved panel
// goes back to X and stays in LDS as the B operand, and every 16-row fragment
// outside the panel that depends on it subtracts T(rows, panel) X_panel on
// MFMA.  X is streamed: a fragment's rows are read and written in global
// memory (L2-resident, the workgroup owns them); the LDS window is one panel.
// Both LDS arrays carry SVB_CH pads for svb_subst_col, zeroed once.
//
// UNIT picks the block's triangle: the strict lower one with a unit diagonal
// (L_kk) or the upper one with its diagonal (U_kk).  TRANS solves with its
// transpose (conj: the conjugate transpose); the transposed upper triangle is
// not served here (k_svb_utdiag, solve_block_t.h, is written out).  The system
// is lower triangular when UNIT != TRANS (FWD, so FWD means L_kk): panels
// ascend and the fragments below a panel are updated; otherwise panels descend
// from the last, possibly partial one and the fragments above are.  Panels start at multiples of SVP, so the rows
// above a panel are whole fragments, and rows below exist only under full
// panels.  The triangle goes to LDS element by element under its mask, along
// the columns of the block either way: nothing past row j0 + nj - 1 of a
// column is addressed, whatever nj.  Without TRANS the A operand of the
// product is the plain lane map down the block's columns; with it, row i of T
// is column i of the block and a lane's K run lies along it (svb_krun), cut
// at the panel's last row where the panel is partial (rows j0 + nj and below
// of a column belong to the L panel or to the next column).
template <typename T, bool UNIT, bool TRANS>
__device__ __forceinline__ void svb_diag(const SvDiag *items, const T *Lval, T *xb, int conj) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int SVP = SvPanel<T>::v, NRB = SvbNr<T>::v, NF = NRB / 16, NW = SVB_DTHREADS / 64;
    constexpr int R = SvbRun<T>::v, KB = 4 * R;
    constexpr bool FWD = UNIT != TRANS;
    static_assert(SVP % KB == 0, "a panel is whole K blocks");
    static_assert(UNIT || !TRANS, "U_kk^T is k_svb_utdiag's own text");
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int w = it.w;
    const int64_t ld = it.ld;
    T *X = xb + (int64_t)it.fst * NRB;
    __shared__ T s_t[SVP][SVP + SVB_CH];
    __shared__ T s_p[SVP + SVB_CH][NRB];
    for (int e = t; e < SVB_CH * NRB; e += SVB_DTHREADS) s_p[SVP + e / NRB][e % NRB] = Sx::zero();
    for (int e = t; e < SVP * SVB_CH; e += SVB_DTHREADS) s_t[e / SVB_CH][SVP + e % SVB_CH] = Sx::zero();
    const int jfirst = FWD ? 0 : ((w - 1) / SVP) * SVP; // panels ascend, or descend from the last one
    for (int j0 = jfirst; FWD ? j0 < w : j0 >= 0; j0 += FWD ? SVP : -SVP) {
        const int nj = min(SVP, w - j0);
        for (int e = t; e < SVP * SVP; e += SVB_DTHREADS) {
            const int r = e % SVP, c = e / SVP; // r runs down column j0 + c of the block
            const int i = TRANS ? c : r, j = TRANS ? r : c;
            const bool tri = FWD ? i > j : (UNIT ? i < j : i <= j); // T(i, j) is in the triangle
            const bool in = tri && (FWD ? i : j) < nj;                               // and in the panel
            T v = in ? gld(L + (j0 + r) + (j0 + c) * ld) : Sx::zero();
            if constexpr (TRANS) v = in ? sv_cj(v, conj) : v;
            s_t[j][i] = v;
        }
        svb_stage_rows<T, SVP, SVB_DTHREADS, false>(s_p, X + (int64_t)j0 * NRB, nj, t);
        __syncthreads();
        if (t < NRB) {
            if constexpr (FWD)
                for (int j = 0; j < nj - 1; ++j) svb_subst_col<T, UNIT>(s_p, s_t[j], t, j, j + 1, nj);
            else
                for (int j = nj - 1; j >= UNIT; --j) svb_subst_col<T, UNIT>(s_p, s_t[j], t, j, 0, j);
        }
        __syncthreads();
        for (int e = t; e < nj * NRB; e += SVB_DTHREADS) X[(int64_t)j0 * NRB + e] = s_p[e / NRB][e % NRB];
        const int mf0 = FWD ? (j0 + SVP) / 16 : 0, mf1 = FWD ? (w + 15) / 16 : j0 / 16;
        for (int mf = mf0 + wv; mf < mf1; mf += NW) {
            const int i = mf * 16 + lr;
            const bool live = !FWD || i < w;
            typename M::acc_t acc[NF];
            svb_acc_zero<T>(acc);
            if constexpr (!TRANS) {
#pragma unroll
                for (int k0 = 0; k0 < SVP; k0 += 4) {
                    const int k = k0 + lk;
                    const T a = (live && k < nj) ? gld(L + i + (j0 + k) * ld) : Sx::zero();
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf) M::step(acc[nf], a, s_p[k][nf * 16 + lr]);
                }
            } else {
                T a[SVP / KB][R];
#pragma unroll
                for (int b = 0; b < SVP / KB; ++b) {
                    const int k0 = b * KB + lk * R;
                    svb_krun<T, R>(L + i * ld + j0 + k0, 0, nj - k0, conj, a[b]); // rows above: all live
                }
#pragma unroll
                for (int b = 0; b < SVP / KB; ++b) svb_krun_step<T>(acc, a[b], s_p, b * KB + lk * R, lr);
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int r = mf * 16 + M::row(lane, ii);
                if (!FWD || r < w) svb_row_sub<T, false>(X + (int64_t)r * NRB + lr, acc, ii);
            }
        }
        __syncthreads();
    }
}

// L_kk Y = B_k: the unit lower triangle, forward
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_ldiag(const SvDiag *items, const T *Lval, T *xb) {
    svb_diag<T, true, false>(items, Lval, xb, 0);
}

// U_kk X = Y: the upper triangle with its diagonal, backward
template <typename T>
__global__ void __launch_bounds__(SVB_DTHREADS)
k_svb_udiag(const SvDiag *items, const T *Lval, T *xb) {
    svb_diag<T, false, false>(items, Lval, xb, 0);
}

// ---- the panel updates ----

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
    const auto [t, lane, wv, lr, lk] = svb_lane();
    const int w = it.w, nb = it.pad;
    const int64_t ld = it.ld;
    const T *L = Lval + it.voff;
    const int rbase = ch.c0 + wv * 32;
    __shared__ T s_y[SVB_KS][NRB];
    typename M::acc_t acc[2][NF];
    svb_acc_zero<T>(acc[0]);
    svb_acc_zero<T>(acc[1]);
    for (int ks = 0; ks < w; ks += SVB_KS) {
        if (ks) __syncthreads();
        svb_stage_rows<T, SVB_KS, SVB_LTHREADS, false>(s_y, xb + (int64_t)(it.fst + ks) * NRB, w - ks, t);
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
            if (r < nb) svb_row_sub<T, true>(xb + (int64_t)grow[r] * NRB + lr, acc[mf], ii);
        }
}

// Y_k -= U(k, chunk of SVU_COLS columns) * X[gc]: the chunk's X rows are
// gathered into LDS as the B operand, A is the skyline segments (column c
// holds rows fst_c..w-1 contiguously; rows above fst_c are zeros that are not
// loaded, k_sv_upanel's guard).  A wave takes every fourth 16-row fragment of
// the supernode; atomics into Y_k's rows, 8 instructions per fragment.  The
// gather's predicate is s_gc's -1 past the chunk's last column, not a count,
// so it is not svb_stage_rows.
template <typename T>
__global__ void __launch_bounds__(SV_THREADS)
k_svb_upanel(const SvChunk *chunks, const SvDiag *diag, const int64_t *coff, const int *ncol,
             const int64_t *ucol_voff, const int *ucol_fst, const int *ucol_gc, const T *Uval, T *xb) {
    using Sx = S<T>;
    using M = Mma<T>;
    constexpr int NRB = SvbNr<T>::v, NF = NRB / 16, NW = SV_THREADS / 64;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = diag[ch.sn];
    const auto [t, lane, wv, lr, lk] = svb_lane();
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
        svb_acc_zero<T>(acc);
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
            if (r < w) svb_row_sub<T, true>(Y + (int64_t)r * NRB + lr, acc, ii);
        }
    }
}

} // namespace slu
