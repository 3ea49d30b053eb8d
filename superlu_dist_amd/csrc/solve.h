// Device-resident triangular solves with the factored supernodal L and U
// (1x1 grid), level-scheduled like the factorization: SURVEY §8(f) row 2,
// the first step of pdgstrs (SRC/pdgstrs.c, SRC/pdgstrs_lsum.c) on the
// factors the engine leaves in HBM.  Included by engine.hip.
//
// Forward  L y = b : per level, (1) unit-lower solve with each supernode's
//                    diagonal block, (2) y_rows_below -= L_panel * y_k
//                    (chunks of 256 panel rows, atomics across supernodes).
// Backward U x = y : per level in reverse, (1) y_k -= U(k,:) x over the
//                    supernode's U row segments (chunks of 256 columns,
//                    atomics), (2) upper solve with the diagonal block.
// The diagonal block holds L\U in the first w rows of the supernode's L
// column block (SRC/pdgstrf2.c:213-269 stores U11 there); the arithmetic per
// element is the reference's dtrsv/dgemv on those blocks (SRC/pdgstrs.c
// dlsum_fmod / dlsum_bmod).
#pragma once
#include "kernels.h"

namespace slu {

struct SvDiag {     // one supernode's diagonal block
    int64_t voff;   // offset of its L column block in Lval
    int ld, w, fst; // nsupr, width, first global row/column
    int pad;
};
struct SvChunk {    // 256 panel rows (forward) or 256 U columns (backward)
    int sn;         // index into the SvDiag / per-supernode tables
    int c0;         // first row below the diagonal block / first U column
};

constexpr int SV_THREADS = 256;  // panel chunks
constexpr int SVD_THREADS = 512; // diagonal solves: one thread per row, w <= MAX_SUPER_SIZE

// value of lane `src` (wavefront-uniform) for every lane: v_readlane into a
// scalar register, no LDS round trip (tools/micro/lat_micro.hip: readlane +
// FMA 56 cycles against 92 for an LDS load)
__device__ inline float sv_shfl(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ inline double sv_shfl(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ inline zc sv_shfl(zc v, int src) { return {sv_shfl(v.r, src), sv_shfl(v.i, src)}; }

// columns per panel of the diagonal solves: 32 (16 complex, to keep the
// thread's panel row in registers); divides the 64-wide wavefront, so a
// panel's rows always sit in one wavefront
template <typename T> struct SvPanel { static constexpr int v = sizeof(T) == 16 ? 16 : 32; };

// Right-hand sides: NR (compile-time, 1 or SV_NR) columns of x with leading
// dimension ldx, of which the first nr (<= NR, uniform) are live; every
// factor element is read once per sweep for all of them.  Dead columns are
// carried as zeros through the arithmetic (never loaded or stored), so the
// NR independent chains stay branch-free and interleave.
constexpr int SV_NR = 8;
template <typename T> struct SvNr { static constexpr int v = sizeof(T) == 16 ? 2 : SV_NR; }; // no spills

// L_kk y_k = b_k, unit lower, blocked by SVP-column panels.  Thread t owns
// row t and holds its SVP panel entries in registers (one coalesced batch of
// loads per panel).  The panel's own rows are solved inside their wavefront
// (y_j passed by lane shuffle, no barrier per column); one barrier publishes
// the panel's y through LDS, then every row below subtracts L(t, panel) y.
template <typename T, int NR>
__global__ void __launch_bounds__(SVD_THREADS)
k_sv_ldiag(const SvDiag *items, const T *Lval, T *x, int64_t ldx, int nr) {
    using Sx = S<T>;
    constexpr int SVP = SvPanel<T>::v;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, w = it.w, ld = it.ld;
    __shared__ T s_y[2][NR][SVP];
    T yi[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) yi[q] = (q < nr && t < w) ? x[it.fst + t + q * ldx] : Sx::zero();
    for (int j0 = 0, buf = 0; j0 < w; j0 += SVP, buf ^= 1) {
        const int nj = min(SVP, w - j0);
        T l[SVP];
#pragma unroll
        for (int j = 0; j < SVP; ++j)
            l[j] = (j < nj && t > j0 + j && t < w) ? L[t + (int64_t)(j0 + j) * ld] : Sx::zero();
        if ((t >> 6) == (j0 >> 6)) {
            const int base = j0 & 63;
#pragma unroll
            for (int j = 0; j < SVP; ++j) {
                const bool upd = t > j0 + j && t < j0 + nj;
#pragma unroll
                for (int q = 0; q < NR; ++q) {
                    const T yj = sv_shfl(yi[q], base + j);
                    if (upd) yi[q] = Sx::fms(yi[q], l[j], yj);
                }
            }
            if (t >= j0 && t < j0 + nj)
#pragma unroll
                for (int q = 0; q < NR; ++q) s_y[buf][q][t - j0] = yi[q];
        }
        __syncthreads();
        if (t >= j0 + nj && t < w) { // only for full panels (a partial one is the last)
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int j = 0; j < SVP; ++j) yi[q] = Sx::fms(yi[q], l[j], s_y[buf][q][j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q < nr && t < w) x[it.fst + t + q * ldx] = yi[q];
}

// U_kk x_k = y_k (upper, non-unit), blocked like k_sv_ldiag from the last
// panel up: in-panel back substitution by lane shuffles, then every row above
// the panel subtracts U(t, panel) x_panel.
template <typename T, int NR>
__global__ void __launch_bounds__(SVD_THREADS)
k_sv_udiag(const SvDiag *items, const T *Lval, T *x, int64_t ldx, int nr) {
    using Sx = S<T>;
    constexpr int SVP = SvPanel<T>::v;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, w = it.w, ld = it.ld;
    __shared__ T s_x[2][NR][SVP];
    T yi[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) yi[q] = (q < nr && t < w) ? x[it.fst + t + q * ldx] : Sx::zero();
    for (int j0 = ((w - 1) / SVP) * SVP, buf = 0; j0 >= 0; j0 -= SVP, buf ^= 1) {
        const int nj = min(SVP, w - j0);
        T u[SVP];
#pragma unroll
        for (int j = 0; j < SVP; ++j)
            u[j] = (j < nj && t < j0 + j) ? L[t + (int64_t)(j0 + j) * ld] : Sx::zero();
        const bool mine = t >= j0 && t < j0 + nj;
        const T d = mine ? L[t + (int64_t)t * ld] : Sx::zero();
        if ((t >> 6) == (j0 >> 6)) {
            const int base = j0 & 63;
#pragma unroll
            for (int j = SVP - 1; j >= 0; --j) {
                if (j < nj) {
                    const bool upd = t >= j0 && t < j0 + j;
#pragma unroll
                    for (int q = 0; q < NR; ++q) {
                        if (t == j0 + j) yi[q] = Sx::div(yi[q], d);
                        const T xj = sv_shfl(yi[q], base + j);
                        if (upd) yi[q] = Sx::fms(yi[q], u[j], xj);
                    }
                }
            }
            if (mine)
#pragma unroll
                for (int q = 0; q < NR; ++q) s_x[buf][q][t - j0] = yi[q];
        }
        __syncthreads();
        if (t < j0) { // the first (last-column) panel may be partial: no stale LDS
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int j = 0; j < SVP; ++j)
                    if (j < nj) yi[q] = Sx::fms(yi[q], u[j], s_x[buf][q][j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q < nr && t < w) x[it.fst + t + q * ldx] = yi[q];
}

// x[rows below] -= L_panel(256-row chunk) * y_k.  The panel descriptor
// (SvDiag fields) points at the first row below the diagonal block: voff =
// its offset in Lval, ld = nsupr, pad = number of rows below (on a 2D grid
// the rank's rows of L(:,k) on its process row; on the diagonal owner they
// follow the diagonal block, elsewhere the column block has none).
template <typename T, int NR>
__global__ void __launch_bounds__(SV_THREADS)
k_sv_lpanel(const SvChunk *chunks, const SvDiag *pan, const int64_t *roff, const int *rows,
            const T *Lval, T *x, int64_t ldx, int nr) {
    using Sx = S<T>;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = pan[ch.sn];
    const int t = threadIdx.x, w = it.w, nb = it.pad;
    __shared__ T s_y[NR][FAST_MAXW * 2];
    for (int q = 0; q < nr; ++q)
        for (int j = t; j < w; j += SV_THREADS) s_y[q][j] = x[it.fst + j + q * ldx];
    __syncthreads();
    const int r = ch.c0 + t;
    if (r >= nb) return;
    const T *L = Lval + it.voff + r;
    T acc[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) acc[q] = Sx::zero();
    constexpr int UN = 16; // columns of loads in flight per thread
    for (int j0 = 0; j0 < w; j0 += UN) {
        T v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) v[u] = j0 + u < w ? L[(int64_t)(j0 + u) * it.ld] : Sx::zero();
#pragma unroll
        for (int q = 0; q < NR; ++q) {
#pragma unroll
            for (int u = 0; u < UN; ++u)
                if (j0 + u < w) acc[q] = Sx::fms(acc[q], v[u], s_y[q][j0 + u]);
        }
    }
    // acc = -(L_r . y)
    const int64_t gr = rows[roff[ch.sn] + r];
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q < nr) Sx::atomic_sub(x + gr + q * ldx, Sx::neg(acc[q]));
}

// y_k -= U(k, chunk of SVU_COLS columns) x: thread t owns rows t, t + 256 of
// the supernode; each U column is a segment of rows fst..w-1 stored
// contiguously (coalesced along t).  Short chunks (many workgroups per
// supernode at the chain-bound top of the tree) and 16 columns of loads in
// flight per thread; partial sums meet in x through atomics.
constexpr int SVU_COLS = 64;
template <typename T, int NR>
__global__ void __launch_bounds__(SV_THREADS)
k_sv_upanel(const SvChunk *chunks, const SvDiag *diag, const int64_t *coff, const int *ncol,
            const int64_t *ucol_voff, const int *ucol_fst, const int *ucol_gc, const T *Uval,
            T *x, int64_t ldx, int nr) {
    using Sx = S<T>;
    constexpr int UN = 16;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = diag[ch.sn];
    const int t = threadIdx.x, w = it.w;
    const int nc = min(SVU_COLS, ncol[ch.sn] - ch.c0);
    __shared__ int64_t s_v[SVU_COLS];
    __shared__ int s_f[SVU_COLS];
    __shared__ T s_x[NR][SVU_COLS];
    if (t < SVU_COLS) {
        const int64_t e = coff[ch.sn] + ch.c0 + t;
        s_v[t] = t < nc ? ucol_voff[e] : 0;
        s_f[t] = t < nc ? ucol_fst[e] - it.fst : w; // first row of the segment, relative
        const int64_t gc = t < nc ? ucol_gc[e] : 0;
#pragma unroll
        for (int q = 0; q < NR; ++q) s_x[q][t] = (t < nc && q < nr) ? x[gc + q * ldx] : Sx::zero();
    }
    __syncthreads();
    for (int i = t; i < w; i += SV_THREADS) { // w <= MAX_SUPER_SIZE = 2 x SV_THREADS
        T acc[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) acc[q] = Sx::zero();
        for (int c0 = 0; c0 < nc; c0 += UN) {
            T v[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int rf = s_f[c0 + u]; // w (no load) past the chunk's last column
                v[u] = i >= rf ? Uval[s_v[c0 + u] + i - rf] : Sx::zero();
            }
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int u = 0; u < UN; ++u) acc[q] = Sx::fms(acc[q], v[u], s_x[q][c0 + u]);
            }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q)
            if (q < nr) Sx::atomic_sub(x + it.fst + i + q * ldx, Sx::neg(acc[q]));
    }
}

// ---------------------------------------------------------------------------
// Transposed sweeps: B^T y = c (or B^H, conj != 0, complex only) on the same
// factors, tables and levels.  U^T z = c runs forward (z_j waits for z_k with
// U(k,j) != 0, the DAG edge k -> j), L^T y = z backward; the roles of L and
// U swap: U's row segments are pushed (k_sv_utpanel), L's panel rows are
// pulled (k_sv_ltpanel), and every product runs along the stored contiguous
// dimension.  A factor element is conjugated as it is loaded, never x.
__device__ inline double sv_cj(double v, int) { return v; }
__device__ inline float sv_cj(float v, int) { return v; }
__device__ inline zc sv_cj(zc v, int conj) { return {v.r, conj ? -v.i : v.i}; }

__device__ inline float sv_xor(float v, int off) { return __shfl_xor(v, off, 64); }
__device__ inline double sv_xor(double v, int off) { return __shfl_xor(v, off, 64); }
__device__ inline zc sv_xor(zc v, int off) { return {__shfl_xor(v.r, off, 64), __shfl_xor(v.i, off, 64)}; }
__device__ inline float sv_add(float a, float b) { return a + b; }
__device__ inline double sv_add(double a, double b) { return a + b; }
__device__ inline zc sv_add(zc a, zc b) { return {a.r + b.r, a.i + b.i}; }
__device__ inline float sv_sel(bool c, float a, float b) { return c ? a : b; }
__device__ inline double sv_sel(bool c, double a, double b) { return c ? a : b; }
__device__ inline zc sv_sel(bool c, zc a, zc b) { return {c ? a.r : b.r, c ? a.i : b.i}; }

template <int N> struct SvLog2 { static constexpr int v = 1 + SvLog2<N / 2>::v; };
template <> struct SvLog2<1> { static constexpr int v = 0; };

// Sums of N values per lane over groups of W consecutive lanes (N, W powers
// of two, W <= 64) by a halving butterfly: at each step a lane keeps one
// half of its values and hands the other half to its partner, so the sums
// cost about N exchanges instead of N log2 W.  With l = lane % W afterwards:
// N >= W: v[i], i < N / W, of lane l is the sum of element l * (N / W) + i;
// N <  W: v[0] of lane l is the sum of element l / (W / N) (held W / N times).
template <typename T, int N, int W = 64> __device__ __forceinline__ void sv_bfly(T (&v)[N], int lane) {
    static_assert(N >= 1 && (N & (N - 1)) == 0 && W >= 1 && W <= 64 && (W & (W - 1)) == 0, "N, W");
    constexpr int STEPS = SvLog2<N>::v < SvLog2<W>::v ? SvLog2<N>::v : SvLog2<W>::v;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int cur = N >> s, off = (W / 2) >> s;
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < cur / 2; ++i) {
            const T send = sv_sel(up, v[i], v[i + cur / 2]);
            const T keep = sv_sel(up, v[i + cur / 2], v[i]);
            v[i] = sv_add(keep, sv_xor(send, off));
        }
    }
    if constexpr (W > N) {
#pragma unroll
        for (int o = W / N / 2; o > 0; o >>= 1) v[0] = sv_add(v[0], sv_xor(v[0], o));
    }
}

// SVP consecutive elements from p (element-aligned only) by 16-byte loads:
// a thread's run down one column of the diagonal block
template <int N> __device__ __forceinline__ void sv_run(const double *p, double (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; j += 2) gld2(p + j, v[j], v[j + 1]);
}
typedef float f4u4 __attribute__((ext_vector_type(4), aligned(4)));
template <int N> __device__ __forceinline__ void sv_run(const float *p, float (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; j += 4) {
        const f4u4 a = *(const __attribute__((address_space(1))) f4u4 *)(p + j);
        v[j] = a.x; v[j + 1] = a.y; v[j + 2] = a.z; v[j + 3] = a.w;
    }
}
template <int N> __device__ __forceinline__ void sv_run(const zc *p, zc (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = gld(p + j);
}

// U_kk^T z_k = c_k (lower, non-unit), blocked like k_sv_ldiag.  U_kk is the
// upper triangle of the first w rows of the column block (ld nsupr), so row t
// of U_kk^T is column t of the block: contiguous for thread t, strided by ld
// across threads.  Each thread reads its SVP-element run of a full panel
// with 16-byte loads (whole cache lines are consumed by the thread that
// fetched them) and masks what lies past the diagonal; the diagonal element
// is picked out of the run.  Only the partial last panel, whose run could
// pass the end of the column, loads element by element.
template <typename T, int NR>
__global__ void __launch_bounds__(SVD_THREADS)
k_sv_utdiag(const SvDiag *items, const T *Lval, T *x, int64_t ldx, int nr, int conj) {
    using Sx = S<T>;
    constexpr int SVP = SvPanel<T>::v;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, w = it.w, ld = it.ld;
    __shared__ T s_z[2][NR][SVP];
    T yi[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) yi[q] = (q < nr && t < w) ? x[it.fst + t + q * ldx] : Sx::zero();
    for (int j0 = 0, buf = 0; j0 < w; j0 += SVP, buf ^= 1) {
        const int nj = min(SVP, w - j0);
        T u[SVP]; // u[j] = U(j0 + j, t), rows above the diagonal of column t
        T d = one_of(T());
        if (t >= j0 && t < w) {
            const T *col = L + (int64_t)t * ld + j0;
            if (nj == SVP) {
                sv_run<SVP>(col, u);
            } else {
#pragma unroll
                for (int j = 0; j < SVP; ++j) u[j] = (j < nj && j0 + j <= t) ? col[j] : Sx::zero();
            }
#pragma unroll
            for (int j = 0; j < SVP; ++j) {
                if (t == j0 + j) d = sv_cj(u[j], conj);
                u[j] = sv_sel(j0 + j < t, sv_cj(u[j], conj), Sx::zero());
            }
        } else {
#pragma unroll
            for (int j = 0; j < SVP; ++j) u[j] = Sx::zero();
        }
        if ((t >> 6) == (j0 >> 6)) {
            const int base = j0 & 63;
#pragma unroll
            for (int j = 0; j < SVP; ++j) {
                if (j < nj) {
                    const bool upd = t > j0 + j && t < j0 + nj;
#pragma unroll
                    for (int q = 0; q < NR; ++q) {
                        if (t == j0 + j) yi[q] = Sx::div(yi[q], d);
                        const T zj = sv_shfl(yi[q], base + j);
                        if (upd) yi[q] = Sx::fms(yi[q], u[j], zj);
                    }
                }
            }
            if (t >= j0 && t < j0 + nj)
#pragma unroll
                for (int q = 0; q < NR; ++q) s_z[buf][q][t - j0] = yi[q];
        }
        __syncthreads();
        if (t >= j0 + nj && t < w) { // only after full panels (a partial one is the last)
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int j = 0; j < SVP; ++j) yi[q] = Sx::fms(yi[q], u[j], s_z[buf][q][j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q < nr && t < w) x[it.fst + t + q * ldx] = yi[q];
}

// L_kk^T y_k = z_k (upper, unit) from the strict lower triangle, from the
// last panel up like k_sv_udiag: row t of L_kk^T is column t of the block
// below its diagonal, read as in k_sv_utdiag.
template <typename T, int NR>
__global__ void __launch_bounds__(SVD_THREADS)
k_sv_ltdiag(const SvDiag *items, const T *Lval, T *x, int64_t ldx, int nr, int conj) {
    using Sx = S<T>;
    constexpr int SVP = SvPanel<T>::v;
    const SvDiag it = items[blockIdx.x];
    const T *L = Lval + it.voff;
    const int t = threadIdx.x, w = it.w, ld = it.ld;
    __shared__ T s_y[2][NR][SVP];
    T yi[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) yi[q] = (q < nr && t < w) ? x[it.fst + t + q * ldx] : Sx::zero();
    for (int j0 = ((w - 1) / SVP) * SVP, buf = 0; j0 >= 0; j0 -= SVP, buf ^= 1) {
        const int nj = min(SVP, w - j0);
        T l[SVP]; // l[j] = L(j0 + j, t), rows below the diagonal of column t
        if (t < j0 + nj) {
            const T *col = L + (int64_t)t * ld + j0;
            if (nj == SVP) {
                sv_run<SVP>(col, l);
            } else {
#pragma unroll
                for (int j = 0; j < SVP; ++j) l[j] = (j < nj && j0 + j > t) ? col[j] : Sx::zero();
            }
#pragma unroll
            for (int j = 0; j < SVP; ++j) l[j] = sv_sel(j0 + j > t, sv_cj(l[j], conj), Sx::zero());
        } else {
#pragma unroll
            for (int j = 0; j < SVP; ++j) l[j] = Sx::zero();
        }
        if ((t >> 6) == (j0 >> 6)) {
            const int base = j0 & 63;
#pragma unroll
            for (int j = SVP - 1; j >= 0; --j) {
                if (j < nj) {
                    const bool upd = t >= j0 && t < j0 + j;
#pragma unroll
                    for (int q = 0; q < NR; ++q) {
                        const T yj = sv_shfl(yi[q], base + j);
                        if (upd) yi[q] = Sx::fms(yi[q], l[j], yj);
                    }
                }
            }
            if (t >= j0 && t < j0 + nj)
#pragma unroll
                for (int q = 0; q < NR; ++q) s_y[buf][q][t - j0] = yi[q];
        }
        __syncthreads();
        if (t < j0) { // the first (last-column) panel may be partial: no stale LDS
#pragma unroll
            for (int q = 0; q < NR; ++q) {
#pragma unroll
                for (int j = 0; j < SVP; ++j)
                    if (j < nj) yi[q] = Sx::fms(yi[q], l[j], s_y[buf][q][j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q < nr && t < w) x[it.fst + t + q * ldx] = yi[q];
}

// Forward push of U^T: x[gc] -= sum_i U(i, gc) z_k[i] for a chunk of SVU_COLS
// U columns of block row k (the chunks of k_sv_upanel).  A column's segment
// rows fst..w-1 is contiguous in Uval, so a group of G lanes runs along i (G
// = the power of two covering w, at most SVT_G = 16: 128 contiguous bytes of
// fp64 per load, and a lane of a wide supernode sums w / 16 rows before the
// group's reduction, whose cost does not depend on w), UC columns at a time
// per group to keep loads in flight, and the group's sum leaves as one atomic
// per column and live right-hand side.  z_k sits in LDS (dead right-hand
// sides as zeros).  Full groups reduce by sv_bfly.
constexpr int SVT_G = 16;
constexpr int SVT_UC = 4;
template <typename T, int NR>
__global__ void __launch_bounds__(SV_THREADS)
k_sv_utpanel(const SvChunk *chunks, const SvDiag *diag, const int64_t *coff, const int *ncol,
             const int64_t *ucol_voff, const int *ucol_fst, const int *ucol_gc, const T *Uval,
             T *x, int64_t ldx, int nr, int conj) {
    using Sx = S<T>;
    constexpr int UC = SVT_UC, N = UC * NR;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = diag[ch.sn];
    const int t = threadIdx.x, w = it.w;
    const int nc = min(SVU_COLS, ncol[ch.sn] - ch.c0);
    __shared__ int64_t s_v[SVU_COLS];
    __shared__ int s_f[SVU_COLS], s_gc[SVU_COLS];
    __shared__ T s_z[NR][FAST_MAXW * 2];
    if (t < nc) {
        const int64_t e = coff[ch.sn] + ch.c0 + t;
        s_v[t] = ucol_voff[e];
        s_f[t] = ucol_fst[e] - it.fst; // first row of the segment, relative
        s_gc[t] = ucol_gc[e];
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        for (int j = t; j < w; j += SV_THREADS) s_z[q][j] = q < nr ? x[it.fst + j + q * ldx] : Sx::zero();
    __syncthreads();
    int G = 1;
    while (G < w && G < SVT_G) G <<= 1;
    const int li = t & (G - 1), g = t / G, NG = SV_THREADS / G;
    for (int cb = 0; cb < nc; cb += NG * UC) { // uniform over the workgroup
        int64_t vo[UC];
        int rf[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int c = cb + g + u * NG;
            rf[u] = c < nc ? s_f[c] : w; // w: nothing to load
            vo[u] = c < nc ? s_v[c] : 0;
        }
        T acc[N];
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = Sx::zero();
#pragma unroll 2
        for (int i = li; i < w; i += G) {
            T v[UC], z[NR];
#pragma unroll
            for (int u = 0; u < UC; ++u) v[u] = i >= rf[u] ? sv_cj(Uval[vo[u] + i - rf[u]], conj) : Sx::zero();
#pragma unroll
            for (int q = 0; q < NR; ++q) z[q] = s_z[q][i];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
#pragma unroll
                for (int q = 0; q < NR; ++q) acc[u * NR + q] = Sx::fms(acc[u * NR + q], v[u], z[q]);
            }
        }
        // acc = -(U(:, c)^T z_k), partial over this lane's rows
        if (G == SVT_G) {
            sv_bfly<T, N, SVT_G>(acc, li);
            constexpr int PER = N >= SVT_G ? N / SVT_G : 1, REP = N >= SVT_G ? 1 : SVT_G / N;
            if (li % REP == 0) {
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const int e = (li / REP) * PER + k, u = e / NR, q = e % NR;
                    const int c = cb + g + u * NG;
                    if (c < nc && q < nr) Sx::atomic_sub(x + s_gc[c] + q * ldx, Sx::neg(acc[k]));
                }
            }
        } else {
            for (int off = G >> 1; off > 0; off >>= 1) {
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] = sv_add(acc[e], sv_xor(acc[e], off));
            }
            if (li == 0) {
#pragma unroll
                for (int u = 0; u < UC; ++u) {
                    const int c = cb + g + u * NG;
#pragma unroll
                    for (int q = 0; q < NR; ++q)
                        if (c < nc && q < nr) Sx::atomic_sub(x + s_gc[c] + q * ldx, Sx::neg(acc[u * NR + q]));
                }
            }
        }
    }
}

__device__ inline void sv_lds_add(float *p, float v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ inline void sv_lds_add(double *p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ inline void sv_lds_add(zc *p, zc v) {
    sv_lds_add(&p->r, v.r);
    sv_lds_add(&p->i, v.i);
}

// Backward pull of L^T: y_k[j] -= sum_r L(r, j) x[rows[r]] over a chunk of
// 256 rows below the diagonal block (the chunks and panel descriptors of
// k_sv_lpanel).  Thread t owns row c0 + t: it gathers x of its row once for
// all right-hand sides and loads down the columns, coalesced along r, JB
// columns at a time.  The JB x NR products of a step are summed over the
// wavefront by sv_bfly (one result per lane), the four wavefronts meet in
// LDS, and the chunk leaves one atomic per column and live right-hand side.
template <typename T, int NR>
__global__ void __launch_bounds__(SV_THREADS)
k_sv_ltpanel(const SvChunk *chunks, const SvDiag *pan, const int64_t *roff, const int *rows,
             const T *Lval, T *x, int64_t ldx, int nr, int conj) {
    using Sx = S<T>;
    constexpr int JB = NR == 1 ? 16 : 8, N = JB * NR, LG = SvLog2<N>::v;
    const SvChunk ch = chunks[blockIdx.x];
    const SvDiag it = pan[ch.sn];
    const int t = threadIdx.x, w = it.w, nb = it.pad, lane = t & 63;
    __shared__ T s_acc[NR][FAST_MAXW * 2];
#pragma unroll
    for (int q = 0; q < NR; ++q)
        for (int j = t; j < w; j += SV_THREADS) s_acc[q][j] = Sx::zero();
    __syncthreads();
    const int r = ch.c0 + t;
    const bool live = r < nb;
    if (ch.c0 + (t & ~63) < nb) { // wavefronts past the panel's last row have nothing to add
        T xr[NR];
        const int64_t gr = live ? rows[roff[ch.sn] + r] : 0;
#pragma unroll
        for (int q = 0; q < NR; ++q) xr[q] = (live && q < nr) ? x[gr + q * ldx] : Sx::zero();
        const T *L = Lval + it.voff + r;
        const int e = lane >> (6 - LG), ju = e / NR, q = e % NR;
        const bool first = (lane & (64 / N - 1)) == 0;
        for (int j0 = 0; j0 < w; j0 += JB) {
            T v[JB];
#pragma unroll
            for (int u = 0; u < JB; ++u)
                v[u] = (live && j0 + u < w) ? sv_cj(L[(int64_t)(j0 + u) * it.ld], conj) : Sx::zero();
            T p[N];
#pragma unroll
            for (int u = 0; u < JB; ++u) {
#pragma unroll
                for (int qq = 0; qq < NR; ++qq) p[u * NR + qq] = Sx::mul(v[u], xr[qq]);
            }
            sv_bfly<T, N>(p, lane);
            if (first && j0 + ju < w) sv_lds_add(&s_acc[q][j0 + ju], p[0]);
        }
    }
    __syncthreads();
    for (int q = 0; q < nr; ++q)
        for (int j = t; j < w; j += SV_THREADS) Sx::atomic_sub(x + it.fst + j + q * ldx, s_acc[q][j]);
}

// Residual of the transposed refinement: r = c - op(B)^T x, s = |B^T||x| +
// |c|.  A row of B^T is a column of B, so thread j runs over column j of the
// CSC of set_a_pattern (entries lo[j] .. hi[j] - 1, rows ci); guards and the
// NaN-wins maximum as in k_resid.
template <typename T>
__global__ void __launch_bounds__(256)
k_resid_t(const unsigned long long *lo, const unsigned long long *hi, const int *ci, const T *a,
          const T *x, const T *b, T *r, int n, double safe1, double safe2,
          unsigned long long *berr, int conj) {
    using Sx = S<T>;
    const int j = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (j < n) {
        T acc = b[j];
        double tmp = Sx::abs1(b[j]);
        for (unsigned long long e = lo[j]; e < hi[j]; ++e) {
            const T av = sv_cj(a[e], conj), xv = x[ci[e]];
            acc = Sx::fms(acc, av, xv);
            tmp += Sx::abs1(av) * Sx::abs1(xv);
        }
        r[j] = acc;
        const double ra = Sx::abs1(acc);
        if (tmp > safe2) s = ra / tmp;
        else if (tmp != 0.0) s = (safe1 + ra) / tmp;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(s, off, 64);
        s = (s != s || o != o) ? __builtin_nan("") : fmax(s, o);
    }
    if ((threadIdx.x & 63) == 0 && !(s <= 0.0))
        atomicMax(berr, (unsigned long long)__double_as_longlong(s));
}
// The CSC view k_resid_t reads, from the rows of A the plan keeps on the
// device (entry q of row i is nonzero re[q] of column rc[q]): the row of
// every nonzero and each column's range of nonzeros (lo = ~0, hi = 0 before).
__global__ void __launch_bounds__(256)
k_csc_of_rows(const int64_t *rp, const int *rc, const int64_t *re, int n, int *ci,
              unsigned long long *lo, unsigned long long *hi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int64_t q = rp[i]; q < rp[i + 1]; ++q) {
        const unsigned long long e = (unsigned long long)re[q];
        ci[e] = i;
        atomicMin(lo + rc[q], e);
        atomicMax(hi + rc[q], e + 1);
    }
}

// ---------------------------------------------------------------------------
// Small kernels of the condition estimate (Hager / Higham, LAPACK dlacn2 /
// zlacn2 as driven by SuperLU's dgscon): one workgroup each, so their sums
// and the first-maximum rule are deterministic; only RcOut crosses PCIe.
struct RcOut {
    double sum;   // sum_i |x_i| before the sign step
    double amax;  // |x_j| at j = the first index of the largest |x_i|
    double xlast; // x_jlast (real; the modulus for complex)
    int j, ndiff; // ndiff: entries whose sign differs from the previous sign vector
};
constexpr int RC_THREADS = 1024;
__device__ inline double rc_abs(double v) { return fabs(v); }
__device__ inline double rc_abs(float v) { return fabs((double)v); }
__device__ inline double rc_abs(zc v) { return hypot(v.r, v.i); }
__device__ inline double rc_sign(double v, double) { return v >= 0.0 ? 1.0 : -1.0; }
__device__ inline float rc_sign(float v, double) { return v >= 0.0f ? 1.0f : -1.0f; }
__device__ inline zc rc_sign(zc v, double a) { // zlacn2: x / |x|, 1 where |x| <= safmin
    return a > 2.2250738585072014e-308 ? zc{v.r / a, v.i / a} : zc{1.0, 0.0};
}
__device__ inline bool rc_differs(double a, double b) { return a != b; }
__device__ inline bool rc_differs(float a, float b) { return a != b; }
__device__ inline bool rc_differs(zc, zc) { return false; } // zlacn2 has no sign test
__device__ inline double rc_real(double v) { return v; }
__device__ inline double rc_real(float v) { return v; }
__device__ inline double rc_real(zc v) { return hypot(v.r, v.i); }
__device__ inline float rc_from(double v, float) { return (float)v; }
__device__ inline double rc_from(double v, double) { return v; }
__device__ inline zc rc_from(double v, zc) { return {v, 0.0}; }

// mode 0: x = 1/n; 1: x = e_j; 2: x_i = (-1)^i (1 + i / (n - 1))
template <typename T> __global__ void __launch_bounds__(256) k_rc_fill(T *x, int n, int mode, int j) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v;
    if (mode == 0) v = 1.0 / n;
    else if (mode == 1) v = i == j ? 1.0 : 0.0;
    else v = (i & 1 ? -1.0 : 1.0) * (1.0 + (n > 1 ? (double)i / (n - 1) : 0.0));
    x[i] = rc_from(v, T());
}
// After a sweep with op: out->sum = ||x||_1; with dosign also ndiff against
// the previous sign vector sgn, then x = sgn = sign(x).
template <typename T>
__global__ void __launch_bounds__(RC_THREADS) k_rc_norm_sign(T *x, T *sgn, int n, int dosign, RcOut *out) {
    __shared__ double s_sum[RC_THREADS / 64];
    __shared__ int s_nd[RC_THREADS / 64];
    double sum = 0.0;
    int nd = 0;
    for (int i = threadIdx.x; i < n; i += RC_THREADS) {
        const T v = x[i];
        const double a = rc_abs(v);
        sum += a;
        if (dosign) {
            const T sg = rc_sign(v, a);
            nd += rc_differs(sg, sgn[i]);
            x[i] = sgn[i] = sg;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        nd += __shfl_xor(nd, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_nd[threadIdx.x >> 6] = nd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < RC_THREADS / 64; ++k) {
            sum += s_sum[k];
            nd += s_nd[k];
        }
        out->sum = sum;
        out->ndiff = nd;
    }
}
// After a sweep with op^T: j = the first index of the largest |x_i| (idamax
// / izmax1), amax = |x_j|, xlast = x_jlast.
template <typename T>
__global__ void __launch_bounds__(RC_THREADS) k_rc_amax(const T *x, int n, int jlast, RcOut *out) {
    __shared__ double s_a[RC_THREADS / 64];
    __shared__ int s_j[RC_THREADS / 64];
    double a = -1.0;
    int j = n;
    for (int i = threadIdx.x; i < n; i += RC_THREADS) {
        const double v = rc_abs(x[i]);
        if (v > a) { // ascending i per thread: the first maximum stays
            a = v;
            j = i;
        }
    }
    auto better = [](double a1, int j1, double a2, int j2) { return a1 > a2 || (a1 == a2 && j1 < j2); };
    for (int off = 32; off > 0; off >>= 1) {
        const double oa = __shfl_xor(a, off, 64);
        const int oj = __shfl_xor(j, off, 64);
        if (better(oa, oj, a, j)) {
            a = oa;
            j = oj;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        s_a[threadIdx.x >> 6] = a;
        s_j[threadIdx.x >> 6] = j;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < RC_THREADS / 64; ++k)
            if (better(s_a[k], s_j[k], a, j)) {
                a = s_a[k];
                j = s_j[k];
            }
        out->j = j;
        out->amax = a;
        out->xlast = (jlast >= 0 && jlast < n) ? rc_real(x[jlast]) : 0.0;
    }
}

// 2D-grid solve helpers (pdgstrs's lsum reduction, SRC/pdgstrs_lsum.c): the
// diagonal owner of a block row adds the nslot partial sums its process row
// sent, stored one after another (x[dst + i] += sum_s slot[src + s*len + i]);
// one item per block row, so no two workgroups update the same x.  Rows this
// rank does not own start a sweep at zero (x[dst + i] = 0 for src < 0).
struct SvAdd {
    int64_t dst, src;
    int len, nslot;
};
template <typename T>
__global__ void __launch_bounds__(256) k_sv_add(const SvAdd *items, T *x, const T *slot) {
    const SvAdd it = items[blockIdx.x];
    for (int i = threadIdx.x; i < it.len; i += 256) {
        if (it.src < 0) {
            x[it.dst + i] = S<T>::zero();
            continue;
        }
        T v = x[it.dst + i];
        for (int q = 0; q < it.nslot; ++q) v = S<T>::sub(v, S<T>::neg(slot[it.src + (int64_t)q * it.len + i]));
        x[it.dst + i] = v;
    }
}

// 2D-grid refinement (pdgsrfs with pdgsmv's distributed product,
// SRC/pdgsrfs.c:197-253, SRC/pdgsmv.c): every entry of A lives on the rank
// of its block, so a rank forms partial rows r_p = -A_p x and s_p = |A_p||x|
// from its own entries (rows in CSR over this rank's nonzeros, x replicated).
template <typename T>
__global__ void __launch_bounds__(256)
k_resid_part(const int64_t *rp, const int *rc, const int64_t *re, const T *a, const T *x, T *r,
             double *s, int n) {
    using Sx = S<T>;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T acc = Sx::zero();
    double tmp = 0.0;
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
        const T av = a[re[e]], xv = x[rc[e]];
        acc = Sx::fms(acc, av, xv);
        tmp += Sx::abs1(av) * Sx::abs1(xv);
    }
    r[i] = acc;
    s[i] = tmp;
}
// The partial rows of a block row go to its diagonal owner along the
// process row (nslot consecutive slots each), and the owner finishes them:
// r = b + sum r_p, s = |b| + sum s_p, berr = max |r_i| / s_i with the
// SAFE1 / SAFE2 guards, NaN winning the max as in k_resid.
struct RfRow {
    int64_t fst, src; // first row; first slot (elements) of the block row
    int len, nslot;
};
template <typename T>
__global__ void __launch_bounds__(256)
k_resid_fin(const RfRow *items, const T *b, T *r, const double *s, const T *slot_r,
            const double *slot_s, double safe1, double safe2, unsigned long long *berr) {
    using Sx = S<T>;
    const RfRow it = items[blockIdx.x];
    double mx = 0.0;
    for (int i = threadIdx.x; i < it.len; i += 256) {
        const int64_t row = it.fst + i;
        T rv = Sx::sub(r[row], Sx::neg(b[row]));
        double sv = s[row] + Sx::abs1(b[row]);
        for (int q = 0; q < it.nslot; ++q) {
            rv = Sx::sub(rv, Sx::neg(slot_r[it.src + (int64_t)q * it.len + i]));
            sv += slot_s[it.src + (int64_t)q * it.len + i];
        }
        r[row] = rv;
        const double ra = Sx::abs1(rv);
        double e = 0.0;
        if (sv > safe2) e = ra / sv;
        else if (sv != 0.0) e = (safe1 + ra) / sv;
        mx = (mx != mx || e != e) ? __builtin_nan("") : fmax(mx, e);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off, 64);
        mx = (mx != mx || o != o) ? __builtin_nan("") : fmax(mx, o);
    }
    if ((threadIdx.x & 63) == 0 && !(mx <= 0.0))
        atomicMax(berr, (unsigned long long)__double_as_longlong(mx));
}

// Residual of the iterative refinement (SRC/pdgsrfs.c:209-230) by rows of A
// (CSR index over the CSC values): r = b - A x, s = |A||x| + |b| (abs1 for
// complex, as pzgsrfs), berr = max_i |r_i| / s_i with the SAFE1 / SAFE2
// guards; the max over rows goes through the bit pattern of non-negative
// doubles (monotone as unsigned integers).
template <typename T>
__global__ void __launch_bounds__(256)
k_resid(const int64_t *rp, const int *rc, const int64_t *re, const T *a, const T *x, const T *b,
        T *r, int n, double safe1, double safe2, unsigned long long *berr) {
    using Sx = S<T>;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (i < n) {
        T acc = b[i];
        double tmp = Sx::abs1(b[i]);
        for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
            const T av = a[re[e]], xv = x[rc[e]];
            acc = Sx::fms(acc, av, xv);
            tmp += Sx::abs1(av) * Sx::abs1(xv);
        }
        r[i] = acc;
        const double ra = Sx::abs1(acc);
        if (tmp > safe2) s = ra / tmp;
        else if (tmp != 0.0) s = (safe1 + ra) / tmp;
    }
    // NaN must win the max, as SUPERLU_MAX lets it through to berr
    // (SRC/pdgsrfs.c:222-226): fmax alone would drop it.  A NaN's bit
    // pattern is above +Inf's as an unsigned integer, so atomicMax keeps it.
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(s, off, 64);
        s = (s != s || o != o) ? __builtin_nan("") : fmax(s, o);
    }
    if ((threadIdx.x & 63) == 0 && !(s <= 0.0))
        atomicMax(berr, (unsigned long long)__double_as_longlong(s));
}

template <typename T> __global__ void __launch_bounds__(256) k_axpy1(T *x, const T *dx, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = S<T>::sub(x[i], S<T>::neg(dx[i]));
}

} // namespace slu
