// MI355X numeric factorization engine: plan construction (host), level-
// synchronous execution of the batched kernels in kernels.h, RCCL panel
// exchange for 2D process grids, and the engine C API of include/slu_mi355x.h.
//
// Algorithm (what replaces the k-loop of SRC/pdgstrf.c:1108-1756):
//   The supernodal dependency DAG (k -> ib for every block L(ib,k), k -> jb
//   for every block U(k,jb)) is levelled once at plan time.  Supernodes of one
//   level are independent, so for each level every rank launches
//     1. k_diag_lu(_blk) on the diagonal blocks of the level it owns
//        (SRC/pdgstrf2.c:213-269),
//     2. (grids) one grouped broadcast of the factored diagonal blocks (+ their
//        inverted 32x32 diagonal sub-blocks) along process rows and columns
//        (SRC/pdgstrf2.c:280-289 sends U(k,k) down the column),
//     3. k_trsm_* on every local L / U panel block of the level
//        (SRC/pdgstrf2.c:302-355, 843-887),
//     4. (grids) one grouped broadcast of the level's L panels along process
//        rows and U panels along process columns (SRC/pdgstrf.c:1020-1729),
//     5. k_schur(_big) over every (L row tile x U column tile) of every
//        supernode of the level, scattering straight into the destination
//        blocks (SRC/dSchCompUdt-2Ddynamic.c, SRC/dscatter.c:110-277).
//   The set of updates and the per-element arithmetic are those of the
//   reference; only the order in which independent updates are applied
//   differs (the reference orders them by its static schedule,
//   SRC/dstatic_schedule.c:39).  Two supernodes of one level that update the
//   same destination block use atomic fp adds for those blocks.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include <type_traits>
#include <condition_variable>
#include <functional>
#include <thread>
#include <vector>

#include "common.h"
#include "devbuf.h"
#include "xport.h"
#include "kernels.h"
#include "diag_strips.h"
#include "diag_wave.h"
#include "fill.h"
#include "solve.h"
#include "solve_block.h"
#include "solve_block_t.h"
#include "solve_block_inv.h"
#include "refine_d2.h"
#include "refine_block.h"
#include "hostio.h"
#include "amalg.h"
#include "amalg_dev.h"
#include "watchdog.h"
#include "slu_mi355x.h"

using std::vector;

namespace slu {

static thread_local std::string g_last_error;
void set_last_error(const std::string &s) { g_last_error = s; }

struct LevelRange {
    int diag_off = 0, diag_n = 0;
    int tl_off = 0, tl_n = 0;
    int tu_off = 0, tu_n = 0;
    int k_off = 0, k_n = 0;
    int tile_off = 0, tile_n = 0;
    int big_off = 0, big_n = 0; // 128x128 Schur tiles (first bigc_n: critical)
    int bigc_n = 0, tilec_n = 0; // critical tiles (destinations in the next level's panels)
    int df_off = 0, df_n = 0;   // fast diag items
    int df_maxw = 0;            // widest of them
    int tf_maxw = 0;            // widest supernode of the fast L / U panel TRSM items
    int lf_off = 0, lf_n = 0;   // fast L-panel TRSM items
    int uf_off = 0, uf_n = 0;   // fast U-panel TRSM items
    int dc_off = 0, dc_n = 0;   // diag-package copy items (2D grids)
    int pc_off = 0, pc_n = 0;   // panel-section copy items (2D grids)
    int ds_off = 0, ds_n = 0;   // diag-package broadcasts
    int ps_off = 0, ps_n = 0;   // panel broadcasts
    double schur_flops = 0, big_flops = 0;
    int atomic_tiles = 0; // tiles of supernodes whose destinations collide within the level
    int fused_n = 0;      // big tiles that carry a deferred tile of the level below as a first K segment
    int mapped_n = 0;     // the same of mapped pairs: the far part of the level below through a row map
    bool big = false;
    // 2D grids: the level's panel exchange in nch chunks (Plan::pchunks).
    // Chunk c = row group c of every L panel and column group c of every U
    // panel; prefix offsets (relative to lf_off, uf_off, pc_off, ps_off and,
    // for the tiles, to the critical / rest parts of big_off / tile_off) of
    // each chunk's TRSM items, pack copies, sections and Schur tiles (a tile
    // waits for the chunks of its rows and of its columns: max of the two)
    static constexpr int NCHM = 4;
    int nch = 1;
    int lf_o[NCHM + 1] = {}, uf_o[NCHM + 1] = {}, pc_o[NCHM + 1] = {}, ps_o[NCHM + 1] = {};
    int bc_o[NCHM + 1] = {}, br_o[NCHM + 1] = {}, sc_o[NCHM + 1] = {}, sr_o[NCHM + 1] = {};
};

// one broadcast of a contiguous section of a device arena
struct Sec {
    int g, root, arena; // arena 0: diag packages, 1: panels
    i64 off, cnt;       // in elements; off < 0: not received here
    uint32_t mask;      // group ranks that receive the section
};

// 3D grids: one chunk (<= ZR_CHUNK values) of a contiguous range of this
// rank's L (arr 0) or U (arr 1) values -- a block column L(:,k) or block row
// U(k,:) of an ancestor supernode -- zeroed, packed into the exchange
// buffer, added from it (ancestor reduction, SRC/pd3dcomm.c:704-730: alpha =
// beta = 1) or copied from it (gather of the factored forests,
// SRC/pd3dcomm.c:733-760: alpha = 0).  HBM-bound copies, lanes over values.
struct ZRange {
    int64_t off, boff;
    int32_t len, arr;
};
enum { ZR_ZERO = 0, ZR_PACK = 1, ZR_ADD = 2, ZR_COPY = 3 };
constexpr int ZR_CHUNK = 1 << 16;

template <typename T>
__global__ void __launch_bounds__(256) k_zranges(const ZRange *r, T *L, T *U, T *buf, int op) {
    const ZRange z = r[blockIdx.x];
    T *v = (z.arr ? U : L) + z.off;
    T *b = buf + z.boff;
    using Sx = S<T>;
    for (int i = threadIdx.x; i < z.len; i += 256) {
        if (op == ZR_ZERO) v[i] = Sx::zero();
        else if (op == ZR_PACK) b[i] = v[i];
        else if (op == ZR_ADD) v[i] = Sx::sub(v[i], Sx::neg(b[i]));
        else v[i] = b[i];
    }
}

// Event timing of one factor() (opts.timing: 0 records nothing, 1 the totals
// in the stats, 2 also a per-level table on stderr).  A span is a pair of
// events around a step on its stream.
struct FactorTimer {
    int timing = 0;
    vector<hipEvent_t> ev;
    // kind: 0 diag, 1 trsm, 2 schur (128x128 tiles), 3 schur (64x64), 4 comm
    struct Span { int a, b, kind, level; };
    vector<Span> spans;
    int cur_level = 0, e_start = -1, e_end = -1, e_ph = -1, zstart = -1;
    vector<int> lvl_end;
    vector<std::array<int, 3>> zmarks; // (phase start, phase end, reduction end) events
    FactorTimer() = default;
    FactorTimer(const FactorTimer &) = delete;
    FactorTimer &operator=(const FactorTimer &) = delete;
    ~FactorTimer() { reset(0); }
    void reset(int timing_) {
        for (auto e : ev) (void)hipEventDestroy(e);
        ev.clear();
        spans.clear();
        lvl_end.clear();
        zmarks.clear();
        timing = timing_;
    }
    int mark(hipStream_t st) {
        if (!timing) return -1;
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(e, st));
        ev.push_back(e);
        return (int)ev.size() - 1;
    }
    template <typename F> void span(int kind, hipStream_t st, F &&fn) {
        const int a = mark(st);
        fn();
        if (timing) spans.push_back({a, mark(st), kind, cur_level});
    }
    void start(hipStream_t st) { e_start = zstart = mark(st); }
    void end(hipStream_t st) { e_end = mark(st); }
    void level(int L) { cur_level = L; }
    void level_end(hipStream_t st) {
        if (timing >= 2) lvl_end.push_back(mark(st));
    }
    // 3D grids: my phase's levels are done / its ancestor reduction is done
    void phase_end(hipStream_t st) { e_ph = mark(st); }
    void reduce_end(hipStream_t st) {
        if (!timing) return;
        const int e_red = mark(st);
        zmarks.push_back({zstart, e_ph, e_red});
        zstart = e_red;
    }
    float ms(int a, int b) const {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, ev[a], ev[b]));
        return t;
    }
    // after the streams are synchronised: the totals into stats, the table
    void finish(slu_plan_stats &stats, const vector<LevelRange> &levels, const vector<vector<int>> &bylev, int iam) {
        if (!timing) return;
        stats.t_total_ms = ms(e_start, e_end);
        stats.t_diag_ms = stats.t_trsm_ms = stats.t_schur_ms = stats.t_schur_big_ms = 0;
        stats.t_comm_ms = 0;
        stats.schur_big_flops = 0;
        vector<std::array<double, 5>> t(levels.size(), {0, 0, 0, 0, 0}); // per level and kind
        for (auto &s : spans) {
            const float d = ms(s.a, s.b);
            t[s.level][s.kind] += d;
            if (s.kind == 0) stats.t_diag_ms += d;
            else if (s.kind == 1) stats.t_trsm_ms += d;
            else if (s.kind == 4) stats.t_comm_ms += d;
            else {
                stats.t_schur_ms += d;
                if (s.kind == 2) stats.t_schur_big_ms += d;
            }
        }
        for (auto &R : levels) stats.schur_big_flops += R.big_flops;
        for (int i = 0; i < 8; ++i) stats.t_phase_ms[i] = 0;
        stats.t_zreduce_ms = 0;
        for (size_t i = 0; i < zmarks.size() && i < 8; ++i) {
            stats.t_phase_ms[i] = ms(zmarks[i][0], zmarks[i][1]);
            stats.t_zreduce_ms += ms(zmarks[i][1], zmarks[i][2]);
        }
        if (timing >= 2) { // per-level breakdown (stderr)
            fprintf(stderr, "[slu rank %d] lvl nsup diag trsm big small atomic  GFLOP  diag_ms trsm_ms big_ms small_ms comm_ms  TF/s wall_ms mapped fused\n", iam);
            for (size_t L = 0; L < levels.size(); ++L) {
                const LevelRange &R = levels[L];
                double sch = t[L][2] + t[L][3];
                const float wall = ms(L ? lvl_end[L - 1] : e_start, lvl_end[L]);
                fprintf(stderr, "[slu rank %d] %3zu %5zu %4d %5d %5d %5d %6d %7.2f %8.3f %7.3f %7.3f %7.3f %7.3f %6.2f %7.3f %5d %5d\n",
                        iam, L, bylev[L].size(), R.diag_n + R.df_n, R.lf_n + R.uf_n + R.tl_n + R.tu_n,
                        R.big_n, R.tile_n, R.atomic_tiles, R.schur_flops / 1e9, t[L][0], t[L][1], t[L][2], t[L][3],
                        t[L][4], sch > 0 ? R.schur_flops / sch / 1e9 : 0.0, (double)wall, R.mapped_n, R.fused_n);
            }
        }
        reset(0);
    }
};

// Device time of a stretch of one stream's work: two events that live as long
// as the object, whichever way its scope is left.  start / stop only record;
// ms() waits for the second event.
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventTimer() {
        HIPCHK(hipEventCreate(&e0));
        const hipError_t err = hipEventCreate(&e1);
        if (err != hipSuccess) (void)hipEventDestroy(e0); // no destructor after a throwing constructor
        HIPCHK(err);
    }
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer() {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    void start(hipStream_t st) { HIPCHK(hipEventRecord(e0, st)); }
    void stop(hipStream_t st) { HIPCHK(hipEventRecord(e1, st)); }
    float ms() {
        float t = 0;
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        return t;
    }
};

// Slot of the overlapped D2H's pinned-slot pipeline (Plan::run_d2h);
// SLU_D2H_SLOT_KB overrides it: tests use tiny slots so that blocks split
// across fills.
inline i64 d2h_slot_bytes() {
    const char *e = getenv("SLU_D2H_SLOT_KB");
    return e ? std::max<i64>(16, atoll(e)) << 10 : 128ll << 20;
}

struct D2HFill {
    int level;          // all blocks final after ev_pan[level]
    int seg_off, seg_n; // PushSeg range
    int hs_off, hs_n;   // HostSeg range
    i64 bytes;
};
struct HostSeg {
    char *host;
    i64 off, bytes; // in the slot
};
// The fills of the overlapped D2H: the plan enumerates its (device range,
// host pointer) pairs level by level, this packs them into slots.
struct D2HFills {
    i64 slot = d2h_slot_bytes(), min_fill = slot / 4;
    static constexpr i64 PIECE = 1ll << 20;
    vector<D2HFill> fills;
    vector<PushSeg> h_push;
    vector<HostSeg> h_unpack;
    DevBuf<PushSeg> d_push;
    i64 fb = 0; // bytes in the open fill
    int seg0 = 0, hs0 = 0;
    void close(int L) {
        if (fb == 0) return;
        fills.push_back({L, seg0, (int)h_push.size() - seg0, hs0, (int)h_unpack.size() - hs0, fb});
        seg0 = (int)h_push.size();
        hs0 = (int)h_unpack.size();
        fb = 0;
    }
    void add(const char *dev, char *host, i64 bytes, int L) {
        i64 done = 0;
        while (done < bytes) {
            const i64 take = std::min(bytes - done, slot - fb);
            for (i64 o = 0; o < take; o += PIECE)
                h_push.push_back({dev + done + o, fb + o, (int)std::min(PIECE, take - o)});
            // host pieces of <= 4 MB so the unpack threads balance
            for (i64 o = 0; o < take; o += 4 * PIECE)
                h_unpack.push_back({host + done + o, fb + o, std::min(4 * PIECE, take - o)});
            fb += (take + 15) & ~(i64)15; // 16-byte aligned slot offsets
            done += take;
            if (fb >= slot) close(L);
        }
    }
    void end_level(int L, bool last) {
        if (fb >= min_fill || last) close(L);
    }
    void finish() { d_push.upload(h_push.empty() ? vector<PushSeg>(1) : h_push); }
};

struct PlanBase {
    virtual ~PlanBase() = default;
    virtual void upload() = 0;
    virtual void factor(double anorm, int *info, int *tiny) = 0;
    virtual void download() = 0;
    virtual void snapshot() = 0;
    virtual void restore() = 0;
    virtual void sync() = 0;
    virtual void set_timing(int timing, int serial) = 0;
    virtual void solve(void *b, int64_t ldb, int nrhs) = 0;
    // L U X = B, SvbNr columns per pass over the factors on MFMA (1x1 plans;
    // solve_block.h); passes, launches and device time of the call in svb_*
    virtual void solve_block(void *b, int64_t ldb, int nrhs, int on_device) = 0;
    int svb_passes = 0;
    int64_t svb_launches = 0;
    double svb_ms = 0;
    // DiagInv for the block sweep (1x1 plans; solve_block_inv.h): the mode,
    // its state, and supernode k's first column, width and inverse block
    virtual void set_diag_inv(int on) = 0;
    virtual void diag_inv_info(int *on, int *valid, int64_t *bytes, int *computes, double *ms) = 0;
    virtual void diag_inv_block(int k, int *fst, int *w, void *out, int64_t ldo) = 0;
    virtual void set_a_pattern(int64_t ncol, const int64_t *xa, const int64_t *asub) = 0;
    virtual void fill_a(const void *a, int on_device) = 0;
    virtual void refine(const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) = 0;
    // B^T / B^H on the same factors (1x1 plans; solve.h), trans = SLU_TRANS / SLU_CONJ
    virtual void solve_t(int trans, void *b, int64_t ldb, int nrhs) = 0;
    virtual void refine_t(int trans, const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) = 0;
    // reciprocal condition estimate; sweeps and device time of the call in rc_*
    virtual void rcond(int norm, double anorm, double *rc) = 0;
    int rc_sweeps = 0;
    double rc_ms = 0;
    // fp32 plans: fp64 values of A, fp64 residual and update (refine_d2.h)
    virtual void fill_a_d2(const double *a, int on_device) = 0;
    virtual void refine_d2(const double *b, double *x, int64_t ld, int nrhs, double *berr, int *steps) = 0;
    // refine / refine_d2 on SvbNr columns per pass (1x1 plans; refine_block.h);
    // passes, block sweeps, residual launches and device time of the call in rfb_*
    virtual void refine_block(const void *b, void *x, int64_t ld, int nrhs, int on_device, double *berr,
                              int *steps) = 0;
    virtual void refine_block_d2(const double *b, double *x, int64_t ld, int nrhs, int on_device, double *berr,
                                 int *steps) = 0;
    int rfb_passes = 0, rfb_sweeps = 0, rfb_resids = 0;
    double rfb_ms = 0;
    // solve_block / refine_block with B^T / B^H (solve_block_t.h); svb_* and rfb_* as above
    virtual void solve_block_t(int trans, void *b, int64_t ldb, int nrhs, int on_device) = 0;
    virtual void refine_block_t(int trans, const void *b, void *x, int64_t ld, int nrhs, int on_device,
                                double *berr, int *steps) = 0;
    virtual void check_exchange(int64_t *nsec, int64_t *nbytes) = 0;
    virtual void gather_layers() { throw Error("gather_layers: not a 3D plan"); }
    virtual void adopt_factors() = 0; // upload host values that are already factors
    slu_plan_stats stats{};
    // kernel launches of the last factor() by dispatch path (host-side counts
    // at the launch sites, slu_plan_path_counts; the order is the ABI):
    // the diagonal kernels, k_trsm_reg per width and PF form, k_trsm_blk,
    // k_trsm_l / k_trsm_u, the Schur kernels, the KInfo's of K-split updates,
    // and the plan's chained pairs with the tile pairs they fuse (SLU_SCHUR_PAIR)
    enum PathCount {
        PC_DIAG_GENERIC, PC_DIAG_F, PC_DIAG_F_SMALL, PC_DIAG_WAVE32, PC_DIAG_WAVE64, PC_DIAG_STRIPS,
        PC_TRSM_REG64_PF, PC_TRSM_REG64_NOPF, PC_TRSM_REG128_PF, PC_TRSM_REG128_NOPF,
        PC_TRSM_REG256_PF, PC_TRSM_REG256_NOPF, PC_TRSM_BLK, PC_TRSM_GENERIC,
        PC_SCHUR_BIG, PC_SCHUR_SMALL, PC_KSPLIT_KINFOS, PC_SCHUR_PAIRS, PC_SCHUR_FUSED_TILES,
        PC_SCHUR_MAP_PAIRS, PC_SCHUR_MAP_FUSED_TILES, PC_N
    };
    int64_t path_counts[PC_N] = {};
};

// One rank's plan for value type T (double / float / zc) over the host
// LUstruct layout LocalLU / LUS.
//
// 2D grid (SRC/superlu_defs.h:260-270): block (I,J) lives on rank
// (I mod Pr, J mod Pc).  For supernode k, rank (r,c) needs
//   * L(:,k) restricted to process row r   -- held by (r, k mod Pc),
//   * U(k,:) restricted to process column c -- held by (k mod Pr, c),
//   * the factored diagonal block           -- held by (k mod Pr, k mod Pc)
//     when r == k mod Pr (U-panel TRSM) or c == k mod Pc (L-panel TRSM).
// The plan exchanges the index arrays once (row / column all-gathers), levels
// the global dependency DAG identically on every rank, and lays out per-level
// broadcast sections so that a level is: diag LU -> diag-package broadcast ->
// panel TRSMs -> L-panel (row) / U-panel (column) broadcasts -> Schur update.
template <typename T, typename HT, typename LocalLU, typename LUS>
struct Plan : PlanBase {
    using value_type = T;
    using host_type = HT;
    using local_type = LocalLU;
    using lus_type = LUS;
    // ---- problem
    int n = 0, nsupers = 0, Pr = 1, Pc = 1, iam = 0, myrow = 0, mycol = 0;
    slu_comm *comm = nullptr;
    slu_engine_opts opts{};
    LUS *LU = nullptr;
    vector<i64> xsup;
    int nlc = 0, nlr = 0;
    hipStream_t stream = nullptr;  // Schur updates that are off the critical path
    hipStream_t pstream = nullptr; // panels, exchanges, critical Schur tiles
    hipStream_t ustream = nullptr; // the U panels' TRSM beside the L panels' (launch_trsm_fast)
    // 2D grids: the exchanges on a stream of their own, between events from
    // the panel stream (packed sections) and to the panel and Schur streams
    // (received chunks): the next chunk's TRSM runs beside the current
    // chunk's transfer, a chunk's Schur tiles start when it is in
    hipStream_t cstream = nullptr;
    hipEvent_t ev_pk = nullptr, ev_dx = nullptr, ev_cx[LevelRange::NCHM] = {};
    vector<hipEvent_t> ev_pan, ev_rest; // per level
    hipEvent_t ev_start = nullptr, ev_pend = nullptr, ev_tu0 = nullptr, ev_tu1 = nullptr;
    bool xmode = false; // 2D grid with exchanges
    Xport X;

    // ---- local storage layout (destinations)
    vector<i64> lval_off, uval_off; // per local column / row, -1 if empty
    vector<int> lval_ld;            // nsupr per local column
    i64 lval_total = 0, uval_total = 0;
    bool l_contig = false, u_contig = false;
    vector<LBlk> lblk;
    vector<int> lblk_ib;
    vector<int> lcol_first, lcol_nblk; // per local column
    RawVec<int> lmap;
    vector<UBlk> ublk;
    vector<int> ublk_jb;
    vector<int> urow_first, urow_nblk;
    RawVec<i64> ucol_voff;
    RawVec<int> ucol_fst;

    // ---- panels of every supernode as seen from this rank
    vector<const int_t *> lidx; // L(:,k) on my process row (reference index format) or null
    vector<const int_t *> uidx; // U(k,:) on my process column or null
    vector<vector<i64>> xL, xU; // received index blobs (own the remote lidx/uidx)
    vector<i64> lpos, upos;     // remote panel value offsets in d_pan (-1: local / none)
    // Chunked panel exchange (2D grids, SLU_PANEL_CHUNKS, default 4; 1 =
    // one exchange per level): supernode k's L panel rows on my process row
    // in groups of lgsz[k] rows (a multiple of 128, so every Schur tile and
    // TRSM slab lies in one group), its U panel columns on my process column
    // in groups of ucsz[k] columns; lgpos / ugpos: each received group's
    // offset in d_pan (an L group column-major with ld = its rows); ugrun:
    // the U panel's value offset at each group's first column
    static constexpr int NCHM = LevelRange::NCHM;
    int pchunks = 1;
    vector<int> lgsz, ucsz, ucols;
    vector<std::array<i64, NCHM>> lgpos, ugpos, ugrun;
    int ngroups(int len, int gsz) const { return len > 0 ? (len + gsz - 1) / gsz : 0; }
    int group_size(int len) const {
        const int per = (len + pchunks - 1) / std::max(pchunks, 1);
        return std::max(128, (per + 127) / 128 * 128);
    }
    vector<i64> pkg;            // diag package offset in d_dpk (2D grids), -1 none
    vector<i64> dscr;           // 1x1: Dinv offset in the per-level scratch
    i64 dpk_total = 0, pan_total = 0, dscr_max = 0;

    // ---- schedule
    vector<int> level_of;
    vector<vector<int>> bylev;
    vector<LevelRange> levels;

    // ---- 3D grids (pdgstrf3d, SRC/pdgstrf3d.c:121-348).  Pz = 2^(maxlvl-1)
    // layers, each a Pr x Pc grid holding the whole LUstruct; the supernodal
    // etree is cut into 2^maxlvl - 1 forests (heap order: 0 = the top
    // ancestors, 2t+1 / 2t+2 the two halves below forest t).  Layer z factors
    // its leaf forest, then (phase p >= 1, layers with z % 2^p == 0) the
    // forest above, after adding the partner layer's partial updates of every
    // ancestor block (reduction at the end of phase p-1 between z and
    // z + 2^(p-1)); only the layer that factors an ancestor forest starts it
    // from A's values, the others from zero (SRC/pd3dcomm.c:754-771).
    bool zmode = false;
    int npdep = 1, zl = 0, maxlvl = 1, my_last = 0;
    vector<int> forest_of, phase_of; // per supernode; phase -1: not factored here
    vector<int> phase_lv;            // my phase p = levels [phase_lv[p], phase_lv[p+1])
    vector<int> zr_off;              // zero ranges [zr_off[0], zr_off[1]); reduction p: [zr_off[p+1], zr_off[p+2])
    vector<i64> zr_cnt;              // values exchanged by reduction p
    vector<ZRange> zr;
    DevBuf<ZRange> d_zr;
    DevBuf<T> d_zbuf;
    vector<i64> uval_len;
    double zbytes = 0; // reduction bytes sent + received per factorization
    // SLU_3D_SOLO=1 (measurement hook, tools/model3d.py): one layer alone on
    // a GPU -- the reductions pack / add but exchange nothing, so each
    // layer's phase times can be taken without the others running beside it
    bool zsolo = env_int("SLU_3D_SOLO", 0) == 1;
    vector<DiagItem<T>> diag_items;
    vector<TrsmLItem<T>> tl_items;
    vector<TrsmUItem<T>> tu_items;
    vector<KInfo<T>> kinfos;
    vector<TileItem> tiles, tiles_big;

    vector<DiagItemF<T>> df_items;
    vector<TrsmItemF<T>> lf_items, uf_items;
    vector<CopyItem<T>> dcopy, pcopy;
    vector<Sec> dsecs, psecs;
    // per-k panel arrays (device copies referenced by KInfo / TrsmUItem)
    RawVec<int> h_rg, h_ra, h_cg, h_cb, h_pair, h_ct0;
    RawVec<i64> h_cvoff;

    // ---- device
    DevBuf<T> d_L, d_U, d_dpk, d_pan, d_dinv;
    DevBuf<LBlk> d_lblk;
    DevBuf<int> d_lmap;
    DevBuf<UBlk> d_ublk;
    DevBuf<i64> d_ucol_voff;
    DevBuf<int> d_ucol_fst;
    DevBuf<DiagItem<T>> d_diag;
    DevBuf<TrsmLItem<T>> d_tl;
    DevBuf<TrsmUItem<T>> d_tu;
    DevBuf<KInfo<T>> d_kinfo;
    DevBuf<TileItem> d_tiles, d_tiles_big;
    DevBuf<DiagItemF<T>> d_df;
    DevBuf<TrsmItemF<T>> d_lf, d_uf;
    DevBuf<CopyItem<T>> d_dcopy, d_pcopy;
    DevBuf<int> d_rg, d_ra, d_cg, d_cb, d_pair, d_ct0;
    DevBuf<DRec> d_prec;
    DevBuf<i64> d_cvoff;
    DevBuf<int> d_counters; // [0] tiny pivots, [1] k_diag_strips hand-off timeout
    DevBuf<unsigned> d_dsflags; // k_diag_strips: per fast diag item, DS_NFLAGS strip flags (A, B)
    unsigned ds_epoch = 0;      // ... set to the factorization's epoch when a strip is published
    DevBuf<int> d_zpiv;     // per supernode: max zero-pivot column + 1
    DevBuf<i64> d_info;     // 2D grids: all-gather of the per-rank info

    static constexpr bool cplx = sizeof(T) == 16;
    static constexpr int PW = PWOf<T>::v;

    int W(i64 k) const { return (int)(xsup[k + 1] - xsup[k]); }
    bool fast_w(int w) const { return w <= FAST_MAXW; }
    i64 dinv_len(int w) const { return fast_w(w) ? 2 * (i64)((w + PW - 1) / PW) * PW * PW : 0; }

    // pre (optional): the L / U value storage allocated ahead by the caller
    // (an amalgamated plan allocates it beside its analysis: fresh HBM costs
    // ~28 ms per GB), adopted when its sizes are this layout's
    Plan(LUS *lu, int n_, int nprow, int npcol, int iam_, slu_comm *c,
         const slu_engine_opts *o, DevBuf<T> *pre = nullptr) {
        LU = lu;
        n = n_;
        Pr = nprow;
        Pc = npcol;
        iam = iam_;
        myrow = iam / Pc;
        mycol = iam % Pc;
        comm = c;
        if (o) opts = *o;
        xmode = Pr * Pc > 1;
        if (xmode) {
            pchunks = std::max(1, std::min(NCHM, env_int("SLU_PANEL_CHUNKS", 4)));
        }
        SLU_REQUIRE(!xmode || (comm && (comm->world || comm->host_fn || comm->host_p2p)),
                    "a %dx%d grid needs a communicator (slu_comm_create)", Pr, Pc);
        zmode = comm && comm->npdep > 1;
        if (zmode) {
            npdep = comm->npdep;
            zl = comm->zlayer;
            while ((1 << (maxlvl - 1)) < npdep) ++maxlvl;
            SLU_REQUIRE(comm->zcomm || comm->host_p2p,
                        "a 3D grid needs RCCL (slu_comm_create3d) or the point-to-point host transport");
            SLU_REQUIRE(!(o && o->overlap_download), "3D grids: no overlapped download (factors are spread over the layers)");
        }
        if (xmode)
            SLU_REQUIRE(comm->nprow == Pr && comm->npcol == Pc && comm->iam == iam,
                        "communicator is for a %dx%d grid rank %d, plan for %dx%d rank %d",
                        comm->nprow, comm->npcol, comm->iam, Pr, Pc, iam);
        dry = opts.schedule_only != 0;
        if (dry)
            SLU_REQUIRE(!xmode || comm->host_p2p,
                        "a schedule-only plan of a grid needs the point-to-point host transport");
        X.c = comm;
        X.host_mem = dry;
        if (dry) {
            // host only (no HIP call): the layout, the index exchange, the
            // levels and the per-level exchange sections, for
            // slu_plan_check_exchange
            int_t *hx = LU->Glu_persist->xsup;
            nsupers = (int)(LU->Glu_persist->supno[n - 1] + 1);
            xsup.assign(hx, hx + nsupers + 1);
            nlc = (nsupers + Pc - 1) / Pc;
            nlr = (nsupers + Pr - 1) / Pr;
            value_layout();
            build_local();
            exchange_index();
            exchange_needs();
            compute_levels();
            layout_values();
            if (zmode) build_zranges(false);
            return;
        }
        if (comm) HIPCHK(hipSetDevice(comm->device));
        // the panel stream carries the critical path (critical Schur tiles,
        // next level's diag LU / TRSM / exchanges): higher priority, so its
        // workgroups are dispatched ahead of the bulk Schur update's
        // (created on a helper thread beside the host-side plan build --
        // the first streams of a process take ~35 ms -- and joined before
        // their first use)
        HelperThread stream_thread;
        stream_thread.start(device(), [this] {
            int prio_lo = 0, prio_hi = 0;
            const auto ts0 = std::chrono::steady_clock::now();
            HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
            HIPCHK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio_lo));
            HIPCHK(hipStreamCreateWithPriority(&pstream, hipStreamNonBlocking, prio_hi));
            HIPCHK(hipStreamCreateWithPriority(&ustream, hipStreamNonBlocking, prio_hi));
            if (xmode) HIPCHK(hipStreamCreateWithPriority(&cstream, hipStreamNonBlocking, prio_hi));
            if (getenv("SLU_PROFILE_PLAN"))
                fprintf(stderr, "[slu plan %d] streams               %6.1f ms (helper thread)\n", iam,
                        ms_since(ts0));
        });
        auto join_streams = [&] {
            if (!stream_thread.running()) return;
            stream_thread.join();
            X.s = pstream;
        };
        int_t *hx = LU->Glu_persist->xsup;
        nsupers = (int)(LU->Glu_persist->supno[n - 1] + 1);
        xsup.assign(hx, hx + nsupers + 1);
        nlc = (nsupers + Pc - 1) / Pc;
        nlr = (nsupers + Pr - 1) / Pr;
        for (int k = 0; k < nsupers; ++k)
            SLU_REQUIRE(W(k) <= 512, "supernode %d has %d columns (> MAX_SUPER_SIZE 512)", k, W(k));
        // k_schur_big reads up to a panel width before a U segment and 127
        // rows past an L column, unclamped, inside the buffers' guards
        static_assert(SB_UGUARD >= 512 + 128, "guards too small for the widest panel");
        const auto t0 = std::chrono::steady_clock::now();
        prof = getenv("SLU_PROFILE_PLAN") != nullptr;
        tprev = t0;
        value_layout();
        if (pre && pre[0].n == (size_t)std::max<i64>(lval_total, 1) && pre[0].guard == SB_UGUARD &&
            pre[1].n == (size_t)std::max<i64>(uval_total, 1) && pre[1].guard == SB_UGUARD) {
            d_L.swap(pre[0]);
            d_U.swap(pre[1]);
        } else {
            d_L.alloc_guarded(std::max<i64>(lval_total, 1), SB_UGUARD);
            d_U.alloc_guarded(std::max<i64>(uval_total, 1), SB_UGUARD);
        }
        tick("layout + alloc");
        if (opts.overlap_upload || xmode || zmode) join_streams();
        if (opts.overlap_upload) {
            // the H2D copy of the values runs beside the rest of the plan
            // build (index exchange, levels, schedule, device tables)
            up_thread.start(device(), [this] { upload_values(); });
        }
        if (opts.overlap_download) {
            // the pinned D2H slots (hipHostMalloc, ~0.1 s the first time in a
            // process) are allocated beside the plan build too
            pin_thread.start(device(), [this] {
                // get() frees slots of another size: never while a
                // run_d2h (which holds `use`) still copies through them
                std::lock_guard<std::mutex> in_use(pinned_pool(1).use);
                pinned_pool(1).get(D2H_NS, d2h.slot);
            });
        }
        // (an exception from here on: the helper threads are joined by their
        // destructors, stream_thread's first)
        build_local();
        tick("build_local");
        exchange_index();
        exchange_needs();
        tick("exchange_index");
        compute_levels();
        tick("compute_levels");
        layout_values();
        tick("layout_values");
        if (zmode) build_zranges(true);
        build_pairs();
        build_schedule();
        if (prof)
            fprintf(stderr, "[slu plan %d]   (add_supernode %.1f ms, merge + atomics %.1f ms: "
                            "resize %.1f, copy %.1f, tiles %.1f)\n",
                    iam, t_addsn, t_merge, t_resize, t_put, t_tiles);
        if (prof && n_pairs) {
            double bigf = 0;
            for (auto &R : levels) bigf += R.big_flops;
            fprintf(stderr, "[slu plan %d]   (chained pairs %lld, fused tiles %lld, %.1f %% of the big-tile flops)\n", iam,
                    (long long)n_pairs, (long long)n_fused_tiles, bigf > 0 ? 100.0 * fused_flops / bigf : 0.0);
        }
        if (prof && n_map_pairs) {
            double bigf = 0;
            for (auto &R : levels) bigf += R.big_flops;
            fprintf(stderr, "[slu plan %d]   (mapped pairs %lld, fused tiles %lld, %.3f GFLOP, %.1f %% of the big-tile flops; "
                            "first-segment work on whole tiles %.1f %% above the far parts')\n", iam,
                    (long long)n_map_pairs, (long long)n_map_fused_tiles, map_fused_flops / 1e9,
                    bigf > 0 ? 100.0 * map_fused_flops / bigf : 0.0,
                    map_useful > 0 ? 100.0 * (map_work / map_useful - 1.0) : 0.0);
        }
        tick("build_schedule");
        join_streams();
        build_device();
        tick("build_device");
        build_d2h();
        tick("build_d2h");
        stats.t_plan_ms = ms_since(t0);
    }

    bool dry = false;  // schedule-only plan (opts.schedule_only): no device state

    // Replays every level's exchange phases of factor() -- the diagonal
    // packages, then the panels, issue() for issue() -- through the
    // transport on host arenas.  Each section carries bytes derived from
    // (level, group, root, mask, position), written by its root and checked
    // by every receiver, so a section that goes to the wrong rank, in the
    // wrong order or with the wrong size fails (or, with a missing send,
    // hangs) here instead of on the RCCL node.
    void check_exchange(int64_t *nsec, int64_t *nbytes) override {
        SLU_REQUIRE(dry, "check_exchange needs a schedule-only plan");
        vector<unsigned char> hd((size_t)std::max<i64>(dpk_total, 1) * sizeof(T)),
            hp((size_t)std::max<i64>(pan_total, 1) * sizeof(T));
        // bytes of the k-th section of root rank gr in phase ph of level L
        // (an owner's diagonal package goes to its column and its row from
        // one buffer, so the group is not part of it)
        auto pat = [](size_t L, int ph, int gr, int k, size_t i) {
            uint64_t h = (uint64_t)(L * 2 + ph) * 0x9E3779B97F4A7C15ull ^
                         (uint64_t)(gr * 1031 + k) * 0xBF58476D1CE4E5B9ull ^
                         (uint64_t)i * 0xD6E8FEB86659FD93ull;
            return (unsigned char)(h ^ (h >> 29) ^ (h >> 43));
        };
        auto root_rank = [&](const Sec &sc) { // global rank of the section's root
            return sc.g == G_ROW ? myrow * Pc + sc.root : sc.root * Pc + mycol;
        };
        i64 ns = 0, nb = 0;
        const int nzp = zmode ? my_last + 1 : 1;
        for (int zp = 0; zp < nzp; ++zp) {
        const size_t L0 = zmode ? phase_lv[zp] : 0, L1 = zmode ? phase_lv[zp + 1] : levels.size();
        for (size_t L = L0; L < L1; ++L) {
            const LevelRange &R = levels[L];
            // phase 0: the diagonal packages; phase 1: the panels, one flush
            // per chunk as factor() issues them
            for (int ph = 0; ph < 2; ++ph) {
                const vector<Sec> &secs = ph ? psecs : dsecs;
                const int off = ph ? R.ps_off : R.ds_off, cnt = ph ? R.ps_n : R.ds_n;
                unsigned char *arena = ph ? hp.data() : hd.data();
                // k = position among the level phase's sections of (group, root)
                vector<int> kth(cnt);
                {
                    std::map<std::pair<int, int>, int> seen;
                    for (int i = 0; i < cnt; ++i) kth[i] = seen[{secs[off + i].g, secs[off + i].root}]++;
                }
                const int nparts = ph ? R.nch : 1;
                for (int part = 0; part < nparts; ++part) {
                const int a0 = ph ? off + R.ps_o[part] : off, a1 = ph ? off + R.ps_o[part + 1] : off + cnt;
                for (int i = a0; i < a1; ++i) {
                    const Sec &sc = secs[i];
                    const int me = sc.g == G_ROW ? mycol : myrow;
                    const size_t bytes = (size_t)sc.cnt * sizeof(T);
                    if (me == sc.root) {
                        SLU_REQUIRE(sc.off >= 0, "root of a section without a buffer");
                        for (size_t b = 0; b < bytes; ++b)
                            arena[(size_t)sc.off * sizeof(T) + b] = pat(L, ph, root_rank(sc), kth[i - off], b);
                    } else if (sc.off >= 0) {
                        memset(arena + (size_t)sc.off * sizeof(T), 0, bytes);
                    }
                }
                issue(secs, a0, a1 - a0, ph ? "L/U panel exchange (replay)" : "diagonal-package exchange (replay)",
                      (int)L, (T *)hd.data(), (T *)hp.data());
                for (int i = a0; i < a1; ++i) {
                    const Sec &sc = secs[i];
                    const int me = sc.g == G_ROW ? mycol : myrow;
                    if (me == sc.root || !(sc.mask >> me & 1)) continue;
                    SLU_REQUIRE(sc.off >= 0, "level %zu: a section for this rank has no buffer", L);
                    const size_t bytes = (size_t)sc.cnt * sizeof(T);
                    for (size_t b = 0; b < bytes; ++b)
                        SLU_REQUIRE(arena[(size_t)sc.off * sizeof(T) + b] ==
                                        pat(L, ph, root_rank(sc), kth[i - off], b),
                                    "level %zu: section (group %d root %d) byte %zu differs", L, sc.g,
                                    sc.root, b);
                    ++ns;
                    nb += (i64)bytes;
                }
                }
            }
        }
        if (zmode && zp < maxlvl - 1) { // the ancestor reduction after my phase zp
            const bool recv = zl % (2 << zp) == 0;
            const int peer = recv ? zl + (1 << zp) : zl - (1 << zp), root = recv ? peer : zl;
            const size_t bytes = (size_t)zr_cnt[zp] * sizeof(T);
            vector<unsigned char> zb(std::max<size_t>(bytes, 1), 0);
            if (!recv)
                for (size_t b = 0; b < bytes; ++b) zb[b] = pat(1000000 + zp, 0, root, iam, b);
            X.section(G_Z, root, 1u << (recv ? zl : peer), zb.data(), bytes);
            X.flush_as("3D ancestor reduction (replay)", zp);
            if (recv && bytes) {
                for (size_t b = 0; b < bytes; ++b)
                    SLU_REQUIRE(zb[b] == pat(1000000 + zp, 0, root, iam, b),
                                "3D reduction %d: byte %zu from layer %d differs", zp, b, root);
                ++ns;
                nb += (i64)bytes;
            }
        }
        }
        // the final info reduction of factor()
        vector<i64> mine(1, iam);
        auto all = X.allgatherv(G_WORLD, mine);
        for (int r = 0; r < Pr * Pc; ++r) SLU_REQUIRE(all[r].size() == 1 && all[r][0] == r, "info all-gather");
        if (zmode) {
            mine[0] = zl;
            auto az = X.allgatherv(G_Z, mine);
            for (int z = 0; z < npdep; ++z) SLU_REQUIRE(az[z].size() == 1 && az[z][0] == z, "3D info all-gather");
        }
        *nsec = ns;
        *nbytes = nb;
    }

    bool prof = false; // SLU_PROFILE_PLAN: phase times of the plan build on stderr
    std::chrono::steady_clock::time_point tprev;
    void tick(const char *what) {
        if (!prof) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[slu plan %d] %-18s %8.1f ms\n", iam, what,
                std::chrono::duration<double, std::milli>(now - tprev).count());
        tprev = now;
    }

    int device() const { return comm ? comm->device : 0; }

    ~Plan() override {
        // (before the streams and events go; the DevBuf members are covered
        // by the declaration order, see up_thread)
        up_thread.wait();
        pin_thread.wait();
        for (auto e : ev_pan) (void)hipEventDestroy(e);
        for (auto e : ev_rest) (void)hipEventDestroy(e);
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_pend) (void)hipEventDestroy(ev_pend);
        if (ev_tu0) (void)hipEventDestroy(ev_tu0);
        if (ev_tu1) (void)hipEventDestroy(ev_tu1);
        if (ev_pk) (void)hipEventDestroy(ev_pk);
        if (ev_dx) (void)hipEventDestroy(ev_dx);
        for (hipEvent_t e : ev_cx)
            if (e) (void)hipEventDestroy(e);
        if (cstream) (void)hipStreamDestroy(cstream);
        if (stream) (void)hipStreamDestroy(stream);
        if (pstream) (void)hipStreamDestroy(pstream);
        if (ustream) (void)hipStreamDestroy(ustream);
    }

    // ------------------------------------------------------- local layout
    // Value offsets of the rank's L block columns / U block rows in d_L /
    // d_U (the order of Lnzval_bc_dat / Unzval_br_dat, so that the upload can
    // start before the rest of the plan exists).
    void value_layout() {
        LocalLU *Llu = LU->Llu;
        lval_off.assign(nlc, -1);
        lval_ld.assign(nlc, 0);
        i64 off = 0;
        l_contig = Llu->Lnzval_bc_dat != nullptr;
        for (int ljb = 0; ljb < nlc; ++ljb) {
            const int_t *index = Llu->Lrowind_bc_ptr[ljb];
            if (!index) continue;
            lval_off[ljb] = off;
            lval_ld[ljb] = (int)index[1];
            if (Llu->Lnzval_bc_dat && (HT *)Llu->Lnzval_bc_ptr[ljb] != (HT *)Llu->Lnzval_bc_dat + off)
                l_contig = false;
            off += (i64)index[1] * W(ljb * Pc + mycol);
        }
        lval_total = off;
        uval_off.assign(nlr, -1);
        uval_len.assign(nlr, 0);
        off = 0;
        u_contig = Llu->Unzval_br_dat != nullptr;
        for (int lb = 0; lb < nlr; ++lb) {
            const int_t *index = Llu->Ufstnz_br_ptr[lb];
            if (!index) continue;
            uval_off[lb] = off;
            uval_len[lb] = index[1];
            if (Llu->Unzval_br_dat && (HT *)Llu->Unzval_br_ptr[lb] != (HT *)Llu->Unzval_br_dat + off)
                u_contig = false;
            off += index[1];
        }
        uval_total = off;
    }

    // Destination tables (LBlk + lmap per L block, UBlk + per-column segment
    // offsets per U block) in two parallel passes: sizes per block column /
    // row, prefix sums, then every column / row fills its own slice.
    void build_local() {
        LocalLU *Llu = LU->Llu;
        // ---- L block columns
        lcol_first.assign(nlc + 1, 0);
        lcol_nblk.assign(nlc, 0);
        vector<i64> mapbase(nlc + 1, 0);
        parallel_for(nlc, [&](int ljb) {
            const int_t *index = Llu->Lrowind_bc_ptr[ljb];
            if (!index) return;
            i64 p = SLU_BC_HEADER, ml = 0;
            for (int b = 0; b < index[0]; ++b) {
                ml += W(index[p]);
                p += SLU_LB_DESCRIPTOR + index[p + 1];
            }
            lcol_nblk[ljb] = (int)index[0];
            mapbase[ljb + 1] = ml;
        });
        for (int j = 0; j < nlc; ++j) {
            lcol_first[j + 1] = lcol_first[j] + lcol_nblk[j];
            mapbase[j + 1] += mapbase[j];
        }
        lblk.assign(lcol_first[nlc], LBlk{});
        lblk_ib.assign(lcol_first[nlc], 0);
        lmap.resize_uninit(mapbase[nlc]);
        parallel_for(nlc, [&](int ljb) {
            const int jb = ljb * Pc + mycol;
            const int_t *index = Llu->Lrowind_bc_ptr[ljb];
            if (!index) return;
            const int nb = (int)index[0], nsupr = (int)index[1];
            i64 p = SLU_BC_HEADER, mo = mapbase[ljb];
            std::fill(&lmap[mapbase[ljb]], &lmap[0] + mapbase[ljb + 1], -1);
            int rs = 0;
            for (int b = 0; b < nb; ++b) {
                const int gb = (int)index[p], nr = (int)index[p + 1];
                SLU_REQUIRE(gb % Pr == myrow, "L block (%d,%d) is not on process row %d", gb, jb, myrow);
                LBlk &L = lblk[lcol_first[ljb] + b];
                L.colvoff = lval_off[ljb];
                L.mapoff = mo;
                L.ld = nsupr;
                L.fcol = (int)xsup[jb];
                L.frow = (int)xsup[gb];
                for (int i = 0; i < nr; ++i) lmap[mo + index[p + 2 + i] - xsup[gb]] = rs + i;
                lblk_ib[lcol_first[ljb] + b] = gb;
                mo += W(gb);
                rs += nr;
                p += SLU_LB_DESCRIPTOR + nr;
            }
            SLU_REQUIRE(rs == nsupr, "L column %d: block rows %d != nsupr %d", jb, rs, nsupr);
        });
        lcol_first.resize(nlc);

        // ---- U block rows
        urow_first.assign(nlr + 1, 0);
        urow_nblk.assign(nlr, 0);
        vector<i64> colbase(nlr + 1, 0);
        parallel_for(nlr, [&](int lb) {
            const int_t *index = Llu->Ufstnz_br_ptr[lb];
            if (!index) return;
            i64 p = SLU_BR_HEADER, nc = 0;
            for (int b = 0; b < index[0]; ++b) {
                nc += W(index[p]);
                p += SLU_UB_DESCRIPTOR + W(index[p]);
            }
            urow_nblk[lb] = (int)index[0];
            colbase[lb + 1] = nc;
        });
        for (int j = 0; j < nlr; ++j) {
            urow_first[j + 1] = urow_first[j] + urow_nblk[j];
            colbase[j + 1] += colbase[j];
        }
        ublk.assign(urow_first[nlr], UBlk{});
        ublk_jb.assign(urow_first[nlr], 0);
        ucol_voff.resize_uninit(colbase[nlr]);
        ucol_fst.resize_uninit(colbase[nlr]);
        parallel_for(nlr, [&](int lb) {
            const int gb = lb * Pr + myrow;
            const int_t *index = Llu->Ufstnz_br_ptr[lb];
            if (!index) return;
            const int nb = (int)index[0];
            const i64 len = index[1], klst = xsup[gb + 1], off = uval_off[lb];
            i64 p = SLU_BR_HEADER, run = 0, co = colbase[lb];
            for (int b = 0; b < nb; ++b) {
                const int jb = (int)index[p];
                SLU_REQUIRE(jb % Pc == mycol, "U block (%d,%d) is not on process column %d", gb, jb, mycol);
                UBlk &U = ublk[urow_first[lb] + b];
                U.coloff = co;
                U.fcol = (int)xsup[jb];
                for (int c = 0; c < W(jb); ++c, ++co) {
                    const i64 fst = index[p + SLU_UB_DESCRIPTOR + c];
                    ucol_voff[co] = off + run;
                    ucol_fst[co] = (int)fst;
                    run += klst - fst;
                }
                ublk_jb[urow_first[lb] + b] = jb;
                p += SLU_UB_DESCRIPTOR + W(jb);
            }
            SLU_REQUIRE(run == len, "U row %d: segment lengths %lld != %lld", gb, (long long)run, (long long)len);
        });
        urow_first.resize(nlr);
    }

    int find_lblk(int ib, int jb) const { // local column jb, block ib
        int ljb = jb / Pc, f = lcol_first[ljb], nb = lcol_nblk[ljb];
        auto b = lblk_ib.begin() + f, e = b + nb;
        auto it = std::lower_bound(b, e, ib);
        SLU_REQUIRE(it != e && *it == ib, "missing L block (%d,%d)", ib, jb);
        return (int)(it - lblk_ib.begin());
    }
    int find_ublk(int ib, int jb) const { // local row ib, block jb
        int lb = ib / Pr, f = urow_first[lb], nb = urow_nblk[lb];
        auto b = ublk_jb.begin() + f, e = b + nb;
        auto it = std::lower_bound(b, e, jb);
        SLU_REQUIRE(it != e && *it == jb, "missing U block (%d,%d)", ib, jb);
        return (int)(it - ublk_jb.begin());
    }

    // length of an index array in the reference formats
    i64 lidx_len(const int_t *ix) const {
        i64 p = SLU_BC_HEADER;
        for (i64 b = 0; b < ix[0]; ++b) p += SLU_LB_DESCRIPTOR + ix[p + 1];
        return p;
    }
    i64 uidx_len(const int_t *ix) const {
        i64 p = SLU_BR_HEADER;
        for (i64 b = 0; b < ix[0]; ++b) p += SLU_UB_DESCRIPTOR + W(ix[p]);
        return p;
    }
    // rows of L(:,k) on my process row below the diagonal block, and the
    // number of rows of the diagonal block stored on top (0 or W(k))
    void lrows(int k, int &m, int &r0) const {
        m = r0 = 0;
        const int_t *ix = lidx[k];
        if (!ix) return;
        i64 p = SLU_BC_HEADER;
        for (i64 b = 0; b < ix[0]; ++b) {
            int nr = (int)ix[p + 1];
            if (ix[p] == k) r0 += nr;
            else m += nr;
            p += SLU_LB_DESCRIPTOR + nr;
        }
    }

    // ------------------------------------------------------- index exchange
    // The reference ships lsub/usub with every panel message
    // (SRC/pdgstrf.c:1039-1044,1330-1335); the structure never changes during
    // the factorization, so it is exchanged once here.
    void exchange_index() {
        LocalLU *Llu = LU->Llu;
        lidx.assign(nsupers, nullptr);
        uidx.assign(nsupers, nullptr);
        for (int ljb = 0; ljb < nlc; ++ljb)
            if (ljb * Pc + mycol < nsupers) lidx[ljb * Pc + mycol] = Llu->Lrowind_bc_ptr[ljb];
        for (int lb = 0; lb < nlr; ++lb)
            if (lb * Pr + myrow < nsupers) uidx[lb * Pr + myrow] = Llu->Ufstnz_br_ptr[lb];
        if (!xmode) return;
        if (Pc > 1) {
            vector<i64> blob;
            for (int ljb = 0; ljb < nlc; ++ljb) {
                const int_t *ix = Llu->Lrowind_bc_ptr[ljb];
                if (!ix) continue;
                i64 len = lidx_len(ix);
                blob.push_back(ljb);
                blob.push_back(len);
                blob.insert(blob.end(), ix, ix + len);
            }
            xL = X.allgatherv(G_ROW, blob);
            for (int c = 0; c < Pc; ++c) {
                if (c == mycol) continue;
                const vector<i64> &v = xL[c];
                for (size_t p = 0; p < v.size();) {
                    i64 ljb = v[p], len = v[p + 1];
                    lidx[ljb * Pc + c] = (const int_t *)&v[p + 2];
                    p += 2 + len;
                }
            }
        }
        if (Pr > 1) {
            vector<i64> blob;
            for (int lb = 0; lb < nlr; ++lb) {
                const int_t *ix = Llu->Ufstnz_br_ptr[lb];
                if (!ix) continue;
                i64 len = uidx_len(ix);
                blob.push_back(lb);
                blob.push_back(len);
                blob.insert(blob.end(), ix, ix + len);
            }
            xU = X.allgatherv(G_COL, blob);
            for (int r = 0; r < Pr; ++r) {
                if (r == myrow) continue;
                const vector<i64> &v = xU[r];
                for (size_t p = 0; p < v.size();) {
                    i64 lb = v[p], len = v[p + 1];
                    uidx[lb * Pr + r] = (const int_t *)&v[p + 2];
                    p += 2 + len;
                }
            }
        }
    }

    // Who needs what (2D grids), as the reference's ToSendR / ToSendD
    // (SRC/pddistribute.c:752-801) but derived from the exchanged structure:
    //   rneed[k*Pc + pc]: U(k,:) has blocks on process column pc -- those
    //     ranks need L(:,k) and the factored diagonal block (U-TRSM on the
    //     owner's process row);
    //   cneed[k*Pr + pr]: L(:,k) has rows below the diagonal block on process
    //     row pr -- those ranks need U(k,:) and the diagonal block (L-TRSM).
    // Each rank knows its own column's / row's entries; one row and one
    // column all-gather make them global on every rank.
    vector<char> rneed, cneed;
    void exchange_needs() {
        if (!xmode) return;
        rneed.assign((size_t)nsupers * Pc, 0);
        cneed.assign((size_t)nsupers * Pr, 0);
        vector<i64> mine_r(nsupers), mine_c(nsupers);
        for (int k = 0; k < nsupers; ++k) {
            mine_r[k] = uidx[k] != nullptr;
            mine_c[k] = lsend(k);
        }
        vector<vector<i64>> ar, ac;
        if (Pc > 1) ar = X.allgatherv(G_ROW, mine_r);
        else ar.push_back(mine_r);
        if (Pr > 1) ac = X.allgatherv(G_COL, mine_c);
        else ac.push_back(mine_c);
        for (int k = 0; k < nsupers; ++k) {
            for (int c = 0; c < Pc; ++c) rneed[(size_t)k * Pc + c] = (char)ar[c][k];
            for (int r = 0; r < Pr; ++r) cneed[(size_t)k * Pr + r] = (char)ac[r][k];
        }
    }
    uint32_t rmask(int k) const {
        uint32_t m = 0;
        for (int c = 0; c < Pc; ++c) m |= (uint32_t)rneed[(size_t)k * Pc + c] << c;
        return m;
    }
    uint32_t cmask(int k) const {
        uint32_t m = 0;
        for (int r = 0; r < Pr; ++r) m |= (uint32_t)cneed[(size_t)k * Pr + r] << r;
        return m;
    }

    // ------------------------------------------------------- levels
    // Dependency DAG k -> ib (L(ib,k) != 0) and k -> jb (U(k,jb) != 0); all
    // edges point to larger supernode numbers, so one ascending sweep gives
    // the longest-path level.  On a grid every rank contributes its local
    // blocks and all ranks compute the same levels.
    void compute_levels() {
        vector<i64> edges;
        for (int ljb = 0; ljb < nlc; ++ljb) {
            int k = ljb * Pc + mycol;
            if (k >= nsupers || !lidx[k]) continue;
            const int_t *ix = lidx[k];
            i64 p = SLU_BC_HEADER;
            for (i64 b = 0; b < ix[0]; ++b) {
                if (ix[p] != k) {
                    edges.push_back(k);
                    edges.push_back(ix[p]);
                }
                p += SLU_LB_DESCRIPTOR + ix[p + 1];
            }
        }
        for (int lb = 0; lb < nlr; ++lb) {
            int k = lb * Pr + myrow;
            if (k >= nsupers || !uidx[k]) continue;
            const int_t *ix = uidx[k];
            i64 p = SLU_BR_HEADER;
            for (i64 b = 0; b < ix[0]; ++b) {
                edges.push_back(k);
                edges.push_back(ix[p]);
                p += SLU_UB_DESCRIPTOR + W(ix[p]);
            }
        }
        vector<vector<i64>> all;
        if (xmode) all = X.allgatherv(G_WORLD, edges);
        else all.push_back(std::move(edges));
        // CSR of the edges by source
        vector<i64> cnt(nsupers + 1, 0);
        for (auto &v : all)
            for (size_t e = 0; e < v.size(); e += 2) cnt[v[e] + 1]++;
        for (int k = 0; k < nsupers; ++k) cnt[k + 1] += cnt[k];
        vector<int> tgt(cnt[nsupers]);
        vector<i64> fill(cnt.begin(), cnt.end() - 1);
        for (auto &v : all)
            for (size_t e = 0; e < v.size(); e += 2) {
                SLU_REQUIRE(v[e + 1] > v[e] && v[e + 1] < nsupers, "bad dependency %lld -> %lld",
                            (long long)v[e], (long long)v[e + 1]);
                tgt[fill[v[e]]++] = (int)v[e + 1];
            }
        if (zmode) return compute_levels_3d(cnt, tgt);
        level_of.assign(nsupers, 0);
        int maxlev = 0;
        for (int k = 0; k < nsupers; ++k) {
            maxlev = std::max(maxlev, level_of[k]);
            for (i64 e = cnt[k]; e < cnt[k + 1]; ++e)
                level_of[tgt[e]] = std::max(level_of[tgt[e]], level_of[k] + 1);
        }
        bylev.assign(maxlev + 1, {});
        for (int k = 0; k < nsupers; ++k) bylev[level_of[k]].push_back(k);
        levels.assign(maxlev + 1, LevelRange{});
        stats.nsupers = nsupers;
        stats.nsupers_in = nsupers;
        stats.nlevels = maxlev + 1;
    }

    // ------------------------------------------------------- 3D forests
    // The forest partition of SRC/supernodalForest.c (getGreedyLoadBalForests
    // :794, iterativeFrPartitioning :618, getLoadImbalance :463): starting
    // from the etree's roots, while the two-way greedy split of the current
    // tree set is more than 20 % imbalanced (and fewer than 1024 trees), the
    // heaviest tree's single-child chain from its root down to the first
    // branching goes to the ancestor forest and the branch's children replace
    // it; the set is then split greedily (heaviest first, into the lighter
    // half) and each half is partitioned the same way one level down; the
    // halves at the bottom are the layers' leaf forests.  The tree is the
    // elimination tree of the block dependency DAG (Liu's algorithm with path
    // compression over the DAG's edges), so every supernode a block column
    // or row of k updates is an ancestor of k -- the property the phases rely
    // on.  Weights estimate each supernode's Schur work, w * m^2 with m the
    // summed widths of its successors (the reference's scuWeight, from the
    // same block structure).
    void compute_forests(const vector<i64> &cnt, const vector<int> &tgt) {
        const int ns = nsupers;
        vector<int> parent(ns, -1), anc(ns, -1);
        {   // edges by target
            vector<i64> rc(ns + 1, 0);
            for (int k = 0; k < ns; ++k)
                for (i64 e = cnt[k]; e < cnt[k + 1]; ++e) rc[tgt[e] + 1]++;
            for (int k = 0; k < ns; ++k) rc[k + 1] += rc[k];
            vector<int> src(rc[ns]);
            vector<i64> f(rc.begin(), rc.end() - 1);
            for (int k = 0; k < ns; ++k)
                for (i64 e = cnt[k]; e < cnt[k + 1]; ++e) src[f[tgt[e]]++] = k;
            for (int t = 0; t < ns; ++t)
                for (i64 e = rc[t]; e < rc[t + 1]; ++e) {
                    int r = src[e];
                    while (anc[r] != -1 && anc[r] != t) { // root of r's current subtree
                        const int nx = anc[r];
                        anc[r] = t;                       // path compression
                        r = nx;
                    }
                    if (anc[r] == -1 && r != t) {
                        parent[r] = t;
                        anc[r] = t;
                    }
                }
        }
        vector<double> wt(ns, 0), sub(ns, 0);
        for (int k = 0; k < ns; ++k) {
            double m = 0;
            for (i64 e = cnt[k]; e < cnt[k + 1]; ++e) m += W(tgt[e]);
            wt[k] = (double)W(k) * (m * m + (double)W(k) * W(k) / 3.0) + 1.0;
        }
        vector<vector<int>> kids(ns);
        vector<int> roots;
        for (int k = 0; k < ns; ++k) {
            sub[k] += wt[k];
            if (parent[k] >= 0) {
                sub[parent[k]] += sub[k];
                kids[parent[k]].push_back(k);
            } else {
                roots.push_back(k);
            }
        }
        const int nf = (1 << maxlvl) - 1;
        forest_of.assign(ns, -1);
        if (opts.forest_map) { // the caller's partition (pdgstrf3d: supernode2treeMap)
            for (int k = 0; k < ns; ++k) {
                SLU_REQUIRE(opts.forest_map[k] >= 0 && opts.forest_map[k] < nf,
                            "forest map: supernode %d in forest %lld of %d", k,
                            (long long)opts.forest_map[k], nf);
                forest_of[k] = (int)opts.forest_map[k];
            }
            return;
        }
        vector<vector<int>> heads((size_t)nf);
        heads[0] = roots;
        auto split2 = [&](vector<int> set, vector<int> *out) {
            std::stable_sort(set.begin(), set.end(), [&](int a, int b) { return sub[a] > sub[b]; });
            double w[2] = {0, 0};
            for (int t : set) {
                const int h = w[0] > w[1] ? 1 : 0;
                w[h] += sub[t];
                if (out) out[h].push_back(t);
            }
            return w[0] + w[1] > 0 ? std::fabs(w[0] - w[1]) / (w[0] + w[1]) : 0.0;
        };
        auto mark_subtrees = [&](const vector<int> &hs, int f) {
            vector<int> st(hs.begin(), hs.end());
            while (!st.empty()) {
                const int v = st.back();
                st.pop_back();
                forest_of[v] = f;
                for (int c : kids[v]) st.push_back(c);
            }
        };
        if (maxlvl == 1) mark_subtrees(heads[0], 0);
        for (int lvl = 0; lvl < maxlvl - 1; ++lvl)
            for (int tr = (1 << lvl) - 1; tr < (1 << (lvl + 1)) - 1; ++tr) {
                vector<int> set = heads[tr];
                while (split2(set, nullptr) > 0.2 && set.size() < 1024) {
                    size_t idx = 0;
                    for (size_t i = 1; i < set.size(); ++i)
                        if (sub[set[i]] > sub[set[idx]]) idx = i;
                    int v = set[idx];
                    while (kids[v].size() == 1) v = kids[v][0];
                    if (kids[v].empty()) break;
                    for (int u = set[idx];; u = kids[u][0]) { // the chain joins the ancestors
                        forest_of[u] = tr;
                        if (u == v) break;
                    }
                    set.erase(set.begin() + idx);
                    set.insert(set.end(), kids[v].begin(), kids[v].end());
                }
                vector<int> half[2];
                split2(set, half);
                if (lvl == maxlvl - 2) {
                    mark_subtrees(half[0], 2 * tr + 1);
                    mark_subtrees(half[1], 2 * tr + 2);
                } else {
                    heads[2 * tr + 1] = half[0];
                    heads[2 * tr + 2] = half[1];
                }
            }
        for (int k = 0; k < ns; ++k) SLU_REQUIRE(forest_of[k] >= 0, "supernode %d in no forest", k);
    }

    // heap index of layer z's forest at level ilvl (0 = leaves), as
    // SRC/supernodal_etree.c:802-812 (getGridTrees)
    int tree_of(int z, int ilvl) const {
        int t = npdep - 1 + z;
        for (int i = 0; i < ilvl; ++i) t = (t - 1) / 2;
        return t;
    }
    int ilvl_of_forest(int f) const { // 0 = leaves
        int d = 0;
        while ((2 << d) - 1 <= f) ++d;
        return maxlvl - 1 - d;
    }

    void compute_levels_3d(const vector<i64> &cnt, const vector<int> &tgt) {
        compute_forests(cnt, tgt);
        my_last = 0;
        while (my_last < maxlvl - 1 && zl % (2 << my_last) == 0) ++my_last;
        phase_of.assign(nsupers, -1);
        for (int k = 0; k < nsupers; ++k) {
            const int il = ilvl_of_forest(forest_of[k]);
            if (forest_of[k] == tree_of(zl, il) && il <= my_last) phase_of[k] = il;
        }
        // every block a factored supernode updates lies on this layer's path
        // of forests at its phase or above (the partition's invariant)
        for (int k = 0; k < nsupers; ++k) {
            if (phase_of[k] < 0) continue;
            for (i64 e = cnt[k]; e < cnt[k + 1]; ++e) {
                const int t = tgt[e], il = ilvl_of_forest(forest_of[t]);
                SLU_REQUIRE(il >= phase_of[k] && forest_of[t] == tree_of(zl, il),
                            "3D forests: supernode %d (phase %d) updates %d outside its path", k,
                            phase_of[k], t);
            }
        }
        vector<int> lin(nsupers, 0);
        vector<int> depth(maxlvl, 0);
        for (int k = 0; k < nsupers; ++k) {
            if (phase_of[k] < 0) continue;
            depth[phase_of[k]] = std::max(depth[phase_of[k]], lin[k] + 1);
            for (i64 e = cnt[k]; e < cnt[k + 1]; ++e)
                if (phase_of[tgt[e]] == phase_of[k]) lin[tgt[e]] = std::max(lin[tgt[e]], lin[k] + 1);
        }
        phase_lv.assign(my_last + 2, 0);
        for (int p = 0; p <= my_last; ++p) phase_lv[p + 1] = phase_lv[p] + depth[p];
        const int nl = phase_lv[my_last + 1];
        level_of.assign(nsupers, -1);
        bylev.assign(nl, {});
        for (int k = 0; k < nsupers; ++k)
            if (phase_of[k] >= 0) {
                level_of[k] = phase_lv[phase_of[k]] + lin[k];
                bylev[level_of[k]].push_back(k);
            }
        levels.assign(nl, LevelRange{});
        int nf = 0;
        for (int k = 0; k < nsupers; ++k) nf += phase_of[k] >= 0;
        stats.npdep = npdep;
        stats.zlayer = zl;
        stats.phase_last = my_last;
        stats.nsupers = nf;
        stats.nsupers_in = nsupers;
        stats.nlevels = nl;
    }

    // local value ranges of supernode k's L block column / U block row,
    // appended to zr in chunks (buffer positions from *bo on)
    void add_zranges(int k, i64 *bo) {
        auto add = [&](i64 off, i64 len, int arr) {
            for (i64 c = 0; c < len; c += ZR_CHUNK) {
                const int l = (int)std::min<i64>(ZR_CHUNK, len - c);
                zr.push_back(ZRange{off + c, *bo, l, arr});
                *bo += l;
            }
        };
        if (k % Pc == mycol && lval_off[k / Pc] >= 0)
            add(lval_off[k / Pc], (i64)lval_ld[k / Pc] * W(k), 0);
        if (k % Pr == myrow && uval_off[k / Pr] >= 0) add(uval_off[k / Pr], uval_len[k / Pr], 1);
    }

    void build_zranges(bool device) {
        zr.clear();
        zr_off.assign(1, 0);
        zr_cnt.clear();
        i64 bo = 0;
        // ancestor forests this layer does not factor start from zero
        for (int k = 0; k < nsupers; ++k) {
            const int il = ilvl_of_forest(forest_of[k]);
            if (il >= 1 && forest_of[k] == tree_of(zl, il) && il > my_last) add_zranges(k, &bo);
        }
        zr_off.push_back((int)zr.size());
        // reduction after phase p: every ancestor forest above it on my path
        i64 mx = 0;
        for (int p = 0; p < maxlvl - 1; ++p) {
            bo = 0;
            if (p <= my_last)
                for (int k = 0; k < nsupers; ++k) {
                    const int il = ilvl_of_forest(forest_of[k]);
                    if (il > p && forest_of[k] == tree_of(zl, il)) add_zranges(k, &bo);
                }
            zr_off.push_back((int)zr.size());
            zr_cnt.push_back(bo);
            if (p < 8) stats.zred_bytes[p] = (double)bo * sizeof(T);
            mx = std::max(mx, bo);
        }
        if (!device) return;
        d_zr.upload(zr);
        d_zbuf.alloc(std::max<i64>(mx, 1));
    }

    void launch_zranges(int a, int b, int op, hipStream_t st) {
        if (b > a)
            hipLaunchKernelGGL(k_zranges<T>, dim3(b - a), dim3(256), 0, st, d_zr.p + a, d_L.p, d_U.p,
                               d_zbuf.p, op);
    }

    // ancestor reduction at the end of phase p (SRC/pd3dcomm.c:786-813):
    // layer z + 2^p sends its partial sums, layer z adds them
    void zreduce(int p, hipStream_t st) {
        const bool recv = zl % (2 << p) == 0;
        const int peer = recv ? zl + (1 << p) : zl - (1 << p);
        const int a = zr_off[p + 1], b = zr_off[p + 2];
        const i64 cnt = zr_cnt[p];
        if (!recv) launch_zranges(a, b, ZR_PACK, st);
        X.s = st;
        if (!zsolo) {
            X.section(G_Z, recv ? peer : zl, 1u << (recv ? zl : peer), d_zbuf.p, (size_t)cnt * sizeof(T));
            X.flush_as("3D ancestor reduction", p);
        }
        zbytes += (double)cnt * sizeof(T);
        if (recv) launch_zranges(a, b, ZR_ADD, st);
    }

    // After factor(): the factored forests travel to layer 0 (every layer's
    // part of it), as pdgssvx3d's dgatherAllFactoredLU (SRC/pd3dcomm.c:816-858).
    void gather_layers() override {
        SLU_REQUIRE(zmode, "gather_layers: not a 3D plan");
        SLU_REQUIRE(vstate == 2, "gather_layers: factor first");
        sync();
        hipStream_t st = stream;
        for (int il = 0; il < maxlvl - 1; ++il) {
            if (zl % (1 << il)) break;
            const bool recv = zl % (2 << il) == 0;
            const int sender = recv ? zl + (1 << il) : zl, peer = recv ? sender : zl - (1 << il);
            // forests the sender's half of the layers factored: at level a
            // <= il, trees (2^(maxlvl-1-a) - 1) + (sender >> a) + [0, 2^(il-a))
            vector<char> want((size_t)(1 << maxlvl), 0);
            for (int a = 0; a <= il; ++a) {
                const int t0 = (1 << (maxlvl - 1 - a)) - 1 + (sender >> a);
                for (int t = t0; t < t0 + (1 << (il - a)); ++t) want[t] = 1;
            }
            vector<ZRange> keep;
            keep.swap(zr);
            i64 bo = 0;
            for (int k = 0; k < nsupers; ++k)
                if (want[forest_of[k]]) add_zranges(k, &bo);
            DevBuf<ZRange> dr;
            dr.upload(zr);
            DevBuf<T> buf;
            buf.alloc(std::max<i64>(bo, 1));
            const int nr = (int)zr.size();
            zr.swap(keep);
            if (!recv && nr)
                hipLaunchKernelGGL(k_zranges<T>, dim3(nr), dim3(256), 0, st, dr.p, d_L.p, d_U.p, buf.p,
                                   (int)ZR_PACK);
            X.s = st;
            X.section(G_Z, sender, 1u << (recv ? zl : peer), buf.p, (size_t)bo * sizeof(T));
            X.flush_as("3D gather to layer 0", il);
            if (recv && nr)
                hipLaunchKernelGGL(k_zranges<T>, dim3(nr), dim3(256), 0, st, dr.p, d_L.p, d_U.p, buf.p,
                                   (int)ZR_COPY);
            HIPCHK(hipStreamSynchronize(st));
            if (!recv) break;
        }
        host_current = false;
    }

    // ------------------------------------------------------- value layout
    // Diagonal packages [w*w factored block, ld w | Dinv] and remote panels
    // are laid out per level in broadcast order: sections of the owners in my
    // process column (root = their process row), then of my process row.
    // Receive buffers are a ring, as the reference's num_lookaheads + 1
    // rotating Lsub_buf_2 / Lval_buf_2 (SRC/pdgstrf.c:454-512): with the
    // one-level look-ahead of factor() only levels L and L+1 are live at a
    // time -- panel(L+2) is issued on the panel stream after it waited for
    // the rest of level L's Schur update (ev_rest[L]) -- so the panels use
    // two slots of the largest level, and the diagonal packages (read only
    // by the TRSMs of their own level, on the same stream) one.
    vector<i64> pan_level; // panel bytes (elements) per level
    bool lsend(int k) const { // L(:,k) on my process row has rows below the diagonal block
        int m, r0;
        lrows(k, m, r0);
        return m > 0;
    }
    // U(k,:) on my process column: its nonempty columns (the Schur update's
    // columns, in order) and the panel's value offset where each group of
    // csz of them starts (the U panel is the concatenation of the columns'
    // segments, SRC/superlu_defs.h:152-198)
    int ucols_runs(int k, int csz, std::array<i64, NCHM> *run) const {
        if (run) run->fill(0);
        if (!uidx[k]) return 0;
        const int_t *ix = uidx[k];
        const i64 klst = xsup[k + 1];
        i64 p = SLU_BR_HEADER, r = 0;
        int nc = 0;
        for (i64 b = 0; b < ix[0]; ++b) {
            const int jb = (int)ix[p];
            for (int c = 0; c < W(jb); ++c) {
                const i64 fst = ix[p + SLU_UB_DESCRIPTOR + c];
                if (fst >= klst) continue;
                if (run && csz > 0 && nc % csz == 0 && nc / csz < NCHM) (*run)[nc / csz] = r;
                ++nc;
                r += klst - fst;
            }
            p += SLU_UB_DESCRIPTOR + W(jb);
        }
        return nc;
    }
    void layout_values() {
        pkg.assign(nsupers, -1);
        dscr.assign(nsupers, -1);
        lpos.assign(nsupers, -1);
        upos.assign(nsupers, -1);
        if (xmode) {
            std::array<i64, NCHM> none;
            none.fill(-1);
            lgsz.assign(nsupers, 0);
            ucsz.assign(nsupers, 0);
            ucols.assign(nsupers, 0);
            lgpos.assign(nsupers, none);
            ugpos.assign(nsupers, none);
            ugrun.assign(nsupers, none);
            for (int k = 0; k < nsupers; ++k) {
                int m, r0;
                lrows(k, m, r0);
                lgsz[k] = group_size(m);
                ucols[k] = ucols_runs(k, 0, nullptr);
                ucsz[k] = group_size(ucols[k]);
                ucols_runs(k, ucsz[k], &ugrun[k]);
            }
        }
        for (size_t L = 0; L < levels.size(); ++L) {
            LevelRange &R = levels[L];
            const vector<int> &ks = bylev[L];
            if (!xmode) { // 1x1: Dinv in a per-level scratch
                i64 off = 0;
                for (int k : ks) {
                    dscr[k] = off;
                    off += dinv_len(W(k));
                }
                dscr_max = std::max(dscr_max, off);
                continue;
            }
            // ---- diag packages: owner (r, mycol) for all r, then (myrow, c),
            // c != mycol.  One section per owner and group; its mask is the
            // union over the owner's supernodes of the ranks that need a
            // package (packages are small: w*w + Dinv per supernode).
            dpk_total = 0;  // per-level cursor (one slot, reused by every level)
            pan_total = 0;  // per-level cursor (the slot base is added below)
            // layout first (owners (r, mycol) for all r, then (myrow, c)), then
            // the sections in the canonical order every member of a group
            // shares: column groups by root row, row groups by root column
            struct Own {
                uint32_t cm = 0, rm = 0;
                i64 start = -1, cnt = 0;
            };
            vector<Own> own(Pr * Pc);
            auto lay_owner = [&](int orow, int ocol) {
                const bool me = orow == myrow && ocol == mycol;
                Own &o = own[orow * Pc + ocol];
                for (int k : ks)
                    if (k % Pr == orow && k % Pc == ocol) {
                        o.cm |= cmask(k);
                        o.rm |= rmask(k);
                        o.cnt += (i64)W(k) * W(k) + dinv_len(W(k));
                    }
                if (!o.cnt) return;
                o.cm &= ~(1u << orow);
                o.rm &= ~(1u << ocol);
                const bool here = me || (ocol == mycol && (o.cm >> myrow & 1)) ||
                                  (orow == myrow && (o.rm >> mycol & 1));
                if (!here) return;
                o.start = dpk_total;
                for (int k : ks)
                    if (k % Pr == orow && k % Pc == ocol) {
                        pkg[k] = dpk_total;
                        dpk_total += (i64)W(k) * W(k) + dinv_len(W(k));
                    }
            };
            for (int r = 0; r < Pr; ++r) lay_owner(r, mycol);
            for (int c = 0; c < Pc; ++c)
                if (c != mycol) lay_owner(myrow, c);
            R.ds_off = (int)dsecs.size();
            auto sec = [&](int g, int root, const Own &o, uint32_t mask) {
                if (!mask || !o.cnt) return;
                const int me = g == G_ROW ? mycol : myrow;
                const bool rcv = me != root && (mask >> me & 1);
                dsecs.push_back({g, root, 0, (me == root || rcv) ? o.start : -1, o.cnt, mask});
                if (me == root) comm_volume += o.cnt * __builtin_popcount(mask);
                else if (rcv) comm_volume += o.cnt;
            };
            if (Pr > 1)
                for (int r = 0; r < Pr; ++r) sec(G_COL, r, own[r * Pc + mycol], own[r * Pc + mycol].cm);
            if (Pc > 1)
                for (int c = 0; c < Pc; ++c) sec(G_ROW, c, own[myrow * Pc + c], own[myrow * Pc + c].rm);
            R.ds_n = (int)dsecs.size() - R.ds_off;
            // ---- panels: L(:,k) along my process row (root = owning column),
            //      U(k,:) along my process column (root = owning row).  The
            //      supernodes of a root are grouped by the set of ranks that
            //      need them (same order on every member), one section per
            //      group and chunk, sent only to those ranks.  Chunk c of a
            //      group holds row group c of its L panels (resp. column group
            //      c of its U panels): the level's sections go out chunk by
            //      chunk, the sender's TRSM of the next chunk beside the
            //      current chunk's transfer, the receivers' Schur tiles of a
            //      chunk as soon as it is in.
            R.ps_off = (int)psecs.size();
            R.pc_off = (int)pcopy.size();
            const int nch = pchunks;
            vector<vector<Sec>> csec(nch);
            vector<vector<CopyItem<T>>> ccp(nch);
            vector<vector<char>> ccp_src(nch);
            auto lay_panels = [&](int g, int root, vector<std::pair<uint32_t, int>> &km) {
                std::sort(km.begin(), km.end());
                const int me = g == G_ROW ? mycol : myrow;
                for (size_t i = 0; i < km.size();) {
                    size_t j = i;
                    while (j < km.size() && km[j].first == km[i].first) ++j;
                    const uint32_t mask = km[i].first;
                    const bool rcv = me != root && (mask >> me & 1);
                    for (int ch = 0; mask && ch < nch; ++ch) {
                        const i64 start = (me == root || rcv) ? pan_total : -1;
                        i64 cnt = 0;
                        for (size_t q = i; q < j; ++q) {
                            const int k = km[q].second;
                            i64 len;
                            if (g == G_ROW) {
                                int m, r0;
                                lrows(k, m, r0);
                                const int gs = lgsz[k], a = ch * gs;
                                if (a >= m) continue;
                                const int rows = std::min(gs, m - a);
                                len = (i64)rows * W(k);
                                if (me == root) {
                                    const int ljb = k / Pc;
                                    add_copy(ccp[ch], ccp_src[ch], /*src*/ 0, lval_off[ljb] + r0 + a,
                                             lval_ld[ljb], 1, pan_total, rows, rows, W(k));
                                } else if (rcv) {
                                    lgpos[k][ch] = pan_total;
                                    if (ch == 0) lpos[k] = pan_total;
                                }
                            } else {
                                const int nc = ucols[k], cs = ucsz[k];
                                if (ch * cs >= nc) continue;
                                const i64 r1 = (ch + 1) * cs < nc ? ugrun[k][ch + 1] : (i64)uidx[k][1];
                                len = r1 - ugrun[k][ch];
                                if (!len) continue;
                                if (me == root) {
                                    add_copy(ccp[ch], ccp_src[ch], /*src*/ 1, uval_off[k / Pr] + ugrun[k][ch], len, 1,
                                             pan_total, len, len, 1);
                                } else if (rcv) {
                                    ugpos[k][ch] = pan_total;
                                    if (ch == 0) upos[k] = pan_total;
                                }
                            }
                            if (me == root || rcv) pan_total += len;
                            cnt += len;
                        }
                        if (!cnt) continue;
                        csec[ch].push_back({g, root, 1, start, cnt, mask});
                        if (me == root) comm_volume += cnt * __builtin_popcount(mask);
                        else if (rcv) comm_volume += cnt;
                    }
                    i = j;
                }
            };
            if (Pc > 1)
                for (int c = 0; c < Pc; ++c) {
                    vector<std::pair<uint32_t, int>> km;
                    for (int k : ks)
                        if (k % Pc == c && lsend(k)) km.push_back({rmask(k) & ~(1u << c), k});
                    lay_panels(G_ROW, c, km);
                }
            if (Pr > 1)
                for (int r = 0; r < Pr; ++r) {
                    vector<std::pair<uint32_t, int>> km;
                    for (int k : ks)
                        if (k % Pr == r && uidx[k]) km.push_back({cmask(k) & ~(1u << r), k});
                    lay_panels(G_COL, r, km);
                }
            R.nch = nch;
            R.ps_o[0] = R.pc_o[0] = 0;
            for (int ch = 0; ch < nch; ++ch) {
                psecs.insert(psecs.end(), csec[ch].begin(), csec[ch].end());
                pcopy.insert(pcopy.end(), ccp[ch].begin(), ccp[ch].end());
                pcopy_src.insert(pcopy_src.end(), ccp_src[ch].begin(), ccp_src[ch].end());
                R.ps_o[ch + 1] = (int)psecs.size() - R.ps_off;
                R.pc_o[ch + 1] = (int)pcopy.size() - R.pc_off;
            }
            R.ps_n = (int)psecs.size() - R.ps_off;
            R.pc_n = (int)pcopy.size() - R.pc_off;
            pan_level.push_back(pan_total);
            dpk_slot = std::max(dpk_slot, dpk_total);
        }
        if (!xmode) return;
        // odd levels use the second panel slot
        // (a 3D layer may factor nothing: no levels)
        const i64 slot = pan_level.empty() ? 0 : *std::max_element(pan_level.begin(), pan_level.end());
        for (size_t L = 1; L < levels.size(); L += 2) {
            const LevelRange &R = levels[L];
            for (int k : bylev[L]) {
                if (lpos[k] >= 0) lpos[k] += slot;
                if (upos[k] >= 0) upos[k] += slot;
                for (int ch = 0; ch < NCHM; ++ch) {
                    if (lgpos[k][ch] >= 0) lgpos[k][ch] += slot;
                    if (ugpos[k][ch] >= 0) ugpos[k][ch] += slot;
                }
            }
            for (int i = R.ps_off; i < R.ps_off + R.ps_n; ++i)
                if (psecs[i].off >= 0) psecs[i].off += slot;
            for (int i = R.pc_off; i < R.pc_off + R.pc_n; ++i)
                pcopy[i].dst = (T *)((intptr_t)pcopy[i].dst + slot);
        }
        pan_total = levels.size() > 1 ? 2 * slot : slot;
        dpk_total = dpk_slot;
    }
    i64 dpk_slot = 0, comm_volume = 0;

    // Copy items are recorded with symbolic bases (src space 0 = L values,
    // 1 = U values; dst = d_dpk (dst_space 0) or d_pan (1)) and relocated in
    // build_device.  Chunked to <= COPY_CHUNK elements.
    vector<char> pcopy_src, dcopy_src;
    static void add_copy(vector<CopyItem<T>> &v, vector<char> &tag, int src_space, i64 src_off,
                         i64 lds, int dst_space, i64 dst_off, i64 ldd, i64 rows, i64 cols) {
        if (cols == 1) {
            for (i64 e = 0; e < rows; e += COPY_CHUNK) {
                CopyItem<T> c{};
                c.src = (const T *)(intptr_t)(src_off + e);
                c.dst = (T *)(intptr_t)(dst_off + e);
                c.lds = c.ldd = 0;
                c.rows = (int)std::min<i64>(COPY_CHUNK, rows - e);
                c.cols = 1;
                v.push_back(c);
                tag.push_back((char)(src_space | (dst_space << 1)));
            }
            return;
        }
        if (lds == rows && ldd == rows) { // contiguous: copy as 1D
            add_copy(v, tag, src_space, src_off, 0, dst_space, dst_off, 0, rows * cols, 1);
            return;
        }
        const i64 cpc = std::max<i64>(1, COPY_CHUNK / std::max<i64>(rows, 1));
        for (i64 c0 = 0; c0 < cols; c0 += cpc) {
            CopyItem<T> c{};
            c.src = (const T *)(intptr_t)(src_off + c0 * lds);
            c.dst = (T *)(intptr_t)(dst_off + c0 * ldd);
            c.lds = lds;
            c.ldd = ldd;
            c.rows = (int)rows;
            c.cols = (int)std::min<i64>(cpc, cols - c0);
            v.push_back(c);
            tag.push_back((char)(src_space | (dst_space << 1)));
        }
    }

    // ------------------------------------------------------- schedule
    // One supernode's (or a chunk of one level's supernodes') share of the
    // schedule; offsets into its own h_* arrays are relocated when merged.
    struct KInfoHost {
        vector<int> dests;
    };
    struct SchedOut {
        vector<DiagItem<T>> diag_items;
        vector<DiagItemF<T>> df_items;
        vector<TrsmLItem<T>> tl_items;
        vector<TrsmUItem<T>> tu_items;
        vector<TrsmItemF<T>> lf_c[NCHM], uf_c[NCHM]; // per exchange chunk
        vector<KInfo<T>> kinfos;
        vector<KInfoHost> khost;
        vector<TileItem> big[2][NCHM], small[2][NCHM]; // [0] critical, [1] rest; per chunk
        vector<CopyItem<T>> dcopy;
        vector<char> dcopy_src;
        vector<int> h_rg, h_ra, h_cg, h_cb, h_pair, h_ct0;
        vector<i64> h_cvoff;
        double panel_flops = 0, schur_flops = 0, schur_flops_padded = 0, scatter_bytes = 0;
        double R_schur_flops = 0, R_big_flops = 0;
        i64 n_diag = 0, n_trsm_items = 0, n_schur_tiles = 0;
        i64 n_ksplit = 0; // KInfo's of updates whose K range is split (SLU_KSPLIT_TILES)
        i64 n_fused = 0;  // tiles that carry a pair's first member as a first K segment
        double fused_flops = 0; // flops of those first segments
        i64 n_mfused = 0;       // the same of mapped pairs (SLU_SCHUR_PAIR_MAP)
        double mfused_flops = 0;
        vector<std::pair<int, int>> far_slots; // (first member of a pair, slot of its far KInfo)
        bool R_big = false;
    };
    vector<KInfoHost> khost;
    i64 n_ksplit_kinfos = 0;

    // ------------------------------------------------------- chained pairs
    // SLU_SCHUR_PAIR (default 1): supernode k and its parent k' one level up
    // form a pair where the rows and U columns of k beyond block k' are
    // exactly the rows and U columns of k' (consecutive members of one
    // separator's chain).  The far x far part of k's update then covers, tile
    // for tile, the update of k'; where the tile of k' is a rest tile, k's is
    // left out at its own level and runs one level later as a first K segment
    // of the tile of k' (TileItem::seg): one prologue and one scatter for
    // both.  Its destinations belong to panels at least three levels up, so
    // nothing reads them before.  Plans of one process only; 0 plans today's
    // schedule exactly.
    int schur_pair = env_int("SLU_SCHUR_PAIR", 1);
    vector<int> pair_next, pair_prev; // the other member of k's pair, or -1
    vector<int> far_kinfo;            // first members: index of the far part's KInfo
    i64 n_pairs = 0, n_fused_tiles = 0;
    double fused_flops = 0; // flops that run as first segments of fused tiles
    static constexpr int SEG_PENDING = INT_MIN; // TileItem::seg = SEG_PENDING + k until the merge
    // SLU_SCHUR_PAIR_MAP (default 1): among the supernodes the exact rule
    // leaves free, k and its parent k' also pair where the far rows and
    // columns of k are in-order subsequences of the rows and columns of k'
    // (k' has rows of other subtrees besides).  A rest tile of k' that holds
    // a row and a column of k runs the far part of k through a row map and
    // mapped column tables as its first K segment (k_schur_big<T, 2>); the far
    // elements of k in critical tile rows / columns of k' (one range of its
    // far rows, one of its far columns, else no pair) run at k's own level as
    // rectangles of their own.  A pair is formed only while the first
    // segments' work on whole tiles of k' stays within 1 +
    // SLU_SCHUR_PAIR_MAP_WASTE (default 0.05) of the far part's own.
    // 0 plans the exact pairs only.
    int schur_pair_map = env_int("SLU_SCHUR_PAIR_MAP", 1);
    double pair_map_waste = [] {
        const char *s = getenv("SLU_SCHUR_PAIR_MAP_WASTE");
        return s && *s ? atof(s) : 0.05;
    }();
    struct MapPair {
        vector<int> rmap, cmap;     // per row / column of k': index among the far rows / columns of k, or -1
        int fm, fn;                 // far rows and columns of k
        int r_lo, r_hi, c_lo, c_hi; // far rows / columns of k in critical tile rows / columns of k'
    };
    vector<MapPair> map_pairs;
    vector<int> pair_map; // first members of mapped pairs: index into map_pairs, else -1
    i64 n_map_pairs = 0, n_map_fused_tiles = 0;
    double map_fused_flops = 0, map_work = 0, map_useful = 0;

    // rows of L(:,k) below the diagonal block: global index and block of each
    void sn_rows(int k, vector<int> &rg, vector<int> &rblk) const {
        rg.clear();
        rblk.clear();
        const int_t *ix = lidx[k];
        i64 p = SLU_BC_HEADER;
        for (i64 b = 0; b < ix[0]; ++b) {
            const int gb = (int)ix[p], nr = (int)ix[p + 1];
            for (int i = 0; gb != k && i < nr; ++i) {
                rg.push_back((int)ix[p + 2 + i]);
                rblk.push_back(gb);
            }
            p += SLU_LB_DESCRIPTOR + nr;
        }
    }
    // nonempty columns of U(k,:): global index, block and segment start of each
    void sn_cols(int k, vector<int> &cg, vector<int> &cblk, vector<int> &t0) const {
        cg.clear();
        cblk.clear();
        t0.clear();
        const int_t *ix = uidx[k];
        const i64 klst = xsup[k + 1];
        i64 p = SLU_BR_HEADER;
        for (i64 b = 0; b < ix[0]; ++b) {
            const int jb = (int)ix[p];
            for (int c = 0; c < W(jb); ++c) {
                const i64 fst = ix[p + SLU_UB_DESCRIPTOR + c];
                if (fst >= klst) continue;
                cg.push_back((int)xsup[jb] + c);
                cblk.push_back(jb);
                t0.push_back((int)(fst - xsup[k]));
            }
            p += SLU_UB_DESCRIPTOR + W(jb);
        }
    }
    void build_pairs() {
        pair_next.assign(nsupers, -1);
        pair_prev.assign(nsupers, -1);
        far_kinfo.assign(nsupers, -1);
        pair_map.assign(nsupers, -1);
        if (!schur_pair || xmode || zmode) return;
        constexpr int BBN = BigCfg<T>::BN;
        // (an update that SLU_KSPLIT_TILES may split is left alone)
        auto may_split = [&](int k) { return ksplit_tiles > 0 && bylev[level_of[k]].size() <= 2; };
        vector<int> rg, rb, cg, cb, t0, rg2, rb2, cg2, cb2, t02;
        // ascending k: along a chain greedily from its first member
        for (int k = 0; k < nsupers; ++k) {
            if (pair_prev[k] >= 0 || !lidx[k] || !uidx[k] || may_split(k)) continue;
            int m = 0, r0 = 0;
            lrows(k, m, r0);
            if (m < SB_BM) continue;
            sn_rows(k, rg, rb);
            sn_cols(k, cg, cb, t0);
            const int n_ = (int)cg.size();
            if (n_ < BBN) continue;
            const int kp = rb[0];
            if (cb[0] != kp || level_of[kp] != level_of[k] + 1 || pair_prev[kp] >= 0) continue;
            if (!lidx[kp] || !uidx[kp] || may_split(kp)) continue;
            int nr0 = 0, nc0 = 0;
            while (nr0 < m && rb[nr0] == kp) ++nr0;
            while (nc0 < n_ && cb[nc0] == kp) ++nc0;
            if (m - nr0 < SB_BM || n_ - nc0 < BBN) continue; // k' runs big tiles too
            sn_rows(kp, rg2, rb2);
            sn_cols(kp, cg2, cb2, t02);
            if ((int)rg2.size() != m - nr0 || (int)cg2.size() != n_ - nc0) continue;
            if (!std::equal(rg2.begin(), rg2.end(), rg.begin() + nr0) ||
                !std::equal(cg2.begin(), cg2.end(), cg.begin() + nc0))
                continue;
            pair_next[k] = kp;
            pair_prev[kp] = k;
            ++n_pairs;
        }
        if (!schur_pair_map) return;
        // second pass: mapped pairs over the supernodes still free
        for (int k = 0; k < nsupers; ++k) {
            if (pair_prev[k] >= 0 || pair_next[k] >= 0 || !lidx[k] || !uidx[k] || may_split(k)) continue;
            int m = 0, r0 = 0;
            lrows(k, m, r0);
            if (m < SB_BM) continue;
            sn_rows(k, rg, rb);
            sn_cols(k, cg, cb, t0);
            const int n_ = (int)cg.size();
            if (n_ < BBN) continue;
            const int kp = rb[0];
            if (cb[0] != kp || level_of[kp] != level_of[k] + 1 || pair_prev[kp] >= 0 || pair_next[kp] >= 0) continue;
            if (!lidx[kp] || !uidx[kp] || may_split(kp)) continue;
            int nr0 = 0, nc0 = 0;
            while (nr0 < m && rb[nr0] == kp) ++nr0;
            while (nc0 < n_ && cb[nc0] == kp) ++nc0;
            const int fm = m - nr0, fn = n_ - nc0;
            if (fm < SB_BM || fn < BBN) continue;
            sn_rows(kp, rg2, rb2);
            sn_cols(kp, cg2, cb2, t02);
            MapPair mp;
            mp.fm = fm;
            mp.fn = fn;
            // in-order subsequence: every far row (column) of k found, in order
            auto submap = [](const vector<int> &sub, int s0, const vector<int> &all, vector<int> &map) {
                map.assign(all.size(), -1);
                size_t p = s0;
                for (size_t q = 0; q < all.size() && p < sub.size(); ++q)
                    if (all[q] == sub[p]) map[q] = (int)(p++ - s0);
                return p == sub.size();
            };
            if (!submap(rg, nr0, rg2, mp.rmap) || !submap(cg, nc0, cg2, mp.cmap)) continue;
            // tiles of k' : the rows and columns of k they hold; critical tile
            // rows and columns of k' (a destination block one level above k')
            const int m2 = (int)rg2.size(), n2 = (int)cg2.size();
            const int tm2 = (m2 + SB_BM - 1) / SB_BM, tn2 = (n2 + BBN - 1) / BBN;
            vector<int> rcnt(tm2, 0), ccnt(tn2, 0);
            vector<char> crow(tm2, 0), ccol(tn2, 0);
            for (int r = 0; r < m2; ++r) {
                rcnt[r / SB_BM] += mp.rmap[r] >= 0;
                if (level_of[rb2[r]] == level_of[kp] + 1) crow[r / SB_BM] = 1;
            }
            for (int c = 0; c < n2; ++c) {
                ccnt[c / BBN] += mp.cmap[c] >= 0;
                if (level_of[cb2[c]] == level_of[kp] + 1) ccol[c / BBN] = 1;
            }
            // the rows (columns) of k in critical tile rows (columns) of k': one range
            auto crange = [](const vector<int> &map, const vector<char> &crit, int B, int &lo, int &hi) {
                int cnt = 0;
                lo = INT_MAX, hi = -1;
                for (size_t q = 0; q < map.size(); ++q)
                    if (map[q] >= 0 && crit[q / B]) {
                        lo = std::min(lo, map[q]);
                        hi = std::max(hi, map[q] + 1);
                        ++cnt;
                    }
                if (!cnt) lo = hi = 0;
                return cnt == hi - lo;
            };
            if (!crange(mp.rmap, crow, SB_BM, mp.r_lo, mp.r_hi) || !crange(mp.cmap, ccol, BBN, mp.c_lo, mp.c_hi)) continue;
            // first-segment MFMA work on the tiles that hold a row and a column of k
            double work = 0;
            i64 el_fused = 0, nfused = 0;
            for (int i = 0; i < tm2; ++i)
                for (int j = 0; j < tn2; ++j) {
                    if (!rcnt[i] || !ccnt[j]) continue;
                    work += (double)std::min(SB_BM, m2 - i * SB_BM) * std::min(BBN, n2 - j * BBN);
                    if (!crow[i] && !ccol[j]) {
                        el_fused += (i64)rcnt[i] * ccnt[j];
                        ++nfused;
                    }
                }
            if (work > (1.0 + pair_map_waste) * fm * fn || !nfused) continue;
            // every far element once: here by a part of k's own, or in one fused tile
            SLU_REQUIRE(el_fused == (i64)(fm - (mp.r_hi - mp.r_lo)) * (fn - (mp.c_hi - mp.c_lo)),
                        "mapped pair (%d, %d): %lld far elements in fused tiles", k, kp, (long long)el_fused);
            pair_next[k] = kp;
            pair_prev[kp] = k;
            pair_map[k] = (int)map_pairs.size();
            map_pairs.push_back(std::move(mp));
            map_work += 2.0 * W(k) * work;
            map_useful += 2.0 * W(k) * fm * fn;
            ++n_map_pairs;
        }
    }

    template <typename V> static void append(V &dst, const V &src) {
        dst.insert(dst.end(), src.begin(), src.end());
    }
    template <typename P> static P *shift(P *p, i64 d) { return (P *)((intptr_t)p + d); }

    double t_addsn = 0, t_merge = 0, t_resize = 0, t_put = 0, t_tiles = 0;
    // Supernodes are scheduled in chunks (a level's supernodes in order, the
    // levels in order) into SchedOut's, all chunks of all levels at once
    // (add_supernode reads only the plan's structure); the tables are then
    // sized once and every chunk copies (and relocates) its slices in
    // parallel, which reproduces the sequential layout exactly.  Sizing per
    // level instead regrew and value-initialised every table once per level,
    // serially (66 of the 131 ms at 100^3).
    void build_schedule() {
        // value buffers first: work items point straight into them
        d_dpk.alloc(std::max<i64>(dpk_total, 1));
        d_pan.alloc_guarded(std::max<i64>(pan_total, 1), SB_UGUARD);
        d_dinv.alloc(std::max<i64>(dscr_max, 1));
        const int NL = (int)levels.size();
        vector<int> first(NL + 1, 0); // chunks of level L: [first[L], first[L+1])
        for (int L = 0; L < NL; ++L) {
            const int nk = (int)bylev[L].size();
            first[L + 1] = first[L] + (nk >= 128 ? std::min(4 * plan_threads(), nk / 32) : 1);
        }
        const int NC = first[NL];
        vector<SchedOut> outs(NC);
        const auto ta = std::chrono::steady_clock::now();
        parallel_for(NC, [&](int t) {
            const int L = (int)(std::upper_bound(first.begin(), first.end(), t) - first.begin()) - 1;
            const vector<int> &ks = bylev[L];
            const i64 nk = (i64)ks.size(), nch = first[L + 1] - first[L], c = t - first[L];
            for (i64 i = nk * c / nch; i < nk * (c + 1) / nch; ++i) add_supernode(ks[i], outs[t]);
        }, 1);
        t_addsn += ms_since(ta);
        const auto tm0 = std::chrono::steady_clock::now();
        enum { V_DIAG, V_DF, V_TL, V_TU, V_LF, V_UF, V_K, V_DC, V_RG, V_CG, V_PAIR, V_N };
        vector<std::array<i64, V_N>> base(NC + 1);
        {
            SLU_REQUIRE(kinfos.empty() && h_rg.empty() && h_cg.empty() && h_pair.empty(),
                        "build_schedule runs once per plan");
            std::array<i64, V_N> b = {(i64)diag_items.size(), (i64)df_items.size(), (i64)tl_items.size(),
                                      (i64)tu_items.size(), (i64)lf_items.size(), (i64)uf_items.size(),
                                      0, (i64)dcopy.size(), 0, 0, 0};
            for (int t = 0; t < NC; ++t) {
                const SchedOut &O = outs[t];
                base[t] = b;
                b[V_DIAG] += O.diag_items.size();
                b[V_DF] += O.df_items.size();
                b[V_TL] += O.tl_items.size();
                b[V_TU] += O.tu_items.size();
                for (int ch = 0; ch < NCHM; ++ch) {
                    b[V_LF] += O.lf_c[ch].size();
                    b[V_UF] += O.uf_c[ch].size();
                }
                b[V_K] += O.kinfos.size();
                b[V_DC] += O.dcopy.size();
                b[V_RG] += O.h_rg.size();
                b[V_CG] += O.h_cg.size();
                b[V_PAIR] += O.h_pair.size();
            }
            base[NC] = b;
            for (int t = 0; t < NC; ++t)
                for (const auto &fs : outs[t].far_slots) far_kinfo[fs.first] = (int)base[t][V_K] + fs.second;
            diag_items.resize(b[V_DIAG]);
            df_items.resize(b[V_DF]);
            tl_items.resize(b[V_TL]);
            tu_items.resize(b[V_TU]);
            lf_items.resize(b[V_LF]);
            uf_items.resize(b[V_UF]);
            kinfos.resize(b[V_K]);
            khost.resize(b[V_K]);
            dcopy.resize(b[V_DC]);
            dcopy_src.resize(b[V_DC]);
            h_rg.resize_uninit(b[V_RG]);
            h_ra.resize_uninit(b[V_RG]);
            h_cg.resize_uninit(b[V_CG]);
            h_cb.resize_uninit(b[V_CG]);
            h_ct0.resize_uninit(b[V_CG]);
            h_cvoff.resize_uninit(b[V_CG]);
            h_pair.resize_uninit(b[V_PAIR]);
        }
        t_resize += ms_since(tm0);
        // the TRSM items of a level chunk by chunk (each chunk's items of all
        // the level's supernode groups together), so that one launch covers
        // a chunk
        vector<std::array<i64, NCHM>> lfpos(NC), ufpos(NC);
        for (int L = 0; L < NL; ++L) {
            LevelRange &R = levels[L];
            i64 pl = base[first[L]][V_LF], pu = base[first[L]][V_UF];
            const i64 l0 = pl, u0 = pu;
            R.lf_o[0] = R.uf_o[0] = 0;
            for (int ch = 0; ch < NCHM; ++ch) {
                for (int t = first[L]; t < first[L + 1]; ++t) {
                    lfpos[t][ch] = pl;
                    ufpos[t][ch] = pu;
                    pl += outs[t].lf_c[ch].size();
                    pu += outs[t].uf_c[ch].size();
                }
                if (ch < R.nch) {
                    R.lf_o[ch + 1] = (int)(pl - l0);
                    R.uf_o[ch + 1] = (int)(pu - u0);
                } else {
                    SLU_REQUIRE(pl - l0 == R.lf_o[R.nch] && pu - u0 == R.uf_o[R.nch],
                                "level %d: TRSM items past the level's %d chunks", L, R.nch);
                }
            }
        }
        const auto tp0 = std::chrono::steady_clock::now();
        parallel_for(NC, [&](int c) {
            SchedOut &O = outs[c];
            const std::array<i64, V_N> &B = base[c];
            const i64 bc = B[V_CG], br = B[V_RG], bp = B[V_PAIR];
            for (auto &k : O.kinfos) {
                k.cvoff = shift(k.cvoff, bc);
                k.ct0 = shift(k.ct0, bc);
                k.cg = shift(k.cg, bc);
                k.cb = shift(k.cb, bc);
                k.rg = shift(k.rg, br);
                k.ra = shift(k.ra, br);
                k.pair = shift(k.pair, bp);
            }
            for (auto &v : O.uf_c)
                for (auto &t : v) {
                    t.voff = shift(t.voff, bc);
                    t.t0 = shift(t.t0, bc);
                }
            for (auto &t : O.tu_items) {
                t.voff = shift(t.voff, bc);
                t.t0 = shift(t.t0, bc);
            }
            auto put = [](auto &dst, const auto &src, i64 at) {
                std::copy(src.begin(), src.end(), dst.data() + at);
            };
            put(diag_items, O.diag_items, B[V_DIAG]);
            put(df_items, O.df_items, B[V_DF]);
            put(tl_items, O.tl_items, B[V_TL]);
            put(tu_items, O.tu_items, B[V_TU]);
            for (int ch = 0; ch < NCHM; ++ch) {
                put(lf_items, O.lf_c[ch], lfpos[c][ch]);
                put(uf_items, O.uf_c[ch], ufpos[c][ch]);
            }
            put(kinfos, O.kinfos, B[V_K]);
            for (size_t i = 0; i < O.khost.size(); ++i) khost[B[V_K] + i] = std::move(O.khost[i]);
            put(dcopy, O.dcopy, B[V_DC]);
            put(dcopy_src, O.dcopy_src, B[V_DC]);
            put(h_rg, O.h_rg, br);
            put(h_ra, O.h_ra, br);
            put(h_cg, O.h_cg, bc);
            put(h_cb, O.h_cb, bc);
            put(h_ct0, O.h_ct0, bc);
            put(h_cvoff, O.h_cvoff, bc);
            put(h_pair, O.h_pair, bp);
        }, 1);
        t_put += ms_since(tp0);
        vector<int> owner(lblk.size() + ublk.size(), -1), touched;
        for (int L = 0; L < NL; ++L) {
            const auto tt0 = std::chrono::steady_clock::now();
            LevelRange &R = levels[L];
            const std::array<i64, V_N> &B0 = base[first[L]], &B1 = base[first[L + 1]];
            R.diag_off = (int)B0[V_DIAG];
            R.tl_off = (int)B0[V_TL];
            R.tu_off = (int)B0[V_TU];
            R.k_off = (int)B0[V_K];
            R.tile_off = (int)tiles.size();
            R.big_off = (int)tiles_big.size();
            R.df_off = (int)B0[V_DF];
            R.lf_off = (int)B0[V_LF];
            R.uf_off = (int)B0[V_UF];
            R.dc_off = (int)B0[V_DC];
            for (int t = first[L]; t < first[L + 1]; ++t) {
                const SchedOut &O = outs[t];
                stats.panel_flops += O.panel_flops;
                stats.schur_flops += O.schur_flops;
                stats.schur_flops_padded += O.schur_flops_padded;
                stats.scatter_bytes += O.scatter_bytes;
                stats.n_diag += O.n_diag;
                stats.n_trsm_items += O.n_trsm_items;
                stats.n_schur_tiles += O.n_schur_tiles;
                n_ksplit_kinfos += O.n_ksplit;
                n_fused_tiles += O.n_fused;
                fused_flops += O.fused_flops;
                R.fused_n += (int)O.n_fused;
                n_map_fused_tiles += O.n_mfused;
                map_fused_flops += O.mfused_flops;
                R.mapped_n += (int)O.n_mfused;
                R.schur_flops += O.R_schur_flops;
                R.big_flops += O.R_big_flops;
                R.big = R.big || O.R_big;
            }
            // critical tiles first: they are launched ahead of the rest so the
            // next level's panels can be factored while the rest runs
            // (chunk by chunk within each class: prefix offsets bc_o / br_o,
            // sc_o / sr_o relative to the class's first tile)
            for (int cls = 0; cls < 2; ++cls) {
                const int b0 = (int)tiles_big.size(), s0 = (int)tiles.size();
                int *bo = cls ? R.br_o : R.bc_o, *so = cls ? R.sr_o : R.sc_o;
                bo[0] = so[0] = 0;
                for (int ch = 0; ch < NCHM; ++ch) {
                    for (int t = first[L]; t < first[L + 1]; ++t) {
                        const int kb = (int)(base[t][V_K] - R.k_off);
                        for (TileItem x : outs[t].big[cls][ch]) {
                            x.kslot += kb;
                            if (x.seg < SEG_PENDING + nsupers) { // fused: the first member's far KInfo
                                const int fk = far_kinfo[x.seg - SEG_PENDING];
                                SLU_REQUIRE(fk >= 0 && fk < R.k_off, "level %d: fused tile without its first segment", L);
                                x.seg = fk - R.k_off;
                            } else {
                                x.seg += kb;
                            }
                            tiles_big.push_back(x);
                        }
                        for (TileItem x : outs[t].small[cls][ch]) {
                            SLU_REQUIRE(x.seg >= 0, "level %d: a 64x64 tile with a deferred first segment", L);
                            x.kslot += kb;
                            x.seg = x.kslot;
                            tiles.push_back(x);
                        }
                    }
                    if (ch < R.nch) {
                        bo[ch + 1] = (int)tiles_big.size() - b0;
                        so[ch + 1] = (int)tiles.size() - s0;
                    } else {
                        SLU_REQUIRE((int)tiles_big.size() - b0 == bo[R.nch] && (int)tiles.size() - s0 == so[R.nch],
                                    "level %d: Schur tiles past the level's %d chunks", L, R.nch);
                    }
                }
                if (cls == 0) {
                    R.bigc_n = bo[R.nch];
                    R.tilec_n = so[R.nch];
                } else if (R.fused_n + R.mapped_n > 0) {
                    // the fused tiles last among the rest tiles, those of
                    // mapped pairs after those of exact pairs: they go out
                    // as launches of the two-segment kernels (one-process
                    // plans only: one chunk)
                    SLU_REQUIRE(!xmode && R.nch == 1, "level %d: fused tiles on a grid", L);
                    auto e = std::stable_partition(tiles_big.begin() + b0, tiles_big.end(),
                                                   [](const TileItem &x) { return x.seg == x.kslot; });
                    auto e2 = std::stable_partition(e, tiles_big.end(), [&](const TileItem &x) {
                        return !kinfos[R.k_off + x.seg].mapped;
                    });
                    SLU_REQUIRE(e2 - e == R.fused_n && tiles_big.end() - e2 == R.mapped_n,
                                "level %d: %d + %d fused tiles, %d + %d counted", L, (int)(e2 - e),
                                (int)(tiles_big.end() - e2), R.fused_n, R.mapped_n);
                }
            }
            R.big_n = (int)tiles_big.size() - R.big_off;
            R.df_n = (int)(B1[V_DF] - B0[V_DF]);
            for (int i = R.df_off; i < R.df_off + R.df_n; ++i) R.df_maxw = std::max(R.df_maxw, df_items[i].w);
            R.lf_n = (int)(B1[V_LF] - B0[V_LF]);
            R.uf_n = (int)(B1[V_UF] - B0[V_UF]);
            for (int i = R.lf_off; i < R.lf_off + R.lf_n; ++i) R.tf_maxw = std::max(R.tf_maxw, lf_items[i].w);
            for (int i = R.uf_off; i < R.uf_off + R.uf_n; ++i) R.tf_maxw = std::max(R.tf_maxw, uf_items[i].w);
            R.diag_n = (int)(B1[V_DIAG] - B0[V_DIAG]);
            R.tl_n = (int)(B1[V_TL] - B0[V_TL]);
            R.tu_n = (int)(B1[V_TU] - B0[V_TU]);
            R.k_n = (int)(B1[V_K] - B0[V_K]);
            R.tile_n = (int)tiles.size() - R.tile_off;
            R.dc_n = (int)(B1[V_DC] - B0[V_DC]);
            t_tiles += ms_since(tt0);
            // conflicting destinations inside the level -> atomics
            touched.clear();
            for (int s = R.k_off; s < R.k_off + R.k_n; ++s) {
                KInfoHost &kh = khost[s];
                for (int h : kh.dests) {
                    int key = h >= 0 ? h : (int)lblk.size() + ~h;
                    if (owner[key] == -1) {
                        owner[key] = s;
                        touched.push_back(key);
                    } else if (owner[key] != s) {
                        kinfos[owner[key]].atomic = 1;
                        kinfos[s].atomic = 1;
                    }
                }
            }
            for (int key : touched) owner[key] = -1;
            for (int i = R.big_off; i < R.big_off + R.big_n; ++i)
                R.atomic_tiles += kinfos[R.k_off + tiles_big[i].kslot].atomic;
            for (int i = R.tile_off; i < R.tile_off + R.tile_n; ++i)
                R.atomic_tiles += kinfos[R.k_off + tiles[i].kslot].atomic;
        }
        t_merge += ms_since(tm0);
        khost.clear();
    }

    void add_supernode(int k, SchedOut &O) const {
        const int w = W(k);
        const int ljb = k / Pc, lb = k / Pr;
        const bool lcol_here = (k % Pc) == mycol && lidx[k];
        const bool urow_here = (k % Pr) == myrow && uidx[k];
        const bool diag_here = lcol_here && (k % Pr) == myrow;
        const bool fast = fast_w(w);
        const int nbk = (w + PW - 1) / PW;
        constexpr int RB = cplx ? RBOf<T>::v : 16 * TR_WAVES;
        // ---- diagonal block: factored in place by its owner; other ranks of
        // its process row / column read the broadcast package
        T *dT = nullptr, *dinv = nullptr;
        int dld = 0;
        if (diag_here) {
            SLU_REQUIRE(lblk_ib[lcol_first[ljb]] == k, "diagonal block of %d is not first", k);
            dT = d_L.p + lval_off[ljb];
            dld = lval_ld[ljb];
            dinv = xmode ? d_dpk.p + pkg[k] + (i64)w * w : d_dinv.p + dscr[k];
        } else if (pkg[k] >= 0) {
            dT = d_dpk.p + pkg[k];
            dld = w;
            dinv = dT + (i64)w * w;
        }
        if (diag_here) {
            if (fast) {
                DiagItemF<T> d{};
                d.a = dT;
                d.dinv = dinv;
                d.ld = dld;
                d.w = w;
                d.k = k;
                d.fcol = (int)xsup[k];
                O.df_items.push_back(d);
            } else {
                DiagItem<T> d{};
                d.a = dT;
                d.ld = dld;
                d.w = w;
                d.k = k;
                d.fcol = (int)xsup[k];
                O.diag_items.push_back(d);
            }
            if (xmode) add_copy(O.dcopy, O.dcopy_src, 0, lval_off[ljb], dld, 0, pkg[k], w, w, w);
            O.n_diag++;
            // SRC/pdgstrf2.c:252,262 (complex weights SRC/pzgstrf2.c:253,263)
            double wd = w, s1 = wd * (wd - 1) / 2, s2 = (wd - 1) * wd * (2 * wd - 1) / 6;
            O.panel_flops += cplx ? 6 * s1 + 10 * wd + 8 * s2 : s1 + 2 * s2;
        }
        // ---- L panel TRSM (rows of column k below the diagonal block)
        int m = 0, r0 = 0;
        lrows(k, m, r0);
        if (lcol_here && m > 0) {
            SLU_REQUIRE(dT, "no diagonal block for the L panel of %d", k);
            if (fast) {
                for (int c0 = 0; c0 < m; c0 += RB) {
                    TrsmItemF<T> t{};
                    t.x = d_L.p + lval_off[ljb] + r0 + c0;
                    t.t = dT;
                    t.dinv = dinv;
                    t.ldx = lval_ld[ljb];
                    t.ldt = dld;
                    t.w = w;
                    t.nrows = std::min(RB, m - c0);
                    O.lf_c[xmode ? c0 / lgsz[k] : 0].push_back(t); // (RB divides the group size)
                    O.n_trsm_items++;
                }
            } else {
                for (int c0 = 0; c0 < m; c0 += TRSM_THREADS) {
                    TrsmLItem<T> t{};
                    t.x = d_L.p + lval_off[ljb] + r0 + c0;
                    t.u = dT;
                    t.ldx = lval_ld[ljb];
                    t.ldu = dld;
                    t.w = w;
                    t.nrows = std::min(TRSM_THREADS, m - c0);
                    O.tl_items.push_back(t);
                    O.n_trsm_items++;
                }
            }
            O.panel_flops += (cplx ? 4.0 : 1.0) * (double)w * (w + 1) * m;
        }
        // ---- U panel: nonempty columns of block row k on my process column
        vector<int> ujb; // U blocks with a nonempty column
        int ncols = 0, kmin = w;
        const int cols_off = (int)O.h_cg.size();
        if (uidx[k]) {
            const int_t *ix = uidx[k];
            const i64 klst = xsup[k + 1];
            const i64 base = urow_here ? uval_off[lb] : upos[k];
            i64 p = SLU_BR_HEADER, run = 0;
            for (i64 b = 0; b < ix[0]; ++b) {
                const int jb = (int)ix[p];
                const int bidx = (int)ujb.size();
                bool any = false;
                for (int c = 0; c < W(jb); ++c) {
                    const i64 fst = ix[p + SLU_UB_DESCRIPTOR + c];
                    if (fst >= klst) continue;
                    any = true;
                    O.h_cg.push_back((int)xsup[jb] + c);
                    O.h_cb.push_back(bidx);
                    if (xmode && !urow_here) { // received in column groups (layout_values)
                        const int g = ncols / ucsz[k];
                        O.h_cvoff.push_back(ugpos[k][g] + run - ugrun[k][g]);
                    } else {
                        O.h_cvoff.push_back(base + run);
                    }
                    const int t0 = (int)(fst - xsup[k]);
                    O.h_ct0.push_back(t0);
                    kmin = std::min(kmin, t0);
                    ++ncols;
                    run += klst - fst;
                    if (urow_here) {
                        double seg = (double)(klst - fst);
                        O.panel_flops += seg * (seg + 1);
                    }
                }
                if (any) ujb.push_back(jb);
                p += SLU_UB_DESCRIPTOR + W(jb);
            }
            SLU_REQUIRE(run == ix[1], "U row %d: segment lengths %lld != %lld", k, (long long)run,
                        (long long)ix[1]);
        }
        if (urow_here && ncols > 0) {
            SLU_REQUIRE(dT, "no diagonal block for the U panel of %d", k);
            for (int c0 = 0; fast && c0 < ncols; c0 += RB) {
                TrsmItemF<T> t{};
                t.x = d_U.p;
                t.voff = (const i64 *)(intptr_t)(cols_off + c0); // relocated
                t.t0 = (const int *)(intptr_t)(cols_off + c0);
                t.t = dT;
                t.dinv = dinv + (i64)nbk * PW * PW;
                t.ldt = dld;
                t.w = w;
                t.nrows = std::min(RB, ncols - c0);
                O.uf_c[xmode ? c0 / ucsz[k] : 0].push_back(t);
                O.n_trsm_items++;
            }
            for (int c0 = 0; !fast && c0 < ncols; c0 += TRSM_THREADS) {
                TrsmUItem<T> t{};
                t.l = dT;
                t.ubase = d_U.p;
                t.ldl = dld;
                t.w = w;
                t.ncols = std::min(TRSM_THREADS, ncols - c0);
                t.voff = (const i64 *)(intptr_t)(cols_off + c0); // relocated
                t.t0 = (const int *)(intptr_t)(cols_off + c0);
                int km = w;
                for (int c = 0; c < t.ncols; ++c) km = std::min(km, O.h_ct0[cols_off + c0 + c]);
                t.kmin = km;
                O.tu_items.push_back(t);
                O.n_trsm_items++;
            }
        }
        if (m == 0 || ncols == 0) return; // nothing to update from k here
        // ---- Schur update of k on this rank's destinations
        KInfo<T> ki{};
        if (!lcol_here) SLU_REQUIRE(lpos[k] >= 0, "L panel %d not received", k);
        SLU_REQUIRE(urow_here || upos[k] >= 0, "U panel %d not received", k);
        ki.ubase = urow_here ? d_U.p : d_pan.p;
        ki.n = ncols;
        ki.kmin = kmin;
        ki.kw = w - kmin;
        ki.nub = (int)ujb.size();
        ki.cvoff = (const i64 *)(intptr_t)cols_off;
        ki.ct0 = (const int *)(intptr_t)cols_off;
        ki.cg = (const int *)(intptr_t)cols_off;
        ki.cb = (const int *)(intptr_t)cols_off;
        const int rows_off = (int)O.h_rg.size();
        vector<int> lib_; // L blocks (ib) of the panel below the diagonal
        {
            const int_t *ix = lidx[k];
            i64 p = SLU_BC_HEADER;
            for (i64 b = 0; b < ix[0]; ++b) {
                const int gb = (int)ix[p], nr = (int)ix[p + 1];
                if (gb != k) {
                    const int a = (int)lib_.size();
                    lib_.push_back(gb);
                    for (int i = 0; i < nr; ++i) {
                        O.h_rg.push_back((int)ix[p + 2 + i]);
                        O.h_ra.push_back(a);
                    }
                }
                p += SLU_LB_DESCRIPTOR + nr;
            }
        }
        const int pair_off = (int)O.h_pair.size();
        KInfoHost kh;
        for (int ib : lib_)
            for (int jb : ujb) {
                int h = ib >= jb ? find_lblk(ib, jb) : ~find_ublk(ib, jb);
                O.h_pair.push_back(h);
                kh.dests.push_back(h);
            }
        ki.pair = (const int *)(intptr_t)pair_off;
        ki.atomic = 0;
        constexpr int BBN = BigCfg<T>::BN; // 128 (d, s) or 64 (z) columns per big tile
        const bool big = m >= SB_BM && ncols >= BBN;
        const int BM = big ? SB_BM : SC_BM, BN = big ? BBN : SC_BN;
        const int tm = (m + BM - 1) / BM, tn = (ncols + BN - 1) / BN;
        // K split near the root: a level of one or two supernodes whose
        // update is a few 128 x 128 tiles leaves most CUs idle for a whole
        // tile's latency (K up to 256: ~90 us).  Its K range is cut into
        // chunks of >= 64, one KInfo per chunk (same tables, kmin / kw
        // moved); the chunks' tiles add into the same destinations, which
        // the level's conflict analysis below turns into atomic scatters.
        int nsplit = 1;
        if (ksplit_tiles > 0 && big && bylev[level_of[k]].size() <= 2 && tm * tn < ksplit_tiles)
            nsplit = std::max(1, std::min({4, (w - kmin) / 64, ksplit_tiles / (tm * tn)}));
        const int kch = ((w - kmin + nsplit - 1) / nsplit + 15) / 16 * 16;
        // A destination (ib,jb) belongs to the panel of supernode min(ib,jb);
        // it is critical when that panel is factored at the next level.  All
        // destinations in a row of L block ib (resp. a column of U block jb)
        // with level(ib) == level(k)+1 are critical, and no others.
        const int nl = level_of[k] + 1;
        vector<char> ccol(tn, 0);
        for (int c = 0; c < ncols; ++c)
            if (level_of[ujb[O.h_cb[cols_off + c]]] == nl) ccol[c / BN] = 1;
        // 2D grids: one KInfo per row group of the L panel (its own rows,
        // base and leading dimension: a received group is column-major with
        // ld = its rows), the tiles of a group in the exchange chunk of their
        // rows and columns
        const int gs = xmode ? lgsz[k] : m, ng = xmode ? ngroups(m, gs) : 1;
        const double mult = cplx ? 4.0 : 1.0; // complex: 8 real flops per multiply-add
        // ---- a pair's members (build_pairs)
        const int knext = pair_next[k], kprev = pair_prev[k];
        vector<int> pcg, pcb, pt0; // second member: the first member's columns
        double fl_fused = 0, fl_deferred = 0, el_deferred = 0;
        double fl_small = 0; // first member: flops of the parts that run 64x64 tiles
        i64 ntiles = (i64)tm * tn;
        if (kprev >= 0) sn_cols(kprev, pcg, pcb, pt0);
        // second member of a mapped pair: rows / columns of the first per tile row / column
        const MapPair *pmp = kprev >= 0 && pair_map[kprev] >= 0 ? &map_pairs[pair_map[kprev]] : nullptr;
        vector<int> prc(pmp ? tm : 0, 0), pcc(pmp ? tn : 0, 0);
        double fl_mfused = 0;
        if (pmp) {
            SLU_REQUIRE(big && (int)pmp->rmap.size() == m && (int)pmp->cmap.size() == ncols,
                        "mapped pair (%d, %d): %d x %d", kprev, k, m, ncols);
            for (int r = 0; r < m; ++r) prc[r / BM] += pmp->rmap[r] >= 0;
            for (int c = 0; c < ncols; ++c) pcc[c / BN] += pmp->cmap[c] >= 0;
        }
        if (knext >= 0) {
            // First member: the update in three parts, each a KInfo with a
            // tile grid of its own: near rows x all columns, far rows x near
            // columns (destinations in the panels of k': critical), and far
            // x far from (nr0, nc0), whose tiles coincide with the tiles of
            // k'.  A far tile is deferred to the twin tile of k' where that
            // one is a rest tile; it runs here, as before, where the twin is
            // critical (destinations in the panels two levels up).
            int nr0 = 0, nc0 = 0;
            while (nr0 < m && lib_[O.h_ra[rows_off + nr0]] == knext) ++nr0;
            while (nc0 < ncols && ujb[O.h_cb[cols_off + nc0]] == knext) ++nc0;
            // (twin: the far part of an exact pair)
            struct Part {
                int r0, c0, m, n;
                bool twin;
            };
            vector<Part> parts = {{0, 0, nr0, ncols, false}, {nr0, 0, m - nr0, nc0, false}};
            const MapPair *mp = pair_map[k] >= 0 ? &map_pairs[pair_map[k]] : nullptr;
            if (!mp) {
                parts.push_back({nr0, nc0, m - nr0, ncols - nc0, true});
            } else {
                // Mapped pair: the far elements in critical tile rows of k'
                // (far rows [r_lo, r_hi) x all far columns) and, of the other
                // far rows, those in its critical tile columns run here; the
                // rest is deferred to the fused tiles of k', which read it
                // through a KInfo of its own: a = the far rows, rg = the row
                // map, ct0 / cvoff per column of k' (an absent column: an
                // empty segment, ct0 = w, at the first far column's values).
                SLU_REQUIRE(mp->fm == m - nr0 && mp->fn == ncols - nc0, "mapped pair (%d, %d): far part", k, knext);
                const int rl = mp->r_lo, rh = mp->r_hi, cl = mp->c_lo, ch = mp->c_hi;
                parts.push_back({nr0 + rl, nc0, rh - rl, mp->fn, false});
                parts.push_back({nr0, nc0 + cl, rl, ch - cl, false});
                parts.push_back({nr0 + rh, nc0 + cl, mp->fm - rh, ch - cl, false});
                for (int c = nc0; c < ncols; ++c) {
                    if (c - nc0 >= cl && c - nc0 < ch) continue;
                    fl_deferred += 2.0 * (mp->fm - (rh - rl)) * (w - O.h_ct0[cols_off + c]);
                }
                el_deferred = (double)(mp->fm - (rh - rl)) * (mp->fn - (ch - cl));
                KInfo<T> ks = ki;
                ks.a = d_L.p + lval_off[ljb] + r0 + nr0;
                ks.lda = lval_ld[ljb];
                ks.m = (int)mp->rmap.size();
                ks.n = (int)mp->cmap.size();
                ks.mapped = 1;
                ks.rg = ks.ra = (const int *)(intptr_t)O.h_rg.size();
                ks.cvoff = (const i64 *)(intptr_t)O.h_cg.size();
                ks.ct0 = ks.cg = ks.cb = (const int *)(intptr_t)O.h_cg.size();
                for (int q : mp->rmap) {
                    O.h_rg.push_back(q);
                    O.h_ra.push_back(0);
                }
                for (int q : mp->cmap) {
                    O.h_cg.push_back(0);
                    O.h_cb.push_back(0);
                    const int t0q = q >= 0 ? O.h_ct0[cols_off + nc0 + q] : w;
                    const i64 voq = O.h_cvoff[cols_off + nc0 + std::max(q, 0)];
                    O.h_ct0.push_back(t0q);
                    O.h_cvoff.push_back(voq);
                }
                O.far_slots.push_back({k, (int)O.kinfos.size()});
                O.kinfos.push_back(ks);
                O.khost.push_back(KInfoHost{}); // (no tile of its own at this level)
            }
            ntiles = 0;
            for (size_t pi = 0; pi < parts.size(); ++pi) {
                const int pr0 = parts[pi].r0, pc0 = parts[pi].c0, pm = parts[pi].m, pn = parts[pi].n;
                const bool twin = parts[pi].twin;
                if (pm <= 0 || pn <= 0) continue;
                KInfo<T> kc = ki;
                kc.a = d_L.p + lval_off[ljb] + r0 + pr0;
                kc.lda = lval_ld[ljb];
                kc.m = pm;
                kc.n = pn;
                kc.rg = kc.ra = (const int *)(intptr_t)(rows_off + pr0);
                kc.cvoff = (const i64 *)(intptr_t)(cols_off + pc0);
                kc.ct0 = kc.cg = kc.cb = (const int *)(intptr_t)(cols_off + pc0);
                const bool pbig = pm >= SB_BM && pn >= BBN;
                const int PBM = pbig ? SB_BM : SC_BM, PBN = pbig ? BBN : SC_BN;
                for (int c = 0; !pbig && c < pn; ++c) fl_small += 2.0 * pm * (w - O.h_ct0[cols_off + pc0 + c]);
                const int ptm = (pm + PBM - 1) / PBM, ptn = (pn + PBN - 1) / PBN;
                // the part's own destination blocks (the parts' are disjoint)
                KInfoHost ph;
                const int a_lo = O.h_ra[rows_off + pr0], a_hi = O.h_ra[rows_off + pr0 + pm - 1];
                const int b_lo = O.h_cb[cols_off + pc0], b_hi = O.h_cb[cols_off + pc0 + pn - 1];
                for (int a = a_lo; a <= a_hi; ++a)
                    for (int b = b_lo; b <= b_hi; ++b) ph.dests.push_back(kh.dests[(size_t)a * ujb.size() + b]);
                // critical at this level / (far part) the twin's class at the next
                vector<char> prow(ptm, 0), pcol(ptn, 0), trow(ptm, 0), tcol(ptn, 0);
                for (int r = 0; r < pm; ++r) {
                    const int lv = level_of[lib_[O.h_ra[rows_off + pr0 + r]]];
                    if (lv == nl) prow[r / PBM] = 1;
                    if (lv == nl + 1) trow[r / PBM] = 1;
                }
                for (int c = 0; c < pn; ++c) {
                    const int lv = level_of[ujb[O.h_cb[cols_off + pc0 + c]]];
                    if (lv == nl) pcol[c / PBN] = 1;
                    if (lv == nl + 1) tcol[c / PBN] = 1;
                }
                const int slot = (int)O.kinfos.size();
                O.kinfos.push_back(kc);
                O.khost.push_back(std::move(ph));
                if (twin) {
                    SLU_REQUIRE(pbig, "pair (%d, %d): far part of %d x %d", k, knext, pm, pn);
                    O.far_slots.push_back({k, slot});
                }
                for (int i = 0; i < ptm; ++i)
                    for (int j = 0; j < ptn; ++j) {
                        if (twin && !(trow[i] || tcol[j])) { // deferred
                            const int rows_t = std::min(PBM, pm - i * PBM), c1 = std::min(pn, (j + 1) * PBN);
                            for (int cc = j * PBN; cc < c1; ++cc)
                                fl_deferred += 2.0 * rows_t * (w - O.h_ct0[cols_off + pc0 + cc]);
                            el_deferred += (double)rows_t * (c1 - j * PBN);
                            continue;
                        }
                        const int cls = (prow[i] || pcol[j]) ? 0 : 1;
                        (pbig ? O.big[cls][0] : O.small[cls][0]).push_back(TileItem{slot, i, j, slot});
                        ++ntiles;
                    }
            }
        }
        for (int g = 0; knext < 0 && g < ng; ++g) {
            const int ga = g * gs, rows = std::min(gs, m - ga);
            KInfo<T> kg = ki;
            if (lcol_here) {
                kg.a = d_L.p + lval_off[ljb] + r0 + ga;
                kg.lda = lval_ld[ljb];
            } else if (xmode) {
                SLU_REQUIRE(lgpos[k][g] >= 0, "L panel %d row group %d not received", k, g);
                kg.a = d_pan.p + lgpos[k][g];
                kg.lda = rows;
            } else {
                kg.a = d_pan.p + lpos[k];
                kg.lda = m;
            }
            kg.m = rows;
            kg.rg = (const int *)(intptr_t)(rows_off + ga);
            kg.ra = (const int *)(intptr_t)(rows_off + ga);
            const int tmg = (rows + BM - 1) / BM;
            vector<char> crow(tmg, 0);
            for (int r = 0; r < rows; ++r)
                if (level_of[lib_[O.h_ra[rows_off + ga + r]]] == nl) crow[r / BM] = 1;
            const int slot0 = (int)O.kinfos.size(); // relocated by the merge
            int ns = nsplit;
            for (int c = 0; c < ns; ++c) {
                KInfo<T> kc = kg;
                kc.kmin = kmin + c * kch;
                kc.kw = std::min(kch, w - kc.kmin);
                if (kc.kw <= 0) {
                    ns = c;
                    break;
                }
                O.kinfos.push_back(kc);
                O.khost.push_back(kh);
            }
            if (ns > 1) O.n_ksplit += ns;
            for (int c = 0; c < ns; ++c)
                for (int i = 0; i < tmg; ++i)
                    for (int j = 0; j < tn; ++j) {
                        const int cls = (crow[i] || ccol[j]) ? 0 : 1;
                        const int ch = xmode ? std::max(g, j * BN / ucsz[k]) : 0;
                        // second member of a pair: its rest tiles run the first
                        // member's far tiles as their first K segment
                        // (mapped pair: those that hold a row and a column of the first member)
                        const bool fuse = kprev >= 0 && cls == 1 && (!pmp || (prc[i] && pcc[j]));
                        (big ? O.big[cls][ch] : O.small[cls][ch])
                            .push_back(TileItem{slot0 + c, i, j, fuse ? SEG_PENDING + kprev : slot0 + c});
                        if (fuse && !pmp) {
                            O.n_fused++;
                            const int rows_t = std::min(BM, rows - i * BM);
                            for (int cc = j * BN; cc < std::min(ncols, (j + 1) * BN); ++cc)
                                fl_fused += 2.0 * rows_t * (W(kprev) - pt0[pt0.size() - ncols + cc]);
                        } else if (fuse) {
                            O.n_mfused++;
                            for (int cc = j * BN; cc < std::min(ncols, (j + 1) * BN); ++cc)
                                if (pmp->cmap[cc] >= 0)
                                    fl_mfused += 2.0 * prc[i] * (W(kprev) - pt0[pt0.size() - pmp->fn + pmp->cmap[cc]]);
                        }
                    }
        }
        // algorithmic work: exact unpadded flops and padded flops
        double fl = 0;
        for (int c = 0; c < ncols; ++c) fl += 2.0 * m * (w - O.h_ct0[cols_off + c]);
        O.schur_flops += fl * mult;
        O.schur_flops_padded += 2.0 * m * ncols * (double)(w - kmin) * mult;
        // (a deferred tile's scatter is its twin's)
        O.scatter_bytes += 3.0 * sizeof(T) * ((double)m * ncols - el_deferred);
        O.n_schur_tiles += ntiles;
        // per level: an update counts where its tiles run, a pair's deferred
        // tiles one level up with the second member
        O.fused_flops += fl_fused * mult;
        O.mfused_flops += fl_mfused * mult;
        fl_fused += fl_mfused;
        O.R_schur_flops += (fl - fl_deferred + fl_fused) * mult;
        if (big) O.R_big_flops += (fl - fl_deferred + fl_fused - fl_small) * mult;
        if (w >= 64 && m >= 256 && ncols >= 256) O.R_big = true;
    }

    // ------------------------------------------------------- device
    void build_device() {
        const auto tb0 = std::chrono::steady_clock::now();
        auto sub = [&](const char *what, double mb) {
            if (prof) fprintf(stderr, "[slu plan %d]   build_device %-10s %6.1f ms %8.1f MB\n", iam, what, ms_since(tb0), mb);
        };
        d_rg.upload(h_rg);
        d_ra.upload(h_ra);
        d_cg.upload(h_cg);
        d_cb.upload(h_cb);
        d_pair.upload(h_pair);
        {
            // destinations resolved once (DRec, kernels.h): the Schur
            // epilogue reads one record per (L block, U block) of a tile
            RawVec<DRec> prec;
            prec.resize_uninit(h_pair.size());
            parallel_for((int)((h_pair.size() + 4095) / 4096), [&](int ch) {
                const size_t e = std::min(h_pair.size(), (size_t)(ch + 1) * 4096);
                for (size_t i = (size_t)ch * 4096; i < e; ++i) {
                    const int h = h_pair[i];
                    DRec d{0, 0, -1, 0};
                    if (h >= 0) {
                        const LBlk &L = lblk[h];
                        d.base = L.colvoff - (i64)L.fcol * L.ld;
                        d.mb = L.mapoff - L.frow;
                        d.ld = L.ld;
                    } else {
                        const UBlk &U = ublk[~h];
                        d.base = U.coloff - U.fcol;
                    }
                    prec[i] = d;
                }
            });
            d_prec.upload(prec);
        }
        d_ct0.upload(h_ct0);
        d_cvoff.upload(h_cvoff);
        sub("panels", (d_rg.bytes() + d_ra.bytes() + d_cg.bytes() + d_cb.bytes() + d_pair.bytes() + d_prec.bytes() +
                       d_ct0.bytes() + d_cvoff.bytes()) / 1e6);
        for (auto &t : tu_items) {
            intptr_t co = (intptr_t)t.voff;
            t.voff = d_cvoff.p + co;
            t.t0 = d_ct0.p + co;
        }
        for (auto &k : kinfos) {
            intptr_t co = (intptr_t)k.cvoff, ro = (intptr_t)k.rg, po = (intptr_t)k.pair;
            k.cvoff = d_cvoff.p + co;
            k.ct0 = d_ct0.p + co;
            k.cg = d_cg.p + co;
            k.cb = d_cb.p + co;
            k.rg = d_rg.p + ro;
            k.ra = d_ra.p + ro;
            k.pair = d_pair.p + po;
            k.prec = d_prec.p + po;
        }
        for (auto &t : uf_items) {
            intptr_t co = (intptr_t)t.voff;
            t.voff = d_cvoff.p + co;
            t.t0 = d_ct0.p + co;
        }
        auto reloc = [&](vector<CopyItem<T>> &v, const vector<char> &tag) {
            for (size_t i = 0; i < v.size(); ++i) {
                const int ss = tag[i] & 1, ds = tag[i] >> 1;
                v[i].src = (ss ? d_U.p : d_L.p) + (intptr_t)v[i].src;
                v[i].dst = (ds ? d_pan.p : d_dpk.p) + (intptr_t)v[i].dst;
            }
        };
        reloc(dcopy, dcopy_src);
        reloc(pcopy, pcopy_src);
        d_df.upload(df_items);
        d_lf.upload(lf_items);
        d_uf.upload(uf_items);
        d_diag.upload(diag_items);
        d_tl.upload(tl_items);
        d_tu.upload(tu_items);
        d_kinfo.upload(kinfos);
        d_tiles.upload(tiles);
        d_tiles_big.upload(tiles_big);
        d_dcopy.upload(dcopy);
        d_pcopy.upload(pcopy);
        sub("items", (d_df.bytes() + d_lf.bytes() + d_uf.bytes() + d_kinfo.bytes() + d_tiles.bytes() +
                      d_tiles_big.bytes()) / 1e6);
        d_lblk.upload(lblk);
        d_lmap.upload(lmap);
        d_ublk.upload(ublk);
        d_ucol_voff.upload(ucol_voff);
        d_ucol_fst.upload(ucol_fst);
        sub("blocks", (d_lblk.bytes() + d_lmap.bytes() + d_ublk.bytes() + d_ucol_voff.bytes() + d_ucol_fst.bytes()) / 1e6);
        d_counters.alloc(4);
        d_zpiv.alloc(nsupers);
        d_dsflags.alloc(std::max<size_t>(df_items.size(), 1) * DS_NFLAGS);
        HIPCHK(hipMemset(d_dsflags.p, 0, d_dsflags.bytes()));
        ev_pan.resize(levels.size());
        ev_rest.resize(levels.size());
        for (size_t L = 0; L < levels.size(); ++L) {
            HIPCHK(hipEventCreateWithFlags(&ev_pan[L], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&ev_rest[L], hipEventDisableTiming));
        }
        HIPCHK(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_pend, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_tu0, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_tu1, hipEventDisableTiming));
        if (xmode) {
            HIPCHK(hipEventCreateWithFlags(&ev_pk, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&ev_dx, hipEventDisableTiming));
            for (hipEvent_t &e : ev_cx) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        d_info.alloc(Pr * Pc);
        stats.lu_bytes = (double)(lval_total + uval_total) * sizeof(T);
        stats.index_bytes = (double)(d_lblk.bytes() + d_lmap.bytes() + d_ublk.bytes() +
                                     d_ucol_voff.bytes() + d_ucol_fst.bytes() + d_diag.bytes() +
                                     d_tl.bytes() + d_tu.bytes() + d_kinfo.bytes() + d_tiles_big.bytes() +
                                     d_df.bytes() + d_lf.bytes() + d_uf.bytes() + d_dinv.bytes() +
                                     d_tiles.bytes() + d_rg.bytes() + d_ra.bytes() +
                                     d_cg.bytes() + d_cb.bytes() + d_pair.bytes() + d_prec.bytes() +
                                     d_ct0.bytes() + d_cvoff.bytes() + d_dcopy.bytes() +
                                     d_pcopy.bytes());
        double zvol = 0; // 3D: the ancestor reductions this layer takes part in
        if (zmode)
            for (int p = 0; p <= std::min(my_last, maxlvl - 2); ++p) zvol += (double)zr_cnt[p] * sizeof(T);
        stats.comm_bytes = (double)comm_volume * sizeof(T) + zvol;
        stats.comm_buf_bytes = (double)(dpk_total + pan_total) * sizeof(T) + (double)d_zbuf.bytes();
        // the tables went up by pageable hipMemcpy on the null stream; the
        // plan's streams are non-blocking, so make sure every copy has landed
        HIPCHK(hipDeviceSynchronize());
    }

    // ------------------------------------------------------- values
    // What the device factor storage holds: 0 nothing, 1 values
    // of A not yet factored (upload / restore / fill_a), 2 factors of them.
    // d_acur = the values of A behind the storage (fill_a only; an upload
    // does not tell which A it came from), a_fact = d_acur of the factors.
    // d_acur64 / a_fact64 / snap_acur64: the same for the fp64 values an
    // fp32 plan got through fill_a_d2 (then d_acur is null: no fp32 A exists).
    int vstate = 0;
    bool dinv_valid = false; // DiagInv's inverses are those of the factors: cleared wherever vstate is assigned
    const T *a_fact = nullptr, *snap_acur = nullptr;
    const double *d_acur64 = nullptr, *a_fact64 = nullptr, *snap_acur64 = nullptr;
    int snap_state = 0;

    // ---- host <-> HBM copies of the values (hostio.h)
    double up_ms = 0;
    bool host_current = false; // the host LUstruct holds what the device holds

    vector<Xfer> value_xfers() {
        LocalLU *Llu = LU->Llu;
        vector<Xfer> xs;
        if (l_contig && lval_total)
            xs.push_back({(char *)d_L.p, (char *)Llu->Lnzval_bc_dat, lval_total * sizeof(T)});
        else
            for (int ljb = 0; ljb < nlc; ++ljb)
                if (lval_off[ljb] >= 0)
                    xs.push_back({(char *)(d_L.p + lval_off[ljb]), (char *)Llu->Lnzval_bc_ptr[ljb],
                                  (size_t)lval_ld[ljb] * W(ljb * Pc + mycol) * sizeof(T)});
        if (u_contig && uval_total)
            xs.push_back({(char *)d_U.p, (char *)Llu->Unzval_br_dat, uval_total * sizeof(T)});
        else
            for (int lb = 0; lb < nlr; ++lb)
                if (uval_off[lb] >= 0)
                    xs.push_back({(char *)(d_U.p + uval_off[lb]), (char *)Llu->Unzval_br_ptr[lb],
                                  (size_t)Llu->Ufstnz_br_ptr[lb][1] * sizeof(T)});
        return merge_xfers(std::move(xs));
    }

    void upload_values() {
        const auto t0 = std::chrono::steady_clock::now();
        vector<Xfer> xs = value_xfers();
        staged_h2d(xs, device());
        double b = 0;
        for (auto &x : xs) b += (double)x.bytes;
        stats.h2d_bytes = b;
        up_ms = ms_since(t0);
    }

    void upload() override {
        const auto t0 = std::chrono::steady_clock::now();
        const bool overlapped = up_thread.running();
        pin_thread.wait();
        up_thread.wait(); // (both have stopped before either's error is thrown)
        pin_thread.join();
        up_thread.join();
        if (!overlapped) upload_values();
        stats.t_upload_wait_ms = ms_since(t0);
        stats.t_upload_ms = up_ms;
        vstate = 1;
        dinv_valid = false;
        d_acur = nullptr;
        d_acur64 = nullptr;
        host_current = true;
    }

    // D2H of the factors while the factorization runs (opts.overlap_download).
    // After the panels of level L are done, the L columns and U rows of its
    // supernodes are final (right-looking LU; later levels only read them).
    // Measured on the box (profiles/r02_pcie_micro.json): pageable D2H needs
    // copies of >= 4 MB to reach 49 GB/s (512 KB: 12 GB/s), while GPU stores
    // into pinned host memory reach 51-56 GB/s with 32-128 workgroups and
    // pinned -> pageable memcpy 60 / 121 GB/s on 4 / 8 host threads.  So the
    // finished blocks are pushed by a small kernel (k_push) into a pinned
    // slot of <= SLOT bytes ("fill"), and host threads scatter the slot into
    // the caller's arrays while the next fill is pushed.
    static constexpr int D2H_NS = 4; // pinned slots in flight
    D2HFills d2h;
    // called on the D2H stream before fill F's push, after its level's
    // panels are done (AmalgPlan: compress the level into the caller's layout)
    std::function<void(int, hipStream_t)> d2h_pre;
    DevBuf<char> d_stage; // HBM staging slots of the D2H (SDMA mode)

    void build_d2h() {
        if (!opts.overlap_download) return;
        LocalLU *Llu = LU->Llu;
        for (size_t L = 0; L < levels.size(); ++L) {
            for (int k : bylev[L]) {
                if (k % Pc == mycol && lval_off[k / Pc] >= 0) {
                    const int ljb = k / Pc;
                    d2h.add((const char *)(d_L.p + lval_off[ljb]), (char *)Llu->Lnzval_bc_ptr[ljb],
                            (i64)lval_ld[ljb] * W(k) * (i64)sizeof(T), (int)L);
                }
                if (k % Pr == myrow && uval_off[k / Pr] >= 0) {
                    const int lb = k / Pr;
                    d2h.add((const char *)(d_U.p + uval_off[lb]), (char *)Llu->Unzval_br_ptr[lb],
                            (i64)Llu->Ufstnz_br_ptr[lb][1] * (i64)sizeof(T), (int)L);
                }
            }
            d2h.end_level((int)L, L + 1 == levels.size());
        }
        d2h.finish();
    }

    // The D2H pipeline (runs on a helper thread during factor()): this
    // thread queues k_push of fill j into slot j % NS as soon as the slot's
    // previous fill has been scattered; an unpack thread scatters fill j once
    // its push event has fired (parallel host memcpy).
    void run_d2h(double &bytes, int64_t &ncopies) {
        double t_wait_push = 0, t_unpack = 0, t_wait_slot = 0;
        HIPCHK(hipSetDevice(device()));
        constexpr int NS = D2H_NS;
        std::lock_guard<std::mutex> in_use(pinned_pool(1).use);
        std::vector<char *> slot = pinned_pool(1).get(NS, d2h.slot);
        hipStream_t cs = nullptr;
        hipEvent_t evf[NS] = {};
        std::mutex mu;
        std::condition_variable cv;
        int pushed = 0, unpacked = 0;
        bool fail = false;
        std::string err;
        auto set_err = [&](const char *what) {
            std::lock_guard<std::mutex> lk(mu);
            if (err.empty()) err = what;
            fail = true;
            cv.notify_all();
        };
        const int nf = (int)d2h.fills.size();
        std::thread unpacker;
        try {
            int prio_lo = 0, prio_hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
            const char *pe = getenv("SLU_D2H_PRIO"); // diagnostics: lo | hi
            HIPCHK(hipStreamCreateWithPriority(&cs, hipStreamNonBlocking,
                                               pe && !strcmp(pe, "hi") ? prio_hi : prio_lo));
            const char *ge = getenv("SLU_D2H_WG");
            const int nwg = ge ? std::max(1, atoi(ge)) : 128; // (32: +25 ms of tail at 100^3, tools/d2h_variants.py)
            const char *me = getenv("SLU_D2H_MODE"); // diagnostics: push (zero-copy) | sdma
            const bool use_sdma = !(me && !strcmp(me, "push"));
            if (use_sdma && d_stage.n < (size_t)NS * d2h.slot) d_stage.alloc((size_t)NS * d2h.slot);
            for (auto &e : evf) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            unpacker = std::thread([&] {
                try {
                    HIPCHK(hipSetDevice(device()));
                    for (int j = 0; j < nf; ++j) {
                        {
                            std::unique_lock<std::mutex> lk(mu);
                            cv.wait(lk, [&] { return pushed > j || fail; });
                            if (fail) return;
                        }
                        const auto tw = std::chrono::steady_clock::now();
                        HIPCHK(hipEventSynchronize(evf[j % NS]));
                        const auto tu = std::chrono::steady_clock::now();
                        t_wait_push += std::chrono::duration<double, std::milli>(tu - tw).count();
                        const D2HFill &F = d2h.fills[j];
                        const char *src = slot[j % NS];
                        parallel_for(F.hs_n, [&](int i) {
                            const HostSeg &h = d2h.h_unpack[F.hs_off + i];
                            memcpy(h.host, src + h.off, (size_t)h.bytes);
                        }, 1);
                        t_unpack += ms_since(tu);
                        for (int i = 0; i < F.hs_n; ++i) bytes += (double)d2h.h_unpack[F.hs_off + i].bytes;
                        ncopies += F.hs_n;
                        std::lock_guard<std::mutex> lk(mu);
                        unpacked = j + 1;
                        cv.notify_all();
                    }
                } catch (const std::exception &e) {
                    set_err(e.what());
                }
            });
            for (int j = 0; j < nf; ++j) {
                {
                    const auto tw = std::chrono::steady_clock::now();
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return unpacked >= j - NS + 1 || fail; });
                    t_wait_slot += ms_since(tw);
                    if (fail) break;
                }
                const D2HFill &F = d2h.fills[j];
                HIPCHK(hipStreamWaitEvent(cs, ev_pan[F.level], 0));
                if (d2h_pre) d2h_pre(F.level, cs); // (amalgamated plan: relayout of the levels)
                if (use_sdma) {
                    // gather into an HBM slot (HBM-bound, microseconds), then
                    // one DMA-engine copy to the pinned slot: the PCIe-bound
                    // part occupies no CU while the factorization runs
                    char *ds = d_stage.p + (size_t)(j % NS) * d2h.slot;
                    hipLaunchKernelGGL(k_push, dim3(std::min(F.seg_n, 4 * nwg)), dim3(256), 0, cs,
                                       (const PushSeg *)(d2h.d_push.p + F.seg_off), F.seg_n, ds);
                    HIPCHK(hipGetLastError());
                    HIPCHK(hipMemcpyAsync(slot[j % NS], ds, (size_t)F.bytes, hipMemcpyDeviceToHost, cs));
                } else {
                    hipLaunchKernelGGL(k_push, dim3(std::min(F.seg_n, nwg)), dim3(256), 0, cs,
                                       (const PushSeg *)(d2h.d_push.p + F.seg_off), F.seg_n, slot[j % NS]);
                    HIPCHK(hipGetLastError());
                }
                HIPCHK(hipEventRecord(evf[j % NS], cs));
                std::lock_guard<std::mutex> lk(mu);
                pushed = j + 1;
                cv.notify_all();
            }
        } catch (const std::exception &e) {
            set_err(e.what());
        }
        if (unpacker.joinable()) unpacker.join();
        if (prof)
            fprintf(stderr, "[slu d2h %d] fills %d, unpack waits for push %.1f ms, unpack %.1f ms, "
                    "push waits for a slot %.1f ms\n", iam, nf, t_wait_push, t_unpack, t_wait_slot);
        if (cs) (void)hipStreamSynchronize(cs);
        for (auto &e : evf)
            if (e) (void)hipEventDestroy(e);
        if (cs) (void)hipStreamDestroy(cs);
        if (!err.empty()) throw Error(err);
    }

    DevBuf<T> d_L0, d_U0; // pristine copies (snapshot)
    void snapshot() override {
        d_L0.alloc(d_L.n);
        d_U0.alloc(d_U.n);
        HIPCHK(hipMemcpyAsync(d_L0.p, d_L.p, d_L.bytes(), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_U0.p, d_U.p, d_U.bytes(), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        snap_state = vstate;
        snap_acur = d_acur;
        snap_acur64 = d_acur64;
    }
    void restore() override {
        SLU_REQUIRE(d_L0.p && d_U0.p, "restore without snapshot");
        vstate = snap_state;
        dinv_valid = false;
        d_acur = snap_acur;
        d_acur64 = snap_acur64;
        host_current = false;
        HIPCHK(hipMemcpyAsync(d_L.p, d_L0.p, d_L.bytes(), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_U.p, d_U0.p, d_U.bytes(), hipMemcpyDeviceToDevice, stream));
    }
    void set_timing(int timing, int serial) override {
        opts.timing = timing;
        opts.serial = serial;
    }
    void adopt_factors() override {
        upload();
        sync();
        vstate = 2;
        dinv_valid = false;
        a_fact = nullptr; // adopted factors: of no A this plan knows
        a_fact64 = nullptr;
    }
    void sync() override {
        HIPCHK(hipStreamSynchronize(pstream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    void download() override {
        LocalLU *Llu = LU->Llu;
        sync();
        if (host_current) return; // overlap_download already wrote them back
        if (l_contig && lval_total) {
            HIPCHK(hipMemcpy(Llu->Lnzval_bc_dat, d_L.p, lval_total * sizeof(T), hipMemcpyDeviceToHost));
        } else {
            for (int ljb = 0; ljb < nlc; ++ljb)
                if (lval_off[ljb] >= 0)
                    HIPCHK(hipMemcpy(Llu->Lnzval_bc_ptr[ljb], d_L.p + lval_off[ljb],
                                     (size_t)lval_ld[ljb] * W(ljb * Pc + mycol) * sizeof(T),
                                     hipMemcpyDeviceToHost));
        }
        if (u_contig && uval_total) {
            HIPCHK(hipMemcpy(Llu->Unzval_br_dat, d_U.p, uval_total * sizeof(T), hipMemcpyDeviceToHost));
        } else {
            for (int lb = 0; lb < nlr; ++lb)
                if (uval_off[lb] >= 0)
                    HIPCHK(hipMemcpy(Llu->Unzval_br_ptr[lb], d_U.p + uval_off[lb],
                                     (size_t)Llu->Ufstnz_br_ptr[lb][1] * sizeof(T),
                                     hipMemcpyDeviceToHost));
        }
    }

    // SLU_KSPLIT_TILES: levels of <= 2 supernodes with fewer big tiles than
    // this split their K range (default 0, off: the chunks of a destination
    // add atomically in no fixed order, so the root levels' factors would not
    // be bit-reproducible from run to run, for ~0.3 ms at 100^3)
    int ksplit_tiles = env_int("SLU_KSPLIT_TILES", 0);
    // SLU_TRSM_NARROW: 0 the 256-wide k_trsm_reg everywhere, 1 the 64-wide
    // instantiation for levels whose TRSM supernodes are <= 64 wide, 2 (default)
    // also the 128-wide one for <= 128
    int trsm_narrow = env_int("SLU_TRSM_NARROW", 2);
    // SLU_TRSM_2STREAM=1 (default): the U panel's TRSM on a stream of its
    // own beside the L panel's (both only wait for the diagonal block; near
    // the root each is a few slabs, latency-bound)
    int trsm_2stream = env_int("SLU_TRSM_2STREAM", 1);
    // SLU_TRSM_PF=1 (default): k_trsm_reg's latency form (next block's T and
    // Dinv loaded during the current block, columns stored when final)
    int trsm_pf = env_int("SLU_TRSM_PF", 1);
    // the level's fast-path TRSM items, or (ch >= 0) those of exchange chunk ch
    void launch_trsm_fast(const LevelRange &R, hipStream_t st, int ch = -1) {
        const int lo = R.lf_off + (ch >= 0 ? R.lf_o[ch] : 0), ln = ch >= 0 ? R.lf_o[ch + 1] - R.lf_o[ch] : R.lf_n;
        const int uo = R.uf_off + (ch >= 0 ? R.uf_o[ch] : 0), un = ch >= 0 ? R.uf_o[ch + 1] - R.uf_o[ch] : R.uf_n;
        // the U launch on ustream when both panels have slabs
        const bool two = trsm_2stream && ustream && st == pstream && ln && un;
        hipStream_t su = two ? ustream : st;
        if (two) {
            HIPCHK(hipEventRecord(ev_tu0, st));
            HIPCHK(hipStreamWaitEvent(ustream, ev_tu0, 0));
        }
        auto go = [&](auto maxw, auto pf) {
            constexpr int MW = decltype(maxw)::value;
            constexpr bool P = decltype(pf)::value;
            if (ln) hipLaunchKernelGGL((k_trsm_reg<T, 0, MW, P>), dim3(ln), dim3(64 * TR_WAVES), 0, st, d_lf.p + lo);
            if (un) hipLaunchKernelGGL((k_trsm_reg<T, 1, MW, P>), dim3(un), dim3(64 * TR_WAVES), 0, su, d_uf.p + uo);
            const int pc = MW == 64 ? PC_TRSM_REG64_PF : MW == 128 ? PC_TRSM_REG128_PF : PC_TRSM_REG256_PF;
            path_counts[pc + (P ? 0 : 1)] += (ln != 0) + (un != 0);
        };
        auto go_pf = [&](auto maxw) {
            if (trsm_pf) go(maxw, std::true_type{});
            else go(maxw, std::false_type{});
        };
        if constexpr (cplx) {
            if (ln) hipLaunchKernelGGL((k_trsm_blk<T, 0>), dim3(ln), dim3(256), 0, st, d_lf.p + lo);
            if (un) hipLaunchKernelGGL((k_trsm_blk<T, 1>), dim3(un), dim3(256), 0, su, d_uf.p + uo);
            path_counts[PC_TRSM_BLK] += (ln != 0) + (un != 0);
        } else if (R.tf_maxw <= 64 && trsm_narrow) {
            // narrow levels: the 64-wide instantiation (several workgroups per CU)
            go_pf(std::integral_constant<int, 64>{});
        } else if (R.tf_maxw <= 128 && trsm_narrow >= 2) {
            go_pf(std::integral_constant<int, 128>{});
        } else {
            go_pf(std::integral_constant<int, FAST_MAXW>{});
        }
        if (two) {
            HIPCHK(hipEventRecord(ev_tu1, ustream));
            HIPCHK(hipStreamWaitEvent(st, ev_tu1, 0));
        }
    }

    // The rest of a level's Schur tiles go out as two launches, the first
    // with rest_split %% of them (SLU_REST_SPLIT: A/B).  The
    // next level's diag LU and TRSM workgroups (150 / 85 KB of LDS, up to 256
    // VGPRs) fit only on a CU that no Schur workgroup holds; inside one
    // launch every freed slot is refilled with the next Schur tile, so they
    // would wait for the whole level.  Where the first launch drains they get
    // CUs and run beside the second (100^3: 363 -> 345 ms; more split points
    // gain nothing further, tools/ab_env.sh).
    int rest_split = env_int("SLU_REST_SPLIT", 30);
    // k_diag_strips (diag_strips.h) for the levels near the root: a few wide
    // real blocks, each factored by one workgroup per 32-column strip
    // (SLU_DIAG_STRIPS=0: k_diag_lu_f everywhere; SLU_DIAG_STRIPS_MAX: the
    // most blocks a level may hold for it, default 32)
    // (SLU_DIAG_STRIPS=2, test hook: every fast level, narrow blocks too)
    int strips_mode = env_int("SLU_DIAG_STRIPS", 1);
    int strips_max = env_int("SLU_DIAG_STRIPS_MAX", 32);
    bool strips_ok(const LevelRange &R) const {
        if (cplx || strips_mode == 0) return false;
        return strips_mode == 2 || (R.df_maxw > DF_SMALLW && R.df_n <= strips_max);
    }
    // k_diag_lu_w (diag_wave.h): one wave per narrow diagonal block, real
    // types (SLU_DIAG_WAVE=0: k_diag_lu_f's 256-thread path instead)
    int diag_wave = env_int("SLU_DIAG_WAVE", 1);
    bool diag_wave_ok() const { return !cplx && diag_wave != 0; }
    void launch_diag_wave(const LevelRange &R, double thresh, hipStream_t st) {
        if constexpr (!cplx) {
            const dim3 g((unsigned)((R.df_n + DW_WAVES - 1) / DW_WAVES)), b(64 * DW_WAVES);
            path_counts[R.df_maxw <= 32 ? PC_DIAG_WAVE32 : PC_DIAG_WAVE64]++;
            if (R.df_maxw <= 32)
                hipLaunchKernelGGL((k_diag_lu_w<T, 32>), g, b, 0, st, d_df.p + R.df_off, R.df_n, thresh,
                                   opts.replace_tiny_pivot, d_counters.p, d_zpiv.p);
            else
                hipLaunchKernelGGL((k_diag_lu_w<T, 64>), g, b, 0, st, d_df.p + R.df_off, R.df_n, thresh,
                                   opts.replace_tiny_pivot, d_counters.p, d_zpiv.p);
        }
    }
    void launch_strips(const LevelRange &R, double thresh, hipStream_t st) {
        if constexpr (!cplx) {
            hipLaunchKernelGGL(k_diag_strips<T>, dim3(ds_grid(R.df_n)), dim3(DS_THREADS), 0, st, d_df.p + R.df_off,
                               R.df_n, d_dsflags.p + (size_t)R.df_off * DS_NFLAGS, ds_epoch, d_counters.p + 1, thresh,
                               opts.replace_tiny_pivot, d_counters.p, d_zpiv.p);
            path_counts[PC_DIAG_STRIPS]++;
        }
    }
    // fused: the tiles of chained pairs that carry a first K segment (the
    // last R.fused_n rest tiles of the level), through the two-segment instantiation
    // (fused = 2: those of mapped pairs, the last R.mapped_n, through the mapped instantiation)
    void launch_big(const LevelRange &R, int off, int cnt, hipStream_t st, int fused = 0) {
        if (fused == 2)
            hipLaunchKernelGGL((k_schur_big<T, 2>), dim3(cnt), dim3(BigCfg<T>::THREADS), 0, st,
                               d_tiles_big.p + off, d_kinfo.p + R.k_off, d_L.p, d_U.p,
                               d_lblk.p, d_lmap.p, d_ublk.p, d_ucol_voff.p, d_ucol_fst.p);
        else if (fused)
            hipLaunchKernelGGL((k_schur_big<T, 1>), dim3(cnt), dim3(BigCfg<T>::THREADS), 0, st,
                               d_tiles_big.p + off, d_kinfo.p + R.k_off, d_L.p, d_U.p,
                               d_lblk.p, d_lmap.p, d_ublk.p, d_ucol_voff.p, d_ucol_fst.p);
        else
            hipLaunchKernelGGL((k_schur_big<T, 0>), dim3(cnt), dim3(BigCfg<T>::THREADS), 0, st,
                               d_tiles_big.p + off, d_kinfo.p + R.k_off, d_L.p, d_U.p,
                               d_lblk.p, d_lmap.p, d_ublk.p, d_ucol_voff.p, d_ucol_fst.p);
        path_counts[PC_SCHUR_BIG]++;
    }
    void launch_small(const LevelRange &R, int off, int cnt, hipStream_t st) {
        hipLaunchKernelGGL(k_schur<T>, dim3(cnt), dim3(SC_THREADS), 0, st, d_tiles.p + off,
                           d_kinfo.p + R.k_off, d_L.p, d_U.p, d_lblk.p, d_lmap.p, d_ublk.p,
                           d_ucol_voff.p, d_ucol_fst.p);
        path_counts[PC_SCHUR_SMALL]++;
    }

    // One exchange group of a level: the sections [off, off + n_) out of the
    // diagonal-package arena dpk / the panel arena pan (factor(): d_dpk /
    // d_pan; check_exchange(): its host arenas)
    void issue(const vector<Sec> &secs, int off, int n_, const char *phase, int level, T *dpk, T *pan) {
        for (int i = off; i < off + n_; ++i) {
            const Sec &s = secs[i];
            T *base = s.arena ? pan : dpk;
            X.section(s.g, s.root, s.mask, s.off >= 0 ? base + s.off : nullptr,
                      (size_t)s.cnt * sizeof(T));
        }
        X.flush_as(phase, level);
    }

    // ------------------------------------------------------- factor
    // Leaf steps of a level, shared by the two level bodies below.  tm is
    // the event timing of the factorization under way.
    FactorTimer tm;

    // the level's diagonal blocks
    void diag_step(const LevelRange &R, double thresh, hipStream_t P) {
        if (R.diag_n)
            tm.span(0, P, [&] {
                hipLaunchKernelGGL(k_diag_lu<T>, dim3(R.diag_n), dim3(DIAG_THREADS), 0, P,
                                   d_diag.p + R.diag_off, thresh, opts.replace_tiny_pivot,
                                   d_counters.p, d_zpiv.p);
                path_counts[PC_DIAG_GENERIC]++;
            });
        if (R.df_n)
            tm.span(0, P, [&] {
                if (strips_ok(R))
                    launch_strips(R, thresh, P);
                else if (R.df_maxw <= DF_SMALLW && diag_wave_ok())
                    launch_diag_wave(R, thresh, P);
                else if (R.df_maxw <= DF_SMALLW) {
                    hipLaunchKernelGGL((k_diag_lu_f<T, DF_SMALLW, DF_SMALL_THREADS>), dim3(R.df_n),
                                       dim3(DF_SMALL_THREADS), 0, P, d_df.p + R.df_off, thresh,
                                       opts.replace_tiny_pivot, d_counters.p, d_zpiv.p);
                    path_counts[PC_DIAG_F_SMALL]++;
                } else {
                    hipLaunchKernelGGL(k_diag_lu_f<T>, dim3(R.df_n), dim3(DF_THREADS), 0, P,
                                       d_df.p + R.df_off, thresh, opts.replace_tiny_pivot,
                                       d_counters.p, d_zpiv.p);
                    path_counts[PC_DIAG_F]++;
                }
            });
    }
    // the generic TRSM items (supernodes wider than the fast path's)
    void trsm_generic(const LevelRange &R, hipStream_t P) {
        if (!R.tl_n && !R.tu_n) return;
        tm.span(1, P, [&] {
            if (R.tl_n)
                hipLaunchKernelGGL(k_trsm_l<T>, dim3(R.tl_n), dim3(TRSM_THREADS), 0, P, d_tl.p + R.tl_off);
            if (R.tu_n)
                hipLaunchKernelGGL(k_trsm_u<T>, dim3(R.tu_n), dim3(TRSM_THREADS), 0, P, d_tu.p + R.tu_off);
            path_counts[PC_TRSM_GENERIC] += (R.tl_n != 0) + (R.tu_n != 0);
        });
    }
    // pack copies (2D grids): the diagonal packages / cnt panel-section items from off
    void pack_diag(const LevelRange &R, hipStream_t P) {
        if (R.dc_n) hipLaunchKernelGGL(k_copy<T>, dim3(R.dc_n), dim3(256), 0, P, d_dcopy.p + R.dc_off);
    }
    void pack_panels(int off, int cnt, hipStream_t P) {
        if (cnt) hipLaunchKernelGGL(k_copy<T>, dim3(cnt), dim3(256), 0, P, d_pcopy.p + off);
    }
    // One Schur launch of n 128x128 tiles from off (its first n1, if any, as
    // a kernel launch of their own: one launch in the stats, two in
    // path_counts) / of n 64x64 tiles
    // (its last nf tiles: fused ones, a launch of their own)
    // (and, after them, its last nm: fused tiles of mapped pairs, one more launch)
    void schur_big(const LevelRange &R, int off, int n_, hipStream_t st, int n1 = 0, int nf = 0, int nm = 0) {
        if (!n_) return;
        tm.span(2, st, [&] {
            if (n1 > 0) launch_big(R, off, n1, st);
            if (n_ - nf - nm > n1) launch_big(R, off + n1, n_ - nf - nm - n1, st);
            if (nf > 0) launch_big(R, off + n_ - nf - nm, nf, st, 1);
            if (nm > 0) launch_big(R, off + n_ - nm, nm, st, 2);
        });
        stats.n_schur_launches++;
        stats.n_schur_big_launches++;
    }
    void schur_small(const LevelRange &R, int off, int n_, hipStream_t st) {
        if (!n_) return;
        tm.span(3, st, [&] { launch_small(R, off, n_, st); });
        stats.n_schur_launches++;
    }

    // Level L of a 2D grid: the exchanges on the comm stream C, the panels in
    // R.nch chunks.  P: TRSM(c) -> pack(c) -> [C: send / receive chunk c] for
    // every c, so chunk c + 1's TRSM runs beside chunk c's transfer; the
    // critical tiles of chunk c (P) and its rest tiles (Schur stream) start
    // when chunk c is in.
    void level_chunked(size_t L, double thresh) {
        const LevelRange &R = levels[L];
        hipStream_t P = pstream, C = cstream;
        diag_step(R, thresh, P);
        auto exchange = [&](const vector<Sec> &secs, int off, int cnt, const char *what, hipEvent_t done) {
            HIPCHK(hipEventRecord(ev_pk, P));
            HIPCHK(hipStreamWaitEvent(C, ev_pk, 0));
            X.s = C;
            if (cnt) tm.span(4, C, [&] { issue(secs, off, cnt, what, (int)L, d_dpk.p, d_pan.p); });
            HIPCHK(hipEventRecord(done, C));
        };
        if (R.dc_n || R.ds_n) {
            if (R.dc_n) tm.span(4, P, [&] { pack_diag(R, P); });
            exchange(dsecs, R.ds_off, R.ds_n, "diagonal-package exchange", ev_dx);
            HIPCHK(hipStreamWaitEvent(P, ev_dx, 0));
        }
        for (int ch = 0; ch < R.nch; ++ch) {
            if (R.lf_o[ch + 1] > R.lf_o[ch] || R.uf_o[ch + 1] > R.uf_o[ch])
                tm.span(1, P, [&] { launch_trsm_fast(R, P, ch); });
            if (ch == 0) trsm_generic(R, P); // (wide supernodes' generic items: all in chunk 0)
            const int pcn = R.pc_o[ch + 1] - R.pc_o[ch];
            if (pcn) tm.span(4, P, [&] { pack_panels(R.pc_off + R.pc_o[ch], pcn, P); });
            exchange(psecs, R.ps_off + R.ps_o[ch], R.ps_o[ch + 1] - R.ps_o[ch], "L/U panel exchange",
                     ev_cx[ch]);
        }
        // critical tiles of L on the panel stream, after the rest of L-1
        if (L > 0) HIPCHK(hipStreamWaitEvent(P, ev_rest[L - 1], 0));
        for (int ch = 0; ch < R.nch; ++ch) {
            HIPCHK(hipStreamWaitEvent(P, ev_cx[ch], 0));
            schur_big(R, R.big_off + R.bc_o[ch], R.bc_o[ch + 1] - R.bc_o[ch], P);
            schur_small(R, R.tile_off + R.sc_o[ch], R.sc_o[ch + 1] - R.sc_o[ch], P);
        }
        HIPCHK(hipEventRecord(ev_pan[L], P));
        // the rest of L on the Schur stream, chunk by chunk as they arrive
        for (int ch = 0; ch < R.nch; ++ch) {
            HIPCHK(hipStreamWaitEvent(stream, ev_cx[ch], 0));
            schur_big(R, R.big_off + R.bigc_n + R.br_o[ch], R.br_o[ch + 1] - R.br_o[ch], stream);
            schur_small(R, R.tile_off + R.tilec_n + R.sr_o[ch], R.sr_o[ch + 1] - R.sr_o[ch], stream);
        }
    }

    // Level L of one rank alone, or of a grid in serial mode: look-ahead of
    // one level on two streams:
    //   pstream: panel(L) -> [wait rest(L-1)] -> critical tiles(L) -> panel(L+1) ...
    //   stream : [wait panel(L)] -> rest tiles(L) -> [rest(L) done] ...
    // Critical tiles update exactly the destinations in the panels of
    // level L+1, so panel(L+1) (diag LU, TRSM, exchanges) runs beside the
    // bulk of level L's Schur update (SRC/pdgstrf.c:1115-1356 look-ahead).
    void level_plain(size_t L, double thresh) {
        const LevelRange &R = levels[L];
        hipStream_t P = opts.serial ? stream : pstream;
        diag_step(R, thresh, P);
        if (R.dc_n || R.ds_n)
            tm.span(4, P, [&] {
                pack_diag(R, P);
                issue(dsecs, R.ds_off, R.ds_n, "diagonal-package exchange", (int)L, d_dpk.p, d_pan.p);
            });
        if (R.lf_n || R.uf_n) tm.span(1, P, [&] { launch_trsm_fast(R, P); });
        trsm_generic(R, P);
        if (R.pc_n || R.ps_n)
            tm.span(4, P, [&] {
                pack_panels(R.pc_off, R.pc_n, P);
                issue(psecs, R.ps_off, R.ps_n, "L/U panel exchange", (int)L, d_dpk.p, d_pan.p);
            });
        HIPCHK(hipEventRecord(ev_pan[L], P));
        // critical tiles of L on the panel stream, after the rest of L-1
        if (L > 0) HIPCHK(hipStreamWaitEvent(P, ev_rest[L - 1], 0));
        schur_big(R, R.big_off, R.bigc_n, P);
        schur_small(R, R.tile_off, R.tilec_n, P);
        // the rest of L on the Schur stream, once the panels of L exist;
        // the first rest_split %% of the big rest tiles as a launch of their own
        HIPCHK(hipStreamWaitEvent(stream, ev_pan[L], 0));
        const int nrest = R.big_n - R.bigc_n;
        const int nplain = nrest - R.fused_n - R.mapped_n;
        const int n1 = rest_split > 0 && !opts.serial ? (int)((i64)nplain * rest_split / 100) : 0;
        schur_big(R, R.big_off + R.bigc_n, nrest, stream, n1, R.fused_n, R.mapped_n);
        schur_small(R, R.tile_off + R.tilec_n, R.tile_n - R.tilec_n, stream);
    }

    // info and the tiny-pivot count of the factorization just synchronised
    void collect_info(int *info, int *tiny) {
        int hc[4];
        HIPCHK(hipMemcpy(hc, d_counters.p, sizeof hc, hipMemcpyDeviceToHost));
        SLU_REQUIRE(hc[1] == 0, "factor: a diagonal-block strip waited more than a second for its left "
                                "neighbour (k_diag_strips hand-off timeout)");
        vector<int> zp(nsupers);
        HIPCHK(hipMemcpy(zp.data(), d_zpiv.p, nsupers * sizeof(int), hipMemcpyDeviceToHost));
        // per-rank info: the zero pivot of the last supernode (in elimination
        // order) that had one (SRC/pdgstrf2.c:246-247 overwrites *info); the
        // grid value is the MIN over ranks (SRC/pdgstrf.c:1927-1931)
        int my_info = 0;
        for (int k = 0; k < nsupers; ++k)
            if (zp[k]) my_info = zp[k];
        if (xmode || zmode) { // MIN over the grid (3D: all layers, SRC/pdgstrf3d.c:351-355)
            vector<i64> mine(1, my_info ? my_info : n + 1);
            i64 g = n + 1;
            if (xmode)
                for (auto &v : X.allgatherv(G_WORLD, mine)) g = std::min(g, v[0]);
            if (zmode && !zsolo) {
                mine[0] = g;
                X.s = stream;
                for (auto &v : X.allgatherv(G_Z, mine)) g = std::min(g, v[0]);
            }
            my_info = g == n + 1 ? 0 : (int)g;
        }
        *info = my_info;
        *tiny = hc[0];
    }

    // diagnostics build (SLU_SB_STAMP): per-tile stamps of k_schur_big, to SLU_STAMP_OUT
    void stamp_reset() {
#ifdef SLU_SB_STAMP
        const unsigned z = 0;
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(slu_stamp_n), &z, sizeof z));
#endif
    }
    void stamp_dump() {
#ifdef SLU_SB_STAMP
        if (const char *fn = getenv("SLU_STAMP_OUT")) {
            unsigned cnt = 0;
            HIPCHK(hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(slu_stamp_n), sizeof cnt));
            cnt = std::min(cnt, SLU_STAMP_MAX);
            vector<uint64_t> h((size_t)cnt * 4);
            if (cnt) HIPCHK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(slu_stamp), h.size() * 8));
            if (FILE *f = fopen(fn, "wb")) {
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
#endif
    }

    void factor(double anorm, int *info, int *tiny) override {
        SLU_REQUIRE(vstate == 1, "factor: no unfactored values on the device (%s)",
                    vstate == 2 ? "already factored; upload / restore / fill_a first"
                                : "upload or fill_a first");
        vstate = 2;
        dinv_valid = false;
        a_fact = d_acur;
        a_fact64 = d_acur64;
        // thresh = smach_dist("Epsilon") * anorm (SRC/pdgstrf.c:412-413); in
        // psgstrf thresh is a float product.
        const float s_eps = 5.9604644775390625e-08f; // FLT_EPSILON * 0.5
        double thresh = sizeof(T) == 4 ? (double)(float)(s_eps * (float)anorm) : (double)s_eps * anorm;
        HIPCHK(hipMemsetAsync(d_counters.p, 0, d_counters.bytes(), stream));
        if (++ds_epoch >= 0x7fffffffu) { // (strip flags: a new epoch per factorization)
            HIPCHK(hipMemsetAsync(d_dsflags.p, 0, d_dsflags.bytes(), stream));
            ds_epoch = 1;
        }
        HIPCHK(hipMemsetAsync(d_zpiv.p, 0, d_zpiv.bytes(), stream));
        stamp_reset();
        tm.reset(opts.timing);
        if (zmode) { // ancestor forests another layer factors start from zero
            launch_zranges(zr_off[0], zr_off[1], ZR_ZERO, stream);
            zbytes = 0;
        }
        tm.start(stream);
        HIPCHK(hipEventRecord(ev_start, stream));
        HIPCHK(hipStreamWaitEvent(pstream, ev_start, 0));
        X.s = opts.serial ? stream : pstream;
        stats.n_schur_launches = 0;
        stats.n_schur_big_launches = 0;
        std::fill(path_counts, path_counts + PC_N, 0);
        path_counts[PC_KSPLIT_KINFOS] = n_ksplit_kinfos;
        path_counts[PC_SCHUR_PAIRS] = n_pairs;
        path_counts[PC_SCHUR_FUSED_TILES] = n_fused_tiles;
        path_counts[PC_SCHUR_MAP_PAIRS] = n_map_pairs;
        path_counts[PC_SCHUR_MAP_FUSED_TILES] = n_map_fused_tiles;
        // 3D grids: my phases one after the other, each followed by its
        // ancestor reduction (SRC/pdgstrf3d.c:300-345)
        const int nph = zmode ? my_last + 1 : 1;
        int last_L = -1;
        for (int ph = 0; ph < nph; ++ph) {
            const size_t L0 = zmode ? phase_lv[ph] : 0, L1 = zmode ? phase_lv[ph + 1] : levels.size();
            for (size_t L = L0; L < L1; ++L) {
                tm.level((int)L);
                last_L = (int)L;
                if (xmode && !opts.serial) level_chunked(L, thresh);
                else level_plain(L, thresh);
                HIPCHK(hipEventRecord(ev_rest[L], stream));
                tm.level_end(stream); // level wall time
            }
            if (zmode) {
                hipStream_t P = opts.serial ? stream : pstream;
                if (last_L >= 0) HIPCHK(hipStreamWaitEvent(P, ev_rest[last_L], 0));
                tm.phase_end(P);
                if (ph < maxlvl - 1) {
                    tm.span(4, P, [&] { zreduce(ph, P); });
                    HIPCHK(hipEventRecord(ev_pend, P));
                    HIPCHK(hipStreamWaitEvent(stream, ev_pend, 0));
                }
                tm.reduce_end(P);
            }
        }
        if (xmode && !opts.serial) { // the comm stream's last group before the end of the factorization
            HIPCHK(hipEventRecord(ev_pend, cstream));
            HIPCHK(hipStreamWaitEvent(stream, ev_pend, 0));
        }
        X.s = opts.serial ? stream : pstream;
        HIPCHK(hipEventRecord(ev_pend, pstream));
        HIPCHK(hipStreamWaitEvent(stream, ev_pend, 0));
        HIPCHK(hipGetLastError());
        tm.end(stream);
        double d2h_ms = 0;
        int64_t ncopies = 0;
        double dbytes = 0;
        const bool overlap_dl = opts.overlap_download != 0;
        // diagnostics: SLU_D2H_AFTER=1 starts the D2H only after the device
        // finished the factorization (no overlap, same copy path)
        const bool d2h_after = overlap_dl && getenv("SLU_D2H_AFTER");
        if (d2h_after) sync();
        HelperThread dl; // (after the locals it writes: joined before they go, on every path)
        if (overlap_dl)
            dl.start(device(), [&] {
                const auto t0 = std::chrono::steady_clock::now();
                try {
                    run_d2h(dbytes, ncopies);
                } catch (const std::exception &e) {
                    throw Error(std::string("factor download: ") + e.what());
                }
                d2h_ms = ms_since(t0);
            });
        sync();
        if (overlap_dl) {
            const auto t1 = std::chrono::steady_clock::now();
            dl.join();
            stats.t_d2h_tail_ms = ms_since(t1);
            stats.t_d2h_ms = d2h_ms;
            stats.d2h_bytes = dbytes;
            stats.n_d2h_copies = ncopies;
        }
        host_current = overlap_dl;
        collect_info(info, tiny);
        tm.finish(stats, levels, bylev, iam);
        stamp_dump();
    }

    // ------------------------------------------------------- device solve
    // (solve.h).  Tables are built on the first call (build_solve) and kept.
    bool sv_ready = false;
    vector<int> sv_d_off, sv_l_off, sv_u_off; // per level: diag items, L chunks, U chunks
    DevBuf<SvDiag> d_sv_diag, d_sv_lvl;       // per supernode / in level order
    DevBuf<i64> d_sv_ioff;                    // beside d_sv_lvl: offset of each item's block of DiagInv's inverses
    vector<i64> sv_ioff;                      // the same per supernode (-1: not this rank's), and their total
    i64 sv_inv_total = 0;
    DevBuf<SvDiag> d_sv_pan;                  // per supernode: this rank's L rows below the diagonal block
    DevBuf<SvChunk> d_sv_lch, d_sv_uch;
    DevBuf<i64> d_sv_roff, d_sv_coff;
    DevBuf<int> d_sv_rows, d_sv_ncol, d_sv_gc;
    DevBuf<T> d_sv_x;

    // One kernel over level L's diagonal items, L chunks or U chunks on
    // `stream`: the table arguments every kernel of that family starts with,
    // then `tail`.  Nothing is launched for an empty level; returns whether
    // it launched.
    template <typename K, typename... A> bool sv_diag(int L, K kernel, unsigned threads, A... tail) {
        const int nd = sv_d_off[L + 1] - sv_d_off[L];
        if (nd)
            hipLaunchKernelGGL(kernel, dim3(nd), dim3(threads), 0, stream, d_sv_lvl.p + sv_d_off[L], d_L.p, tail...);
        return nd > 0;
    }
    template <typename K, typename... A> bool sv_lpan(int L, K kernel, unsigned threads, A... tail) {
        const int nc = sv_l_off[L + 1] - sv_l_off[L];
        if (nc)
            hipLaunchKernelGGL(kernel, dim3(nc), dim3(threads), 0, stream, d_sv_lch.p + sv_l_off[L], d_sv_pan.p,
                               d_sv_roff.p, d_sv_rows.p, d_L.p, tail...);
        return nc > 0;
    }
    template <typename K, typename... A> bool sv_upan(int L, K kernel, unsigned threads, A... tail) {
        const int nc = sv_u_off[L + 1] - sv_u_off[L];
        if (nc)
            hipLaunchKernelGGL(kernel, dim3(nc), dim3(threads), 0, stream, d_sv_uch.p + sv_u_off[L], d_sv_diag.p,
                               d_sv_coff.p, d_sv_ncol.p, d_ucol_voff.p, d_ucol_fst.p, d_sv_gc.p, d_U.p, tail...);
        return nc > 0;
    }

    // L and U sweeps over nr <= SV_NR device vectors xv (ld ldx, in place), on `stream`
    template <int NR> void sweep_nr(T *xv, i64 ldx, int nr) {
        const int nl = (int)bylev.size();
        for (int L = 0; L < nl; ++L) { // L y = b
            sv_diag(L, k_sv_ldiag<T, NR>, SVD_THREADS, xv, ldx, nr);
            sv_lpan(L, k_sv_lpanel<T, NR>, SV_THREADS, xv, ldx, nr);
        }
        for (int L = nl - 1; L >= 0; --L) { // U x = y
            sv_upan(L, k_sv_upanel<T, NR>, SV_THREADS, xv, ldx, nr);
            sv_diag(L, k_sv_udiag<T, NR>, SVD_THREADS, xv, ldx, nr);
        }
        HIPCHK(hipGetLastError());
    }
    void sweep(T *xv, i64 ldx = 0, int nr = 1) {
        if (nr == 1) sweep_nr<1>(xv, ldx, 1);
        else sweep_nr<SvNr<T>::v>(xv, ldx, nr);
    }
    // the transposed sweeps over the same levels and tables: U^T z = c
    // ascending (solve, then push along U's rows), L^T y = z descending (pull
    // down L's columns, then solve); conj: B^H (complex plans)
    template <int NR> void sweep_t_nr(T *xv, i64 ldx, int nr, int conj) {
        const int nl = (int)bylev.size();
        for (int L = 0; L < nl; ++L) {
            sv_diag(L, k_sv_utdiag<T, NR>, SVD_THREADS, xv, ldx, nr, conj);
            sv_upan(L, k_sv_utpanel<T, NR>, SV_THREADS, xv, ldx, nr, conj);
        }
        for (int L = nl - 1; L >= 0; --L) {
            sv_lpan(L, k_sv_ltpanel<T, NR>, SV_THREADS, xv, ldx, nr, conj);
            sv_diag(L, k_sv_ltdiag<T, NR>, SVD_THREADS, xv, ldx, nr, conj);
        }
        HIPCHK(hipGetLastError());
    }
    void sweep_t(T *xv, int conj, i64 ldx = 0, int nr = 1) {
        if (nr == 1) sweep_t_nr<1>(xv, ldx, 1, conj);
        else sweep_t_nr<SvNr<T>::v>(xv, ldx, nr, conj);
    }
    // op(B)^-1 on the device vectors: trans 0 = B, 1 = B^T, 2 = B^H
    void sweep_op(int trans, T *xv, i64 ldx = 0, int nr = 1) {
        if (trans) sweep_t(xv, trans == SLU_CONJ, ldx, nr);
        else sweep(xv, ldx, nr);
    }
    // what the transposed calls and rcond refuse (`what` names the call)
    void require_1x1_factors(const char *what) {
        SLU_REQUIRE(!zmode, "%s: not on 3D plans (the transposed sweep runs on 1x1 plans only)", what);
        SLU_REQUIRE(!xmode, "%s: not on a %dx%d grid (the transposed sweep swaps the roles of process "
                    "rows and columns; 1x1 plans only)", what, Pr, Pc);
        SLU_REQUIRE(vstate == 2, "%s: the device storage holds no factors (factor first)", what);
    }
    // the same rules in the words of the block sweep's callers; the grid
    // part alone is what set_diag_inv refuses (it needs no factors)
    void require_1x1_block(const char *what) {
        SLU_REQUIRE(!zmode, "%s: not on 3D plans (the block sweep runs on 1x1 plans only)", what);
        SLU_REQUIRE(!xmode, "%s: not on a %dx%d grid (the block sweep has no exchanges; "
                    "1x1 plans only)", what, Pr, Pc);
    }
    void require_1x1_factors_block(const char *what = "solve_block") {
        require_1x1_block(what);
        SLU_REQUIRE(vstate == 2, "%s: the device storage holds no factors (factor first)", what);
    }

    // ---- 2D grids: the distributed supernodal solve of pdgstrs
    // (SRC/pdgstrs.c, pdgstrs_lsum.c), level-scheduled.  Block row k's partial
    // sums (lsum) live on its process row; per level they are sent to the
    // diagonal owner (k mod Pr, k mod Pc) along the row and added there; the
    // owner solves with the diagonal block; the solved piece goes down the
    // owner's process column to the ranks whose L(:,k) (forward) or U(:,k)
    // (backward) blocks use it, which push -L(i,k) y_k into their partial
    // sums of rows i (forward) or pull -U(i,k) x_k into rows i (backward).
    // b comes in and x goes out replicated on every rank (n values); each
    // rank starts from b on the block rows it owns and zero elsewhere.
    struct SvRed {                       // one partial-sum section of a level
        int k, c;                        // block row, sending process column
        i64 slot;                        // owner: offset of its slot in d_sv_slot
    };
    vector<vector<SvRed>> sv_red;        // per level, this rank's process row's sections
    vector<int> sv_add_off;              // per level: owner's slot-add items
    DevBuf<SvAdd> d_sv_add, d_sv_zero;
    DevBuf<T> d_sv_slot;
    vector<int> sv_own;                  // per supernode: this rank is the diagonal owner

    // The tables of every sweep, on 1x1 plans and grids alike.  A 1x1 plan
    // is the grid whose one rank owns every supernode: the panel of L(:,k)
    // starts below the W(k) rows of the diagonal block, and the exchange
    // lists (zero, adds, sv_red) come out empty.
    void build_solve() {
        const int nl = (int)bylev.size();
        vector<SvDiag> dg(nsupers), pan(nsupers), lvl;
        vector<i64> roff(nsupers, 0), coff(nsupers, 0);
        vector<int> rows, ncol(nsupers, 0), gc;
        sv_own.assign(nsupers, 0);
        vector<SvAdd> zero;
        for (int k = 0; k < nsupers; ++k) {
            SvDiag d{};
            d.w = W(k);
            d.fst = (int)xsup[k];
            d.ld = 0;
            d.voff = 0;
            const bool lcol = k % Pc == mycol, own = lcol && k % Pr == myrow;
            sv_own[k] = own;
            if (!own) zero.push_back({(i64)xsup[k], -1, W(k), 0});
            SvDiag pd = d;
            pd.pad = 0;
            roff[k] = (i64)rows.size();
            const bool held = lcol && lidx[k]; // the diagonal block is part of L(:,k): its owner holds the column
            SLU_REQUIRE(held ? lval_off[k / Pc] >= 0 : !own, "supernode %d has no L column block", k);
            if (held) {
                const int ljb = k / Pc;
                d.voff = lval_off[ljb];
                d.ld = lval_ld[ljb];
                int m = 0, r0 = 0;
                lrows(k, m, r0);
                SLU_REQUIRE(r0 == (own ? W(k) : 0), "supernode %d: diagonal block rows %d", k, r0);
                SLU_REQUIRE(m == d.ld - r0, "supernode %d: panel rows", k);
                pd.voff = lval_off[ljb] + r0;
                pd.ld = lval_ld[ljb];
                pd.pad = m;
                const int_t *ix = lidx[k];
                i64 p = SLU_BC_HEADER;
                for (i64 b = 0; b < ix[0]; ++b) {
                    const int gb = (int)ix[p], nr = (int)ix[p + 1];
                    if (gb != k)
                        for (int i = 0; i < nr; ++i) rows.push_back((int)ix[p + 2 + i]);
                    p += SLU_LB_DESCRIPTOR + nr;
                }
            }
            dg[k] = d;
            pan[k] = pd;
            if (k % Pr == myrow) {
                const int lb = k / Pr;
                if (uval_off[lb] >= 0 && urow_nblk[lb] > 0) {
                    coff[k] = ublk[urow_first[lb]].coloff;
                    for (int b = urow_first[lb]; b < urow_first[lb] + urow_nblk[lb]; ++b)
                        ncol[k] += W(ublk_jb[b]);
                }
            }
        }
        gc.resize(ucol_voff.size());
        for (size_t b = 0; b < ublk.size(); ++b)
            for (int c = 0; c < W(ublk_jb[b]); ++c) gc[ublk[b].coloff + c] = ublk[b].fcol + c;
        vector<SvChunk> lch, uch;
        vector<SvAdd> adds;
        vector<i64> ioff;
        sv_ioff.assign(nsupers, -1);
        sv_inv_total = 0;
        sv_d_off.assign(nl + 1, 0);
        sv_l_off.assign(nl + 1, 0);
        sv_u_off.assign(nl + 1, 0);
        sv_add_off.assign(nl + 1, 0);
        sv_red.assign(nl, {});
        i64 slot_max = 0;
        for (int L = 0; L < nl; ++L) {
            sv_d_off[L] = (int)lvl.size();
            sv_l_off[L] = (int)lch.size();
            sv_u_off[L] = (int)uch.size();
            sv_add_off[L] = (int)adds.size();
            i64 slot = 0;
            for (int k : bylev[L]) {
                if (sv_own[k]) {
                    lvl.push_back(dg[k]);
                    sv_ioff[k] = sv_inv_total;
                    ioff.push_back(sv_inv_total);
                    sv_inv_total += (i64)W(k) * W(k);
                }
                for (int r0 = 0; r0 < pan[k].pad; r0 += SV_THREADS) lch.push_back({k, r0});
                for (int c0 = 0; c0 < ncol[k]; c0 += SVU_COLS) uch.push_back({k, c0});
                if (k % Pr != myrow) continue;
                if (sv_own[k] && Pc > 1) adds.push_back({(i64)xsup[k], slot, W(k), Pc - 1});
                for (int c = 0; c < Pc; ++c) {
                    if (c == k % Pc) continue;
                    SvRed r{k, c, -1};
                    if (sv_own[k]) {
                        r.slot = slot; // the Pc - 1 slots of k are consecutive
                        slot += W(k);
                    }
                    sv_red[L].push_back(r);
                }
            }
            slot_max = std::max(slot_max, slot);
        }
        sv_d_off[nl] = (int)lvl.size();
        sv_l_off[nl] = (int)lch.size();
        sv_u_off[nl] = (int)uch.size();
        sv_add_off[nl] = (int)adds.size();
        d_sv_diag.upload(dg);
        d_sv_pan.upload(pan);
        d_sv_lvl.upload(lvl.empty() ? vector<SvDiag>(1) : lvl);
        d_sv_ioff.upload(ioff.empty() ? vector<i64>(1, 0) : ioff);
        d_sv_lch.upload(lch.empty() ? vector<SvChunk>(1) : lch);
        d_sv_uch.upload(uch.empty() ? vector<SvChunk>(1) : uch);
        d_sv_roff.upload(roff);
        d_sv_coff.upload(coff);
        d_sv_rows.upload(rows.empty() ? vector<int>(1, 0) : rows);
        d_sv_ncol.upload(ncol);
        d_sv_gc.upload(gc.empty() ? vector<int>(1, 0) : gc);
        d_sv_add.upload(adds.empty() ? vector<SvAdd>(1) : adds);
        d_sv_zero.upload(zero.empty() ? vector<SvAdd>(1) : zero);
        d_sv_slot.alloc(std::max<i64>(slot_max, 1));
        d_sv_x.alloc(std::max(n, 1));
        HIPCHK(hipDeviceSynchronize()); // pageable table uploads landed (non-blocking streams)
        sv_ready = true;
    }

    // partial sums of the level's block rows to their owners, added there
    void sv_reduce(int L, T *xv) {
        for (const SvRed &r : sv_red[L]) {
            const int own_c = r.k % Pc;
            T *buf = mycol == r.c ? xv + xsup[r.k] : (mycol == own_c ? d_sv_slot.p + r.slot : nullptr);
            X.section(G_ROW, r.c, 1u << own_c, buf, (size_t)W(r.k) * sizeof(T));
        }
        X.flush_as("solve: partial sums to the diagonal owners", L);
        const int na = sv_add_off[L + 1] - sv_add_off[L];
        if (na)
            hipLaunchKernelGGL(k_sv_add<T>, dim3(na), dim3(256), 0, stream, d_sv_add.p + sv_add_off[L],
                               xv, (const T *)d_sv_slot.p);
    }
    // the solved pieces of the level down their owners' process columns
    void sv_bcast(int L, T *xv, bool fwd) {
        const uint32_t all = Pr >= 32 ? ~0u : (1u << Pr) - 1;
        for (int k : bylev[L]) {
            if (k % Pc != mycol) continue;
            X.section(G_COL, k % Pr, fwd ? cmask(k) : all, xv + xsup[k], (size_t)W(k) * sizeof(T));
        }
        X.flush();
    }

    // sweep_nr<1> on the replicated xv, with the exchanges of each level
    void sweep_2d(T *xv) {
        const int nl = (int)bylev.size();
        const i64 ldx = n;
        X.s = stream;
        const unsigned nz = (unsigned)(nsupers - std::accumulate(sv_own.begin(), sv_own.end(), 0));
        auto zero_others = [&] { // the block rows of other owners
            if (nz) hipLaunchKernelGGL(k_sv_add<T>, dim3(nz), dim3(256), 0, stream, d_sv_zero.p, xv, (const T *)nullptr);
        };
        zero_others();
        for (int L = 0; L < nl; ++L) { // L y = b
            sv_reduce(L, xv);
            sv_diag(L, k_sv_ldiag<T, 1>, SVD_THREADS, xv, ldx, 1);
            sv_bcast(L, xv, true);
            sv_lpan(L, k_sv_lpanel<T, 1>, SV_THREADS, xv, ldx, 1);
        }
        const bool fwd_only = getenv("SLU_SV_FWD_ONLY") != nullptr; // diagnostics: y = L^-1 b
        if (!fwd_only) zero_others();
        for (int L = fwd_only ? -1 : nl - 1; L >= 0; --L) { // U x = y
            sv_upan(L, k_sv_upanel<T, 1>, SV_THREADS, xv, ldx, 1);
            sv_reduce(L, xv);
            sv_diag(L, k_sv_udiag<T, 1>, SVD_THREADS, xv, ldx, 1);
            sv_bcast(L, xv, false);
        }
        sv_gather(xv);
        HIPCHK(hipGetLastError());
    }
    // each diagonal owner's block rows of xv to every rank (xv replicated)
    void sv_gather(T *xv) {
        for (int k = 0; k < nsupers; ++k)
            X.section(G_WORLD, (k % Pr) * Pc + k % Pc, ~0u, xv + xsup[k], (size_t)W(k) * sizeof(T));
        X.flush();
    }

    // right-hand sides in batches of SvNr<T>: every factor element is read once
    // per batch and sweep
    void solve(void *b, int64_t ldb, int nrhs) override { solve_op(SLU_NOTRANS, b, ldb, nrhs); }
    void solve_t(int trans, void *b, int64_t ldb, int nrhs) override {
        SLU_REQUIRE(trans >= SLU_NOTRANS && trans <= SLU_CONJ, "solve_t: trans = %d is none of SLU_NOTRANS, SLU_TRANS, SLU_CONJ", trans);
        if (trans != SLU_NOTRANS) require_1x1_factors("solve_t");
        solve_op(trans, b, ldb, nrhs);
    }
    // columns c0 .. c0 + nc of the host array b (ld ldb, elements of E's
    // size: T's, or doubles for the mixed-precision calls) to / from nc device
    // vectors of n values at dv, on `stream`
    template <typename E> void cols_h2d(E *dv, const void *b, i64 ldb, int c0, int nc) {
        for (int q = 0; q < nc; ++q)
            HIPCHK(hipMemcpyAsync(dv + (i64)q * n, (const char *)b + (i64)(c0 + q) * ldb * sizeof(E),
                                  (size_t)n * sizeof(E), hipMemcpyHostToDevice, stream));
    }
    template <typename E> void cols_d2h(void *b, i64 ldb, int c0, int nc, const E *dv) {
        for (int q = 0; q < nc; ++q)
            HIPCHK(hipMemcpyAsync((char *)b + (i64)(c0 + q) * ldb * sizeof(E), dv + (i64)q * n,
                                  (size_t)n * sizeof(E), hipMemcpyDeviceToHost, stream));
    }
    void solve_op(int trans, void *b, int64_t ldb, int nrhs) {
        SLU_REQUIRE(!zmode, "solve: 3D plans hold the factors spread over the layers (gather them to a 2D plan)");
        SLU_REQUIRE(vstate == 2, "solve: the device storage holds no factors (factor first)");
        if (!sv_ready) build_solve();
        SLU_REQUIRE(ldb >= n && nrhs >= 0, "solve: ldb %lld < n %d", (long long)ldb, n);
        const int NB = xmode ? 1 : SvNr<T>::v; // grids: one right-hand side per sweep_2d
        if (xmode) HIPCHK(hipStreamSynchronize(pstream));
        else if (nrhs > 1 && d_sv_x.n < (size_t)n * NB) d_sv_x.alloc((size_t)std::max(n, 1) * NB);
        EventTimer tm;
        float total = 0;
        for (int r0 = 0; r0 < nrhs; r0 += NB) {
            const int nr = std::min(NB, nrhs - r0);
            cols_h2d(d_sv_x.p, b, ldb, r0, nr);
            tm.start(stream);
            if (xmode) sweep_2d(d_sv_x.p);
            else sweep_op(trans, d_sv_x.p, n, nr);
            tm.stop(stream);
            cols_d2h(b, ldb, r0, nr, d_sv_x.p);
            HIPCHK(hipStreamSynchronize(stream));
            total += tm.ms();
        }
        stats.t_solve_ms = total;
    }

    // ---- block solve (solve_block.h): SvbNr right-hand sides per pass over
    // the factors, in a row-major working buffer allocated on first use
    DevBuf<T> d_svb_x, d_svb_stage;

    // ---- DiagInv (solve_block_inv.h): with the mode on, sweep_block applies
    // inverted diagonal blocks by MFMA products.  The inverses are those of
    // the device factors while dinv_valid holds; a block sweep's caller
    // recomputes them first when it does not (diag_inv_ensure), outside the
    // sweep's own timers.  The transposed block sweep keeps substituting.
    bool dinv_on = false;
    DevBuf<T> d_svb_inv; // sv_inv_total elements at d_sv_ioff's offsets, allocated at the first computation
    int dinv_computes = 0;
    double dinv_ms = 0;
    void set_diag_inv(int on) override {
        require_1x1_block("set_diag_inv");
        dinv_on = on != 0;
        if (!dinv_on) {
            d_svb_inv.release();
            dinv_valid = false;
        }
    }
    void diag_inv_info(int *on, int *valid, int64_t *bytes, int *computes, double *ms) override {
        if (on) *on = dinv_on;
        if (valid) *valid = dinv_on && dinv_valid;
        if (bytes) *bytes = (int64_t)d_svb_inv.bytes();
        if (computes) *computes = dinv_computes;
        if (ms) *ms = dinv_ms;
    }
    // every diagonal block of the device factors inverted into d_svb_inv: one
    // launch, timed on its own
    void diag_inv_compute() {
        if (!sv_ready) build_solve();
        if (d_svb_inv.n != (size_t)sv_inv_total) d_svb_inv.alloc((size_t)sv_inv_total);
        const int nd = sv_d_off[bylev.size()];
        EventTimer tm;
        HIPCHK(hipStreamSynchronize(pstream));
        tm.start(stream);
        if (nd)
            hipLaunchKernelGGL(k_svb_inv<T>, dim3(nd), dim3(SVB_ITHREADS), 0, stream, (const SvDiag *)d_sv_lvl.p,
                               (const T *)d_L.p, (const i64 *)d_sv_ioff.p, d_svb_inv.p);
        HIPCHK(hipGetLastError());
        tm.stop(stream);
        dinv_ms = tm.ms();
        ++dinv_computes;
        dinv_valid = true;
    }
    void diag_inv_ensure() {
        if (dinv_on && !dinv_valid) diag_inv_compute();
    }
    void diag_inv_block(int k, int *fst, int *w, void *out, int64_t ldo) override {
        require_1x1_block("diag_inv_block");
        SLU_REQUIRE(k >= 0 && k < nsupers, "diag_inv_block: supernode %d is none of the plan's %d", k, nsupers);
        const int wk = W(k);
        if (fst) *fst = (int)xsup[k];
        if (w) *w = wk;
        if (!out) return;
        SLU_REQUIRE(ldo >= wk, "diag_inv_block: ldo %lld < the supernode's width %d", (long long)ldo, wk);
        SLU_REQUIRE(dinv_on, "diag_inv_block: the mode is off (slu_plan_set_diag_inv first)");
        SLU_REQUIRE(vstate == 2, "diag_inv_block: the device storage holds no factors (factor first)");
        diag_inv_ensure();
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy2D(out, (size_t)ldo * sizeof(T), d_svb_inv.p + sv_ioff[k], (size_t)wk * sizeof(T),
                           (size_t)wk * sizeof(T), (size_t)wk, hipMemcpyDeviceToHost));
    }
    // the level order of sweep_nr on the row-major X; returns the launches
    i64 sweep_block(T *xb) {
        const int nl = (int)bylev.size();
        i64 nk = 0;
        const bool inv = dinv_on; // the callers have made the inverses valid (diag_inv_ensure)
        const T *mi = d_svb_inv.p;
        for (int L = 0; L < nl; ++L) { // L Y = B
            nk += inv ? sv_diag(L, k_svb_minv<T, false>, SVB_ITHREADS, d_sv_ioff.p + sv_d_off[L], mi, xb)
                      : sv_diag(L, k_svb_ldiag<T>, SVB_DTHREADS, xb);
            nk += sv_lpan(L, k_svb_lpanel<T>, SVB_LTHREADS, xb);
        }
        for (int L = nl - 1; L >= 0; --L) { // U X = Y
            nk += sv_upan(L, k_svb_upanel<T>, SV_THREADS, xb);
            nk += inv ? sv_diag(L, k_svb_minv<T, true>, SVB_ITHREADS, d_sv_ioff.p + sv_d_off[L], mi, xb)
                      : sv_diag(L, k_svb_udiag<T>, SVB_DTHREADS, xb);
        }
        HIPCHK(hipGetLastError());
        return nk;
    }
    // the transposed block sweep (solve_block_t.h): the level walk of
    // sweep_t_nr on the row-major X; returns the launches
    i64 sweep_block_t(T *xb, int conj) {
        const int nl = (int)bylev.size();
        i64 nk = 0;
        for (int L = 0; L < nl; ++L) { // U^T Z = C
            nk += sv_diag(L, k_svb_utdiag<T>, SVB_DTHREADS, xb, conj);
            nk += sv_upan(L, k_svb_utpanel<T>, SV_THREADS, xb, conj);
        }
        for (int L = nl - 1; L >= 0; --L) { // L^T Y = Z
            nk += sv_lpan(L, k_svb_ltpanel<T>, SVB_LTHREADS, xb, conj);
            nk += sv_diag(L, k_svb_ltdiag<T>, SVB_DTHREADS, xb, conj);
        }
        HIPCHK(hipGetLastError());
        return nk;
    }
    // op(B)^-1 on the row-major X: trans 0 = B, 1 = B^T, 2 = B^H
    i64 sweep_block_op(int trans, T *xb) {
        return trans ? sweep_block_t(xb, trans == SLU_CONJ) : sweep_block(xb);
    }
    void solve_block(void *b, int64_t ldb, int nrhs, int on_device) override {
        solve_block_op("solve_block", SLU_NOTRANS, b, ldb, nrhs, on_device);
    }
    void solve_block_t(int trans, void *b, int64_t ldb, int nrhs, int on_device) override {
        SLU_REQUIRE(trans >= SLU_NOTRANS && trans <= SLU_CONJ,
                    "solve_block_t: trans = %d is none of SLU_NOTRANS, SLU_TRANS, SLU_CONJ", trans);
        solve_block_op(trans ? "solve_block_t" : "solve_block", trans, b, ldb, nrhs, on_device);
    }
    void solve_block_op(const char *what, int trans, void *b, int64_t ldb, int nrhs, int on_device) {
        require_1x1_factors_block(what);
        SLU_REQUIRE(ldb >= n && nrhs >= 0, "%s: ldb %lld < n %d or nrhs %d < 0", what, (long long)ldb, n, nrhs);
        svb_passes = 0;
        svb_launches = 0;
        svb_ms = 0;
        stats.t_solve_ms = 0;
        if (nrhs == 0 || n == 0) return;
        if (!sv_ready) build_solve();
        if (!trans) diag_inv_ensure();
        constexpr int NRB = SvbNr<T>::v;
        const size_t nn = (size_t)n;
        if (d_svb_x.n < nn * NRB) d_svb_x.alloc(nn * NRB);
        if (!on_device && d_svb_stage.n < nn * NRB) d_svb_stage.alloc(nn * NRB);
        EventTimer tm;
        const unsigned tb = (unsigned)((n + SVB_TR_ROWS - 1) / SVB_TR_ROWS);
        float total = 0;
        for (int r0 = 0; r0 < nrhs; r0 += NRB) {
            const int nr = std::min(NRB, nrhs - r0);
            T *cols = on_device ? (T *)b + (i64)r0 * ldb : d_svb_stage.p; // the pass's columns on the device
            const i64 ldc = on_device ? ldb : (i64)n;
            if (!on_device) cols_h2d(cols, b, ldb, r0, nr);
            tm.start(stream);
            hipLaunchKernelGGL((k_svb_in<T>), dim3(tb), dim3(256), 0, stream, (const T *)cols, ldc, n, nr, d_svb_x.p);
            svb_launches += 2 + sweep_block_op(trans, d_svb_x.p);
            hipLaunchKernelGGL((k_svb_out<T>), dim3(tb), dim3(256), 0, stream, (const T *)d_svb_x.p, n, nr, cols, ldc);
            HIPCHK(hipGetLastError());
            tm.stop(stream);
            if (!on_device) cols_d2h(b, ldb, r0, nr, cols);
            HIPCHK(hipStreamSynchronize(stream));
            total += tm.ms();
            ++svb_passes;
        }
        svb_ms = total;
        stats.t_solve_ms = total;
    }

    // Iterative refinement on the device (SRC/pdgsrfs.c:197-253, 1x1 grid,
    // permuted coordinates): R = B - A X and S = |A||X| + |B| by rows of A
    // (k_resid), componentwise backward error berr = max |R_i| / S_i with the
    // SAFE1/SAFE2 guards (:219-230); while berr > eps, berr halves and fewer
    // than ITMAX = 20 steps: solve A dx = R with the device factors, X += dx.
    // A is the matrix of the last slu_plan_fill_a.
    DevBuf<i64> d_rp;
    DevBuf<int> d_rc;
    DevBuf<i64> d_re;
    const T *d_acur = nullptr;
    DevBuf<T> d_rf_b, d_rf_x, d_rf_r;
    DevBuf<unsigned long long> d_rf_berr;

    // 2D grids: the same loop with pdgsmv's distributed residual (solve.h
    // k_resid_part / k_resid_fin): partial rows from each rank's entries of
    // A, reduced along process rows to the diagonal owners, berr = the max
    // over the owners, R gathered to every rank, then the 2D solve.
    vector<RfRow> rf_rows_h;
    DevBuf<RfRow> d_rf_rows;
    DevBuf<double> d_rf_s, d_rf_ss;
    DevBuf<T> d_rf_sr;
    vector<std::array<i64, 3>> rf_secs; // (block row, sending column, owner slot)

    void build_refine_2d() {
        rf_rows_h.clear();
        rf_secs.clear();
        i64 slot = 0;
        for (int k = 0; k < nsupers; ++k) {
            if (k % Pr != myrow) continue;
            const bool own = k % Pc == mycol;
            if (own) rf_rows_h.push_back({(i64)xsup[k], slot, W(k), Pc - 1});
            for (int c = 0; c < Pc; ++c) {
                if (c == k % Pc) continue;
                rf_secs.push_back({k, c, own ? slot : -1});
                if (own) slot += W(k);
            }
        }
        d_rf_rows.upload(rf_rows_h.empty() ? vector<RfRow>(1) : rf_rows_h);
        d_rf_sr.alloc(std::max<i64>(slot, 1));
        d_rf_ss.alloc(std::max<i64>(slot, 1));
        d_rf_s.alloc(std::max(n, 1));
        HIPCHK(hipDeviceSynchronize());
    }

    // this process row's partial residual rows r (elements of rsz bytes) and
    // partial sums d_rf_s to the diagonal owners' slots sr and d_rf_ss
    void rf_reduce(void *r, void *sr, size_t rsz) {
        for (const auto &q : rf_secs) {
            const int k = (int)q[0], c = (int)q[1], oc = k % Pc;
            const size_t w = (size_t)W(k);
            void *br = mycol == c ? (char *)r + xsup[k] * rsz : mycol == oc ? (char *)sr + q[2] * rsz : nullptr;
            void *bs = mycol == c ? (void *)(d_rf_s.p + xsup[k]) : mycol == oc ? (void *)(d_rf_ss.p + q[2]) : nullptr;
            X.section(G_ROW, c, 1u << oc, br, w * rsz);
            X.section(G_ROW, c, 1u << oc, bs, w * sizeof(double));
        }
        X.flush();
    }

    double resid_2d(double safe1, double safe2) {
        const unsigned rb = (unsigned)((n + 255) / 256);
        X.s = stream;
        hipLaunchKernelGGL(k_resid_part<T>, dim3(rb), dim3(256), 0, stream, d_rp.p, d_rc.p, d_re.p,
                           a_fact, d_rf_x.p, d_rf_r.p, d_rf_s.p, n);
        rf_reduce(d_rf_r.p, d_rf_sr.p, sizeof(T));
        HIPCHK(hipMemsetAsync(d_rf_berr.p, 0, sizeof(unsigned long long), stream));
        if (!rf_rows_h.empty())
            hipLaunchKernelGGL(k_resid_fin<T>, dim3((unsigned)rf_rows_h.size()), dim3(256), 0, stream,
                               d_rf_rows.p, d_rf_b.p, d_rf_r.p, d_rf_s.p, d_rf_sr.p, d_rf_ss.p, safe1,
                               safe2, d_rf_berr.p);
        HIPCHK(hipGetLastError());
        unsigned long long bits = 0;
        HIPCHK(hipMemcpyAsync(&bits, d_rf_berr.p, sizeof bits, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        // the max over the owners (bit patterns of non-negative doubles, NaN above +Inf)
        auto all = X.allgatherv(G_WORLD, vector<i64>(1, (i64)bits));
        unsigned long long m = 0;
        for (auto &v : all) m = std::max(m, (unsigned long long)v[0]);
        double be;
        memcpy(&be, &m, sizeof be);
        return be;
    }

    void refine(const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        refine_op(SLU_NOTRANS, b, x, ld, nrhs, berr, steps);
    }
    void refine_t(int trans, const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        SLU_REQUIRE(trans >= SLU_NOTRANS && trans <= SLU_CONJ, "refine_t: trans = %d is none of SLU_NOTRANS, SLU_TRANS, SLU_CONJ", trans);
        if (trans != SLU_NOTRANS) require_1x1_factors("refine_t");
        refine_op(trans, b, x, ld, nrhs, berr, steps);
    }

    // The CSC view of A for the transposed residual (k_resid_t), made on the
    // device from the rows of set_a_pattern at the first transposed refine.
    bool csc_ready = false;
    DevBuf<int> d_csc_ci;
    DevBuf<unsigned long long> d_csc_lo, d_csc_hi;
    void build_csc() {
        const size_t nn = (size_t)std::max(n, 1);
        d_csc_ci.alloc(std::max<i64>(a_nnz, 1));
        d_csc_lo.alloc(nn);
        d_csc_hi.alloc(nn);
        HIPCHK(hipMemsetAsync(d_csc_lo.p, 0xff, nn * sizeof(unsigned long long), stream));
        HIPCHK(hipMemsetAsync(d_csc_hi.p, 0, nn * sizeof(unsigned long long), stream));
        if (n)
            hipLaunchKernelGGL(k_csc_of_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                               d_rp.p, d_rc.p, d_re.p, n, d_csc_ci.p, d_csc_lo.p, d_csc_hi.p);
        HIPCHK(hipGetLastError());
        csc_ready = true;
    }

    // r <- op(B)^-1 r with the device factors (grids: R from its owners to
    // every rank first, then the 2D solve)
    void correct(int trans, T *r) {
        if (xmode) {
            sv_gather(r);
            sweep_2d(r);
        } else {
            sweep_op(trans, r);
        }
    }

    // The loop of pdgsrfs over right-hand sides and steps; t_refine_ms.
    // load(j) puts b and x of column j on the device, resid() returns berr of
    // the current x, step() adds one correction to x, store(j) copies x back.
    template <typename Ld, typename Rs, typename Cx, typename St>
    void refine_loop(double eps, int nrhs, double *berr, int *steps, Ld load, Rs resid, Cx step, St store) {
        EventTimer tm;
        HIPCHK(hipStreamSynchronize(pstream));
        tm.start(stream);
        for (int j = 0; j < nrhs; ++j) {
            load(j);
            int count = 0;
            double lstres = 3.0, be = 0.0;
            while (true) {
                be = resid();
                if (!(be > eps && be * 2 <= lstres && count < 20)) break;
                step();
                lstres = be;
                ++count;
            }
            store(j);
            HIPCHK(hipStreamSynchronize(stream));
            if (berr) berr[j] = be;
            if (steps) steps[j] = count;
        }
        tm.stop(stream);
        HIPCHK(hipStreamSynchronize(stream));
        stats.t_refine_ms = tm.ms();
    }

    void refine_op(int trans, const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) {
        SLU_REQUIRE(!zmode, "refine: not on 3D plans");
        SLU_REQUIRE(vstate == 2, "refine: the device storage holds no factors (factor first)");
        SLU_REQUIRE(a_fact != nullptr,
                    "refine needs the values of A the factors came from (slu_plan_fill_a "
                    "before slu_plan_factor)");
        SLU_REQUIRE(ld >= n && nrhs >= 0, "refine: ld %lld < n %d", (long long)ld, n);
        if (!sv_ready) build_solve();
        const bool dbl = !std::is_same<T, float>::value;
        const double eps = dbl ? 0.5 * 2.220446049250313e-16 : 0.5 * 1.1920928955078125e-07;
        const double safmin = dbl ? 2.2250738585072014e-308 : 1.1754943508222875e-38;
        const double safe1 = (double)(n + 1) * safmin, safe2 = safe1 / eps;
        d_rf_b.alloc(std::max(n, 1));
        d_rf_x.alloc(std::max(n, 1));
        d_rf_r.alloc(std::max(n, 1));
        d_rf_berr.alloc(1);
        if (xmode && rf_rows_h.empty() && rf_secs.empty()) build_refine_2d();
        if (trans && !csc_ready) build_csc();
        const unsigned rb = (unsigned)((n + 255) / 256);
        refine_loop(
            eps, nrhs, berr, steps,
            [&](int j) {
                cols_h2d(d_rf_b.p, b, ld, j, 1);
                cols_h2d(d_rf_x.p, x, ld, j, 1);
            },
            [&] {
                if (xmode) return resid_2d(safe1, safe2);
                HIPCHK(hipMemsetAsync(d_rf_berr.p, 0, sizeof(unsigned long long), stream));
                if (trans)
                    hipLaunchKernelGGL(k_resid_t<T>, dim3(rb), dim3(256), 0, stream, d_csc_lo.p, d_csc_hi.p,
                                       d_csc_ci.p, a_fact, d_rf_x.p, d_rf_b.p, d_rf_r.p, n, safe1, safe2,
                                       d_rf_berr.p, (int)(trans == SLU_CONJ));
                else
                    hipLaunchKernelGGL(k_resid<T>, dim3(rb), dim3(256), 0, stream, d_rp.p, d_rc.p, d_re.p,
                                       a_fact, d_rf_x.p, d_rf_b.p, d_rf_r.p, n, safe1, safe2, d_rf_berr.p);
                HIPCHK(hipGetLastError());
                unsigned long long bits = 0;
                HIPCHK(hipMemcpyAsync(&bits, d_rf_berr.p, sizeof bits, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                double be;
                memcpy(&be, &bits, sizeof be);
                return be;
            },
            [&] {
                correct(trans, d_rf_r.p);
                hipLaunchKernelGGL(k_axpy1<T>, dim3(rb), dim3(256), 0, stream, d_rf_x.p, d_rf_r.p, n);
            },
            [&](int j) { cols_d2h(x, ld, j, 1, d_rf_x.p); });
    }

    // Mixed-precision refinement of an fp32 plan (refine_d2.h): the loop of
    // refine() with fp64's constants on the fp64 A of fill_a_d2; b, x, the
    // residual and the update in fp64, the correction from the fp32 sweep of
    // the residual scaled by 2^-e, rmax = m 2^e with m in [0.5, 1).
    DevBuf<double> d_d2_b, d_d2_x, d_d2_r, d_d2_sr;
    DevBuf<unsigned long long> d_d2_max; // bit patterns of berr, rmax

    // berr and rmax of the current x: mx[0], mx[1]
    void resid_d2(double safe1, double safe2, double mx[2]) {
        const unsigned rb = (unsigned)((n + 255) / 256);
        unsigned long long bits[2] = {0, 0};
        HIPCHK(hipMemsetAsync(d_d2_max.p, 0, sizeof bits, stream));
        if (!xmode) {
            hipLaunchKernelGGL(k_resid_d2, dim3(rb), dim3(256), 0, stream, d_rp.p, d_rc.p, d_re.p, a_fact64,
                               d_d2_x.p, d_d2_b.p, d_d2_r.p, n, safe1, safe2, d_d2_max.p);
        } else {
            X.s = stream;
            hipLaunchKernelGGL(k_resid_part_d2, dim3(rb), dim3(256), 0, stream, d_rp.p, d_rc.p, d_re.p,
                               a_fact64, d_d2_x.p, d_d2_r.p, d_rf_s.p, n);
            rf_reduce(d_d2_r.p, d_d2_sr.p, sizeof(double)); // the sections of resid_2d, r_p as doubles
            if (!rf_rows_h.empty())
                hipLaunchKernelGGL(k_resid_fin_d2, dim3((unsigned)rf_rows_h.size()), dim3(256), 0, stream,
                                   d_rf_rows.p, d_d2_b.p, d_d2_r.p, d_rf_s.p, d_d2_sr.p, d_rf_ss.p, safe1,
                                   safe2, d_d2_max.p);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(bits, d_d2_max.p, sizeof bits, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (xmode) { // the maxima over the diagonal owners (NaN above +Inf as a bit pattern)
            auto all = X.allgatherv(G_WORLD, vector<i64>{(i64)bits[0], (i64)bits[1]});
            bits[0] = bits[1] = 0;
            for (auto &v : all)
                for (int t = 0; t < 2; ++t) bits[t] = std::max(bits[t], (unsigned long long)v[t]);
        }
        memcpy(mx, bits, sizeof bits);
    }

    void refine_d2(const double *b, double *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        if constexpr (std::is_same<T, float>::value) {
            SLU_REQUIRE(!zmode, "refine_d2: not on 3D plans");
            SLU_REQUIRE(vstate == 2, "refine_d2: the device storage holds no factors (factor first)");
            SLU_REQUIRE(a_fact64 != nullptr,
                        "refine_d2 needs the fp64 values of A the factors came from "
                        "(slu_plan_fill_a_d2 before slu_plan_factor)");
            SLU_REQUIRE(ld >= n && nrhs >= 0, "refine_d2: ld %lld < n %d", (long long)ld, n);
            if (!sv_ready) build_solve();
            const double eps = 0.5 * 2.220446049250313e-16, safmin = 2.2250738585072014e-308;
            const double safe1 = (double)(n + 1) * safmin, safe2 = safe1 / eps;
            const size_t nn = (size_t)std::max(n, 1);
            if (d_d2_b.n != nn) {
                d_d2_b.alloc(nn);
                d_d2_x.alloc(nn);
                d_d2_r.alloc(nn);
                d_d2_max.alloc(2);
            }
            if (d_rf_r.n != nn) d_rf_r.alloc(nn); // the fp32 residual / correction
            if (xmode) {
                if (rf_rows_h.empty() && rf_secs.empty()) build_refine_2d();
                if (d_d2_sr.n != d_rf_sr.n) d_d2_sr.alloc(d_rf_sr.n);
            }
            const unsigned rb = (unsigned)((n + 255) / 256);
            const size_t nb = (size_t)n * sizeof(double);
            double mx[2] = {0.0, 0.0};
            refine_loop(
                eps, nrhs, berr, steps,
                [&](int j) {
                    HIPCHK(hipMemcpyAsync(d_d2_b.p, b + (i64)j * ld, nb, hipMemcpyHostToDevice, stream));
                    HIPCHK(hipMemcpyAsync(d_d2_x.p, x + (i64)j * ld, nb, hipMemcpyHostToDevice, stream));
                },
                [&] {
                    resid_d2(safe1, safe2, mx);
                    return mx[0];
                },
                [&] {
                    int e = 0;
                    if (mx[1] > 0.0 && std::isfinite(mx[1])) (void)frexp(mx[1], &e);
                    hipLaunchKernelGGL(k_scale_cvt_d2, dim3(rb), dim3(256), 0, stream, d_d2_r.p, d_rf_r.p, n, e);
                    correct(SLU_NOTRANS, d_rf_r.p); // the owners' rows of r32 on grids
                    hipLaunchKernelGGL(k_axpy_d2, dim3(rb), dim3(256), 0, stream, d_d2_x.p, d_rf_r.p, n, e);
                },
                [&](int j) { HIPCHK(hipMemcpyAsync(x + (i64)j * ld, d_d2_x.p, nb, hipMemcpyDeviceToHost, stream)); });
        } else {
            throw Error(fmt("refine_d2: fp32 plans only, this plan's dtype is %s", dtype_name()));
        }
    }

    // ---- block refinement (refine_block.h): the loop of refine_loop on a
    // pass of SvbNr columns at once.  X, B and R of the pass are row-major
    // buffers of n rows of SvbNr values of E (T, or double on an fp32 plan's
    // mixed-precision loop), three sections of d_rfb, allocated on first use
    // and kept.  A host array's columns are staged through R, which holds
    // nothing while a pass loads or stores.
    DevBuf<char> d_rfb;
    DevBuf<unsigned long long> d_rfb_max; // per column: bit patterns of berr, then (D2) of rmax

    // Per column the rule of refine_loop: count / lstres / berr arrays, one
    // D2H of the bit patterns per step, a stopped column frozen.
    // resid(xb, bb, rb, rg, out) launches the residual kernel of the pass on
    // rg workgroups (R and the per-column maxima `out`); step(xb, rb, act,
    // live, mx) turns R into the correction of the columns of `act` and adds
    // it to X (live = the pass's columns, mx = the residual's maxima).
    template <typename E, bool D2, typename Rs, typename Cx>
    void refine_block_loop(const char *what, double eps, const void *b, void *x, i64 ld, int nrhs, int on_device,
                           double *berr, int *steps, Rs resid, Cx step) {
        constexpr int NRB = SvbNr<E>::v, NMAX = D2 ? 2 * NRB : NRB;
        SLU_REQUIRE(ld >= n && nrhs >= 0, "%s: ld %lld < n %d or nrhs %d < 0", what, (long long)ld, n, nrhs);
        rfb_passes = rfb_sweeps = rfb_resids = 0;
        rfb_ms = 0;
        stats.t_refine_ms = 0;
        if (nrhs == 0 || n == 0) return;
        if (!sv_ready) build_solve();
        const size_t sec = (size_t)n * NRB * sizeof(E);
        if (d_rfb.n < 3 * sec) d_rfb.alloc(3 * sec);
        if (d_rfb_max.n < (size_t)NMAX) d_rfb_max.alloc(NMAX);
        E *xb = (E *)d_rfb.p, *bb = (E *)(d_rfb.p + sec), *rb = (E *)(d_rfb.p + 2 * sec);
        const unsigned tb = (unsigned)((n + SVB_TR_ROWS - 1) / SVB_TR_ROWS);
        const unsigned rg = (unsigned)((n + RFB_THREADS / NRB - 1) / (RFB_THREADS / NRB));
        EventTimer tm;
        HIPCHK(hipStreamSynchronize(pstream));
        tm.start(stream);
        for (int r0 = 0; r0 < nrhs; r0 += NRB) {
            const int nr = std::min(NRB, nrhs - r0);
            const i64 ldc = on_device ? ld : (i64)n;
            // b, then x: column-major on the device (the caller's, or staged in R) -> row-major
            for (int w = 0; w < 2; ++w) {
                const E *cols = on_device ? (const E *)(w ? x : b) + (i64)r0 * ld : rb;
                if (!on_device) cols_h2d(rb, w ? x : b, ld, r0, nr);
                hipLaunchKernelGGL((k_svb_in<E>), dim3(tb), dim3(256), 0, stream, cols, ldc, n, nr, w ? xb : bb);
            }
            const unsigned live = nr == 32 ? ~0u : (1u << nr) - 1;
            unsigned act = live;
            int count[NRB] = {};
            double lstres[NRB], be[NRB] = {}, mx[NMAX];
            std::fill(lstres, lstres + NRB, 3.0);
            while (true) {
                unsigned long long bits[NMAX];
                HIPCHK(hipMemsetAsync(d_rfb_max.p, 0, sizeof bits, stream));
                resid((const E *)xb, (const E *)bb, rb, rg, d_rfb_max.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(bits, d_rfb_max.p, sizeof bits, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                ++rfb_resids;
                memcpy(mx, bits, sizeof bits);
                unsigned go = 0;
                for (int q = 0; q < nr; ++q) {
                    if (!((act >> q) & 1u)) continue;
                    be[q] = mx[q];
                    if (be[q] > eps && be[q] * 2 <= lstres[q] && count[q] < 20) go |= 1u << q;
                }
                act = go;
                if (!act) break;
                step(xb, rb, act, live, mx);
                HIPCHK(hipGetLastError());
                for (int q = 0; q < nr; ++q) {
                    if (!((act >> q) & 1u)) continue;
                    lstres[q] = be[q];
                    ++count[q];
                }
                ++rfb_sweeps;
            }
            E *cols = on_device ? (E *)x + (i64)r0 * ld : rb;
            hipLaunchKernelGGL((k_svb_out<E>), dim3(tb), dim3(256), 0, stream, (const E *)xb, n, nr, cols, ldc);
            HIPCHK(hipGetLastError());
            if (!on_device) cols_d2h(x, ld, r0, nr, (const E *)rb);
            HIPCHK(hipStreamSynchronize(stream));
            for (int q = 0; q < nr; ++q) {
                if (berr) berr[r0 + q] = be[q];
                if (steps) steps[r0 + q] = count[q];
            }
            ++rfb_passes;
        }
        tm.stop(stream);
        rfb_ms = stats.t_refine_ms = tm.ms();
    }

    // the untransposed residual of a pass: k_rfb_resid over the rows of A
    template <typename E, bool D2> auto rfb_resid_rows(const E *a, double safe1, double safe2) {
        return [=](const E *xb, const E *bb, E *rb, unsigned rg, unsigned long long *out) {
            hipLaunchKernelGGL((k_rfb_resid<E, D2>), dim3(rg), dim3(RFB_THREADS), 0, stream, d_rp.p, d_rc.p,
                               d_re.p, a, xb, bb, rb, n, safe1, safe2, out);
        };
    }

    void refine_block(const void *b, void *x, int64_t ld, int nrhs, int on_device, double *berr,
                      int *steps) override {
        refine_block_op("refine_block", SLU_NOTRANS, b, x, ld, nrhs, on_device, berr, steps);
    }
    void refine_block_t(int trans, const void *b, void *x, int64_t ld, int nrhs, int on_device, double *berr,
                        int *steps) override {
        SLU_REQUIRE(trans >= SLU_NOTRANS && trans <= SLU_CONJ,
                    "refine_block_t: trans = %d is none of SLU_NOTRANS, SLU_TRANS, SLU_CONJ", trans);
        refine_block_op(trans ? "refine_block_t" : "refine_block", trans, b, x, ld, nrhs, on_device, berr, steps);
    }
    // trans != 0: the residual by columns of A (k_rfb_resid_t over build_csc's
    // view) and the transposed block sweep, the rest of the loop unchanged
    void refine_block_op(const char *what, int trans, const void *b, void *x, int64_t ld, int nrhs, int on_device,
                         double *berr, int *steps) {
        require_1x1_factors_block(what);
        SLU_REQUIRE(a_fact != nullptr,
                    "%s needs the values of A the factors came from (slu_plan_fill_a "
                    "before slu_plan_factor)", what);
        const bool dbl = !std::is_same<T, float>::value;
        const double eps = dbl ? 0.5 * 2.220446049250313e-16 : 0.5 * 1.1920928955078125e-07;
        const double safmin = dbl ? 2.2250738585072014e-308 : 1.1754943508222875e-38;
        const double safe1 = (double)(n + 1) * safmin, safe2 = safe1 / eps;
        const i64 total = (i64)n * SvbNr<T>::v;
        const unsigned eb = (unsigned)((total + RFB_THREADS - 1) / RFB_THREADS);
        const int conj = trans == SLU_CONJ;
        auto step = [&](T *xb, T *rb, unsigned act, unsigned live, const double *) {
            if (act != live)
                hipLaunchKernelGGL(k_rfb_mask<T>, dim3(eb), dim3(RFB_THREADS), 0, stream, rb, total, act);
            sweep_block_op(trans, rb);
            hipLaunchKernelGGL(k_rfb_axpy<T>, dim3(eb), dim3(RFB_THREADS), 0, stream, xb, (const T *)rb, total, act);
        };
        if (!trans) {
            if (ld >= n && nrhs > 0 && n > 0) diag_inv_ensure();
            refine_block_loop<T, false>(what, eps, b, x, ld, nrhs, on_device, berr, steps,
                                        rfb_resid_rows<T, false>(a_fact, safe1, safe2), step);
            return;
        }
        if (ld >= n && nrhs > 0 && n > 0 && !csc_ready) build_csc();
        refine_block_loop<T, false>(
            what, eps, b, x, ld, nrhs, on_device, berr, steps,
            [&](const T *xb, const T *bb, T *rb, unsigned rg, unsigned long long *out) {
                hipLaunchKernelGGL(k_rfb_resid_t<T>, dim3(rg), dim3(RFB_THREADS), 0, stream, d_csc_lo.p, d_csc_hi.p,
                                   d_csc_ci.p, a_fact, xb, bb, rb, n, safe1, safe2, out, conj);
            },
            step);
    }

    // the block loop with refine_d2's step: per column rmax = m 2^e, the fp32
    // block sweep of (float)(r 2^-e) in d_svb_x, x += 2^e dx in fp64
    void refine_block_d2(const double *b, double *x, int64_t ld, int nrhs, int on_device, double *berr,
                         int *steps) override {
        require_1x1_factors_block("refine_block_d2");
        if constexpr (std::is_same<T, float>::value) {
            SLU_REQUIRE(a_fact64 != nullptr,
                        "refine_block_d2 needs the fp64 values of A the factors came from "
                        "(slu_plan_fill_a_d2 before slu_plan_factor)");
            constexpr int NRB = SvbNr<float>::v;
            const double eps = 0.5 * 2.220446049250313e-16, safmin = 2.2250738585072014e-308;
            const double safe1 = (double)(n + 1) * safmin, safe2 = safe1 / eps;
            const i64 total = (i64)n * NRB;
            const unsigned eb = (unsigned)((total + RFB_THREADS - 1) / RFB_THREADS);
            if (ld >= n && nrhs > 0 && d_svb_x.n < (size_t)total) d_svb_x.alloc((size_t)total);
            if (ld >= n && nrhs > 0 && n > 0) diag_inv_ensure();
            refine_block_loop<double, true>(
                "refine_block_d2", eps, b, x, ld, nrhs, on_device, berr, steps,
                rfb_resid_rows<double, true>(a_fact64, safe1, safe2),
                [&](double *xb, double *rb, unsigned act, unsigned, const double *mx) {
                    RfbExp ex;
                    for (int q = 0; q < NRB; ++q) {
                        const double rmax = mx[NRB + q];
                        ex.e[q] = 0;
                        if (rmax > 0.0 && std::isfinite(rmax)) (void)frexp(rmax, &ex.e[q]);
                    }
                    hipLaunchKernelGGL(k_rfb_scale_cvt_d2, dim3(eb), dim3(RFB_THREADS), 0, stream,
                                       (const double *)rb, d_svb_x.p, total, ex, act);
                    sweep_block(d_svb_x.p);
                    hipLaunchKernelGGL(k_rfb_axpy_d2, dim3(eb), dim3(RFB_THREADS), 0, stream, xb,
                                       (const float *)d_svb_x.p, total, ex, act);
                });
        } else {
            throw Error(fmt("refine_block_d2: fp32 plans only, this plan's dtype is %s", dtype_name()));
        }
    }

    // Reciprocal condition estimate of the factored B, what sequential
    // SuperLU's dgscon returns: Hager / Higham's 1-norm estimator of B^-1 as
    // in LAPACK dlacn2 / zlacn2 (sign vector, first-maximum index, at most 5
    // iterations, the alternating-sign final vector), the host loop over one
    // device vector.  Each step is one sweep (B^-1, kase 1) or transposed
    // sweep (B^-H, kase 2) plus a one-workgroup kernel; RcOut is all that
    // crosses PCIe.  norm 'I' swaps the two (||B^-1||_inf = ||B^-H||_1).
    DevBuf<T> d_rc_x, d_rc_sgn;
    DevBuf<RcOut> d_rc_out;
    void rcond(int norm, double anorm, double *rc) override {
        const bool one = norm == '1' || norm == 'O' || norm == 'o';
        SLU_REQUIRE(one || norm == 'I' || norm == 'i', "rcond: norm is '1' or 'I', not %d", norm);
        SLU_REQUIRE(rc != nullptr, "rcond: no place for the result");
        require_1x1_factors("rcond");
        if (!sv_ready) build_solve();
        const bool real = sizeof(T) != sizeof(zc);
        const int adj = real ? SLU_TRANS : SLU_CONJ;
        const int op1 = one ? SLU_NOTRANS : adj, op2 = one ? adj : SLU_NOTRANS;
        const size_t nn = (size_t)std::max(n, 1);
        if (d_rc_x.n != nn) {
            d_rc_x.alloc(nn);
            d_rc_sgn.alloc(nn);
            d_rc_out.alloc(1);
        }
        const unsigned fb = (unsigned)((n + 255) / 256);
        int sweeps = 0;
        auto fill = [&](int mode, int j) {
            if (n) hipLaunchKernelGGL(k_rc_fill<T>, dim3(fb), dim3(256), 0, stream, d_rc_x.p, n, mode, j);
        };
        auto apply = [&](int op) {
            sweep_op(op, d_rc_x.p);
            ++sweeps;
        };
        auto fetch = [&]() {
            RcOut o;
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&o, d_rc_out.p, sizeof o, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            return o;
        };
        auto norm_sign = [&](int dosign) {
            hipLaunchKernelGGL(k_rc_norm_sign<T>, dim3(1), dim3(RC_THREADS), 0, stream, d_rc_x.p,
                               d_rc_sgn.p, n, dosign, d_rc_out.p);
            return fetch();
        };
        auto amax = [&](int jlast) {
            hipLaunchKernelGGL(k_rc_amax<T>, dim3(1), dim3(RC_THREADS), 0, stream, (const T *)d_rc_x.p, n,
                               jlast, d_rc_out.p);
            return fetch();
        };
        EventTimer tm;
        HIPCHK(hipStreamSynchronize(pstream));
        tm.start(stream);
        HIPCHK(hipMemsetAsync(d_rc_sgn.p, 0, nn * sizeof(T), stream));
        double est = 0.0;
        bool ok = n > 0;
        if (ok) {
            fill(0, 0);
            apply(op1);
            est = norm_sign(n > 1).sum;
            ok = std::isfinite(est);
        }
        if (ok && n > 1) {
            apply(op2);
            int j = amax(-1).j;
            for (int iter = 2; ok && j < n;) {
                fill(1, j);
                apply(op1);
                const double estold = est;
                const RcOut o = norm_sign(1);
                est = o.sum;
                ok = std::isfinite(est);
                // a repeated sign vector (real) or no growth: converged
                if (!ok || (real && o.ndiff == 0) || est <= estold) break;
                apply(op2);
                const RcOut m = amax(j);
                j = m.j;
                if (!(m.xlast != m.amax && iter < 5)) break;
                ++iter;
            }
            if (ok) { // the alternating-sign vector catches what the iteration cancels
                fill(2, 0);
                apply(op1);
                const double temp = 2.0 * (norm_sign(0).sum / (3.0 * n));
                ok = std::isfinite(temp);
                if (temp > est) est = temp;
            }
        }
        tm.stop(stream);
        HIPCHK(hipStreamSynchronize(stream));
        rc_sweeps = sweeps;
        rc_ms = tm.ms();
        *rc = (ok && anorm != 0.0 && std::isfinite(anorm) && est != 0.0) ? 1.0 / (anorm * est) : 0.0;
    }

    // ------------------------------------------------------- values of A
    // SamePattern_SameRowPerm refill (SRC/pddistribute.c:545-672) on the
    // device: the destination of every nonzero of A in this rank's L/U
    // storage is resolved once per pattern, with the reference's rules --
    // row block gb < column block jb goes to U(gb,jb) at the segment offset of
    // column j (:598-618), otherwise to L(:,jb) at the row's position in the
    // block column (:619-656); entries of other process rows / columns are
    // skipped (:587,596).
    DevBuf<i64> d_amap;
    DevBuf<T> d_aval;
    DevBuf<double> d_aval64; // fill_a_d2's host values (allocated at first use)
    i64 a_nnz = -1;

    bool has_block(int gb, int jb) const { // this rank holds L(gb,jb) (gb >= jb) or U(gb,jb)
        const vector<int> &ids = gb < jb ? ublk_jb : lblk_ib;
        const int f = gb < jb ? urow_first[gb / Pr] : lcol_first[jb / Pc];
        const int nb = gb < jb ? urow_nblk[gb / Pr] : lcol_nblk[jb / Pc];
        return std::binary_search(ids.begin() + f, ids.begin() + f + nb, gb < jb ? jb : gb);
    }

    void set_a_pattern(int64_t ncol, const int64_t *xa, const int64_t *asub) override {
        SLU_REQUIRE(ncol == n, "A has %lld columns, the LU structure %d", (long long)ncol, n);
        SLU_REQUIRE(xa[0] == 0 && xa[n] >= 0, "A: bad column pointers");
        const int_t *supno = LU->Glu_persist->supno;
        const i64 nnz = xa[n];
        const bool aprof = getenv("SLU_PROFILE_PLAN") != nullptr;
        auto ta = std::chrono::steady_clock::now();
        auto atick = [&](const char *what) { // SLU_PROFILE_PLAN: phase times on stderr
            if (!aprof) return;
            fprintf(stderr, "[slu plan %d] a_pattern %-16s %7.1f ms\n", iam, what, ms_since(ta));
            ta = std::chrono::steady_clock::now();
        };
        vector<i64> map((size_t)nnz, -1);
        // columns on the host threads: each nonzero belongs to one column, so
        // the writes to map are disjoint
        parallel_for(n, [&](int j) {
            thread_local vector<std::pair<i64, i64>> col; // (destination, nonzero) of one column
            const int jb = (int)supno[j];
            SLU_REQUIRE(xa[j + 1] >= xa[j], "A: column pointers decrease at %d", j);
            if (jb % Pc != mycol) return;
            const int jc = (int)(j - xsup[jb]);
            col.clear();
            for (i64 e = xa[j]; e < xa[j + 1]; ++e) {
                const i64 irow = asub[e];
                SLU_REQUIRE(irow >= 0 && irow < n, "A(%lld,%d): row out of range", (long long)irow, j);
                const int gb = (int)supno[irow];
                if (gb % Pr != myrow) continue;
                i64 m;
                if (!has_block(gb, jb))
                    throw Error(fmt("A(%lld,%d) is outside the %c structure (no block (%d,%d))",
                                    (long long)irow, j, gb < jb ? 'U' : 'L', gb, jb));
                if (gb < jb) {
                    const UBlk &B = ublk[find_ublk(gb, jb)];
                    const i64 c = B.coloff + jc;
                    SLU_REQUIRE(irow >= ucol_fst[c], "A(%lld,%d) is outside the U structure",
                                (long long)irow, j);
                    m = 2 * (ucol_voff[c] + irow - ucol_fst[c]) + 1;
                } else {
                    const LBlk &B = lblk[find_lblk(gb, jb)];
                    const int pos = lmap[B.mapoff + irow - xsup[gb]];
                    SLU_REQUIRE(pos >= 0, "A(%lld,%d) is outside the L structure", (long long)irow, j);
                    m = 2 * (B.colvoff + (i64)jc * B.ld + pos);
                }
                col.push_back({m, e});
            }
            // a duplicated (row, column): the later entry wins, as in the SPA
            std::sort(col.begin(), col.end());
            for (size_t i = 0; i < col.size(); ++i)
                if (i + 1 == col.size() || col[i + 1].first != col[i].first)
                    map[col[i].second] = col[i].first;
        }, 512);
        atick("map");
        d_amap.upload(map.empty() ? vector<i64>(1, -1) : map);
        d_aval.alloc(std::max<i64>(nnz, 1));
        atick("map upload");
        a_nnz = nnz;
        d_acur = a_fact = snap_acur = nullptr; // the previous pattern's values are gone
        d_acur64 = a_fact64 = snap_acur64 = nullptr;
        csc_ready = false;
        {   // rows of A for the refinement's residual (k_resid): all of A on a
            // 1x1 grid, this rank's entries (those of its blocks) on a 2D grid
            auto mine = [&](i64 e, int j) {
                return !xmode || ((int)supno[j] % Pc == mycol && (int)supno[asub[e]] % Pr == myrow);
            };
            // a counting sort by row on the host threads: the columns in NCH
            // chunks of about equal nnz, per (chunk, row) counts, then each
            // chunk fills its slice of every row (chunk order = column order,
            // so each row's entries come in column order, as serially)
            const int NCH = std::max(1, std::min(plan_threads(), (int)std::min<i64>(16, nnz / 65536 + 1)));
            SLU_REQUIRE(nnz < INT32_MAX, "A: %lld nonzeros", (long long)nnz);
            vector<int> cb(NCH + 1, 0);
            for (int c = 1; c < NCH; ++c)
                cb[c] = std::max(cb[c - 1], (int)(std::lower_bound(xa, xa + n + 1, nnz * c / NCH) - xa));
            cb[NCH] = n;
            vector<int32_t> cc((size_t)NCH * n, 0); // [chunk][row] counts, then fill cursors
            parallel_for(NCH, [&](int c) {
                int32_t *cnt = cc.data() + (size_t)c * n;
                for (int j = cb[c]; j < cb[c + 1]; ++j)
                    for (i64 e = xa[j]; e < xa[j + 1]; ++e)
                        if (mine(e, j)) ++cnt[asub[e]];
            }, 1);
            vector<i64> rp(n + 1, 0);
            const int NB = (n + 65535) / 65536;
            parallel_for(NB, [&](int t) {
                for (int i = t * 65536; i < std::min(n, (t + 1) * 65536); ++i) {
                    i64 tot = 0;
                    for (int c = 0; c < NCH; ++c) tot += cc[(size_t)c * n + i];
                    rp[i + 1] = tot;
                }
            }, 1);
            for (int i = 0; i < n; ++i) rp[i + 1] += rp[i];
            parallel_for(NB, [&](int t) {
                for (int i = t * 65536; i < std::min(n, (t + 1) * 65536); ++i) {
                    i64 pos = rp[i];
                    for (int c = 0; c < NCH; ++c) {
                        const int32_t k = cc[(size_t)c * n + i];
                        cc[(size_t)c * n + i] = (int32_t)pos;
                        pos += k;
                    }
                }
            }, 1);
            vector<i64> re((size_t)rp[n]);
            vector<int> rc((size_t)rp[n]);
            parallel_for(NCH, [&](int c) {
                int32_t *nx = cc.data() + (size_t)c * n;
                for (int j = cb[c]; j < cb[c + 1]; ++j)
                    for (i64 e = xa[j]; e < xa[j + 1]; ++e) {
                        if (!mine(e, j)) continue;
                        const i64 q = nx[asub[e]]++;
                        rc[q] = j;
                        re[q] = e;
                    }
            }, 1);
            atick("rows");
            d_rp.upload(rp);
            d_rc.upload(rc.empty() ? vector<int>(1, 0) : rc);
            d_re.upload(re.empty() ? vector<i64>(1, 0) : re);
            atick("rows upload");
            HIPCHK(hipDeviceSynchronize());
            atick("device sync");
        }
    }

    void fill_a(const void *a, int on_device) override {
        SLU_REQUIRE(a_nnz >= 0, "fill_a before set_a_pattern");
        const T *src = (const T *)a;
        if (!on_device) {
            if (a_nnz)
                HIPCHK(hipMemcpyAsync(d_aval.p, a, (size_t)a_nnz * sizeof(T), hipMemcpyHostToDevice, stream));
            src = d_aval.p;
        }
        d_acur = src;
        d_acur64 = nullptr;
        fill_storage([&](unsigned blocks) {
            hipLaunchKernelGGL(k_fill_a<T>, dim3(blocks), dim3(FILL_THREADS), 0, stream,
                               d_amap.p, src, a_nnz, d_L.p, d_U.p);
        });
    }

    // zero this rank's L and U, scatter A's values with `launch`; t_fill_ms
    template <typename F> void fill_storage(F &&launch) {
        vstate = 1;
        dinv_valid = false;
        host_current = false;
        EventTimer tm;
        HIPCHK(hipStreamSynchronize(pstream));
        tm.start(stream);
        if (d_L.n) HIPCHK(hipMemsetAsync(d_L.p, 0, d_L.bytes(), stream));
        if (d_U.n) HIPCHK(hipMemsetAsync(d_U.p, 0, d_U.bytes(), stream));
        if (a_nnz) {
            launch((unsigned)std::min<i64>((a_nnz + FILL_THREADS - 1) / FILL_THREADS, 65536));
            HIPCHK(hipGetLastError());
        }
        tm.stop(stream);
        HIPCHK(hipStreamSynchronize(stream));
        stats.t_fill_ms = tm.ms();
    }

    static const char *dtype_name() {
        return std::is_same<T, float>::value ? "s (fp32)" : std::is_same<T, double>::value ? "d (fp64)" : "z (complex fp64)";
    }

    // fill_a of an fp32 plan from fp64 values: L / U get the rounded values
    // in the one pass that reads the doubles, which stay on the device as the
    // A of refine_d2's residual (no fp32 copy of A exists afterwards, so the
    // plain refine refuses such factors).
    void fill_a_d2(const double *a, int on_device) override {
        if constexpr (std::is_same<T, float>::value) {
            SLU_REQUIRE(a_nnz >= 0, "fill_a_d2 before set_a_pattern");
            const double *src = a;
            if (!on_device) {
                if (d_aval64.n != (size_t)std::max<i64>(a_nnz, 1)) d_aval64.alloc(std::max<i64>(a_nnz, 1));
                if (a_nnz)
                    HIPCHK(hipMemcpyAsync(d_aval64.p, a, (size_t)a_nnz * sizeof(double), hipMemcpyHostToDevice, stream));
                src = d_aval64.p;
            }
            d_acur = nullptr;
            d_acur64 = src;
            fill_storage([&](unsigned blocks) {
                hipLaunchKernelGGL(k_fill_a_d2, dim3(blocks), dim3(FILL_THREADS), 0, stream,
                                   d_amap.p, src, a_nnz, d_L.p, d_U.p);
            });
        } else {
            throw Error(fmt("fill_a_d2: fp32 plans only, this plan's dtype is %s", dtype_name()));
        }
    }

    // ---- helper threads of the plan build: the H2D copy of the values and
    // the pinned-slot allocation.  Declared last: they use the DevBuf members
    // above, and members are destroyed in reverse order, so the threads are
    // joined before any buffer is freed (also when the constructor throws).
    HelperThread up_thread, pin_thread;
};

template <typename P> PlanBase *make_plan(void *LU, int n, int pr, int pc, int iam, slu_comm *c,
                                          const slu_engine_opts *o) {
    return new P((decltype(std::declval<P>().LU))LU, n, pr, pc, iam, c, o);
}

} // namespace slu

#include "plan_amalg.h" // the amalgamated plans over Plan, make_plan_any

struct slu_plan {
    int dtype = 0;
    std::unique_ptr<slu::PlanBase> impl;
};

using namespace slu;

// Fills the whole LDS of every CU with NaN (test hook: a kernel that reads
// LDS it did not write, even to multiply it by zero, then fails every time
// instead of depending on what the previous kernel left there).
__global__ void __launch_bounds__(1024) k_poison_lds(double v, int bytes) {
    extern __shared__ double s_poison[];
    const int n = bytes / (int)sizeof(double);
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_poison[i] = v;
    __syncthreads();
    if (s_poison[(threadIdx.x * 7) % n] != s_poison[(threadIdx.x * 7) % n] && threadIdx.x == 1u << 30)
        s_poison[0] = 0; // never true; keeps the stores
}

// No exception leaves the C ABI: runs fn and returns 0 (or fn's pointer); on
// an exception stores its text for slu_last_error() and returns -1 (nullptr).
template <typename F> static auto guarded(F &&fn) {
    using R = decltype(fn());
    try {
        if constexpr (std::is_void<R>::value) {
            fn();
            return 0;
        } else {
            return fn();
        }
    } catch (const std::exception &e) {
        set_last_error(e.what());
        if constexpr (std::is_void<R>::value) return -1;
        else return R(nullptr);
    }
}

static slu_comm *new_comm(int nprow, int npcol, int iam, int device) {
    auto *c = new slu_comm;
    c->nprow = nprow;
    c->npcol = npcol;
    c->iam = iam;
    c->myrow = iam / npcol;
    c->mycol = iam % npcol;
    c->device = device;
    return c;
}

extern "C" {

int slu_debug_poison_lds(int device) {
    return guarded([&] {
        HIPCHK(hipSetDevice(device));
        // the whole 160 KB per workgroup where the runtime allows it, else 64 KB
        int bytes = 160 * 1024;
        if (hipFuncSetAttribute((const void *)k_poison_lds,
                                hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
            (void)hipGetLastError();
            bytes = 64 * 1024;
        }
        hipLaunchKernelGGL(k_poison_lds, dim3(4096), dim3(1024), bytes, 0, __builtin_nan(""), bytes);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    });
}

const char *slu_last_error(void) { return g_last_error.c_str(); }

int slu_comm_unique_id(void *uid) {
    return guarded([&] {
        ncclUniqueId id;
        NCCLCHK(ncclGetUniqueId(&id));
        memcpy(uid, &id, sizeof id);
    });
}

slu_comm *slu_comm_create(const void *uid, int nprow, int npcol, int iam, int device) {
    return guarded([&]() -> slu_comm * {
        slu_comm *c = new_comm(nprow, npcol, iam, device);
        HIPCHK(hipSetDevice(device));
        if (nprow * npcol > 1) {
            SLU_REQUIRE(uid != nullptr, "uid required for a %dx%d grid", nprow, npcol);
            ncclUniqueId id;
            memcpy(&id, uid, sizeof id);
            NCCLCHK(ncclCommInitRank(&c->world, nprow * npcol, id, iam));
            NCCLCHK(ncclCommSplit(c->world, c->myrow, c->mycol, &c->row, nullptr));
            NCCLCHK(ncclCommSplit(c->world, c->mycol, c->myrow, &c->col, nullptr));
        }
        return c;
    });
}

slu_comm *slu_comm_create3d(const void *uid, int nprow, int npcol, int npdep, int iam3d, int device) {
    return guarded([&]() -> slu_comm * {
        const int P = nprow * npcol;
        SLU_REQUIRE(nprow > 0 && npcol > 0 && npdep > 0 && (npdep & (npdep - 1)) == 0,
                    "3D grid %dx%dx%d: Pz must be a power of two", nprow, npcol, npdep);
        SLU_REQUIRE(iam3d >= 0 && iam3d < P * npdep, "rank %d outside a %dx%dx%d grid", iam3d, nprow,
                    npcol, npdep);
        slu_comm *c = new_comm(nprow, npcol, iam3d % P, device);
        c->npdep = npdep;
        c->zlayer = iam3d / P;
        HIPCHK(hipSetDevice(device));
        if (P * npdep > 1) {
            SLU_REQUIRE(uid != nullptr, "uid required for a %dx%dx%d grid", nprow, npcol, npdep);
            ncclUniqueId id;
            memcpy(&id, uid, sizeof id);
            NCCLCHK(ncclCommInitRank(&c->all, P * npdep, id, iam3d));
            NCCLCHK(ncclCommSplit(c->all, c->zlayer, c->iam, &c->world, nullptr));
            NCCLCHK(ncclCommSplit(c->all, c->iam, c->zlayer, &c->zcomm, nullptr));
            NCCLCHK(ncclCommSplit(c->world, c->myrow, c->mycol, &c->row, nullptr));
            NCCLCHK(ncclCommSplit(c->world, c->mycol, c->myrow, &c->col, nullptr));
        }
        return c;
    });
}

slu_comm *slu_comm_create_host_p2p3d(slu_host_p2p_fn fn, void *ctx, int nprow, int npcol, int npdep,
                                     int iam3d, int device) {
    return guarded([&]() -> slu_comm * {
        SLU_REQUIRE(npdep > 0 && (npdep & (npdep - 1)) == 0, "Pz = %d is not a power of two", npdep);
        slu_comm *c = slu_comm_create_host_p2p(fn, ctx, nprow, npcol, iam3d % (nprow * npcol), device);
        if (!c) return nullptr;
        c->npdep = npdep;
        c->zlayer = iam3d / (nprow * npcol);
        return c;
    });
}

slu_comm *slu_comm_create_host(slu_host_bcast_fn fn, void *ctx, int nprow, int npcol, int iam,
                               int device) {
    return guarded([&]() -> slu_comm * {
        SLU_REQUIRE(fn != nullptr, "host transport needs a broadcast callback");
        slu_comm *c = new_comm(nprow, npcol, iam, device);
        c->host_fn = fn;
        c->host_ctx = ctx;
        HIPCHK(hipSetDevice(device));
        return c;
    });
}

slu_comm *slu_comm_create_host_p2p(slu_host_p2p_fn fn, void *ctx, int nprow, int npcol, int iam,
                                   int device) {
    return guarded([&]() -> slu_comm * {
        SLU_REQUIRE(fn != nullptr, "point-to-point host transport needs a callback");
        slu_comm *c = new_comm(nprow, npcol, iam, device);
        c->host_p2p = fn;
        c->host_ctx = ctx;
        if (device >= 0) HIPCHK(hipSetDevice(device)); // -1: schedule-only plans, no GPU
        return c;
    });
}

int slu_comm_size(const slu_comm *c, int group) {
    if (!c) return -1;
    if (c->world || c->zcomm) { // what RCCL itself reports for the communicator
        int n = -1;
        ncclComm_t cm = group == 0 ? c->world : group == 1 ? c->row : group == 2 ? c->col : c->zcomm;
        if (!cm) return 1;
        if (ncclCommCount(cm, &n) != ncclSuccess) return -1;
        return n;
    }
    return group == 0 ? c->nprow * c->npcol : group == 1 ? c->npcol : group == 2 ? c->nprow : c->npdep;
}

void slu_comm_destroy(slu_comm *c) {
    if (!c) return;
    c->wd.reset(); // (its thread polls the communicators)
    if (c->row) ncclCommDestroy(c->row);
    if (c->col) ncclCommDestroy(c->col);
    if (c->world) ncclCommDestroy(c->world);
    if (c->zcomm) ncclCommDestroy(c->zcomm);
    if (c->all) ncclCommDestroy(c->all);
    delete c;
}

slu_plan *slu_plan_create(int dtype, void *LU, int n, int nprow, int npcol, int iam,
                          slu_comm *comm, const slu_engine_opts *opts, char *err, int errlen) {
    try {
        auto *p = new slu_plan;
        p->dtype = dtype;
        switch (dtype) {
        case SLU_D:
            p->impl.reset(make_plan_any<Plan<double, double, dLocalLU_t, dLUstruct_t>>(LU, n, nprow, npcol, iam, comm, opts));
            break;
        case SLU_S:
            p->impl.reset(make_plan_any<Plan<float, float, sLocalLU_t, sLUstruct_t>>(LU, n, nprow, npcol, iam, comm, opts));
            break;
        case SLU_Z:
            p->impl.reset(make_plan_any<Plan<zc, doublecomplex, zLocalLU_t, zLUstruct_t>>(LU, n, nprow, npcol, iam, comm, opts));
            break;
        default:
            throw Error(fmt("bad dtype %d", dtype));
        }
        return p;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        if (err && errlen > 0) snprintf(err, errlen, "%s", e.what());
        return nullptr;
    }
}

int slu_plan_gather3d(slu_plan *p) {
    return guarded([&] {
        p->impl->gather_layers();
    });
}

int slu_plan_adopt_factors(slu_plan *p) {
    return guarded([&] {
        p->impl->adopt_factors();
    });
}

int slu_plan_upload(slu_plan *p) {
    return guarded([&] {
        p->impl->upload();
    });
}

int slu_plan_factor(slu_plan *p, double anorm, int *info, int *tiny) {
    return guarded([&] {
        int i = 0, t = 0;
        p->impl->factor(anorm, &i, &t);
        if (info) *info = i;
        if (tiny) *tiny = t;
    });
}

int slu_plan_solve(slu_plan *p, void *b, int64_t ldb, int nrhs) {
    return guarded([&] {
        p->impl->solve(b, ldb, nrhs);
    });
}

int slu_plan_solve_block(slu_plan *p, void *b, int64_t ldb, int nrhs, int on_device) {
    return guarded([&] {
        p->impl->solve_block(b, ldb, nrhs, on_device);
    });
}

int slu_plan_solve_block_info(const slu_plan *p, int *passes, int64_t *launches, double *ms) {
    if (passes) *passes = p->impl->svb_passes;
    if (launches) *launches = p->impl->svb_launches;
    if (ms) *ms = p->impl->svb_ms;
    return 0;
}

int slu_plan_set_diag_inv(slu_plan *p, int on) {
    return guarded([&] {
        p->impl->set_diag_inv(on);
    });
}

int slu_plan_diag_inv_info(const slu_plan *p, int *on, int *valid, int64_t *bytes, int *computes, double *ms) {
    return guarded([&] {
        p->impl->diag_inv_info(on, valid, bytes, computes, ms);
    });
}

int slu_plan_diag_inv_block(slu_plan *p, int k, int *fst, int *w, void *out, int64_t ldo) {
    return guarded([&] {
        p->impl->diag_inv_block(k, fst, w, out, ldo);
    });
}

int slu_plan_set_a_pattern(slu_plan *p, int64_t ncol, const int64_t *xa, const int64_t *asub) {
    return guarded([&] {
        p->impl->set_a_pattern(ncol, xa, asub);
    });
}

int slu_plan_fill_a(slu_plan *p, const void *a, int on_device) {
    return guarded([&] {
        p->impl->fill_a(a, on_device);
    });
}

int slu_plan_refine(slu_plan *p, const void *b, void *x, int64_t ld, int nrhs, double *berr,
                    int *steps) {
    return guarded([&] {
        p->impl->refine(b, x, ld, nrhs, berr, steps);
    });
}

int slu_plan_solve_t(slu_plan *p, int trans, void *b, int64_t ldb, int nrhs) {
    return guarded([&] {
        p->impl->solve_t(trans, b, ldb, nrhs);
    });
}

int slu_plan_refine_t(slu_plan *p, int trans, const void *b, void *x, int64_t ld, int nrhs,
                      double *berr, int *steps) {
    return guarded([&] {
        p->impl->refine_t(trans, b, x, ld, nrhs, berr, steps);
    });
}

int slu_plan_rcond(slu_plan *p, int norm, double anorm, double *rcond) {
    return guarded([&] {
        p->impl->rcond(norm, anorm, rcond);
    });
}

int slu_plan_rcond_info(const slu_plan *p, int *sweeps, double *ms) {
    if (sweeps) *sweeps = p->impl->rc_sweeps;
    if (ms) *ms = p->impl->rc_ms;
    return 0;
}

int slu_plan_fill_a_d2(slu_plan *p, const double *a, int on_device) {
    return guarded([&] {
        p->impl->fill_a_d2(a, on_device);
    });
}

int slu_plan_refine_d2(slu_plan *p, const double *b, double *x, int64_t ld, int nrhs, double *berr,
                       int *steps) {
    return guarded([&] {
        p->impl->refine_d2(b, x, ld, nrhs, berr, steps);
    });
}

int slu_plan_refine_block(slu_plan *p, const void *b, void *x, int64_t ld, int nrhs, int on_device,
                          double *berr, int *steps) {
    return guarded([&] {
        p->impl->refine_block(b, x, ld, nrhs, on_device, berr, steps);
    });
}

int slu_plan_refine_block_d2(slu_plan *p, const double *b, double *x, int64_t ld, int nrhs, int on_device,
                             double *berr, int *steps) {
    return guarded([&] {
        p->impl->refine_block_d2(b, x, ld, nrhs, on_device, berr, steps);
    });
}

int slu_plan_solve_block_t(slu_plan *p, int trans, void *b, int64_t ldb, int nrhs, int on_device) {
    return guarded([&] {
        p->impl->solve_block_t(trans, b, ldb, nrhs, on_device);
    });
}

int slu_plan_refine_block_t(slu_plan *p, int trans, const void *b, void *x, int64_t ld, int nrhs,
                            int on_device, double *berr, int *steps) {
    return guarded([&] {
        p->impl->refine_block_t(trans, b, x, ld, nrhs, on_device, berr, steps);
    });
}

int slu_plan_refine_block_info(const slu_plan *p, int *passes, int *sweeps, int *resids, double *ms) {
    if (passes) *passes = p->impl->rfb_passes;
    if (sweeps) *sweeps = p->impl->rfb_sweeps;
    if (resids) *resids = p->impl->rfb_resids;
    if (ms) *ms = p->impl->rfb_ms;
    return 0;
}

int slu_plan_download(slu_plan *p) {
    return guarded([&] {
        p->impl->download();
    });
}

int slu_plan_snapshot(slu_plan *p) {
    return guarded([&] {
        p->impl->snapshot();
    });
}

int slu_plan_restore(slu_plan *p) {
    return guarded([&] {
        p->impl->restore();
    });
}

int slu_plan_check_exchange(slu_plan *p, int64_t *nsections, int64_t *nbytes) {
    return guarded([&] {
        p->impl->check_exchange(nsections, nbytes);
    });
}

int slu_plan_set_timing(slu_plan *p, int timing, int serial) {
    return guarded([&] {
        p->impl->set_timing(timing, serial);
    });
}

int slu_plan_sync(slu_plan *p) {
    return guarded([&] {
        p->impl->sync();
    });
}

void slu_plan_destroy(slu_plan *p) { delete p; }

int slu_plan_get_stats(const slu_plan *p, slu_plan_stats *st) {
    *st = p->impl->stats;
    return 0;
}

int slu_plan_path_counts(const slu_plan *p, int64_t *out, int n) {
    for (int i = 0; i < n && i < PlanBase::PC_N; ++i) out[i] = p->impl->path_counts[i];
    return PlanBase::PC_N;
}

} // extern "C"
