// The amalgamated plans (csrc/amalg.h) and the choice of a plan for a
// caller's LUstruct.  Part of engine.hip's translation unit: included there
// after Plan, which these wrap.
#pragma once

namespace slu {

// ---------------------------------------------------------------- amalgamation
// What the two amalgamated plans share.  The inner plan is an ordinary Plan
// built on a coarse LUstruct's index arrays (held here, no host values); the
// device-resident state between upload and download -- what factor(),
// snapshot / restore, fill_a, solve and refine work on -- is the coarse
// layout.  A subclass builds the coarse index arrays and moves the caller's
// values between their own layout on the device (d_oL / d_oU) and the coarse
// one: expand at upload, compress at download.
template <typename T, typename HT, typename LocalLU, typename LUS>
struct CoarsePlan : PlanBase {
    using Inner = Plan<T, HT, LocalLU, LUS>;
    LUS *LU = nullptr;
    int n = 0, ns = 0;
    slu_engine_opts opts{};
    // the coarse LUstruct the inner plan reads (index arrays only)
    LUS mlu{};
    LocalLU mllu{};
    Glu_persist_t mglu{};
    vector<int_t *> mlidx, muidx;
    std::unique_ptr<Inner> in;
    bool coarse_current = false; // d_oL / d_oU stale: the coarse storage holds newer values
    double t_expand = 0, t_compress = 0, t_d2h = 0;

    // the inner plan over mlidx / muidx (filled by the subclass) and the
    // coarse partition xsup2 / supno2
    void make_inner(int_t *xsup2, int_t *supno2, int pr, int pc, int iam, slu_comm *c, DevBuf<T> *pre = nullptr) {
        mglu.xsup = xsup2;
        mglu.supno = supno2;
        mllu.Lrowind_bc_ptr = mlidx.data();
        mllu.Ufstnz_br_ptr = muidx.data();
        mlu.Glu_persist = &mglu;
        mlu.Llu = &mllu;
        slu_engine_opts io = opts;
        io.overlap_upload = io.overlap_download = 0;
        in.reset(new Inner(&mlu, n, pr, pc, iam, c, &io, pre));
    }

    virtual void sync_stats() = 0;
    virtual vector<Xfer> xfers() = 0; // caller layout: host arrays <-> d_oL / d_oU
    virtual void compress() = 0;      // coarse -> d_oL / d_oU
    // the caller's arrays already hold what the device holds
    virtual bool host_done_now() const { return false; }
    // the coarse storage got values the caller-layout copies do not have
    virtual void coarse_changed() { coarse_current = true; }

    // the inner plan's stats, with the caller's partition's algorithmic
    // work F (what the reference's pdgstrf does on this LUstruct); the coarse
    // partition's own counts (explicit zeros included) stay in the
    // kernel-level fields (schur_big_flops, schur_flops_padded)
    void caller_flops(const AmalgFlops &F) {
        stats = in->stats;
        std::copy(in->path_counts, in->path_counts + PlanBase::PC_N, this->path_counts);
        stats.schur_flops = F.schur_flops(sizeof(T) == 16);
        stats.panel_flops = F.panel_flops(sizeof(T) == 16);
        stats.nsupers_in = ns;
    }

    void download() override {
        in->sync();
        if (host_done_now()) return;
        if (coarse_current) {
            compress();
            coarse_current = false;
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (const Xfer &x : xfers()) HIPCHK(hipMemcpy(x.host, x.dev, x.bytes, hipMemcpyDeviceToHost));
        t_d2h = ms_since(t0);
        sync_stats();
    }
    void snapshot() override { in->snapshot(); }
    void restore() override {
        in->restore();
        coarse_changed();
    }
    void sync() override { in->sync(); }
    void set_timing(int timing, int serial) override { in->set_timing(timing, serial); }
    void solve(void *b, int64_t ldb, int nrhs) override {
        in->solve(b, ldb, nrhs);
        sync_stats();
    }
    void sync_svb() {
        svb_passes = in->svb_passes;
        svb_launches = in->svb_launches;
        svb_ms = in->svb_ms;
        sync_stats();
    }
    void solve_block(void *b, int64_t ldb, int nrhs, int on_device) override {
        in->solve_block(b, ldb, nrhs, on_device);
        sync_svb();
    }
    void solve_block_t(int trans, void *b, int64_t ldb, int nrhs, int on_device) override {
        in->solve_block_t(trans, b, ldb, nrhs, on_device);
        sync_svb();
    }
    void set_diag_inv(int on) override { in->set_diag_inv(on); }
    void diag_inv_info(int *on, int *valid, int64_t *bytes, int *computes, double *ms) override {
        in->diag_inv_info(on, valid, bytes, computes, ms);
    }
    void diag_inv_block(int k, int *fst, int *w, void *out, int64_t ldo) override {
        in->diag_inv_block(k, fst, w, out, ldo);
    }
    void set_a_pattern(int64_t ncol, const int64_t *xa, const int64_t *asub) override {
        in->set_a_pattern(ncol, xa, asub);
        sync_stats();
    }
    void fill_a(const void *a, int on_device) override {
        in->fill_a(a, on_device);
        coarse_changed();
        sync_stats();
    }
    void refine(const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        in->refine(b, x, ld, nrhs, berr, steps);
        sync_stats();
    }
    void solve_t(int trans, void *b, int64_t ldb, int nrhs) override {
        in->solve_t(trans, b, ldb, nrhs);
        sync_stats();
    }
    void refine_t(int trans, const void *b, void *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        in->refine_t(trans, b, x, ld, nrhs, berr, steps);
        sync_stats();
    }
    void rcond(int norm, double anorm, double *rc) override {
        in->rcond(norm, anorm, rc);
        rc_sweeps = in->rc_sweeps;
        rc_ms = in->rc_ms;
    }
    void fill_a_d2(const double *a, int on_device) override {
        in->fill_a_d2(a, on_device);
        coarse_changed();
        sync_stats();
    }
    void refine_d2(const double *b, double *x, int64_t ld, int nrhs, double *berr, int *steps) override {
        in->refine_d2(b, x, ld, nrhs, berr, steps);
        sync_stats();
    }
    void sync_rfb() {
        rfb_passes = in->rfb_passes;
        rfb_sweeps = in->rfb_sweeps;
        rfb_resids = in->rfb_resids;
        rfb_ms = in->rfb_ms;
        sync_stats();
    }
    void refine_block(const void *b, void *x, int64_t ld, int nrhs, int on_device, double *berr,
                      int *steps) override {
        in->refine_block(b, x, ld, nrhs, on_device, berr, steps);
        sync_rfb();
    }
    void refine_block_t(int trans, const void *b, void *x, int64_t ld, int nrhs, int on_device, double *berr,
                        int *steps) override {
        in->refine_block_t(trans, b, x, ld, nrhs, on_device, berr, steps);
        sync_rfb();
    }
    void refine_block_d2(const double *b, double *x, int64_t ld, int nrhs, int on_device, double *berr,
                         int *steps) override {
        in->refine_block_d2(b, x, ld, nrhs, on_device, berr, steps);
        sync_rfb();
    }
    void check_exchange(int64_t *nsec, int64_t *nbytes) override {
        in->check_exchange(nsec, nbytes);
        sync_stats();
    }
};

// A 1x1 plan over the coarse partition of csrc/amalg.h: the caller's values
// are relaid on the device by the programs of the analysis.
template <typename T, typename HT, typename LocalLU, typename LUS>
struct AmalgPlan : CoarsePlan<T, HT, LocalLU, LUS> {
    using Base = CoarsePlan<T, HT, LocalLU, LUS>;
    using typename Base::Inner;
    using Base::LU; using Base::n; using Base::ns; using Base::opts; using Base::in; using Base::stats;
    using Base::mlidx; using Base::muidx; using Base::coarse_current;
    using Base::t_expand; using Base::t_compress; using Base::t_d2h;
    Amalg A;
    // caller layout on the device, and the relayout programs
    DevBuf<T> d_oL, d_oU;
    DevBuf<LColX> d_lx;
    DevBuf<int32_t> d_lrow, d_ucd;
    DevBuf<uint16_t> d_ucl;
    DevBuf<UChunk> d_ur;
    DevBuf<i64> d_D;
    vector<i64> usrc; // caller U value offset per block row
    // the coarse L / U storage, allocated beside the analysis as soon as its
    // sizes are known (after pass 3a: alloc_thread), adopted by the inner plan
    DevBuf<T> pre[2];
    std::mutex o_mu; // ensure_o: the upload thread or the D2H program build
    // fresh HBM is mapped at its first touch; the caller-layout buffers are
    // touched first thing on the upload thread (o_mapped), and the D2H warm-up
    // (pinned slots) waits for that
    std::mutex map_mu;
    std::condition_variable map_cv;
    bool o_mapped = false;
    double t_omap = 0;
    std::chrono::steady_clock::time_point t_born = std::chrono::steady_clock::now();
    void set_mapped() {
        std::lock_guard<std::mutex> lk(map_mu);
        o_mapped = true;
        map_cv.notify_all();
    }
    // the D2H's pinned slots and HBM staging slots, allocated and touched
    // (one DMA through each) beside the plan build (warm_thread): lazily, the
    // first factorization paid ~70 ms more D2H tail for them
    DevBuf<char> warm_stage;
    double up_ms = 0, h2d_bytes = 0;
    double t_amalg = 0, t_plan = 0;

    // Returns nullptr when nothing merges (the caller then builds a Plan).
    static AmalgPlan *make(LUS *lu, int n_, const slu_engine_opts *o, double zero_frac, int maxw) {
        auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<AmalgPlan> P(new AmalgPlan);
        P->LU = lu;
        P->n = n_;
        if (o) P->opts = *o;
        const int_t *xsup = lu->Glu_persist->xsup;
        P->ns = (int)(lu->Glu_persist->supno[n_ - 1] + 1);
        LocalLU *L = lu->Llu;
        const int ns = P->ns;
        // caller value layout: contiguous per block column / row in supernode order
        i64 lv = 0, uv = 0;
        P->usrc.assign(ns + 1, 0);
        for (int s = 0; s < ns; ++s) {
            if (L->Lrowind_bc_ptr[s]) lv += (i64)L->Lrowind_bc_ptr[s][1] * (xsup[s + 1] - xsup[s]);
            if (L->Ufstnz_br_ptr[s]) uv += L->Ufstnz_br_ptr[s][1];
            P->usrc[s + 1] = uv;
        }
        const bool prof = getenv("SLU_PROFILE_PLAN") != nullptr;
        auto tk = t0;
        auto tick = [&](const char *what) { // SLU_PROFILE_PLAN: phase times on stderr
            if (!prof) return;
            fprintf(stderr, "[slu amalg plan] %-22s %7.1f ms\n", what, ms_since(tk));
            tk = std::chrono::steady_clock::now();
        };
        HIPCHK(hipSetDevice(0));
        tick("caller layout");
        P->o_lv = lv;
        P->o_uv = uv;
        // the caller-layout copies only where values cross PCIe: a plan fed
        // by fill_a and read by solve never allocates them (the upload thread
        // allocates them itself, beside the analysis)
        if (!P->opts.overlap_upload && P->opts.overlap_download) P->ensure_o();
        tick("caller-layout alloc");
        P->A.on_sizes = [raw = P.get()](int64_t lv2, int64_t uv2) {
            raw->alloc_thread.start(0, [raw, lv2, uv2] {
                const auto ta = std::chrono::steady_clock::now();
                const double at = ms_since(raw->t_born);
                raw->pre[0].alloc_guarded(std::max<i64>(lv2, 1), SB_UGUARD);
                raw->pre[1].alloc_guarded(std::max<i64>(uv2, 1), SB_UGUARD);
                if (getenv("SLU_PROFILE_PLAN"))
                    fprintf(stderr, "[slu amalg plan]   (coarse storage %.1f GB mapped in %.1f ms, from %.1f ms)\n",
                            (lv2 + uv2) * sizeof(T) / 1e9, ms_since(ta), at);
            });
        };
        if (P->opts.overlap_upload) {
            AmalgPlan *raw = P.get();
            P->up_thread.start(0, [raw] {
                struct Mapped { // (also on failure: the warm-up waits for it)
                    AmalgPlan *p;
                    ~Mapped() { p->set_mapped(); }
                } mapped{raw};
                raw->h2d();
            });
        }
        if (P->opts.overlap_download) {
            AmalgPlan *raw = P.get();
            raw->warm_thread.start(0, [raw] {
                // after the caller-layout buffers' mapping: beside it the
                // pinned allocation made that mapping 102-274 instead of
                // 34-37 ms (profiles/r04y)
                if (raw->opts.overlap_upload) {
                    std::unique_lock<std::mutex> lk(raw->map_mu);
                    raw->map_cv.wait(lk, [raw] { return raw->o_mapped; });
                }
                const i64 slot = d2h_slot_bytes();
                constexpr int NS = Inner::D2H_NS;
                std::lock_guard<std::mutex> in_use(pinned_pool(1).use);
                std::vector<char *> slots = pinned_pool(1).get(NS, slot);
                raw->warm_stage.alloc((size_t)NS * slot);
                hipStream_t st = nullptr;
                HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
                HIPCHK(hipMemsetAsync(raw->warm_stage.p, 0, raw->warm_stage.bytes(), st));
                for (int i = 0; i < NS; ++i)
                    HIPCHK(hipMemcpyAsync(slots[i], raw->warm_stage.p + (i64)i * slot, (size_t)slot,
                                          hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipStreamDestroy(st));
            });
        }
        // (leaving early, by return or exception: P's helper threads are
        // joined by their destructors)
        vector<const int_t *> li(L->Lrowind_bc_ptr, L->Lrowind_bc_ptr + ns),
            ui(L->Ufstnz_br_ptr, L->Ufstnz_br_ptr + ns);
        const auto ta = std::chrono::steady_clock::now();
        P->A.defer_programs = true;
        if (!P->A.build(n_, ns, xsup, li.data(), ui.data(), zero_frac, maxw)) return nullptr;
        SLU_REQUIRE(P->A.lval1 == lv && P->A.uval1 == uv, "amalgamation: value counts");
        P->t_amalg = ms_since(ta);
        tick("analysis");
        // the relayout programs (host pass 4; beside the coarse plan's
        // build it only slowed both down on the box's 16 cores).  Only an
        // upload or a download of the caller-layout values runs them: a
        // plan fed by fill_a whose factors stay in HBM (the device-
        // resident drop-in) builds them when one first happens
        const bool progs_now = P->opts.overlap_upload || P->opts.overlap_download;
        if (progs_now) {
            P->A.build_programs();
            tick("programs (host)");
        }
        P->build_inner();
        tick("coarse plan");
        if (progs_now) {
            P->build_programs();
            P->progs = true;
            tick("relayout programs");
        }
        if (P->opts.overlap_download) P->build_d2h();
        tick("d2h programs");
        P->t_plan = ms_since(t0);
        P->sync_stats();
        return P.release();
    }

    void build_inner() {
        const int ns2 = A.ns2;
        mlidx.assign(ns2, nullptr);
        muidx.assign(ns2, nullptr);
        for (int J = 0; J < ns2; ++J) {
            if (A.Loff2[J] >= 0) mlidx[J] = A.Lidx2.data() + A.Loff2[J];
            if (A.Uoff2[J] >= 0) muidx[J] = A.Uidx2.data() + A.Uoff2[J];
        }
        const auto tj = std::chrono::steady_clock::now();
        alloc_thread.wait();
        if (getenv("SLU_PROFILE_PLAN"))
            fprintf(stderr, "[slu amalg plan]   (coarse storage: waited %.1f ms)\n", ms_since(tj));
        alloc_thread.join();
        this->make_inner(A.xsup2.data(), A.supno2.data(), 1, 1, 0, nullptr, pre);
    }

    // Programs in level order of the coarse plan (so the D2H can compress a
    // level as soon as its panels are done): lx / ublks items of the groups
    // of level L at [lx_lev[L], lx_lev[L+1]) / [ub_lev[L], ub_lev[L+1]).
    vector<int> lx_lev, ub_lev; // (ub_lev: U chunks)
    bool progs = false;         // the relayout programs are built
    void ensure_programs() {
        if (progs) return;
        // (the index pointer tables of the LUstruct as it is now: those
        // make() had are gone; the structure is the plan's by the cache key)
        LocalLU *L = LU->Llu;
        const vector<const int_t *> li(L->Lrowind_bc_ptr, L->Lrowind_bc_ptr + ns),
            ui(L->Ufstnz_br_ptr, L->Ufstnz_br_ptr + ns);
        A.set_index(li.data(), ui.data());
        A.build_programs();
        build_programs();
        progs = true;
    }
    void build_programs() {
        const int nl = (int)in->levels.size();
        auto lev = [&](int s) { return in->level_of[A.grp[s]]; };
        // L: column ranges of <= 64 K values per workgroup
        vector<vector<LColX>> bl(nl);
        for (int s = 0; s < ns; ++s) {
            const Amalg::LCol &C = A.lcols[s];
            if (!C.nsupr) continue;
            const int cpi = std::max(1, (int)(65536 / C.nsupr));
            for (int c0 = 0; c0 < C.w; c0 += cpi)
                bl[lev(s)].push_back({C.src, C.dst, C.map, C.nsupr, c0, std::min(C.w, c0 + cpi), C.ld2});
        }
        vector<LColX> lx;
        lx_lev.assign(nl + 1, 0);
        for (int L = 0; L < nl; ++L) {
            lx.insert(lx.end(), bl[L].begin(), bl[L].end());
            lx_lev[L + 1] = (int)lx.size();
        }
        // U: the original block rows in level order, in chunks of <= 64
        // non-empty columns (chunk counts in order, then the rows in parallel)
        ur_h.clear();
        {
            vector<vector<int>> rows(nl);
            for (int s = 0; s < ns; ++s)
                if (A.urows[s].nc) rows[lev(s)].push_back(s);
            vector<int> order;
            order.reserve(ns);
            vector<i64> first(ns + 1, 0);
            ub_lev.assign(nl + 1, 0);
            i64 nch = 0;
            for (int L = 0; L < nl; ++L) {
                for (int s : rows[L]) {
                    first[order.size()] = nch;
                    order.push_back(s);
                    nch += (A.urows[s].nc + 63) / 64;
                }
                ub_lev[L + 1] = (int)nch;
            }
            ur_h.resize(nch);
            parallel_for((int)order.size(), [&](int i) {
                const Amalg::URowX &R = A.urows[order[i]];
                i64 src = R.src, k = first[i];
                for (int c0 = 0; c0 < R.nc; c0 += 64) {
                    const int nc = std::min(64, R.nc - c0);
                    ur_h[k++] = {src, R.c0 + c0, nc, R.end};
                    for (int c = c0; c < c0 + nc; ++c) src += A.ucl[R.c0 + c] + 1;
                }
            }, 256);
        }
        nlx = (int)lx.size();
        if (lx.empty()) lx.push_back({0, 0, 0, 0, 0, 0, 0});
        if (ur_h.empty()) ur_h.resize(1);
        lx_h = std::move(lx);
        // the tables go up on a helper thread (1.5 GB at 100^3): the first
        // relayout joins it (programs_ready)
        prog_thread.start(0, [this] {
            auto up = [](auto &d, const auto &h) { // (a 1-element buffer for an empty table)
                if (h.empty()) d.alloc(1);
                else d.upload(h.data(), h.size());
            };
            up(d_lx, lx_h);
            up(d_ur, ur_h);
            up(d_lrow, A.lrow);
            up(d_ucd, A.ucd);
            up(d_ucl, A.ucl);
            up(d_D, A.D);
        });
    }
    vector<LColX> lx_h;
    vector<UChunk> ur_h;
    std::mutex prog_mu;
    void programs_ready() {
        std::lock_guard<std::mutex> lk(prog_mu);
        prog_thread.join();
    }
    int nlx = 0;

    // levels [L0, L1) of the relayout on stream st
    void relayout_levels(int dir, int L0, int L1, hipStream_t st) {
        ensure_programs();
        programs_ready();
        const int a = lx_lev[L0], b = lx_lev[L1];
        if (b > a)
            hipLaunchKernelGGL((k_amalg_l<T>), dim3(b - a), dim3(256), 0, st, d_lx.p + a, d_lrow.p,
                               d_oL.p, in->d_L.p, dir);
        const int u0 = ub_lev[L0], nr = ub_lev[L1] - u0;
        if (nr > 0)
            hipLaunchKernelGGL((k_amalg_u<T>), dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, st,
                               d_ur.p + u0, nr, d_ucd.p, d_ucl.p, d_D.p, (i64)A.DL0, d_oU.p, in->d_L.p,
                               in->d_U.p, dir);
        HIPCHK(hipGetLastError());
    }

    // The overlapped D2H of the drop-in path (opts.overlap_download): the
    // inner plan's pinned-slot pipeline (run_d2h) with fills that carry the
    // caller's layout: a coarse group's members are consecutive supernodes,
    // so its values are one range of d_oL and one of d_oU; before a fill is
    // pushed, d2h_pre compresses every level up to the fill's into d_oL /
    // d_oU on the D2H stream.
    int compressed_to = 0;
    void build_d2h() {
        ensure_o(); // (the push programs address d_oL / d_oU)
        Inner &P = *in;
        warm_thread.join();
        if (warm_stage.p) P.d_stage.swap(warm_stage);
        LocalLU *Llu = LU->Llu;
        const int_t *xsup = LU->Glu_persist->xsup;
        const int nl = (int)P.levels.size();
        vector<i64> lsrc(ns + 1, 0);
        for (int s = 0; s < ns; ++s)
            lsrc[s + 1] = lsrc[s] + (Llu->Lrowind_bc_ptr[s] ? (i64)Llu->Lrowind_bc_ptr[s][1] * (xsup[s + 1] - xsup[s]) : 0);
        vector<int> g0(A.ns2 + 1, ns); // first original supernode of each group
        for (int s = ns - 1; s >= 0; --s) g0[A.grp[s]] = s;
        // one piece per group and factor where the caller's arrays are
        // contiguous over the group's members (pddistribute's *_dat layout),
        // else one per member
        for (int L = 0; L < nl; ++L) {
            for (int J : P.bylev[L]) {
                for (int pass = 0; pass < 2; ++pass) {
                    const vector<i64> &off = pass ? usrc : lsrc;
                    const T *dbase = pass ? d_oU.p : d_oL.p;
                    auto hptr = [&](int s) -> char * {
                        if (pass) return Llu->Ufstnz_br_ptr[s] ? (char *)Llu->Unzval_br_ptr[s] : nullptr;
                        return Llu->Lrowind_bc_ptr[s] ? (char *)Llu->Lnzval_bc_ptr[s] : nullptr;
                    };
                    int a = g0[J];
                    while (a < g0[J + 1]) {
                        int b = a;
                        while (b < g0[J + 1] && (off[b + 1] == off[b] || !hptr(b))) ++b; // empty
                        if (b == g0[J + 1]) break;
                        char *h0 = hptr(b);
                        int e = b + 1;
                        while (e < g0[J + 1] && (off[e + 1] == off[e] ||
                                                 hptr(e) == h0 + (off[e] - off[b]) * (i64)sizeof(T)))
                            ++e;
                        P.d2h.add((const char *)(dbase + off[b]), h0, (off[e] - off[b]) * (i64)sizeof(T), L);
                        a = e;
                    }
                }
            }
            P.d2h.end_level(L, L + 1 == nl);
        }
        P.d2h.finish();
        P.d2h_pre = [this](int L, hipStream_t st) {
            if (L + 1 > compressed_to) {
                relayout_levels(1, compressed_to, L + 1, st);
                compressed_to = L + 1;
            }
        };
        P.opts.overlap_download = 1;
    }

    i64 o_lv = 0, o_uv = 0;
    void ensure_o() {
        std::lock_guard<std::mutex> lk(o_mu);
        if (d_oL.p) return;
        d_oL.alloc(std::max<i64>(o_lv, 1));
        d_oU.alloc(std::max<i64>(o_uv, 1));
    }
    vector<Xfer> xfers() override {
        ensure_o();
        LocalLU *L = LU->Llu;
        vector<Xfer> xs;
        const int_t *xsup = LU->Glu_persist->xsup;
        i64 lo = 0;
        for (int s = 0; s < ns; ++s) {
            if (!L->Lrowind_bc_ptr[s]) continue;
            const i64 cnt = (i64)L->Lrowind_bc_ptr[s][1] * (xsup[s + 1] - xsup[s]);
            xs.push_back({(char *)(d_oL.p + lo), (char *)L->Lnzval_bc_ptr[s], (size_t)cnt * sizeof(T)});
            lo += cnt;
        }
        for (int s = 0; s < ns; ++s)
            if (L->Ufstnz_br_ptr[s])
                xs.push_back({(char *)(d_oU.p + usrc[s]), (char *)L->Unzval_br_ptr[s],
                              (size_t)(usrc[s + 1] - usrc[s]) * sizeof(T)});
        return merge_xfers(std::move(xs));
    }
    void h2d() {
        const auto t0 = std::chrono::steady_clock::now();
        vector<Xfer> xs = xfers();
        if (!o_mapped) {
            hipStream_t st = nullptr;
            HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            HIPCHK(hipMemsetAsync(d_oL.p, 0, sizeof(T), st));
            HIPCHK(hipMemsetAsync(d_oU.p, 0, sizeof(T), st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipStreamDestroy(st));
            t_omap = ms_since(t0);
            if (getenv("SLU_PROFILE_PLAN"))
                fprintf(stderr, "[slu amalg plan]   (caller-layout storage %.1f GB mapped in %.1f ms, at %.1f ms)\n",
                        (d_oL.bytes() + d_oU.bytes()) / 1e9, t_omap, ms_since(t_born));
            set_mapped();
        }
        staged_h2d(xs, 0);
        h2d_bytes = 0;
        for (auto &x : xs) h2d_bytes += (double)x.bytes;
        up_ms = ms_since(t0);
    }

    void relayout(int dir) {
        ensure_o();
        hipStream_t st = in->stream;
        if (dir == 0) {
            HIPCHK(hipMemsetAsync(in->d_L.p, 0, in->d_L.bytes(), st));
            HIPCHK(hipMemsetAsync(in->d_U.p, 0, in->d_U.bytes(), st));
        }
        relayout_levels(dir, 0, (int)in->levels.size(), st);
        HIPCHK(hipStreamSynchronize(st));
    }

    void sync_stats() override {
        this->caller_flops(A.fl);
        stats.amalg_groups = A.n_merged_groups;
        stats.amalg_zeros = (double)A.zeros;
        stats.t_amalg_ms = t_amalg;
        stats.t_plan_ms = t_plan;
        stats.t_upload_ms = up_ms;
        stats.h2d_bytes = h2d_bytes;
        stats.t_expand_ms = t_expand;
        stats.t_compress_ms = t_compress;
        stats.t_d2h_ms = t_d2h;
        stats.d2h_bytes = (double)(d_oL.bytes() + d_oU.bytes());
    }

    void upload() override {
        const auto t0 = std::chrono::steady_clock::now();
        if (up_thread.running()) up_thread.join();
        else h2d();
        const auto t1 = std::chrono::steady_clock::now();
        relayout(0);
        t_expand = ms_since(t1);
        in->vstate = 1;
        in->dinv_valid = false;
        in->d_acur = nullptr;
        in->d_acur64 = nullptr;
        in->host_current = false;
        coarse_current = false;
        host_done = false;
        sync_stats();
        stats.t_upload_wait_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    void adopt_factors() override {
        upload();
        in->sync();
        in->vstate = 2;
        in->dinv_valid = false;
        in->a_fact = nullptr; // adopted factors: of no A this plan knows
        in->a_fact64 = nullptr;
        coarse_current = true;
        host_done = true; // the caller's arrays hold these factors already
    }
    void factor(double anorm, int *info, int *tiny) override {
        compressed_to = 0;
        in->factor(anorm, info, tiny);
        // overlap_download: the caller's arrays already hold the factors
        coarse_current = !in->host_current;
        host_done = in->host_current;
        sync_stats();
        if (host_done) {
            stats.t_d2h_ms = in->stats.t_d2h_ms;
            stats.t_d2h_tail_ms = in->stats.t_d2h_tail_ms;
            stats.d2h_bytes = in->stats.d2h_bytes;
            stats.n_d2h_copies = in->stats.n_d2h_copies;
        }
    }
    bool host_done = false; // overlap_download / adopt_factors: nothing to download
    bool host_done_now() const override { return host_done; }
    void coarse_changed() override {
        coarse_current = true;
        host_done = false;
    }
    void compress() override {
        const auto t0 = std::chrono::steady_clock::now();
        relayout(1);
        t_compress = ms_since(t0);
    }

    // ---- helper threads: the H2D copy of the caller's values, the coarse
    // storage's allocation, the D2H warm-up and the upload of the relayout
    // programs.  Declared last: they use the DevBuf members above (and the
    // base's inner plan), and members are destroyed in reverse order, so
    // every thread is joined before a buffer is freed, on every exit path.
    HelperThread up_thread, alloc_thread, warm_thread, prog_thread;
};

// ------------------------------------------------------------ grid amalgamation
// The coarse partition on a Pr x Pc grid (csrc/amalg.h, "grids"): the
// analysis runs on the ranks' supernode ranges, every fine block goes to
// the owner of its coarse block (structure once, values at every upload and
// back at download), and the inner Plan -- the ordinary grid plan -- runs on
// each rank's local coarse LUstruct with the caller's communicator.  The
// value relayout on the device: pack (k_amalg_l over the caller's L with a
// row map, k_ranges over its U blocks) into one send buffer ordered by
// destination, one section per ordered rank pair over the transport (RCCL
// send / receive on the world communicator, or the host transports), unpack
// (k_amalg_l / k_amalg_u) into the zeroed coarse storage; download runs the
// same programs backwards.
template <typename T, typename HT, typename LocalLU, typename LUS>
struct GridAmalgPlan : CoarsePlan<T, HT, LocalLU, LUS> {
    using Base = CoarsePlan<T, HT, LocalLU, LUS>;
    using typename Base::Inner;
    using Base::LU; using Base::n; using Base::ns; using Base::opts; using Base::in; using Base::stats;
    using Base::mlidx; using Base::muidx; using Base::coarse_current;
    using Base::t_expand; using Base::t_compress; using Base::t_d2h;
    int Pr = 1, Pc = 1, iam = 0, P = 1;
    slu_comm *comm = nullptr;
    bool dry = false;
    GaFine f;
    vector<const int_t *> flidx, fuidx;
    GaChains ch;
    GaPartition g;
    GaRelay r;
    vector<vector<i64>> cnt; // cnt[p][q]: values rank p sends rank q
    Xport X;
    hipStream_t xs = nullptr; // plan-time exchanges before the inner plan exists
    // device: caller layout, send / receive buffers, programs
    DevBuf<T> d_oL, d_oU, d_send, d_recv;
    DevBuf<LColX> d_pl, d_ul;
    DevBuf<int32_t> d_plrow, d_ulrow, d_uucd;
    DevBuf<uint16_t> d_uucl;
    DevBuf<GaSpan> d_pu;
    DevBuf<UChunk> d_uu;
    DevBuf<i64> d_D;
    double t_relay_plan = 0, t_h2d = 0;

    // nullptr when nothing merges (every rank decides the same: the
    // partition is all-gathered)
    static GridAmalgPlan *make(LUS *lu, int n_, int pr, int pc, int iam_, slu_comm *c,
                               const slu_engine_opts *o, double zero_frac, int maxw) {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<GridAmalgPlan> G(new GridAmalgPlan);
        G->LU = lu;
        G->n = n_;
        G->Pr = pr;
        G->Pc = pc;
        G->P = pr * pc;
        G->iam = iam_;
        G->comm = c;
        if (o) G->opts = *o;
        G->dry = G->opts.schedule_only != 0;
        SLU_REQUIRE(c && (c->world || c->host_fn || c->host_p2p), "a %dx%d grid needs a communicator", pr, pc);
        SLU_REQUIRE(G->P <= 32, "grid amalgamation: at most 32 ranks");
        if (!G->dry) {
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipStreamCreateWithFlags(&G->xs, hipStreamNonBlocking));
        }
        G->X.c = c;
        G->X.s = G->xs;
        G->X.host_mem = G->dry;
        LocalLU *L = lu->Llu;
        GaFine &f = G->f;
        f.n = n_;
        f.ns = G->ns = (int)(lu->Glu_persist->supno[n_ - 1] + 1);
        f.Pr = pr;
        f.Pc = pc;
        f.myrow = iam_ / pc;
        f.mycol = iam_ % pc;
        f.xsup = lu->Glu_persist->xsup;
        G->flidx.assign(L->Lrowind_bc_ptr, L->Lrowind_bc_ptr + f.nlc());
        G->fuidx.assign(L->Ufstnz_br_ptr, L->Ufstnz_br_ptr + f.nlr());
        f.lidx = G->flidx.data();
        f.uidx = G->fuidx.data();
        // 1. structure to the analysis owners, chains of my range
        G->ch = ga_analyse(f, G->X.alltoallv(ga_structure_out(f)), zero_frac, maxw);
        // 2. the partition
        G->g = ga_partition(f, G->X.allgatherv(G_WORLD, G->ch.gstart));
        if (G->g.ns2 == G->ns) return nullptr;
        // 3. relayout: my pieces' structure to the coarse owners, my coarse
        // LUstruct and programs from what arrives; everybody's counts
        ga_send_side(f, G->g, G->r);
        ga_receive_side(f, G->g, G->X.alltoallv(G->r.sstruct), G->r);
        G->cnt = G->X.allgatherv(G_WORLD, G->r.scount);
        for (int p = 0; p < G->P; ++p)
            SLU_REQUIRE(G->cnt[p][iam_] == G->r.rcount[p], "grid amalgamation: counts %d -> %d", p, iam_);
        G->t_relay_plan = ms_since(t0);
        G->build_inner();
        if (!G->dry) G->build_programs();
        G->sync_stats();
        G->stats.t_plan_ms = ms_since(t0);
        return G.release();
    }

    void build_inner() {
        mlidx.assign(r.nlc2, nullptr);
        muidx.assign(r.nlr2, nullptr);
        for (int j = 0; j < r.nlc2; ++j)
            if (!r.Lidx2[j].empty()) mlidx[j] = r.Lidx2[j].data();
        for (int j = 0; j < r.nlr2; ++j)
            if (!r.Uidx2[j].empty()) muidx[j] = r.Uidx2[j].data();
        this->make_inner(g.xsup2.data(), g.supno2.data(), Pr, Pc, iam, comm);
        if (!dry) X.s = in->stream; // the relayout's sections go on the kernels' stream
    }

    template <typename V> static void up(DevBuf<V> &d, const vector<V> &h) {
        if (h.empty()) d.upload(vector<V>(1));
        else d.upload(h);
    }
    void build_programs() {
        up(d_pl, r.pack_l);
        up(d_plrow, r.pack_lrow);
        up(d_pu, r.pack_u);
        up(d_ul, r.unpack_l);
        up(d_ulrow, r.unpack_lrow);
        up(d_uu, r.unpack_u);
        up(d_uucd, r.unpack_ucd);
        up(d_uucl, r.unpack_ucl);
        up(d_D, r.D);
        d_send.alloc(std::max<i64>(r.soff[P], 1));
        d_recv.alloc(std::max<i64>(r.received, 1));
    }
    void ensure_o() {
        if (d_oL.p) return;
        d_oL.alloc(std::max<i64>(r.lval, 1));
        d_oU.alloc(std::max<i64>(r.uval, 1));
    }
    // (the caller's local values)
    vector<Xfer> xfers() override {
        ensure_o();
        LocalLU *L = LU->Llu;
        vector<Xfer> v;
        for (int j = 0; j < f.nlc(); ++j)
            if (L->Lrowind_bc_ptr[j] && r.lsrc[j + 1] > r.lsrc[j])
                v.push_back({(char *)(d_oL.p + r.lsrc[j]), (char *)L->Lnzval_bc_ptr[j],
                             (size_t)(r.lsrc[j + 1] - r.lsrc[j]) * sizeof(T)});
        for (int j = 0; j < f.nlr(); ++j)
            if (L->Ufstnz_br_ptr[j] && r.usrc[j + 1] > r.usrc[j])
                v.push_back({(char *)(d_oU.p + r.usrc[j]), (char *)L->Unzval_br_ptr[j],
                             (size_t)(r.usrc[j + 1] - r.usrc[j]) * sizeof(T)});
        return merge_xfers(std::move(v));
    }

    void launch_l(const DevBuf<LColX> &items, size_t nitems, const DevBuf<int32_t> &lrow, T *o, T *m, int dir,
                  hipStream_t st) {
        if (nitems)
            hipLaunchKernelGGL((k_amalg_l<T>), dim3((unsigned)nitems), dim3(256), 0, st, items.p, lrow.p, o, m, dir);
    }
    // the value all-to-all: forward p -> q from send to receive regions,
    // backward q -> p the other way; my own pair is a device copy
    void exchange(bool forward) {
        hipStream_t st = in->stream;
        const int me = iam;
        if (r.scount[me])
            HIPCHK(hipMemcpyAsync(forward ? d_recv.p + r.roff[me] : d_send.p + r.soff[me],
                                  forward ? d_send.p + r.soff[me] : d_recv.p + r.roff[me],
                                  (size_t)r.scount[me] * sizeof(T), hipMemcpyDeviceToDevice, st));
        for (int p = 0; p < P; ++p)
            for (int q = 0; q < P; ++q) {
                if (p == q || !cnt[p][q]) continue;
                const int root = forward ? p : q, dest = forward ? q : p;
                T *buf = nullptr;
                if (me == p) buf = d_send.p + r.soff[q];
                else if (me == q) buf = d_recv.p + r.roff[p];
                X.section(G_WORLD, root, 1u << dest, buf, (size_t)cnt[p][q] * sizeof(T));
            }
        X.flush_as(forward ? "grid amalgamation relayout (values to the coarse owners)"
                           : "grid amalgamation relayout (factors back to the caller layout)");
    }

    void expand() { // caller layout (d_oL / d_oU) -> coarse
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = in->stream;
        launch_l(d_pl, r.pack_l.size(), d_plrow, d_send.p, d_oL.p, 1, st);
        if (!r.pack_u.empty())
            hipLaunchKernelGGL((k_ranges<T>), dim3((unsigned)((r.pack_u.size() + 255) / 256)), dim3(256), 0, st,
                               d_pu.p, (int)r.pack_u.size(), d_oU.p, d_send.p, 0);
        HIPCHK(hipGetLastError());
        exchange(true);
        HIPCHK(hipMemsetAsync(in->d_L.p, 0, in->d_L.bytes(), st));
        HIPCHK(hipMemsetAsync(in->d_U.p, 0, in->d_U.bytes(), st));
        launch_l(d_ul, r.unpack_l.size(), d_ulrow, d_recv.p, in->d_L.p, 0, st);
        if (!r.unpack_u.empty())
            hipLaunchKernelGGL((k_amalg_u<T>), dim3((unsigned)((r.unpack_u.size() + 3) / 4)), dim3(256), 0, st,
                               d_uu.p, (int)r.unpack_u.size(), d_uucd.p, d_uucl.p, d_D.p, (i64)r.DL0, d_recv.p, in->d_L.p,
                               in->d_U.p, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        t_expand = ms_since(t0);
    }
    void compress() override {
        ensure_o();
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t st = in->stream;
        launch_l(d_ul, r.unpack_l.size(), d_ulrow, d_recv.p, in->d_L.p, 1, st);
        if (!r.unpack_u.empty())
            hipLaunchKernelGGL((k_amalg_u<T>), dim3((unsigned)((r.unpack_u.size() + 3) / 4)), dim3(256), 0, st,
                               d_uu.p, (int)r.unpack_u.size(), d_uucd.p, d_uucl.p, d_D.p, (i64)r.DL0, d_recv.p, in->d_L.p,
                               in->d_U.p, 1);
        HIPCHK(hipGetLastError());
        exchange(false);
        launch_l(d_pl, r.pack_l.size(), d_plrow, d_send.p, d_oL.p, 0, st);
        if (!r.pack_u.empty())
            hipLaunchKernelGGL((k_ranges<T>), dim3((unsigned)((r.pack_u.size() + 255) / 256)), dim3(256), 0, st,
                               d_pu.p, (int)r.pack_u.size(), d_oU.p, d_send.p, 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        t_compress = ms_since(t0);
    }

    void sync_stats() override {
        this->caller_flops(ch.fl); // my analysis range's share of the caller partition's work
        i64 groups = 0;
        for (size_t i = 0; i < ch.gstart.size(); ++i) {
            const i64 e = i + 1 < ch.gstart.size() ? ch.gstart[i + 1]
                                                   : (i64)ga_range(ns, P, iam + 1);
            groups += e - ch.gstart[i] > 1;
        }
        stats.amalg_groups = groups;
        stats.t_amalg_ms = t_relay_plan;
        stats.t_expand_ms = t_expand;
        stats.t_compress_ms = t_compress;
        stats.t_upload_ms = t_h2d;
        stats.t_d2h_ms = t_d2h;
        stats.h2d_bytes = (double)(r.lval + r.uval) * sizeof(T);
        stats.d2h_bytes = stats.h2d_bytes;
    }

    void upload() override {
        const auto t0 = std::chrono::steady_clock::now();
        staged_h2d(xfers(), comm->device);
        t_h2d = ms_since(t0);
        expand();
        in->vstate = 1;
        in->dinv_valid = false;
        in->d_acur = nullptr;
        in->d_acur64 = nullptr;
        in->host_current = false;
        coarse_current = false;
        sync_stats();
    }
    void adopt_factors() override {
        upload();
        in->sync();
        in->vstate = 2;
        in->dinv_valid = false;
        in->a_fact = nullptr; // adopted factors: of no A this plan knows
        in->a_fact64 = nullptr;
    }
    void factor(double anorm, int *info, int *tiny) override {
        in->factor(anorm, info, tiny);
        coarse_current = true;
        sync_stats();
    }
    ~GridAmalgPlan() override {
        in.reset();
        if (xs) (void)hipStreamDestroy(xs);
    }
};

// The plan for a caller's LUstruct: the amalgamated one when chains merge
// (1x1: AmalgPlan; 2D grids: GridAmalgPlan; SLU_AMALG=0 turns it off;
// SLU_AMALG_ZERO sets the explicit zero fraction, default 0.10), else the
// plain plan.  3D grids factor the caller's partition (its forests).
template <typename P> PlanBase *make_plan_any(void *LU, int n, int pr, int pc, int iam, slu_comm *c,
                                              const slu_engine_opts *o) {
    using A = AmalgPlan<typename P::value_type, typename P::host_type, typename P::local_type,
                        typename P::lus_type>;
    using GA = GridAmalgPlan<typename P::value_type, typename P::host_type, typename P::local_type,
                             typename P::lus_type>;
    const char *e = getenv("SLU_AMALG");
    const bool on = !(e && !strcmp(e, "0"));
    const char *z = getenv("SLU_AMALG_ZERO");
    const double zf = z ? atof(z) : 0.10;
    if (on && pr * pc == 1 && !(o && o->schedule_only) && !(c && c->npdep > 1)) {
        if (PlanBase *p = A::make((typename P::lus_type *)LU, n, o, zf, FAST_MAXW)) return p;
    } else if (on && pr * pc > 1 && !(c && c->npdep > 1)) {
        if (PlanBase *p = GA::make((typename P::lus_type *)LU, n, pr, pc, iam, c, o, zf, FAST_MAXW)) return p;
    }
    return make_plan<P>(LU, n, pr, pc, iam, c, o);
}

} // namespace slu
