// The communicator of a process grid (slu_comm) and the grouped exchanges
// the plans run over it (Xport): RCCL, or the host transports of the tests.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "devbuf.h"
#include "watchdog.h"
#include "slu_mi355x.h"

// ------------------------------------------------------------------ comm
// One rank per GPU.  Production transport: RCCL communicators for the whole
// grid, its process rows and its process columns (the reference's
// grid->comm / rscp / cscp, SRC/superlu_grid.c:158-172).  Test transport
// (slu_comm_create_host): host-staged broadcasts through a caller callback,
// for several ranks sharing one GPU where RCCL refuses duplicate devices.
struct slu_comm {
    int nprow = 1, npcol = 1, iam = 0, myrow = 0, mycol = 0, device = 0;
    ncclComm_t world = nullptr, row = nullptr, col = nullptr;
    // 3D grids (SRC/superlu_grid3d.c: Pz layers of a Pr x Pc grid, the
    // reference's grid3d->zscp): world / row / col above are the layer's,
    // zcomm joins the ranks at my (row, column) position of every layer
    int npdep = 1, zlayer = 0;
    ncclComm_t all = nullptr, zcomm = nullptr;
    slu_host_bcast_fn host_fn = nullptr;
    slu_host_p2p_fn host_p2p = nullptr; // point-to-point test transport
    void *host_ctx = nullptr;
    // exchange watchdog (watchdog.h), created with the first exchange
    std::unique_ptr<slu::Watchdog> wd;
    bool wd_init = false;
    slu::Watchdog *watchdog() {
        if (wd_init) return wd.get();
        wd_init = true;
        const double b = slu::Watchdog::bound_from_env();
        if (b <= 0) return nullptr;
        wd.reset(new slu::Watchdog);
        wd->bound_s = b;
        wd->device = device;
        char w[160];
        snprintf(w, sizeof w, "rank %d of a %dx%d%s grid (row %d, column %d%s), %s transport", iam, nprow, npcol,
                 npdep > 1 ? ("x" + std::to_string(npdep)).c_str() : "", myrow, mycol,
                 npdep > 1 ? (", layer " + std::to_string(zlayer)).c_str() : "",
                 world || zcomm ? "RCCL" : host_p2p ? "host point-to-point" : "host broadcast");
        wd->who = w;
        if (world || zcomm) {
            ncclComm_t cs[5] = {row, col, world, zcomm, all};
            wd->abort_comms = [cs] {
                for (ncclComm_t cm : cs)
                    if (cm) ncclCommAbort(cm);
            };
            wd->async_error = [cs]() -> std::string {
                static const char *names[5] = {"row", "column", "layer", "z", "world"};
                for (int i = 0; i < 5; ++i) {
                    ncclResult_t r = ncclSuccess;
                    if (!cs[i] || ncclCommGetAsyncError(cs[i], &r) != ncclSuccess) continue;
                    if (r != ncclSuccess && r != ncclInProgress)
                        return std::string(names[i]) + " communicator: " + ncclGetErrorString(r);
                }
                return "";
            };
        }
        return wd.get();
    }
};

namespace slu {

using i64 = int64_t;

enum { G_WORLD = 0, G_ROW = 1, G_COL = 2, G_Z = 3 };

// Grouped broadcasts of device buffers within the world / a process row /
// a process column.  Ops are queued and issued together by flush() (one
// ncclGroupStart/End); every member of a communicator queues the same ops in
// the same order, which the plan guarantees by construction.
struct Xport {
    slu_comm *c = nullptr;
    hipStream_t s = nullptr;
    struct Op {
        int g, root;
        void *buf; // null on a member that does not need the section
        size_t bytes;
        uint32_t mask; // members (group ranks) that receive it
    };
    vector<Op> ops;
    vector<char> hbuf;
    double sent = 0, recvd = 0; // bytes this rank moved (RCCL sections)
    // what the next flush() is, for the watchdog's diagnostics
    const char *phase = "plan-time exchange";
    int level = -1;
    int gsize(int g) const {
        return g == G_WORLD ? c->nprow * c->npcol : g == G_ROW ? c->npcol : g == G_COL ? c->nprow : c->npdep;
    }
    int grank(int g) const {
        return g == G_WORLD ? c->iam : g == G_ROW ? c->mycol : g == G_COL ? c->myrow : c->zlayer;
    }
    ncclComm_t comm_of(int g) const {
        return g == G_WORLD ? c->world : g == G_ROW ? c->row : g == G_COL ? c->col : c->zcomm;
    }
    void bcast(int g, int root, void *buf, size_t bytes) {
        if (bytes && gsize(g) > 1) ops.push_back({g, root, buf, bytes, ~0u});
    }
    // A section of root's data for the members in mask (the reference sends
    // L(:,k) only to the process columns flagged in ToSendR,
    // SRC/pdgstrf.c:1039-1044, SRC/pddistribute.c:779).  Every member of the
    // group queues the op (buf = null when not in mask), so that the host
    // transport, which can only broadcast, stays in step.
    void section(int g, int root, uint32_t mask, void *buf, size_t bytes) {
        if (bytes && gsize(g) > 1 && (mask & ~(1u << root))) ops.push_back({g, root, buf, bytes, mask});
    }
    // This rank's point-to-point calls for the queued group, in issue order:
    // a section (and a broadcast, mask = all) becomes the root's sends to
    // every other member in the mask, in member order, and each member's
    // receive from the root.  The RCCL branch issues exactly this list as
    // ncclSend / ncclRecv inside one ncclGroupStart / End, and the
    // point-to-point test transport hands exactly this list to its callback
    // (staged through host memory, all posted before any completes), so the
    // send / receive pairing every grid test runs is the one the RCCL node
    // runs (tests/test_grid.py::test_rccl_call_sequence_is_the_tested_one_cpu
    // compares the two lists and checks the pairing across ranks).
    struct P2P {
        int g, peer, send; // group, group rank of the other side, 1 = send
        size_t bytes;
        int op; // index into ops
    };
    vector<P2P> expand() const {
        vector<P2P> q;
        for (size_t i = 0; i < ops.size(); ++i) {
            const Op &o = ops[i];
            const int me = grank(o.g), P = gsize(o.g);
            if (me == o.root) {
                for (int m = 0; m < P; ++m)
                    if (m != me && (o.mask >> m & 1)) q.push_back({o.g, m, 1, o.bytes, (int)i});
            } else if (o.mask >> me & 1) {
                q.push_back({o.g, o.root, 0, o.bytes, (int)i});
            }
        }
        return q;
    }
    int world_of(int g, int m) const {
        return g == G_WORLD ? m : g == G_ROW ? c->myrow * c->npcol + m : g == G_COL ? m * c->npcol + c->mycol : c->iam;
    }
    // SLU_XPORT_TRACE=<dir>: every flush appends this rank's call list to
    // <dir>/xport_<kind>.<world rank> (kind: the list the transport ran, and
    // on the host transports also "rccl", the calls the RCCL branch would
    // issue for the same group, recorded by a dry run of flush_rccl)
    const char *trace_dir = getenv("SLU_XPORT_TRACE");
    long trace_seq = 0;
    void trace(const char *kind, const vector<P2P> &q) const {
        if (!trace_dir) return;
        char fn[1024];
        snprintf(fn, sizeof fn, "%s/xport_%s.%d", trace_dir, kind, c->iam);
        FILE *f = fopen(fn, "a");
        if (!f) return;
        fprintf(f, "F %ld %s %d\n", trace_seq, phase, level);
        for (const P2P &p : q)
            fprintf(f, "%c %d %d %zu\n", p.send ? 'S' : 'R', p.g, world_of(p.g, p.peer), p.bytes);
        fclose(f);
    }
    vector<vector<char>> p2p_bufs;
    bool host_mem = false; // schedule-only plans: buffers are host memory
    void flush_p2p() {
        const vector<P2P> q0 = expand();
        trace("host", q0);
        if (trace_dir) flush_rccl(true);
        vector<slu_host_p2p_op> q;
        if (host_mem) {
            // no staging: the host buffers go to the transport as they are
            for (const P2P &p : q0) {
                const Op &o = ops[p.op];
                SLU_REQUIRE(o.buf, "section of group %d root %d has no buffer", o.g, o.root);
                q.push_back({p.g, p.peer, p.send, 0, o.buf, (int64_t)p.bytes});
                (p.send ? sent : recvd) += (double)p.bytes;
            }
            if (!q.empty())
                SLU_REQUIRE(c->host_p2p(c->host_ctx, (int)q.size(), q.data()) == 0,
                            "host point-to-point group of %zu ops failed", q.size());
            return;
        }
        HIPCHK(hipStreamSynchronize(s));
        // one host staging buffer per op: the root's D2H once, its sends read it
        p2p_bufs.resize(std::max(p2p_bufs.size(), ops.size()));
        vector<char> staged(ops.size(), 0);
        for (const P2P &p : q0) {
            const Op &o = ops[p.op];
            SLU_REQUIRE(o.buf, "section of group %d root %d has no buffer", o.g, o.root);
            vector<char> &hb = p2p_bufs[p.op];
            hb.resize(o.bytes);
            if (p.send && !staged[p.op]) {
                HIPCHK(hipMemcpyAsync(hb.data(), o.buf, o.bytes, hipMemcpyDeviceToHost, s));
                staged[p.op] = 1;
            }
            q.push_back({p.g, p.peer, p.send, 0, hb.data(), (int64_t)p.bytes});
            (p.send ? sent : recvd) += (double)p.bytes;
        }
        HIPCHK(hipStreamSynchronize(s));
        if (!q.empty())
            SLU_REQUIRE(c->host_p2p(c->host_ctx, (int)q.size(), q.data()) == 0,
                        "host point-to-point group of %zu ops failed", q.size());
        for (const P2P &p : q0)
            if (!p.send)
                HIPCHK(hipMemcpyAsync(ops[p.op].buf, p2p_bufs[p.op].data(), p.bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    // this rank's part of the queued group, for the watchdog
    std::string describe() const {
        static const char *gn[4] = {"layer", "row", "column", "z"};
        std::string s = phase;
        if (level >= 0) s += " of level " + std::to_string(level);
        int shown = 0, more = 0;
        double sb = 0, rb = 0;
        std::string lst;
        auto add = [&](bool send, int g, int m, size_t bytes) {
            (send ? sb : rb) += (double)bytes;
            if (shown == 12) {
                ++more;
                return;
            }
            char b[160];
            if (g == G_Z)
                snprintf(b, sizeof b, "%s layer %d: %zu bytes", send ? "send to" : "receive from", m, bytes);
            else
                snprintf(b, sizeof b, "%s %s peer %d (rank %d): %zu bytes", send ? "send to" : "receive from",
                         gn[g], m, world_of(g, m), bytes);
            lst += (shown++ ? "; " : "") + std::string(b);
        };
        for (const P2P &p : expand()) add(p.send != 0, p.g, p.peer, p.bytes);
        char b[160];
        snprintf(b, sizeof b, " (%zu ops; this rank sends %.0f and receives %.0f bytes): ", ops.size(), sb, rb);
        s += b + lst;
        if (more) s += "; ... " + std::to_string(more) + " more";
        return s;
    }
    void flush() {
        if (ops.empty()) return;
        ++trace_seq;
        Watchdog *wd = c->watchdog();
        if (c->host_p2p || c->host_fn) {
            // host transports block in the callback: the record is open for its duration
            const uint64_t id = wd ? wd->open(describe(), nullptr) : 0;
            if (c->host_p2p) flush_host_p2p();
            else {
                if (trace_dir) flush_rccl(true);
                flush_host_bcast();
            }
            if (wd) wd->close(id);
            ops.clear();
            return;
        }
        flush_rccl(false);
        if (wd) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            HIPCHK(hipEventRecord(e, s));
            wd->open(describe(), e);
        }
        ops.clear();
    }
    // flush() named for the watchdog and the trace (level < 0: none)
    void flush_as(const char *ph, int lvl = -1) {
        phase = ph;
        level = lvl;
        flush();
        phase = "plan-time exchange";
        level = -1;
    }
    void flush_host_p2p() { flush_p2p(); }
    void flush_host_bcast() {
        {
            HIPCHK(hipStreamSynchronize(s));
            for (auto &o : ops) {
                hbuf.resize(o.bytes);
                const int me = grank(o.g);
                const bool root = me == o.root;
                // copies on the transport's stream and waited for: a pageable
                // hipMemcpy returns once the host buffer is staged, before the
                // DMA has landed, and kernels on a non-blocking stream could
                // read the destination first
                if (root) {
                    HIPCHK(hipMemcpyAsync(hbuf.data(), o.buf, o.bytes, hipMemcpyDeviceToHost, s));
                    HIPCHK(hipStreamSynchronize(s));
                }
                SLU_REQUIRE(c->host_fn(c->host_ctx, o.g, o.root, hbuf.data(), (int64_t)o.bytes) == 0,
                            "host broadcast (group %d, root %d, %zu bytes) failed", o.g, o.root,
                            o.bytes);
                if (!root && (o.mask >> me & 1)) {
                    SLU_REQUIRE(o.buf, "section of group %d root %d has no buffer", o.g, o.root);
                    HIPCHK(hipMemcpyAsync(o.buf, hbuf.data(), o.bytes, hipMemcpyHostToDevice, s));
                    HIPCHK(hipStreamSynchronize(s));
                }
            }
        }
    }
    // Every op as direct sends from the root to each member that needs it
    // (xGMI is point to point: a root's sends to its row / column peers use
    // distinct links; the plan-time all-gathers' broadcasts too, so there is
    // one call sequence, expand()'s, for RCCL and the tested transport).
    // dry: record the calls (SLU_XPORT_TRACE, kind "rccl") instead of
    // issuing them -- the host transports' check of this very code path.
    void flush_rccl(bool dry) {
        const vector<P2P> q = expand();
        if (dry) {
            trace("rccl", q);
            return;
        }
        trace("rccl", q);
        NCCLCHK(ncclGroupStart());
        for (const P2P &p : q) {
            const Op &o = ops[p.op];
            if (p.send) NCCLCHK(ncclSend(o.buf, o.bytes, ncclChar, p.peer, comm_of(o.g), s));
            else NCCLCHK(ncclRecv(o.buf, o.bytes, ncclChar, p.peer, comm_of(o.g), s));
            (p.send ? sent : recvd) += (double)p.bytes;
        }
        NCCLCHK(ncclGroupEnd());
    }
    // plan-time all-to-all of variable-length int64 blobs in the world
    // group: out[q] goes to rank q, the result's [p] came from rank p.  Sizes
    // first (an all-gather), then one section per ordered pair, queued in
    // the same order on every rank.
    vector<vector<i64>> alltoallv(const vector<vector<i64>> &out) {
        const int P = gsize(G_WORLD), me = grank(G_WORLD);
        SLU_REQUIRE((int)out.size() == P && P <= 32, "alltoallv over %d ranks", P);
        vector<vector<i64>> in(P);
        in[me] = out[me];
        if (P == 1) return in;
        vector<i64> mine(P);
        for (int q = 0; q < P; ++q) mine[q] = (i64)out[q].size();
        const vector<vector<i64>> sz = allgatherv(G_WORLD, mine); // sz[p][q]
        for (int p = 0; p < P; ++p)
            if (p != me) in[p].resize(sz[p][me]);
        if (host_mem) {
            for (int p = 0; p < P; ++p)
                for (int q = 0; q < P; ++q) {
                    if (p == q || !sz[p][q]) continue;
                    void *buf = me == p ? (void *)out[q].data() : me == q ? (void *)in[p].data() : nullptr;
                    section(G_WORLD, p, 1u << q, buf, (size_t)sz[p][q] * sizeof(i64));
                }
            flush();
            return in;
        }
        vector<i64> so(P + 1, 0), ro(P + 1, 0);
        for (int q = 0; q < P; ++q) {
            so[q + 1] = so[q] + (q == me ? 0 : sz[me][q]);
            ro[q + 1] = ro[q] + (q == me ? 0 : sz[q][me]);
        }
        DevBuf<i64> ds, dr;
        ds.alloc(std::max<i64>(so[P], 1));
        dr.alloc(std::max<i64>(ro[P], 1));
        for (int q = 0; q < P; ++q)
            if (q != me && sz[me][q])
                HIPCHK(hipMemcpy(ds.p + so[q], out[q].data(), sz[me][q] * sizeof(i64), hipMemcpyHostToDevice));
        for (int p = 0; p < P; ++p)
            for (int q = 0; q < P; ++q) {
                if (p == q || !sz[p][q]) continue;
                void *buf = me == p ? (void *)(ds.p + so[q]) : me == q ? (void *)(dr.p + ro[p]) : nullptr;
                section(G_WORLD, p, 1u << q, buf, (size_t)sz[p][q] * sizeof(i64));
            }
        flush();
        HIPCHK(hipStreamSynchronize(s));
        for (int p = 0; p < P; ++p)
            if (p != me && sz[p][me])
                HIPCHK(hipMemcpy(in[p].data(), dr.p + ro[p], sz[p][me] * sizeof(i64), hipMemcpyDeviceToHost));
        return in;
    }
    // plan-time all-gather of variable-length int64 blobs within group g
    vector<vector<i64>> allgatherv(int g, const vector<i64> &mine) {
        const int P = gsize(g), me = grank(g);
        vector<vector<i64>> out(P);
        if (P == 1) {
            out[0] = mine;
            return out;
        }
        if (host_mem) { // the same broadcasts over host buffers
            vector<i64> sz(P, 0);
            sz[me] = (i64)mine.size();
            for (int r = 0; r < P; ++r) bcast(g, r, &sz[r], sizeof(i64));
            flush();
            for (int r = 0; r < P; ++r) {
                out[r] = r == me ? mine : vector<i64>(sz[r]);
                bcast(g, r, out[r].data(), sz[r] * sizeof(i64));
            }
            flush();
            return out;
        }
        DevBuf<i64> dsz;
        dsz.alloc(P);
        vector<i64> sz(P, 0);
        sz[me] = (i64)mine.size();
        HIPCHK(hipMemcpy(dsz.p, sz.data(), P * sizeof(i64), hipMemcpyHostToDevice));
        for (int r = 0; r < P; ++r) bcast(g, r, dsz.p + r, sizeof(i64));
        flush();
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(sz.data(), dsz.p, P * sizeof(i64), hipMemcpyDeviceToHost));
        vector<i64> off(P + 1, 0);
        for (int r = 0; r < P; ++r) off[r + 1] = off[r] + sz[r];
        DevBuf<i64> d;
        d.alloc(std::max<i64>(off[P], 1));
        if (!mine.empty())
            HIPCHK(hipMemcpy(d.p + off[me], mine.data(), mine.size() * sizeof(i64),
                             hipMemcpyHostToDevice));
        for (int r = 0; r < P; ++r) bcast(g, r, d.p + off[r], sz[r] * sizeof(i64));
        flush();
        HIPCHK(hipStreamSynchronize(s));
        for (int r = 0; r < P; ++r) {
            out[r].resize(sz[r]);
            if (sz[r])
                HIPCHK(hipMemcpy(out[r].data(), d.p + off[r], sz[r] * sizeof(i64),
                                 hipMemcpyDeviceToHost));
        }
        return out;
    }
};

} // namespace slu
