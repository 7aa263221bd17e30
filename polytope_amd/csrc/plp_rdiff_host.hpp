// plp_rdiff_host.hpp -- the device side of plp_region_diff_search, private to plp_capi.hip (it reports through `fail` and
// `check_launch` of that unit): the backend plp_rdiff_search.hpp hands its sub-batches to.  Every list is a Chebyshev LP
// on a row subset of one table resident in HBM (plp_rdiff.hip), solved by the resident LP server through a host-mapped
// mailbox (d <= 4) or by a launch per batch.
#pragma once
#include "plp_hostcall.hpp"
#include "plp_rdiff_search.hpp"

namespace {

// the environment of one search, read once when it starts
struct RdiffEnv {
    bool server, wide, stats;
    unsigned srv_idle;   // empty mailbox polls (~2 us each) before the server retires
    // workgroups of the server (one wavefront each).  Measured at config 4 (751 batches, ~120 lists each): waiting for the
    // device 22.4 / 16.6 / 14.1 / 12.7 / 12.3 ms with 32 / 64 / 128 / 256 / 1024 (launch path: 4.3 ms of launches + 11.3)
    int srv_wgs;
    int wide_mind;       // (A/B: smallest d that takes the one-LP-per-wavefront kernel)
    // A/B knobs of the speculation (scripts/debug/rdiff_spec_sweep.sh).  Rounds 3-4 tuned it for the fewest
    // batches (SIB = 600, DEEP = 1: 751 batches of 89 724 LPs at config 4); the host pays ~50 ns per speculated list
    // (assembling + storing) and only 8 833 radii are ever read.  Measured: SIB = 100, DEEP = 0 -> 808 batches of 41 335
    // LPs, the call 21.2-23 -> 18.8-19.2 ms; no speculation beyond the chain (SIB = 0): 985 batches, 19.8-20.6 ms.
    plp::rdiff::Spec spec;
    RdiffEnv() {
        auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
        auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        server = !off("PLP_RDIFF_SERVER");
        wide = !off("PLP_RDIFF_WIDE");
        stats = getenv("PLP_RDIFF_STATS") != nullptr;
        srv_idle = (unsigned)num("PLP_RDIFF_SERVER_IDLE", 1500);
        srv_wgs = std::max(1, num("PLP_RDIFF_SERVER_WGS", 256));
        wide_mind = num("PLP_RDIFF_WIDE_MIND", 5);
        spec.sib = num("PLP_RDIFF_SPEC_SIB", spec.sib);
        spec.chain_scan = num("PLP_RDIFF_SPEC_CHAIN_SCAN", spec.chain_scan);
        spec.chain_node = num("PLP_RDIFF_SPEC_CHAIN_NODE", spec.chain_node);
        spec.deep = num("PLP_RDIFF_SPEC_DEEP", spec.deep);
        spec.child = num("PLP_RDIFF_SPEC_CHILD", spec.child);
    }
};

// the host-mapped block of the launch path: [off (n + 1) | sel (n) | rows (nr)] of a batch | radii | sequence word
constexpr size_t RD_CAP_LP = 1 << 15, RD_CAP_ROWS = RD_CAP_LP * 64;
constexpr size_t RD_RADII = (2 * RD_CAP_LP + 1 + RD_CAP_ROWS) * 4, RD_SEQ = RD_RADII + RD_CAP_LP * 8, RD_BYTES = RD_SEQ + 64;
// ... and of the server: mailbox word | "running" word (at 72) | (radius, batch word) per list | records by size class
constexpr size_t SRV_MAXLP = 2048, SRV_RUNNING = 72, SRV_OUT = 128, SRV_REC = SRV_OUT + SRV_MAXLP * 16;
constexpr size_t SRV_BYTES = SRV_REC + SRV_MAXLP * 66 * 4;
constexpr unsigned long long SRV_EXIT = ~0ull;

// the search's own codes (negative) in the library's words; the backend's (positive) come with their message set
static_assert(PLP_EINVAL > 0 && PLP_EUNSUPPORTED > 0 && PLP_EHIP > 0, "plp::rdiff::Err takes the negative codes");
inline int rdiff_fail(int code, int N, int too_long) {
    using namespace plp::rdiff;
    if (code == SCAN_MEMO) return fail(PLP_EUNSUPPORTED, "region_diff: a scan over %d cells does not fit the radius memo", N);
    if (code == RADIUS_MISSING) return fail(PLP_EHIP, "region_diff: the radius of the current node is missing after its batch");
    if (code == BAD_INDEX) return fail(PLP_EINVAL, "region_diff: row index out of range (the reference raises IndexError here)");
    if (code == LIST_TOO_LONG) return fail(PLP_EUNSUPPORTED, "region_diff: a row list of %d rows exceeds the staging buffer", too_long);
    return code;
}

struct RdiffBackend {
    using Clock = std::chrono::steady_clock;
    plp_ctx* ctx = nullptr;
    const RdiffEnv env;
    int d = 0;
    double *dA = nullptr, *dB = nullptr;
    unsigned long long seq = 0;
    bool srv_on = false, srv_running = false;
    long long n_lps = 0, n_batches = 0, n_srv_batches = 0, n_srv_starts = 0;
    long long n_lps_long = 0, n_batches_long = 0;   // LPs of more than 64 rows (LDS engine) / batches that hold at least one
    double t_launch = 0.0, t_wait = 0.0;            // seconds spent enqueueing / waiting for the device

    size_t cap_lp() const { return RD_CAP_LP; }
    size_t cap_rows() const { return RD_CAP_ROWS; }
    volatile unsigned long long* srv_word(size_t at) { return reinterpret_cast<volatile unsigned long long*>(ctx->rd_srv + at); }

    // a host-mapped, coherent block and a device buffer beside it, committed only when every call succeeded
    template <class T>
    static hipError_t alloc_mapped(size_t host_bytes, size_t dev_bytes, char*& host, char*& host_dev, T*& dev) {
        char *hp = nullptr, *hp_dev = nullptr;
        T* dp = nullptr;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&hp), host_bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&hp_dev), hp, 0);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dp), dev_bytes);
        if (e != hipSuccess) {
            if (hp) (void)hipHostFree(hp);
            (void)hipGetLastError();
            return e;
        }
        host = hp; host_dev = hp_dev; dev = dp;
        return hipSuccess;
    }
    int init(plp_ctx* c, int d_, long long nrows, const double* A, const double* b) {
        ctx = c; d = d_;
        if (!ctx->rd_pin) {
            // the kernels read the index block and publish the radii through it (no copies, no stream synchronisation per
            // batch: the host spins on a sequence word the last kernel of the batch raises)
            hipError_t e = alloc_mapped(RD_BYTES, RD_CAP_LP * 8, ctx->rd_pin, ctx->rd_pin_dev, ctx->rd_out);
            if (e != hipSuccess) return fail(PLP_EHIP, "region_diff: staging buffers: %s", hipGetErrorString(e));
            *reinterpret_cast<volatile unsigned long long*>(ctx->rd_pin + RD_SEQ) = 0ull;
            ctx->rd_seq = 0;
        }
        const size_t need = (size_t)nrows * (d + 1) * 8 + 64;
        if (need > ctx->rd_tab_bytes) {
            if (ctx->rd_tab) HIP_TRY(hipFree(ctx->rd_tab));
            ctx->rd_tab = nullptr;
            ctx->rd_tab_bytes = 0;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->rd_tab), need + need / 2));
            ctx->rd_tab_bytes = need + need / 2;
        }
        dA = ctx->rd_tab;
        dB = ctx->rd_tab + (size_t)nrows * d;
        seq = ctx->rd_seq;
        HIP_TRY(hipMemcpyAsync(dA, A, (size_t)nrows * d * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dB, b, (size_t)nrows * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (!env.server || d > 4) return PLP_OK;
        if (!ctx->rd_srv) {
            if (alloc_mapped(SRV_BYTES, 64, ctx->rd_srv, ctx->rd_srv_dev, ctx->rd_srv_state) != hipSuccess)
                return PLP_OK;   // no server: the launch path serves the search
            memset(ctx->rd_srv, 0, 128);
            ctx->rd_srv_seq = 0;
            ctx->rd_srv_word = 0;
        }
        srv_on = true;
        return PLP_OK;
    }
    void release() { if (ctx) { srv_stop(); (void)hipStreamSynchronize(ctx->stream); ctx->rd_seq = seq; } }
    // last: the mailbox word of the last batch that was answered.  pending: the next batch is in the mailbox already (the
    // server retired while it was on its way) -- the new server finds it there; else the mailbox says "nothing new".
    int srv_start(unsigned long long last, bool pending) {
        if (!pending) __atomic_store_n(srv_word(0), last, __ATOMIC_RELEASE);
        __atomic_store_n(srv_word(SRV_RUNNING), 1ull, __ATOMIC_RELEASE);
        ctx->rd_srv_init[0] = ctx->rd_srv_init[2] = ctx->rd_srv_init[3] = 0ull;   // word 0: "retire" flag
        ctx->rd_srv_init[1] = last;                                                // word 1: the mailbox as the device republishes it
        HIP_TRY(hipMemcpyAsync(ctx->rd_srv_state, ctx->rd_srv_init, 32, hipMemcpyHostToDevice, ctx->stream));
        if (plp::launch_rdiff_server(d, env.srv_wgs, reinterpret_cast<const unsigned long long*>(ctx->rd_srv_dev),
                                     reinterpret_cast<const int*>(ctx->rd_srv_dev + SRV_REC), ctx->rd_srv_dev + SRV_OUT,
                                     reinterpret_cast<unsigned long long*>(ctx->rd_srv_dev + SRV_RUNNING), ctx->rd_srv_state,
                                     dA, dB, last, env.srv_idle, ctx->stream))
            return fail(PLP_EUNSUPPORTED, "region_diff: no LP server for d=%d", d);
        int rc = check_launch("rdiff_server");
        if (rc) return rc;
        srv_running = true;
        ++n_srv_starts;
        return PLP_OK;
    }
    void srv_stop() {
        if (!srv_running) return;
        __atomic_store_n(srv_word(0), SRV_EXIT, __ATOMIC_RELEASE);
        (void)hipStreamSynchronize(ctx->stream);
        srv_running = false;
    }
    // size classes: 0 / 1 / 2 = lists of up to 16 / 32 / 64 rows on the lane-group kernels (d <= 4), 3 = beyond 64 rows
    // (LDS engine), 4 = d >= 5, up to 64 rows: one LP per wavefront (cheby_gather_w_kernel; PLP_RDIFF_WIDE=0: d = 5..8
    // on the lane groups, d >= 9 on the LDS engine)
    int cls_of(int len) const {
        if (len > 64) return 3;
        if (d >= env.wide_mind && env.wide) return 4;
        return d > 8 ? 3 : (len > 32 ? 2 : (len > 16 ? 1 : 0));
    }
    // one sub-batch of the search: list k = rows[off[k] .. off[k + 1]) -> its radius at radii[k * stride]
    int solve(const int32_t* off, const int32_t* rows, size_t n, const double** radii, size_t* stride) {
        int cnt[5] = {0, 0, 0, 0, 0}, max_len = 0;
        for (size_t k = 0; k < n; ++k) {
            const int len = off[k + 1] - off[k];
            max_len = len > max_len ? len : max_len;
            cnt[cls_of(len)]++;
        }
        const bool on_server = srv_on && n <= SRV_MAXLP && !cnt[3] && !cnt[4];
        int rc = on_server ? solve_on_server(off, rows, n, cnt) : solve_by_launch(off, rows, n, cnt, max_len);
        if (rc) return rc;
        *radii = reinterpret_cast<const double*>(on_server ? ctx->rd_srv + SRV_OUT : ctx->rd_pin + RD_RADII);
        *stride = on_server ? 2 : 1;
        n_lps += (long long)n;
        n_batches += 1;
        return PLP_OK;
    }
    // the resident server takes the batch: records by size class, header, sequence word; spin on the word beside each radius
    int solve_on_server(const int32_t* off, const int32_t* rows, size_t n, const int* cnt) {
        const auto tp0 = Clock::now();
        int32_t* rec = reinterpret_cast<int32_t*>(ctx->rd_srv + SRV_REC);
        int32_t* rc_[3] = {rec, rec + (size_t)cnt[0] * 18, rec + (size_t)cnt[0] * 18 + (size_t)cnt[1] * 34};
        static const int cap_[3] = {16, 32, 64};
        for (size_t k = 0; k < n; ++k) {
            const int len = off[k + 1] - off[k];
            const int c = cls_of(len);
            int32_t* r = rc_[c];
            r[0] = (int32_t)k;
            r[1] = len;
            memcpy(r + 2, rows + off[k], (size_t)len * 4);
            rc_[c] = r + cap_[c] + 2;
        }
        if (!srv_running || __atomic_load_n(srv_word(SRV_RUNNING), __ATOMIC_ACQUIRE) == 0ull) {
            if (srv_running) { (void)hipStreamSynchronize(ctx->stream); srv_running = false; }   // it retired (idle)
            int rc = srv_start(ctx->rd_srv_word, false);
            if (rc) return rc;
        }
        // one word: [batch number : 28 | n2 : 12 | n1 : 12 | n0 : 12] (never 0, never all ones)
        const unsigned long long last_word = ctx->rd_srv_word;
        ctx->rd_srv_seq = (ctx->rd_srv_seq % 0xffffff0ull) + 1ull;
        const unsigned long long sq = (ctx->rd_srv_seq << 36) | ((unsigned long long)cnt[2] << 24) |
                                      ((unsigned long long)cnt[1] << 12) | (unsigned long long)cnt[0];
        __atomic_store_n(srv_word(0), sq, __ATOMIC_RELEASE);
        const auto tp1 = Clock::now();
        // every radius arrives beside the batch's word (one 16-byte store of the lane group that solved it)
        const volatile unsigned long long* sres = srv_word(SRV_OUT);
        unsigned long long spins = 0;
        for (size_t k = 0; k < n;) {
            if (__atomic_load_n(&sres[2 * k + 1], __ATOMIC_ACQUIRE) == sq) { ++k; continue; }
            if ((++spins & 0x3fffull) == 0ull) {
                if (__atomic_load_n(srv_word(SRV_RUNNING), __ATOMIC_ACQUIRE) == 0ull) {
                    // the server retired while the batch was on its way (or part of it did the batch and part did
                    // not): start it again, it finds the batch in the mailbox and solves it (again)
                    (void)hipStreamSynchronize(ctx->stream);
                    int rc = srv_start(last_word, true);
                    if (rc) return rc;
                }
                if (spins > 4000000000ull) return fail(PLP_EHIP, "region_diff: the LP server did not answer batch %llu", sq);
            }
        }
        t_launch += std::chrono::duration<double>(tp1 - tp0).count();
        t_wait += std::chrono::duration<double>(Clock::now() - tp1).count();
        ctx->rd_srv_word = sq;
        n_srv_batches += 1;
        return PLP_OK;
    }
    // a launch per batch: one contiguous index block [off | sel | rows] the kernels read across PCIe, the lists selected
    // by size class, up to three gather launches, a publish kernel that raises the sequence word the host spins on
    int solve_by_launch(const int32_t* qoff, const int32_t* qrows, size_t n, const int* cnt, int max_len) {
        srv_stop();   // (the launches below queue behind it on the same stream)
        int32_t* off = reinterpret_cast<int32_t*>(ctx->rd_pin);
        int32_t* sel = off + n + 1;
        for (size_t k = 0; k <= n; ++k) off[k] = qoff[k] - qoff[0];
        memcpy(sel + n, qrows + qoff[0], (size_t)off[n] * 4);
        size_t start[5], fill[5];
        start[0] = fill[0] = 0;
        for (int c = 1; c < 5; ++c) start[c] = fill[c] = start[c - 1] + cnt[c - 1];
        for (size_t k = 0; k < n; ++k) sel[fill[cls_of(off[k + 1] - off[k])]++] = (int32_t)k;
        hipStream_t st = ctx->stream;
        const auto tp0 = Clock::now();
        const int32_t* d_off = reinterpret_cast<const int32_t*>(ctx->rd_pin_dev);
        const int32_t* d_sel = d_off + n + 1;
        const int32_t* d_rows = d_sel + n;
        double* dOut = ctx->rd_out;
        if ((cnt[0] | cnt[1] | cnt[2]) &&
            plp::launch_cheby_gather_r(d, cnt[0], cnt[1], cnt[2], d_off, d_rows, d_sel, dA, dB, dOut, st))
            return fail(PLP_EUNSUPPORTED, "region_diff: gather kernel does not apply (d=%d)", d);
        if (cnt[3] && plp::launch_cheby_gather_lds(d, max_len, cnt[3], d_off, d_rows, d_sel + start[3], dA, dB, dOut, st))
            return fail(PLP_EUNSUPPORTED, "region_diff: a stack of %d rows does not fit the LDS engine", max_len);
        if (cnt[4] && plp::launch_cheby_gather_w(d, cnt[4], d_off, d_rows, d_sel + start[4], dA, dB, dOut, st))
            return fail(PLP_EUNSUPPORTED, "region_diff: gather kernel does not apply (d=%d)", d);
        ++seq;
        plp::launch_rdiff_publish((long long)n, dOut, reinterpret_cast<double*>(ctx->rd_pin_dev + RD_RADII),
                                  reinterpret_cast<unsigned long long*>(ctx->rd_pin_dev + RD_SEQ), seq, st);
        int rc = check_launch("cheby_gather");
        if (rc) return rc;
        const auto tp1 = Clock::now();
        // spin on the sequence word (bounded: fall back to a stream synchronisation, which also reports errors)
        const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(ctx->rd_pin + RD_SEQ);
        unsigned long long spins = 0;
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
            if (++spins > 400000000ull) { HIP_TRY(hipStreamSynchronize(st)); break; }
        }
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
            HIP_TRY(hipStreamSynchronize(st));
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return fail(PLP_EHIP, "region_diff: batch %llu did not complete", seq);
        }
        t_launch += std::chrono::duration<double>(tp1 - tp0).count();
        t_wait += std::chrono::duration<double>(Clock::now() - tp1).count();
        n_lps_long += cnt[3];
        n_batches_long += cnt[3] ? 1 : 0;
        return PLP_OK;
    }
};

}  // namespace
