// plp_capi.hip -- extern "C" boundary of libplp_hip.so (declared in include/plp.h).
// Host-pointer entry points stage through a grow-only device scratch arena owned by the
// context, call the *_dev entry point on the context's stream and synchronise.
#include <initializer_list>

#include "plp_hostcall.hpp"
#include "plp_locate.hpp"
#include "plp_lp_plan.hpp"
#include "plp_pair_stack.hpp"

namespace {

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PLP_EHIP, "%s launch: %s", what, hipGetErrorString(e));
    return PLP_OK;
}

bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace

extern "C" {

int plp_version(void) { return 300; }  // 200: round 2 (LPs beyond 64 rows, plp_region_diff_search, plp_quickhull_run); 210: plp_ctx_set_check_finite, plp_bbox_batch for d <= 16; 300: round 3 (plp_reduce_wide_batch, F2 presolve)

int plp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int k = 0;
    for (int i = 0; i < n; ++i) k += is_gfx950(i) ? 1 : 0;
    return k;
}

const char* plp_last_error(void) { return g_err; }

int plp_ctx_create(int device, plp_ctx** out) {
    if (!out) return fail(PLP_EINVAL, "plp_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(PLP_ENODEVICE, "no HIP device visible");
    }
    if (device < 0 || device >= n) return fail(PLP_EINVAL, "device %d out of range [0,%d)", device, n);
    if (!is_gfx950(device)) return fail(PLP_ENODEVICE, "device %d is not gfx950 (MI355X)", device);
    HIP_TRY(hipSetDevice(device));
    plp_ctx* ctx = new plp_ctx();
    ctx->device = device;
    ctx->arena = nullptr;
    ctx->arena_bytes = 0;
    ctx->pin = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(PLP_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return PLP_OK;
}

int plp_ctx_set_check_finite(plp_ctx* ctx, int on) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    ctx->check_finite = on != 0;
    return PLP_OK;
}

int plp_ctx_destroy(plp_ctx* ctx) {
    if (!ctx) return PLP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->rd_pin) (void)hipHostFree(ctx->rd_pin);
    if (ctx->rd_srv) (void)hipHostFree(ctx->rd_srv);
    if (ctx->rd_srv_state) (void)hipFree(ctx->rd_srv_state);
    if (ctx->rd_out) (void)hipFree(ctx->rd_out);
    if (ctx->rd_tab) (void)hipFree(ctx->rd_tab);
    if (ctx->mf_buf) (void)hipFree(ctx->mf_buf);
    if (ctx->reduce_ctr) (void)hipFree(ctx->reduce_ctr);
    if (ctx->retry_ring) (void)hipFree(ctx->retry_ring);
    for (auto& kv : ctx->as_scratch) if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->vf_scratch) if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->vf_basis) if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : ctx->ps_scratch) if (kv.second.p) (void)hipFree(kv.second.p);
    if (ctx->mf_ev) (void)hipEventDestroy(ctx->mf_ev);
    if (ctx->hull_spare.full) {
        (void)hipFree(ctx->hull_spare.X); (void)hipFree(ctx->hull_spare.owner); (void)hipFree(ctx->hull_spare.dist);
        if (ctx->hull_spare.dead) (void)hipFree(ctx->hull_spare.dead);
        if (ctx->hull_spare.io) (void)hipFree(ctx->hull_spare.io);
        if (ctx->hull_spare.pin) (void)hipHostFree(ctx->hull_spare.pin);
    }
    delete ctx->pool;
    if (ctx->stage) (void)hipHostFree(ctx->stage);
    for (int i = 0; i < ctx->stage_nev; ++i) (void)hipEventDestroy(ctx->stage_ev[i]);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PLP_OK;
}

int plp_ctx_synchronize(plp_ctx* ctx, void* stream) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return PLP_OK;
}

// Every answer of the LP engines passes the verifier before it leaves the library (plp_verify.hip; PLP_VERIFY=0: A/B)
static int verify_lp_answers(plp_ctx* ctx, hipStream_t st, int64_t B, int m_max, int n, const double* c, const double* G,
                             const double* h, const int32_t* m, double* x, double* fun, int32_t* status) {
    if (!plp::verify_enabled()) return PLP_OK;
    void* sc = stream_buf(ctx->vf_scratch, (void*)st, plp::verify_scratch_bytes(B, m_max));
    if (!sc) return fail(PLP_EHIP, "verifier: no device memory for its scratch (%zu bytes)", plp::verify_scratch_bytes(B, m_max));
    if (plp::launch_verify_lp(B, m_max, n, c, G, h, m, x, fun, status, sc, (int)(ctx->vf_scratch[(void*)st].calls++ & 1u), st))
        return fail(PLP_EUNSUPPORTED, "verifier: unsupported size");
    return check_launch("verify_x_kernel");
}
static int verify_cheby_answers(plp_ctx* ctx, hipStream_t st, int64_t B, int m_max, int d, const double* A, const double* b,
                                const int32_t* m, double* r, double* xc, int32_t* status) {
    if (!plp::verify_enabled()) return PLP_OK;
    void* sc = stream_buf(ctx->vf_scratch, (void*)st, plp::verify_scratch_bytes(B, m_max));
    if (!sc) return fail(PLP_EHIP, "verifier: no device memory for its scratch (%zu bytes)", plp::verify_scratch_bytes(B, m_max));
    if (plp::launch_verify_cheby(B, m_max, d, A, b, m, r, xc, status, sc, (int)(ctx->vf_scratch[(void*)st].calls++ & 1u), st))
        return fail(PLP_EUNSUPPORTED, "verifier: unsupported size");
    return check_launch("verify_x_kernel");
}

int plp_verify_counters(plp_ctx* ctx, void* stream, int64_t* careful_lps) {
    if (!ctx || !careful_lps) return fail(PLP_EINVAL, "NULL pointer");
    *careful_lps = 0;
    auto it = ctx->vf_scratch.find(stream);
    if (it == ctx->vf_scratch.end()) {   // (host-pointer calls run on the context's own stream)
        stream = (void*)ctx->stream;
        it = ctx->vf_scratch.find(stream);
    }
    if (it == ctx->vf_scratch.end() || !it->second.p || it->second.calls == 0) return PLP_OK;   // nothing verified on this stream yet
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    // the list counter of the last launch: the two counters (64 B apart) are used in turn, the last call took (calls - 1) & 1
    unsigned cnt = 0;
    const char* base = static_cast<const char*>(it->second.p) + (((it->second.calls - 1) & 1u) ? 64 : 0);
    HIP_TRY(hipMemcpy(&cnt, base, sizeof(cnt), hipMemcpyDeviceToHost));
    *careful_lps = (int64_t)cnt;
    return PLP_OK;
}

// Each operation below: its argument checks, shared by the device-pointer entry point and its host-pointer twin (sizes,
// NULL pointers, then the envelope: all before a host buffer is read; rc == PLP_OK with an empty batch means "nothing to
// do"), the device-pointer entry point, and the host-pointer one on a HostCall.
// ------------------------------------------------------------------------------- lp_solve
static int check_lp(plp_ctx* ctx, int64_t B, int m_max, int n, const double* c, const double* G, const double* h,
                    const double* x, const double* fun, const int32_t* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || n < 1) return fail(PLP_EINVAL, "bad sizes B=%lld m_max=%d n=%d", (long long)B, m_max, n);
    if (B == 0) return PLP_OK;
    if (!c || !h || !x || !fun || !status || (!G && m_max > 0)) return fail(PLP_EINVAL, "NULL pointer");
    if (n > plp::MAX_D + 1 || (m_max > plp::MAX_M && !plp::lds_lp_bytes(m_max, n + 1)))
        return fail(PLP_EUNSUPPORTED, "m_max=%d n=%d outside envelope (n<=17; rows: the dictionary must fit 160 KB of LDS)", m_max, n);
    return PLP_OK;
}

int plp_lp_solve_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int n, const double* c,
                           const double* G, const double* h, const int32_t* m, double* x, double* fun,
                           int32_t* status, int32_t* iters) {
    int rc = check_lp(ctx, B, m_max, n, c, G, h, x, fun, status);
    if (rc || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream
    if (plp::launch_lp(B, m_max, n, c, G, h, m, x, fun, status, iters, st))
        return fail(PLP_EUNSUPPORTED, "lp kernel: unsupported size");
    rc = check_launch("lp_kernel");
    if (rc) return rc;
    return verify_lp_answers(ctx, st, B, m_max, n, c, G, h, m, x, fun, status);
}

int plp_lp_solve_batch(plp_ctx* ctx, int64_t B, int m_max, int n, const double* c, const double* G,
                       const double* h, const int32_t* m, double* x, double* fun, int32_t* status,
                       int32_t* iters) {
    int rc = check_lp(ctx, B, m_max, n, c, G, h, x, fun, status);
    if (rc || B == 0) return rc;
    const size_t nc = (size_t)B * n, mn = (size_t)m_max * n;
    double *dc, *dG, *dh, *dx, *dfun;
    int32_t *dm, *dst, *dit;
    HostCall hc(ctx);
    hc.in(dc, c, nc, n, true);
    hc.in(dG, G, (size_t)B * mn, mn, true);
    hc.in(dh, h, (size_t)B * m_max, m_max, true);
    hc.in(dm, m, B, 1);
    hc.out(dx, x, nc);
    hc.out(dfun, fun, B);
    hc.out(dst, status, B);
    hc.out(dit, iters, B);
    rc = hc.reserve();
    if (rc) return rc;
    hipStream_t st = hc.st;
    bool staged = false;  // large batches: chunked upload, kernels of earlier chunks running meanwhile (plp_stage.hpp)
    int more = 0;
    rc = hc.upload_staged(B, 64,
                          [&](int64_t lo, int64_t hi) {
                              return plp_lp_solve_batch_dev(ctx, st, hi - lo, m_max, n, dc, dG, dh, dm, dx + (size_t)lo * n,
                                                            dfun + lo, dst + lo, dit + lo);
                          },
                          &staged);
    if (rc) return rc;
    if (!staged) {
        rc = hc.upload();
        if (rc) return rc;
        // small batches: the fast kernels now; the general kernel only if a status, host-visible below anyway, asks for it
        if (B <= 16384 && !plp::verify_enabled()) {
            if (plp::launch_lp_phase(B, m_max, n, dc, dG, dh, dm, dx, dfun, dst, dit, st, 1, &more))
                return fail(PLP_EUNSUPPORTED, "lp kernel: unsupported size");
            rc = check_launch("lp_kernel");
        } else {  // (with the verifier behind the engines both passes are launched: it has to see final answers)
            rc = plp_lp_solve_batch_dev(ctx, st, B, m_max, n, dc, dG, dh, dm, dx, dfun, dst, dit);
        }
        if (rc) return rc;
    }
    rc = hc.download();
    if (rc || !more) return rc;
    bool again = false;
    for (int64_t k = 0; k < B && !again; ++k) again = status[k] == plp::ST_RETRY;
    if (!again) return PLP_OK;
    if (plp::launch_lp_phase(B, m_max, n, dc, dG, dh, dm, dx, dfun, dst, dit, st, 2, nullptr))
        return fail(PLP_EUNSUPPORTED, "lp kernel: unsupported size");
    rc = check_launch("lp_kernel");
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- cheby
// (cheby, bbox and reduce take the same inputs: `outs_ok` is the operation's own "no output pointer is NULL")
static int check_Abm(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, bool outs_ok) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (B > 0 && (!outs_ok || ((!A || !b) && m_max > 0))) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}

static int check_cheby(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const double* r,
                       const double* xc, const int32_t* status) {
    int rc = check_Abm(ctx, B, m_max, d, A, b, r && xc && status);
    if (rc || B == 0) return rc;
    if (d > plp::MAX_D || (m_max > plp::MAX_M && !plp::lds_lp_bytes(m_max, d + 1)))
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (d<=16; rows: the dictionary must fit 160 KB of LDS)", m_max, d);
    return PLP_OK;
}

int plp_cheby_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A,
                        const double* b, const int32_t* m, double* r, double* xc, int32_t* status) {
    int rc = check_cheby(ctx, B, m_max, d, A, b, r, xc, status);
    if (rc || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream
    if (plp::launch_cheby(B, m_max, d, A, b, m, r, xc, status, st))
        return fail(PLP_EUNSUPPORTED, "cheby kernel: unsupported size");
    rc = check_launch("cheby_kernel");
    if (rc) return rc;
    return verify_cheby_answers(ctx, st, B, m_max, d, A, b, m, r, xc, status);
}

int plp_cheby_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b,
                    const int32_t* m, double* r, double* xc, int32_t* status) {
    int rc = check_cheby(ctx, B, m_max, d, A, b, r, xc, status);
    if (rc || B == 0) return rc;
    double *dA, *db, *dr, *dxc;
    int32_t *dm, *dst;
    HostCall hc(ctx);
    declare_Abm(hc, B, m_max, d, dA, A, db, b, dm, m);
    hc.out(dr, r, B);
    hc.out(dxc, xc, (size_t)B * d);
    hc.out(dst, status, B);
    return run_Abm(hc, B, 64, [&](int64_t lo, int64_t hi) {
        return plp_cheby_batch_dev(ctx, hc.st, hi - lo, m_max, d, dA, db, dm, dr + lo, dxc + (size_t)lo * d, dst + lo);
    });
}

// ------------------------------------------------------------------------------- bounding box
static int check_bbox(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const double* lb,
                      const double* ub, const int32_t* status) {
    int rc = check_Abm(ctx, B, m_max, d, A, b, lb && ub && status);
    if (rc || B == 0) return rc;
    if (m_max > plp::MAX_M || d > plp::MAX_D)
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (m<=64, d<=16)", m_max, d);
    if (m_max < 1) return fail(PLP_EUNSUPPORTED, "bbox kernel: m_max=%d (needs m_max >= 1)", m_max);
    return PLP_OK;
}

int plp_bbox_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                       const int32_t* m, double* lb, double* ub, int32_t* status) {
    int rc = check_bbox(ctx, B, m_max, d, A, b, lb, ub, status);
    if (rc || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream
    // the verifier behind the fused kernels (plp_verify.hip): they hand over each box LP's final basis + the centre, or the
    // point the LP ended on; one buffer per stream: [bases 2 d d bytes | centres d doubles | points 2 d d doubles] per polytope
    plp::BoxHandover ho{nullptr, nullptr, nullptr};
    void* vsc = nullptr;
    int mode = 0;   // which of it the planned launch fills: 1 bases + centres, 2 points (the one-LP-per-lane form)
    if (plp::verify_enabled()) {
        mode = plp::plan_bbox(B, m_max, d, plp::lp_env()).handover;
        const size_t nb8 = ((size_t)B * 2 * d * d + 255) & ~(size_t)255, nct = (size_t)B * d * 8;
        const size_t nxf = mode == 2 ? (size_t)B * 2 * d * d * 8 : 0;
        char* hb = static_cast<char*>(stream_buf(ctx->vf_basis, stream, nb8 + nct + nxf + 256));
        vsc = stream_buf(ctx->vf_scratch, stream, plp::verify_scratch_bytes(B * 2 * d, m_max));
        if (!hb || !vsc) return fail(PLP_EHIP, "verifier: no device memory for its scratch");
        ho.basis8 = reinterpret_cast<signed char*>(hb);
        ho.centre = reinterpret_cast<double*>(hb + nb8);
        ho.xfin = mode == 2 ? reinterpret_cast<double*>(hb + nb8 + nct) : nullptr;
    }
    if (plp::launch_bbox(B, m_max, d, A, b, m, lb, ub, status, st, &ho))
        return fail(PLP_EUNSUPPORTED, "bbox kernel: unsupported size");
    rc = check_launch("bbox_r_kernel");
    if (rc || !mode) return rc;
    if (plp::launch_verify_box(B, m_max, d, A, b, m, lb, ub, status, mode == 1 ? ho.basis8 : nullptr,
                               mode == 1 ? ho.centre : nullptr, mode == 2 ? ho.xfin : nullptr, vsc,
                               (int)(ctx->vf_scratch[stream].calls++ & 1u), st))
        return fail(PLP_EUNSUPPORTED, "verifier: unsupported size");
    return check_launch("verify_box_kernel");
}

int plp_bbox_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                   double* lb, double* ub, int32_t* status) {
    int rc = check_bbox(ctx, B, m_max, d, A, b, lb, ub, status);
    if (rc || B == 0) return rc;
    double *dA, *db, *dlb, *dub;
    int32_t *dm, *dst;
    HostCall hc(ctx);
    declare_Abm(hc, B, m_max, d, dA, A, db, b, dm, m);
    hc.out(dlb, lb, (size_t)B * d);
    hc.out(dub, ub, (size_t)B * d);
    hc.out(dst, status, B);
    return run_Abm(hc, B, 64, [&](int64_t lo, int64_t hi) {
        return plp_bbox_batch_dev(ctx, hc.st, hi - lo, m_max, d, dA, db, dm, dlb + (size_t)lo * d, dub + (size_t)lo * d,
                                  dst + lo);
    });
}

// ------------------------------------------------------------------------------- reduce
static int check_reduce(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const uint64_t* keep,
                        const int32_t* flags, const double* r, const double* xc, const int32_t* nlp) {
    int rc = check_Abm(ctx, B, m_max, d, A, b, keep && flags && r && xc && nlp);
    if (rc || B == 0) return rc;
    if (m_max > plp::MAX_M || d > plp::MAX_D)
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (m<=64, d<=16)", m_max, d);
    return PLP_OK;
}

int plp_reduce_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A,
                         const double* b, const int32_t* m, double abs_tol, uint64_t* keep, int32_t* flags,
                         double* r, double* xc, int32_t* nlp) {
    int rc = check_reduce(ctx, B, m_max, d, A, b, keep, flags, r, xc, nlp);
    if (rc || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream
    if (!ctx->retry_ring) {
        if (hipMalloc(reinterpret_cast<void**>(&ctx->retry_ring), 64 * 8) == hipSuccess) {
            if (hipMemset(ctx->retry_ring, 0, 64 * 8) != hipSuccess) { (void)hipFree(ctx->retry_ring); ctx->retry_ring = nullptr; }
        } else {
            ctx->retry_ring = nullptr;
        }
        (void)hipGetLastError();
    }
    ctx->reduce_epoch += 1;
    const plp::ReduceArgs args{B, m_max, A, b, m, abs_tol, reinterpret_cast<unsigned long long*>(keep), flags, r, xc, nlp,
                               ctx->reduce_ctr, ctx->retry_ring ? ctx->retry_ring + (ctx->reduce_epoch & 63ull) : nullptr,
                               ctx->reduce_epoch};
    const int lrc = plp::launch_reduce(d, args, 0, st);
    if (lrc) return fail(PLP_EUNSUPPORTED, "reduce kernel: unsupported size");
    return check_launch("reduce_kernel");
}

int plp_reduce_counters(plp_ctx* ctx, void* stream, uint64_t* simplex_runs, int reset) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    constexpr size_t CTR_BYTES = (size_t)plp::PLP_CTR_SLOTS * 64;
    if (!ctx->reduce_ctr) {   // first call: from now on the kernels launched through this context count
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->reduce_ctr), CTR_BYTES));
        HIP_TRY(hipMemsetAsync(ctx->reduce_ctr, 0, CTR_BYTES, st));
    }
    std::vector<unsigned long long> host(CTR_BYTES / 8);
    HIP_TRY(hipMemcpyAsync(host.data(), ctx->reduce_ctr, CTR_BYTES, hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(hipMemsetAsync(ctx->reduce_ctr, 0, CTR_BYTES, st));
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long v = 0ull;   // (two's-complement partial sums: the total is what counts)
    for (int k = 0; k < plp::PLP_CTR_SLOTS; ++k) v += host[(size_t)k * 8];
    if (simplex_runs) *simplex_runs = (uint64_t)v;
    return PLP_OK;
}

int plp_reduce_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b,
                     const int32_t* m, double abs_tol, uint64_t* keep, int32_t* flags, double* r, double* xc,
                     int32_t* nlp) {
    int rc = check_reduce(ctx, B, m_max, d, A, b, keep, flags, r, xc, nlp);
    if (rc || B == 0) return rc;
    double *dA, *db, *dr, *dxc;
    int32_t *dm, *dfl, *dnlp;
    uint64_t* dkeep;
    HostCall hc(ctx);
    declare_Abm(hc, B, m_max, d, dA, A, db, b, dm, m);
    declare_reduce_outs(hc, B, d, 1, dkeep, keep, dfl, flags, dr, r, dxc, xc, dnlp, nlp);
    rc = hc.reserve();
    if (rc) return rc;
    hipStream_t st = hc.st;
    // large batches: chunked upload with the kernels of earlier chunks running meanwhile (tiles hold 16 polytopes)
    bool staged = false;
    rc = hc.upload_staged(B, 16,
                          [&](int64_t lo, int64_t hi) {
                              return plp_reduce_batch_dev(ctx, st, hi - lo, m_max, d, dA, db, dm, abs_tol, dkeep + lo, dfl + lo,
                                                          dr + lo, dxc + (size_t)lo * d, dnlp + lo);
                          },
                          &staged);
    if (rc) return rc;
    bool two_step = false;
    // (the two-step path counts no simplex runs and uses no retry word: null counter and word)
    const plp::ReduceArgs args{B, m_max, dA, db, dm, abs_tol, reinterpret_cast<unsigned long long*>(dkeep), dfl, dr,
                               dxc, dnlp, nullptr, nullptr, 0ull};
    if (!staged) {
        rc = hc.upload();
        if (rc) return rc;
        // small batches: only the first launch now; the pass that redoes polytopes flagged for the general engine runs
        // when the flags, host-visible below anyway, ask for it (it is a launch that normally finds nothing to do)
        two_step = B <= 16384;
        if (two_step) {
            if (plp::launch_reduce(d, args, 1, st))
                return fail(PLP_EUNSUPPORTED, "reduce kernel: unsupported size");
            rc = check_launch("reduce_kernel");
        } else {
            rc = plp_reduce_batch_dev(ctx, st, B, m_max, d, dA, db, dm, abs_tol, dkeep, dfl, dr, dxc, dnlp);
        }
        if (rc) return rc;
    }
    rc = hc.download();
    if (rc || !two_step) return rc;
    bool again = false;
    for (int64_t k = 0; k < B && !again; ++k) again = (flags[k] & plp::RF_RETRY) != 0;
    if (!again) return PLP_OK;
    if (plp::launch_reduce(d, args, 2, st))
        return fail(PLP_EUNSUPPORTED, "reduce kernel: unsupported size");
    rc = check_launch("reduce_kernel");
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- reduce beyond 64 rows
static int check_reduce_wide(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b,
                             const uint64_t* keep, const int32_t* flags, const double* r, const double* xc,
                             const int32_t* nlp) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 1 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (!keep || !flags || !r || !xc || !nlp || !A || !b) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    return PLP_OK;
}

int plp_reduce_wide_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A,
                              const double* b, const int32_t* m, double abs_tol, uint64_t* keep, int32_t* flags,
                              double* r, double* xc, int32_t* nlp) {
    int rc = check_reduce_wide(ctx, B, m_max, d, A, b, keep, flags, r, xc, nlp);
    if (rc || B == 0) return rc;
    if (m_max <= plp::MAX_M)  // one word per polytope: the register-resident kernels
        return plp_reduce_batch_dev(ctx, stream, B, m_max, d, A, b, m, abs_tol, keep, flags, r, xc, nlp);
    if (plp::launch_reduce_lds(B, m_max, d, A, b, m, abs_tol, reinterpret_cast<unsigned long long*>(keep), flags, r, xc,
                               nlp, (hipStream_t)stream))  // NULL = the HIP default stream
        return fail(PLP_EUNSUPPORTED, "reduce: a polytope of %d rows in dimension %d does not fit the LDS of a CU", m_max, d);
    return check_launch("reduce_lds_kernel");
}

int plp_reduce_wide_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, double abs_tol, uint64_t* keep, int32_t* flags, double* r, double* xc,
                          int32_t* nlp) {
    int rc = check_reduce_wide(ctx, B, m_max, d, A, b, keep, flags, r, xc, nlp);
    if (rc || B == 0) return rc;
    if (m_max <= plp::MAX_M) return plp_reduce_batch(ctx, B, m_max, d, A, b, m, abs_tol, keep, flags, r, xc, nlp);
    double *dA, *db, *dr, *dxc;
    int32_t *dm, *dfl, *dnlp;
    uint64_t* dkeep;
    HostCall hc(ctx);
    const size_t md = (size_t)m_max * d;
    hc.in(dA, A, (size_t)B * md, 0, true);  // (not staged: the LDS kernel's batches are small)
    hc.in(db, b, (size_t)B * m_max, 0, true);
    hc.in(dm, m, B);
    declare_reduce_outs(hc, B, d, (size_t)(m_max + 63) / 64, dkeep, keep, dfl, flags, dr, r, dxc, xc, dnlp, nlp);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_reduce_wide_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, abs_tol, dkeep, dfl, dr, dxc, dnlp);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- contains
static int check_contains(plp_ctx* ctx, int P, int m_max, int d, const double* A, const double* b, int64_t N,
                          const double* X, int mode, const uint8_t* out) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (P < 0 || m_max < 0 || d < 1 || N < 0 || (mode != 0 && mode != 1)) return fail(PLP_EINVAL, "bad sizes/mode");
    if (N == 0) return PLP_OK;
    if (!X || !out || ((!A || !b) && P > 0 && m_max > 0)) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    return PLP_OK;
}

int plp_contains_dev(plp_ctx* ctx, void* stream, int P, int m_max, int d, const double* A, const double* b,
                     const int32_t* m, int64_t N, const double* X, double abs_tol, int mode, uint8_t* out) {
    int rc = check_contains(ctx, P, m_max, d, A, b, N, X, mode, out);
    if (rc || N == 0) return rc;
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default stream
    // per-row thresholds: a grow-only buffer of the context, handed from stream to stream in order
    void* scratch = nullptr;
    if (P > 0 && m_max > 0) {
        const size_t need = plp::contains_scratch_bytes(P, m_max);
        if (!ctx->mf_ev && hipEventCreateWithFlags(&ctx->mf_ev, hipEventDisableTiming) != hipSuccess) {
            ctx->mf_ev = nullptr;
            (void)hipGetLastError();
        }
        if (need > ctx->mf_bytes) {
            // growing: the last launch that used the old buffer must have finished before it is freed (an event of
            // the context, not the caller's stream handle, which may no longer exist)
            if (ctx->mf_buf) {
                if (ctx->mf_used && ctx->mf_ev) (void)hipEventSynchronize(ctx->mf_ev);
                else if (ctx->mf_used) (void)hipDeviceSynchronize();
                (void)hipFree(ctx->mf_buf);
            }
            ctx->mf_buf = nullptr;
            ctx->mf_bytes = 0;
            ctx->mf_used = false;
            if (hipMalloc(&ctx->mf_buf, need + need / 4) == hipSuccess) ctx->mf_bytes = need + need / 4;
            else (void)hipGetLastError();
        } else if (ctx->mf_used) {
            // the previous user of the buffer may have run on another stream: order the streams on the device, the host
            // does not wait (a no-op when it is the same stream)
            if (ctx->mf_ev) HIP_TRY(hipStreamWaitEvent(st, ctx->mf_ev, 0));
            else (void)hipDeviceSynchronize();
        }
        if (ctx->mf_buf) scratch = ctx->mf_buf;
    }
    if (plp::launch_contains(P, m_max, d, A, b, m, N, X, abs_tol, mode, out, scratch, st))
        return fail(PLP_EUNSUPPORTED, "contains kernel: unsupported size");
    rc = check_launch("contains_kernel");
    if (scratch && rc == PLP_OK) {
        ctx->mf_used = true;
        if (ctx->mf_ev) HIP_TRY(hipEventRecord(ctx->mf_ev, st));
    }
    return rc;
}

int plp_contains(plp_ctx* ctx, int P, int m_max, int d, const double* A, const double* b, const int32_t* m,
                 int64_t N, const double* X, double abs_tol, int mode, uint8_t* out) {
    int rc = check_contains(ctx, P, m_max, d, A, b, N, X, mode, out);
    if (rc || N == 0) return rc;
    double *dA, *db, *dX;
    int32_t* dm;
    uint8_t* dout;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)P * m_max * d);
    hc.in(db, b, (size_t)P * m_max);
    hc.in(dm, m, P);
    hc.in(dX, X, (size_t)N * d);
    hc.out(dout, out, mode == 1 ? (size_t)P * N : (size_t)N);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_contains_dev(ctx, hc.st, P, m_max, d, dA, db, dm, N, dX, abs_tol, mode, dout);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- locate
namespace {
int grid_cells(const plp_locate_grid* g) {
    int G = 1;
    for (int j = 0; j < g->naxes; ++j) G *= g->res[j];
    return G;
}

int check_locate(plp_ctx* ctx, int P, int m_max, int d, const double* A, const double* b, int64_t N, const double* X,
                 const plp_locate_grid* grid, const int32_t* cell_start, const int32_t* cell_items, const int32_t* first) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (P < 0 || m_max < 0 || d < 1 || N < 0) return fail(PLP_EINVAL, "bad sizes");
    if (N == 0) return PLP_OK;
    if (!X || !first || ((!A || !b) && P > 0 && m_max > 0)) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    if (grid && P > 0 && !cell_start) return fail(PLP_EINVAL, "NULL pointer");
    (void)cell_items;  // (may be NULL: a grid without a single entry)
    return PLP_OK;
}

int check_locate_grid(plp_ctx* ctx, int P, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                      const int32_t* cell_start, const void* other) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (P < 0 || d < 1 || !(pad >= 0.0)) return fail(PLP_EINVAL, "bad sizes");
    if (!grid || !cell_start || !other || (P > 0 && (!lb || !ub))) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    return PLP_OK;
}
}  // namespace

int plp_locate_dev(plp_ctx* ctx, void* stream, int P, int m_max, int d, const double* A, const double* b, const int32_t* m,
                   int64_t N, const double* X, double abs_tol, const plp_locate_grid* grid, const int32_t* cell_start,
                   const int32_t* cell_items, int32_t* first, int32_t* count) {
    int rc = check_locate(ctx, P, m_max, d, A, b, N, X, grid, cell_start, cell_items, first);
    if (rc || N == 0) return rc;
    if (plp::launch_locate(P, m_max, d, A, b, m, N, X, abs_tol, grid, cell_start, cell_items, first, count, (hipStream_t)stream))
        return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");
    return check_launch("locate_kernel");
}

int plp_locate(plp_ctx* ctx, int P, int m_max, int d, const double* A, const double* b, const int32_t* m, int64_t N,
               const double* X, double abs_tol, const plp_locate_grid* grid, const int32_t* cell_start,
               const int32_t* cell_items, int32_t* first, int32_t* count) {
    int rc = check_locate(ctx, P, m_max, d, A, b, N, X, grid, cell_start, cell_items, first);
    if (rc || N == 0) return rc;
    if (grid && plp::loc::grid_bad(*grid, d))
        return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");  // (before cell_start[G] is read)
    const bool lists = grid && P > 0;
    const size_t G = lists ? (size_t)grid_cells(grid) : 0;
    const size_t items = lists ? (size_t)(cell_start[G] < 0 ? 0 : cell_start[G]) : 0;
    double *dA, *db, *dX;
    int32_t *dm, *dcs, *dci, *dfirst, *dcount;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)P * m_max * d);
    hc.in(db, b, (size_t)P * m_max);
    hc.in(dm, m, P);
    hc.in(dX, X, (size_t)N * d);
    hc.in(dcs, lists ? cell_start : nullptr, G + 1);
    hc.in(dci, lists && items ? cell_items : nullptr, items);
    hc.out(dfirst, first, (size_t)N);
    hc.out(dcount, count, count ? (size_t)N : 0);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_locate_dev(ctx, hc.st, P, m_max, d, dA, db, dm, N, dX, abs_tol, grid, dcs, dci, dfirst, count ? dcount : nullptr);
    if (rc) return rc;
    return hc.download();
}

int plp_locate_grid_count_dev(plp_ctx* ctx, void* stream, int P, int d, const double* lb, const double* ub, double pad,
                              const plp_locate_grid* grid, int32_t* cell_start, int32_t* max_len) {
    int rc = check_locate_grid(ctx, P, d, lb, ub, pad, grid, cell_start, max_len);
    if (rc) return rc;
    const int lr_count = plp::launch_locate_grid_count(P, d, lb, ub, pad, grid, cell_start, max_len, (hipStream_t)stream);
    if (lr_count == 3) return fail(PLP_EHIP, "locate grid: hipMemsetAsync failed");
    if (lr_count) return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");
    return check_launch("locate_grid_count_kernel");
}

int plp_locate_grid_count(plp_ctx* ctx, int P, int d, const double* lb, const double* ub, double pad,
                          const plp_locate_grid* grid, int32_t* cell_start, int32_t* max_len) {
    int rc = check_locate_grid(ctx, P, d, lb, ub, pad, grid, cell_start, max_len);
    if (rc) return rc;
    if (plp::loc::grid_bad(*grid, d))
        return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");
    double *dlb, *dub;
    int32_t *dcs, *dml;
    HostCall hc(ctx);
    hc.in(dlb, lb, (size_t)P * d);
    hc.in(dub, ub, (size_t)P * d);
    hc.out(dcs, cell_start, (size_t)grid_cells(grid) + 1);
    hc.out(dml, max_len, 1);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_locate_grid_count_dev(ctx, hc.st, P, d, dlb, dub, pad, grid, dcs, dml);
    if (rc) return rc;
    return hc.download();
}

int plp_locate_grid_fill_dev(plp_ctx* ctx, void* stream, int P, int d, const double* lb, const double* ub, double pad,
                             const plp_locate_grid* grid, const int32_t* cell_start, int32_t* cursor, int32_t* cell_items) {
    int rc = check_locate_grid(ctx, P, d, lb, ub, pad, grid, cell_start, cursor);
    if (rc) return rc;
    const int lr_fill = plp::launch_locate_grid_fill(P, d, lb, ub, pad, grid, cell_start, cursor, cell_items, (hipStream_t)stream);
    if (lr_fill == 3) return fail(PLP_EHIP, "locate grid: hipMemsetAsync failed");
    if (lr_fill) return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");
    return check_launch("locate_grid_fill_kernel");
}

// (host-pointer form: cursor may be NULL -- the scratch lives in the arena either way)
int plp_locate_grid_fill(plp_ctx* ctx, int P, int d, const double* lb, const double* ub, double pad,
                         const plp_locate_grid* grid, const int32_t* cell_start, int32_t* cursor, int32_t* cell_items) {
    int rc = check_locate_grid(ctx, P, d, lb, ub, pad, grid, cell_start, grid);
    if (rc) return rc;
    if (plp::loc::grid_bad(*grid, d))
        return fail(PLP_EINVAL, "bad sizes (locate: grid descriptor)");
    const size_t G = (size_t)grid_cells(grid);
    const size_t items = (size_t)(cell_start[G] < 0 ? 0 : cell_start[G]);
    if (items && !cell_items) return fail(PLP_EINVAL, "NULL pointer");
    double *dlb, *dub;
    int32_t *dcs, *dcur, *dci;
    HostCall hc(ctx);
    hc.in(dlb, lb, (size_t)P * d);
    hc.in(dub, ub, (size_t)P * d);
    hc.in(dcs, cell_start, G + 1);
    hc.out(dcur, (int32_t*)nullptr, G);
    hc.out(dci, cell_items, items);
    (void)cursor;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_locate_grid_fill_dev(ctx, hc.st, P, d, dlb, dub, pad, grid, dcs, dcur, dci);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- assign
static int check_assign(plp_ctx* ctx, int64_t N, int d, const double* X, int F, const double* normals,
                        const double* offsets, double abs_tol, const int32_t* fop, const double* dist,
                        const int64_t* argmax, const double* maxd) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (N < 0 || d < 1 || F < 1 || !(abs_tol >= 0.0)) return fail(PLP_EINVAL, "bad sizes (need F>=1, abs_tol>=0)");
    if (!normals || !offsets || !argmax || !maxd || (N > 0 && (!X || !fop || !dist)))
        return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    return PLP_OK;
}

int plp_assign_dev(plp_ctx* ctx, void* stream, int64_t N, int d, const double* X, int F, const double* normals,
                   const double* offsets, double abs_tol, int32_t* fop, double* dist, int64_t* argmax,
                   double* maxd) {
    int rc = check_assign(ctx, N, d, X, F, normals, offsets, abs_tol, fop, dist, argmax, maxd);
    if (rc) return rc;
    // few facets: the workgroups' partials (plp_ctx::as_scratch); without the buffer the general kernel takes the call
    const size_t need = plp::assign_scratch_bytes(N, F);
    void* scratch = need ? stream_buf(ctx->as_scratch, stream, need) : nullptr;
    if (plp::launch_assign(N, d, X, F, normals, offsets, abs_tol, fop, dist, reinterpret_cast<long long*>(argmax),
                           maxd, scratch, scratch ? ctx->as_scratch[stream].bytes : 0, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "assign kernel: unsupported size");
    return check_launch("assign_kernel");
}

int plp_assign(plp_ctx* ctx, int64_t N, int d, const double* X, int F, const double* normals,
               const double* offsets, double abs_tol, int32_t* fop, double* dist, int64_t* argmax, double* maxd) {
    int rc = check_assign(ctx, N, d, X, F, normals, offsets, abs_tol, fop, dist, argmax, maxd);
    if (rc) return rc;
    double *dX, *dn, *dof, *ddist, *dmx;
    int32_t* dfop;
    int64_t* dam;
    HostCall hc(ctx);
    hc.in(dX, X, (size_t)N * d);
    hc.in(dn, normals, (size_t)F * d);
    hc.in(dof, offsets, F);
    hc.out(dfop, fop, N);
    hc.out(ddist, dist, N);
    hc.out(dam, argmax, F);
    hc.out(dmx, maxd, F);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_assign_dev(ctx, hc.st, N, d, dX, F, dn, dof, abs_tol, dfop, ddist, dam, dmx);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- hull session
int plp_hull_reassign_dev(plp_ctx* ctx, void* stream, int64_t N, int d, const double* X, int32_t* owner, double* dist,
                          const uint8_t* dead, int new_id0, int n_new, const double* normals, const double* offsets,
                          double abs_tol, int64_t* argmax, double* maxd, int64_t* count) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (N < 0 || d < 1 || n_new < 1 || new_id0 < 0 || !(abs_tol >= 0.0))
        return fail(PLP_EINVAL, "bad sizes (need n_new>=1, new_id0>=0, abs_tol>=0)");
    if (!normals || !offsets || !argmax || !maxd || !count || (new_id0 > 0 && !dead) ||
        (N > 0 && (!X || !owner || !dist)))
        return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    if (plp::launch_hull_reassign(N, d, X, owner, dist, dead, new_id0, n_new, normals, offsets, abs_tol,
                                  reinterpret_cast<long long*>(argmax), maxd, reinterpret_cast<long long*>(count),
                                  (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "hull kernel: unsupported size");
    return check_launch("hull_reassign_kernel");
}

// ------------------------------------------------------------------------------- Fourier-Motzkin step
namespace {
int fm_check(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const uint64_t* keep, int kw,
             int col) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1 || (keep && kw < (m_max + 63) / 64)) return fail(PLP_EINVAL, "bad sizes");
    if (B > 0 && m_max > 0 && (!A || !b)) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    if (col >= d || (col >= 0 && d < 2)) return fail(PLP_EINVAL, "column %d of a polytope in dimension %d", col, d);
    if (plp::fm_lds_bytes(m_max, d) > 160 * 1024)
        return fail(PLP_EUNSUPPORTED, "fm: a polytope of %d rows in dimension %d does not fit the LDS of a CU", m_max, d);
    return PLP_OK;
}
}  // namespace

int plp_fm_count_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                     const int32_t* m, const uint64_t* keep, int kw, const int32_t* flags, int col, int first,
                     double abs_tol, int32_t* count) {
    int rc = fm_check(ctx, B, m_max, d, A, b, keep, kw, col);
    if (rc) return rc;
    if (B == 0) return PLP_OK;
    if (!count) return fail(PLP_EINVAL, "NULL pointer");
    if (plp::launch_fm(0, B, m_max, d, A, b, m, reinterpret_cast<const unsigned long long*>(keep), kw, flags, col, first,
                       abs_tol, count, 0, nullptr, nullptr, nullptr, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "fm: unsupported size");
    return check_launch("fm_kernel (count)");
}

int plp_fm_emit_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                    const int32_t* m, const uint64_t* keep, int kw, const int32_t* flags, int col, int first,
                    double abs_tol, int mo_max, double* A_out, double* b_out, int32_t* m_out) {
    int rc = fm_check(ctx, B, m_max, d, A, b, keep, kw, col);
    if (rc) return rc;
    if (B == 0) return PLP_OK;
    if (mo_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (!m_out || (mo_max > 0 && (!A_out || !b_out))) return fail(PLP_EINVAL, "NULL pointer");
    if (plp::launch_fm(1, B, m_max, d, A, b, m, reinterpret_cast<const unsigned long long*>(keep), kw, flags, col, first,
                       abs_tol, nullptr, mo_max, A_out, b_out, m_out, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "fm: unsupported size");
    return check_launch("fm_kernel (emit)");
}

namespace {
// the host-pointer pair: inputs staged through the arena, outputs copied back (count: mo_max < 0)
int fm_host(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
            const uint64_t* keep, int kw, const int32_t* flags, int col, int first, double abs_tol, int32_t* count,
            int mo_max, double* A_out, double* b_out, int32_t* m_out) {
    int rc = fm_check(ctx, B, m_max, d, A, b, keep, kw, col);
    if (rc) return rc;
    if (B == 0) return PLP_OK;
    const int dout = col >= 0 ? d - 1 : d;
    const size_t mo = mo_max > 0 ? (size_t)mo_max : 0;
    double *dA, *db, *dAo = nullptr, *dbo = nullptr;
    int32_t *dm, *dfl, *dout_n;
    uint64_t* dk;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d);
    hc.in(db, b, (size_t)B * m_max);
    hc.in(dm, m, B);
    hc.in(dk, keep, keep ? (size_t)B * kw : 0);
    hc.in(dfl, flags, B);
    hc.out(dout_n, count ? count : m_out, B);
    if (!count) {
        hc.out(dAo, A_out, (size_t)B * mo * dout);
        hc.out(dbo, b_out, (size_t)B * mo);
    }
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    if (count) rc = plp_fm_count_dev(ctx, hc.st, B, m_max, d, dA, db, dm, dk, kw, dfl, col, first, abs_tol, dout_n);
    else rc = plp_fm_emit_dev(ctx, hc.st, B, m_max, d, dA, db, dm, dk, kw, dfl, col, first, abs_tol, mo_max, dAo, dbo, dout_n);
    if (rc) return rc;
    return hc.download();
}
}  // namespace

int plp_fm_count(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                 const uint64_t* keep, int kw, const int32_t* flags, int col, int first, double abs_tol, int32_t* count) {
    if (!count && B > 0) return fail(PLP_EINVAL, "NULL pointer");
    return fm_host(ctx, B, m_max, d, A, b, m, keep, kw, flags, col, first, abs_tol, count, -1, nullptr, nullptr, nullptr);
}

int plp_fm_emit(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                const uint64_t* keep, int kw, const int32_t* flags, int col, int first, double abs_tol, int mo_max,
                double* A_out, double* b_out, int32_t* m_out) {
    if (mo_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B > 0 && (!m_out || (mo_max > 0 && (!A_out || !b_out)))) return fail(PLP_EINVAL, "NULL pointer");
    return fm_host(ctx, B, m_max, d, A, b, m, keep, kw, flags, col, first, abs_tol, nullptr, mo_max, A_out, b_out, m_out);
}

// ------------------------------------------------------------------------------- Monte-Carlo volume
namespace {
int volume_check(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const double* lb,
                 const double* ub, const uint64_t* state, const uint64_t* inc, int64_t N, const uint32_t* hits,
                 const int32_t* flags) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (N < 1 || N > 0x7fffffffll) return fail(PLP_EINVAL, "volume: N=%lld samples, need 1 <= N <= 2^31 - 1", (long long)N);
    if (B > 0 && (!lb || !ub || !state || !inc || !hits || !flags || (m_max > 0 && (!A || !b))))
        return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    if (m_max > plp::MAX_M) return fail(PLP_EUNSUPPORTED, "volume: m_max=%d > 64 rows", m_max);
    return PLP_OK;
}
}  // namespace

int plp_volume_hits_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                        const int32_t* m, const double* lb, const double* ub, const uint64_t* state, const uint64_t* inc,
                        int64_t N, uint32_t* hits, int32_t* flags) {
    int rc = volume_check(ctx, B, m_max, d, A, b, lb, ub, state, inc, N, hits, flags);
    if (rc) return rc;
    if (B == 0) return PLP_OK;
    if (plp::launch_volume_hits(B, m_max, d, A, b, m, lb, ub, reinterpret_cast<const unsigned long long*>(state),
                                reinterpret_cast<const unsigned long long*>(inc), N, hits, flags, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "volume: unsupported size");
    return check_launch("volume_hits_kernel");
}

int plp_volume_hits(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                    const double* lb, const double* ub, const uint64_t* state, const uint64_t* inc, int64_t N,
                    uint32_t* hits, int32_t* flags) {
    int rc = volume_check(ctx, B, m_max, d, A, b, lb, ub, state, inc, N, hits, flags);
    if (rc) return rc;
    if (B == 0) return PLP_OK;
    const size_t nd = (size_t)B * d;
    double *dA, *db, *dlb, *dub;
    int32_t *dm, *dfl;
    uint64_t *dst, *din;
    uint32_t* dh;
    HostCall hc(ctx);
    // (a box may hold +-inf: those polytopes come back flagged, so the arrays are not checked for finiteness here)
    hc.in(dA, A, (size_t)B * m_max * d);
    hc.in(db, b, (size_t)B * m_max);
    hc.in(dm, m, B);
    hc.in(dlb, lb, nd);
    hc.in(dub, ub, nd);
    hc.in(dst, state, (size_t)B * 2);
    hc.in(din, inc, (size_t)B * 2);
    hc.out(dh, hits, B);
    hc.out(dfl, flags, B);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_volume_hits_dev(ctx, hc.st, B, m_max, d, dA, db, dm, dlb, dub, dst, din, N, dh, dfl);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- the shared-row kernels
namespace {
// the arguments every entry of the family checks (plp_row_tile.hpp): `what` the call, `items` its K things per polytope;
// need: the pointers that may not be NULL
int shared_row_check(const char* what, const char* items, plp_ctx* ctx, int64_t B, int m_max, int d, const double* A,
                     const double* b, int K, std::initializer_list<const void*> need) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (d > 4 || m_max > plp::MAX_M)
        return fail(PLP_EUNSUPPORTED, "%s: m_max=%d d=%d outside the shared-row kernel (m<=64, d<=4)", what, m_max, d);
    if (K < 1) return fail(PLP_EUNSUPPORTED, "%s: K=%d %s (needs K >= 1)", what, K, items);
    if (B > 2147483647ll / K) return fail(PLP_EUNSUPPORTED, "%s: B * K exceeds 2^31 - 1", what);
    bool null = m_max > 0 && (!A || !b);
    for (const void* q : need) null = null || !q;
    return null ? fail(PLP_EINVAL, "NULL pointer") : PLP_OK;
}
}  // namespace

// ------------------------------------------------------------------------------- support functions
int plp_support_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, int K, const double* C, int c_shared, const double* xc, double* val, double* x,
                          int32_t* status) {
    int rc = shared_row_check("support", "directions", ctx, B, m_max, d, A, b, K, {C, xc, val, status});
    if (rc || B == 0) return rc;
    if (plp::launch_support(B, m_max, d, A, b, m, K, C, c_shared, xc, val, x, status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "support: unsupported size");
    return check_launch("support_kernel");
}

int plp_support_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m, int K,
                      const double* C, int c_shared, const double* xc, double* val, double* x, int32_t* status) {
    int rc = shared_row_check("support", "directions", ctx, B, m_max, d, A, b, K, {C, xc, val, status});
    if (rc || B == 0) return rc;
    const size_t lps = (size_t)B * K;
    double *dA, *db, *dC, *dxc, *dval, *dx;
    int32_t *dm, *dst;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d, 0, true);
    hc.in(db, b, (size_t)B * m_max, 0, true);
    hc.in(dm, m, B);
    hc.in(dC, C, (c_shared ? (size_t)K : lps) * d, 0, true);
    hc.in(dxc, xc, (size_t)B * d);   // (a centre may be NaN: that polytope comes back as status 1)
    hc.out(dval, val, lps);
    hc.out(dx, x, x ? lps * d : 0);
    hc.out(dst, status, lps);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_support_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, K, dC, c_shared, dxc, dval, x ? dx : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- nearest points
int plp_nearest_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, int K, const double* X, int x_shared, double* dist, double* x, uint64_t* face,
                          double* lam, int32_t* status) {
    int rc = shared_row_check("nearest", "points", ctx, B, m_max, d, A, b, K, {X, dist, status});
    if (rc || B == 0) return rc;
    if (plp::launch_nearest(B, m_max, d, A, b, m, K, X, x_shared, dist, x, (unsigned long long*)face, lam, status,
                            (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "nearest: unsupported size");
    return check_launch("nearest_kernel");
}

int plp_nearest_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m, int K,
                      const double* X, int x_shared, double* dist, double* x, uint64_t* face, double* lam, int32_t* status) {
    int rc = shared_row_check("nearest", "points", ctx, B, m_max, d, A, b, K, {X, dist, status});
    if (rc || B == 0) return rc;
    const size_t n = (size_t)B * K;
    double *dA, *db, *dX, *ddist, *dx, *dlam;
    uint64_t* dface;
    int32_t *dm, *dst;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d, 0, true);
    hc.in(db, b, (size_t)B * m_max, 0, true);
    hc.in(dm, m, B);
    hc.in(dX, X, (x_shared ? (size_t)K : n) * d, 0, true);
    hc.out(ddist, dist, n);
    hc.out(dx, x, x ? n * d : 0);
    hc.out(dface, face, face ? n : 0);
    hc.out(dlam, lam, lam ? n * d : 0);
    hc.out(dst, status, n);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_nearest_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, K, dX, x_shared, ddist, x ? dx : nullptr,
                               face ? dface : nullptr, lam ? dlam : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- distances of listed cell pairs
namespace {
int pair_dist_check(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const double* xc, int64_t K,
                    const int32_t* pairs, const double* dist, const int32_t* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (n < 0 || K < 0 || m_max < 0 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (n == 0 || K == 0) return PLP_OK;
    if (d > 4 || m_max > plp::MAX_M)
        return fail(PLP_EUNSUPPORTED, "pair_dist: m_max=%d d=%d outside the shared-row kernel (m<=64, d<=4)", m_max, d);
    if (K > 2147483647ll) return fail(PLP_EUNSUPPORTED, "pair_dist: K exceeds 2^31 - 1");
    if ((m_max > 0 && (!A || !b)) || !xc || !pairs || !dist || !status) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}
}  // namespace

// (no scratch: the kernel keeps its state in registers and LDS, so there is nothing per stream to reserve)
int plp_pair_dist_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                      const double* xc, int64_t K, const int32_t* pairs, double* dist, double* lb, double* x, double* y,
                      int32_t* status) {
    int rc = pair_dist_check(ctx, n, m_max, d, A, b, xc, K, pairs, dist, status);
    if (rc || n == 0 || K == 0) return rc;
    if (plp::launch_pair_dist(n, m_max, d, A, b, m, xc, K, pairs, dist, lb, x, y, status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "pair_dist: unsupported size");
    return check_launch("pair_dist_kernel");
}

int plp_pair_dist(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m, const double* xc,
                  int64_t K, const int32_t* pairs, double* dist, double* lb, double* x, double* y, int32_t* status) {
    int rc = pair_dist_check(ctx, n, m_max, d, A, b, xc, K, pairs, dist, status);
    if (rc || n == 0 || K == 0) return rc;
    for (int64_t t = 0; t < K; ++t) {
        const int32_t i = pairs[2 * t], j = pairs[2 * t + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j)
            return fail(PLP_EINVAL, "pair %lld = (%d, %d): indices must be two different cells of [0, %d)", (long long)t, i, j, n);
    }
    const size_t kd = (size_t)K * d;
    double *dA, *db, *dxc, *ddist, *dlb, *dx, *dy;
    int32_t *dm, *dpairs, *dst;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)n * m_max * d, 0, true);
    hc.in(db, b, (size_t)n * m_max, 0, true);
    hc.in(dm, m, n);
    hc.in(dxc, xc, (size_t)n * d);   // (a centre may be NaN: its pairs come back as status 1)
    hc.in(dpairs, pairs, (size_t)K * 2);
    hc.out(ddist, dist, K);
    hc.out(dlb, lb, lb ? K : 0);
    hc.out(dx, x, x ? kd : 0);
    hc.out(dy, y, y ? kd : 0);
    hc.out(dst, status, K);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_pair_dist_dev(ctx, hc.st, n, m_max, d, dA, db, dm, dxc, K, dpairs, ddist, lb ? dlb : nullptr, x ? dx : nullptr,
                           y ? dy : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- vertex enumeration
namespace {
int extreme_check(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, int v_max, const double* V,
                  const int32_t* count, const int32_t* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (d > 4 || m_max > plp::MAX_M)
        return fail(PLP_EUNSUPPORTED, "extreme: m_max=%d d=%d outside the enumeration kernel (m<=64, d<=4)", m_max, d);
    if (v_max < 1) return fail(PLP_EINVAL, "extreme: v_max=%d (needs v_max >= 1)", v_max);
    if (B > 2147483647ll) return fail(PLP_EUNSUPPORTED, "extreme: B exceeds 2^31 - 1");
    if (!V || !count || !status || (m_max > 0 && (!A || !b))) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}
}  // namespace

int plp_extreme_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, const uint64_t* keep, int v_max, double* V, int32_t* count, int32_t* basis,
                          int32_t* status) {
    int rc = extreme_check(ctx, B, m_max, d, A, b, v_max, V, count, status);
    if (rc || B == 0) return rc;
    if (plp::launch_extreme(B, m_max, d, A, b, m, reinterpret_cast<const unsigned long long*>(keep), v_max, V, count, basis,
                            status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "extreme: unsupported size");
    return check_launch("extreme_kernel");
}

int plp_extreme_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                      const uint64_t* keep, int v_max, double* V, int32_t* count, int32_t* basis, int32_t* status) {
    int rc = extreme_check(ctx, B, m_max, d, A, b, v_max, V, count, status);
    if (rc || B == 0) return rc;
    const size_t slots = (size_t)B * v_max * d;
    double *dA, *db, *dV;
    int32_t *dm, *dcount, *dbasis, *dst;
    uint64_t* dkeep;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d, 0, true);
    hc.in(db, b, (size_t)B * m_max, 0, true);
    hc.in(dm, m, B);
    hc.in(dkeep, keep, B);
    hc.out(dV, V, slots);
    hc.out(dcount, count, B);
    hc.out(dbasis, basis, basis ? slots : 0);
    hc.out(dst, status, B);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_extreme_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, dkeep, v_max, dV, dcount, basis ? dbasis : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- facet enumeration
namespace {
int hull_enum_check(plp_ctx* ctx, int64_t B, int n_max, int d, const double* X, int f_max, const double* Ao, const double* bo,
                    const uint64_t* on, const int32_t* count, const int32_t* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || n_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (d < 1 || d > 4 || n_max > plp::MAX_M)
        return fail(PLP_EUNSUPPORTED, "hull: n_max=%d d=%d outside the enumeration kernel (n<=64, 1<=d<=4)", n_max, d);
    if (f_max < 1) return fail(PLP_EINVAL, "hull: f_max=%d (needs f_max >= 1)", f_max);
    if (B > 2147483647ll) return fail(PLP_EUNSUPPORTED, "hull: B=%lld exceeds 2^31 - 1", (long long)B);
    if (!Ao || !bo || !on || !count || !status || (n_max > 0 && !X)) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}
}  // namespace

int plp_hull_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int n_max, int d, const double* X, const int32_t* n,
                       const uint64_t* keep, int f_max, double* Ao, double* bo, uint64_t* on, int32_t* count, int32_t* basis,
                       int32_t* status) {
    int rc = hull_enum_check(ctx, B, n_max, d, X, f_max, Ao, bo, on, count, status);
    if (rc || B == 0) return rc;
    if (plp::launch_hull_enum(B, n_max, d, X, n, reinterpret_cast<const unsigned long long*>(keep), f_max, Ao, bo,
                              reinterpret_cast<unsigned long long*>(on), count, basis, status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "hull: unsupported size");
    return check_launch("hull_enum_kernel");
}

int plp_hull_batch(plp_ctx* ctx, int64_t B, int n_max, int d, const double* X, const int32_t* n, const uint64_t* keep, int f_max,
                   double* Ao, double* bo, uint64_t* on, int32_t* count, int32_t* basis, int32_t* status) {
    int rc = hull_enum_check(ctx, B, n_max, d, X, f_max, Ao, bo, on, count, status);
    if (rc || B == 0) return rc;
    const size_t slots = (size_t)B * f_max;
    double *dX, *dA, *db;
    int32_t *dn, *dcount, *dbasis, *dst;
    uint64_t *dkeep, *don;
    HostCall hc(ctx);
    hc.in(dX, X, (size_t)B * n_max * d, 0, true);
    hc.in(dn, n, B);
    hc.in(dkeep, keep, B);
    hc.out(dA, Ao, slots * d);
    hc.out(db, bo, slots);
    hc.out(don, on, slots);
    hc.out(dcount, count, B);
    hc.out(dbasis, basis, basis ? slots * d : 0);
    hc.out(dst, status, B);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_hull_batch_dev(ctx, hc.st, B, n_max, d, dX, dn, dkeep, f_max, dA, db, don, dcount, basis ? dbasis : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- exact volume
namespace {
int volume_exact_check(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const double* volume,
                       const int32_t* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (d < 1 || d > 4 || m_max > plp::MAX_M)
        return fail(PLP_EUNSUPPORTED, "volume_exact: m_max=%d d=%d outside the kernel (m<=64, 1<=d<=4)", m_max, d);
    if (B > 2147483647ll) return fail(PLP_EUNSUPPORTED, "volume_exact: B=%lld exceeds 2^31 - 1", (long long)B);
    if (!volume || !status || (m_max > 0 && (!A || !b))) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}
}  // namespace

int plp_vol_exact_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                               const int32_t* m, const uint64_t* keep, const double* xc, const double* scale, double* volume,
                               double* area, int32_t* status) {
    int rc = volume_exact_check(ctx, B, m_max, d, A, b, volume, status);
    if (rc || B == 0) return rc;
    if (plp::launch_volume_exact(B, m_max, d, A, b, m, reinterpret_cast<const unsigned long long*>(keep), xc, scale, volume, area,
                                 status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "volume_exact: unsupported size");
    return check_launch("volume_exact_kernel");
}

int plp_vol_exact_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                           const uint64_t* keep, const double* xc, const double* scale, double* volume, double* area,
                           int32_t* status) {
    int rc = volume_exact_check(ctx, B, m_max, d, A, b, volume, status);
    if (rc || B == 0) return rc;
    double *dA, *db, *dxc, *dscale, *dvol, *darea;
    int32_t *dm, *dst;
    uint64_t* dkeep;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d, 0, true);
    hc.in(db, b, (size_t)B * m_max, 0, true);
    hc.in(dm, m, B);
    hc.in(dkeep, keep, B);
    hc.in(dxc, xc, (size_t)B * d, 0, true);
    hc.in(dscale, scale, B, 0, true);
    hc.out(dvol, volume, B);
    hc.out(darea, area, area ? (size_t)B * m_max : 0);
    hc.out(dst, status, B);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_vol_exact_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, dkeep, dxc, dscale, dvol, area ? darea : nullptr, dst);
    if (rc) return rc;
    return hc.download();
}

}  // extern "C"

struct plp_hull {
    plp_ctx* ctx;
    int64_t N;
    int d;
    double* X;
    int32_t* owner;
    double* dist;
    size_t X_bytes, owner_bytes, dist_bytes;   // capacities (buffers may come from the context's spare set)
    uint8_t* dead;     // one byte per facet id handed out so far (grow-only)
    size_t dead_cap;
    int next_id;       // next facet id to hand out
    // Per-call staging, grow-only: one device block and its pinned host mirror with the layout
    // [dead ids | normals | offsets | argmax | maxd | count] (reassign) or [point indices] (drop), so that a
    // call is one H2D copy, its kernels and one D2H copy.  (Pageable copies of a few hundred bytes cost
    // 30-50 us each and made an iteration of quickhull 0.4 ms.)
    char* io;
    char* pin;
    size_t io_bytes;
    bool pending;      // an asynchronous drop still reads `pin`
};

namespace {

int hull_ensure(plp_hull* h, size_t ids_needed, size_t io_needed) {
    if (ids_needed > h->dead_cap) {
        size_t want = h->dead_cap ? h->dead_cap : 4096;
        while (want < ids_needed) want *= 2;
        uint8_t* nd = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&nd), want));
        HIP_TRY(hipMemsetAsync(nd, 0, want, h->ctx->stream));
        if (h->dead) {
            HIP_TRY(hipMemcpyAsync(nd, h->dead, h->dead_cap, hipMemcpyDeviceToDevice, h->ctx->stream));
            HIP_TRY(hipStreamSynchronize(h->ctx->stream));
            HIP_TRY(hipFree(h->dead));
        }
        h->dead = nd;
        h->dead_cap = want;
    }
    if (io_needed > h->io_bytes) {
        HIP_TRY(hipStreamSynchronize(h->ctx->stream));
        h->pending = false;
        if (h->io) HIP_TRY(hipFree(h->io));
        if (h->pin) HIP_TRY(hipHostFree(h->pin));
        h->io = nullptr;
        h->pin = nullptr;
        h->io_bytes = 0;
        const size_t want = io_needed * 2 + 4096;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->io), want));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->pin), want, hipHostMallocDefault));
        h->io_bytes = want;
    }
    return PLP_OK;
}

}  // namespace

extern "C" {

int plp_hull_destroy(plp_hull* h) {
    if (!h) return PLP_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    plp_ctx::HullSpare& sp = h->ctx->hull_spare;
    if (!sp.full && h->X && h->owner && h->dist) {   // park the buffers for the next session of this context
        sp.X = h->X; sp.owner = h->owner; sp.dist = h->dist; sp.dead = h->dead; sp.io = h->io; sp.pin = h->pin;
        sp.X_bytes = h->X_bytes; sp.owner_bytes = h->owner_bytes; sp.dist_bytes = h->dist_bytes;
        sp.dead_cap = h->dead_cap; sp.io_bytes = h->io_bytes;
        sp.full = true;
        delete h;
        return PLP_OK;
    }
    if (h->X) (void)hipFree(h->X);
    if (h->owner) (void)hipFree(h->owner);
    if (h->dist) (void)hipFree(h->dist);
    if (h->dead) (void)hipFree(h->dead);
    if (h->io) (void)hipFree(h->io);
    if (h->pin) (void)hipHostFree(h->pin);
    delete h;
    return PLP_OK;
}

int plp_hull_create(plp_ctx* ctx, int64_t N, int d, const double* X, plp_hull** out) {
    if (!out) return fail(PLP_EINVAL, "plp_hull_create: out is NULL");
    *out = nullptr;
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (N < 0 || d < 1 || (N > 0 && !X)) return fail(PLP_EINVAL, "bad sizes / NULL points");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    HIP_TRY(hipSetDevice(ctx->device));
    plp_hull* h = new plp_hull();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    h->N = N;
    h->d = d;
    h->next_id = 1;  // id 0: the virtual facet owning every point (owner[] is zero-filled)
    const size_t n1 = N > 0 ? (size_t)N : 1;
    hipError_t e = hipSuccess;
    plp_ctx::HullSpare& sp = ctx->hull_spare;
    if (sp.full && sp.X_bytes >= n1 * d * 8 && sp.owner_bytes >= n1 * 4 && sp.dist_bytes >= n1 * 8) {
        h->X = sp.X; h->owner = sp.owner; h->dist = sp.dist; h->dead = sp.dead; h->io = sp.io; h->pin = sp.pin;
        h->X_bytes = sp.X_bytes; h->owner_bytes = sp.owner_bytes; h->dist_bytes = sp.dist_bytes;
        h->dead_cap = sp.dead_cap; h->io_bytes = sp.io_bytes;
        sp = plp_ctx::HullSpare();
        if (h->dead) e = hipMemsetAsync(h->dead, 0, h->dead_cap, ctx->stream);   // no facet id is dead yet
    } else {
        h->X_bytes = n1 * d * 8; h->owner_bytes = n1 * 4; h->dist_bytes = n1 * 8;
        e = hipMalloc(reinterpret_cast<void**>(&h->X), h->X_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->owner), h->owner_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->dist), h->dist_bytes);
    }
    if (e == hipSuccess) e = hipMemsetAsync(h->owner, 0, n1 * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->dist, 0, n1 * 8, ctx->stream);
    if (e == hipSuccess && N > 0) e = hipMemcpyAsync(h->X, X, (size_t)N * d * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        plp_hull_destroy(h);
        return fail(PLP_EHIP, "plp_hull_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return PLP_OK;
}

// asynchronous: ordered before the next call of this session on the context's stream
int plp_hull_drop(plp_hull* h, int64_t n, const int64_t* idx) {
    if (!h) return fail(PLP_EINVAL, "hull is NULL");
    if (n < 0 || (n > 0 && !idx)) return fail(PLP_EINVAL, "bad index list");
    if (n == 0) return PLP_OK;
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= h->N) return fail(PLP_EINVAL, "point index %lld out of range", (long long)idx[i]);
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    if (h->pending) {  // the previous drop may not have consumed the pinned block yet
        HIP_TRY(hipStreamSynchronize(st));
        h->pending = false;
    }
    int rc = hull_ensure(h, 0, (size_t)n * 8);
    if (rc) return rc;
    memcpy(h->pin, idx, (size_t)n * 8);
    HIP_TRY(hipMemcpyAsync(h->io, h->pin, (size_t)n * 8, hipMemcpyHostToDevice, st));
    plp::launch_hull_drop(n, reinterpret_cast<const long long*>(h->io), h->owner, st);
    rc = check_launch("hull_drop_kernel");
    if (rc) return rc;
    h->pending = true;
    return PLP_OK;
}

int plp_hull_reassign(plp_hull* h, int n_dead, const int32_t* dead_ids, int n_new, const double* normals,
                      const double* offsets, double abs_tol, int32_t* new_id0, int64_t* argmax, double* maxd,
                      int64_t* count) {
    if (!h) return fail(PLP_EINVAL, "hull is NULL");
    if (n_dead < 0 || n_new < 1 || !(abs_tol >= 0.0)) return fail(PLP_EINVAL, "bad sizes (need n_new>=1, abs_tol>=0)");
    if ((n_dead > 0 && !dead_ids) || !normals || !offsets || !new_id0 || !argmax || !maxd || !count)
        return fail(PLP_EINVAL, "NULL pointer");
    for (int i = 0; i < n_dead; ++i)
        if (dead_ids[i] < 0 || dead_ids[i] >= h->next_id)
            return fail(PLP_EINVAL, "dead facet id %d was never handed out", dead_ids[i]);
    if ((long long)h->next_id + n_new > 0x7fffffffll) return fail(PLP_EUNSUPPORTED, "facet ids exhausted");
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    if (h->pending) {
        HIP_TRY(hipStreamSynchronize(st));
        h->pending = false;
    }
    const int id0 = h->next_id;
    const int d = h->d;
    const size_t b_ids = pad((size_t)(n_dead ? n_dead : 1) * 4), b_n = pad((size_t)n_new * d * 8),
                 b_f = pad((size_t)n_new * 8);
    const size_t in_bytes = b_ids + b_n + b_f, out_bytes = 3 * b_f;
    int rc = hull_ensure(h, (size_t)id0 + n_new, in_bytes + out_bytes);
    if (rc) return rc;
    memcpy(h->pin, dead_ids, (size_t)n_dead * 4);
    memcpy(h->pin + b_ids, normals, (size_t)n_new * d * 8);
    memcpy(h->pin + b_ids + b_n, offsets, (size_t)n_new * 8);
    HIP_TRY(hipMemcpyAsync(h->io, h->pin, in_bytes, hipMemcpyHostToDevice, st));
    int32_t* d_ids = reinterpret_cast<int32_t*>(h->io);
    double* d_n = reinterpret_cast<double*>(h->io + b_ids);
    double* d_o = reinterpret_cast<double*>(h->io + b_ids + b_n);
    int64_t* d_am = reinterpret_cast<int64_t*>(h->io + in_bytes);
    double* d_mx = reinterpret_cast<double*>(h->io + in_bytes + b_f);
    int64_t* d_cn = reinterpret_cast<int64_t*>(h->io + in_bytes + 2 * b_f);
    plp::launch_hull_mark(n_dead, d_ids, h->dead, st);
    rc = plp_hull_reassign_dev(h->ctx, st, h->N, d, h->X, h->owner, h->dist, h->dead, id0, n_new, d_n, d_o, abs_tol,
                               d_am, d_mx, d_cn);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->pin + in_bytes, h->io + in_bytes, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(argmax, h->pin + in_bytes, (size_t)n_new * 8);
    memcpy(maxd, h->pin + in_bytes + b_f, (size_t)n_new * 8);
    memcpy(count, h->pin + in_bytes + 2 * b_f, (size_t)n_new * 8);
    h->next_id = id0 + n_new;
    *new_id0 = id0;
    return PLP_OK;
}

int plp_hull_read(plp_hull* h, int32_t* owner, double* dist) {
    if (!h) return fail(PLP_EINVAL, "hull is NULL");
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    if (owner && h->N) HIP_TRY(hipMemcpyAsync(owner, h->owner, (size_t)h->N * 4, hipMemcpyDeviceToHost, st));
    if (dist && h->N) HIP_TRY(hipMemcpyAsync(dist, h->dist, (size_t)h->N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->pending = false;
    return PLP_OK;
}

}  // extern "C"

extern "C" {

// ------------------------------------------------------------------------------- adjacency
// The four pair operations share their checks (`bad_counts` / `empty`: the operation's own conditions on its cell counts)
static int check_pairs(plp_ctx* ctx, bool bad_counts, bool empty, int m_max, int d, const double* A, const double* b,
                       const uint8_t* out) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (bad_counts || m_max < 1 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (empty) return PLP_OK;
    if (!A || !b || !out) return fail(PLP_EINVAL, "NULL pointer");
    if (2 * m_max > plp::MAX_M || d > plp::MAX_D)
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)", m_max, d);
    return PLP_OK;
}

static int check_cross(plp_ctx* ctx, int n1, int n2, int m_max, int d, const double* A, const double* b, const uint8_t* out) {
    int rc = check_pairs(ctx, n1 < 0 || n2 < 0, n1 == 0 || n2 == 0, m_max, d, A, b, out);
    if (rc == PLP_OK && (long long)n1 + n2 > 2147483647ll) return fail(PLP_EUNSUPPORTED, "too many cells");
    return rc;
}

// (`validate_empty`: the device-pointer call checks an empty range against the pair count like any other; the host-pointer
// call accepts it wherever it lies, it reads nothing)
static int check_pair_range(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, int64_t pair_lo,
                            int64_t pair_hi, const uint8_t* out, bool validate_empty) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (n < 0 || m_max < 1 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (pair_lo == pair_hi && !validate_empty) return PLP_OK;
    const int64_t npairs = (int64_t)n * (n - 1) / 2;
    if (pair_lo < 0 || pair_hi > npairs || pair_lo > pair_hi)
        return fail(PLP_EINVAL, "pair range [%lld, %lld) outside [0, %lld)", (long long)pair_lo, (long long)pair_hi,
                    (long long)npairs);
    if (pair_lo == pair_hi) return PLP_OK;
    if (!A || !b || !out) return fail(PLP_EINVAL, "NULL pointer");
    if (2 * m_max > plp::MAX_M || d > plp::MAX_D)
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)", m_max, d);
    return PLP_OK;
}

// the scratch of the pair calls' careful pass (plp_verify.hip: launch_careful_pairs); nullptr, no such pass, with PLP_VERIFY=0
static int pair_scratch(plp_ctx* ctx, void* stream, void** sc) {
    *sc = nullptr;
    if (!plp::verify_enabled()) return PLP_OK;
    *sc = stream_buf(ctx->vf_scratch, stream, plp::pair_careful_scratch_bytes());
    if (!*sc) return fail(PLP_EHIP, "pair LPs: no device memory for the careful pass (%zu bytes)", plp::pair_careful_scratch_bytes());
    return PLP_OK;
}

int plp_adjacent_pairs_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b,
                           const int32_t* m, double abs_tol, uint8_t* adj) {
    int rc = check_pairs(ctx, n < 0, n == 0, m_max, d, A, b, adj);
    if (rc || n == 0) return rc;
    void* sc;
    if ((rc = pair_scratch(ctx, stream, &sc))) return rc;
    if (plp::launch_adjacent(n, m_max, d, A, b, m, abs_tol, abs_tol / 10, adj, 0, 0, nullptr, (hipStream_t)stream, 0, sc))
        return fail(PLP_EUNSUPPORTED, "adjacent kernel: unsupported size");
    return check_launch("adjacent_r_kernel");
}

int plp_overlap_pairs_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, double abs_tol, uint8_t* out) {
    int rc = check_pairs(ctx, n < 0, n == 0, m_max, d, A, b, out);
    if (rc || n == 0) return rc;
    void* sc;
    if ((rc = pair_scratch(ctx, stream, &sc))) return rc;
    if (plp::launch_adjacent(n, m_max, d, A, b, m, 0.0, abs_tol, out, 0, 0, nullptr, (hipStream_t)stream, 0, sc))
        return fail(PLP_EUNSUPPORTED, "adjacent kernel: unsupported size");
    return check_launch("adjacent_r_kernel");
}

int plp_overlap_cross_dev(plp_ctx* ctx, void* stream, int n1, int n2, int m_max, int d, const double* A, const double* b,
                          const int32_t* m, double thresh, uint8_t* out) {
    int rc = check_cross(ctx, n1, n2, m_max, d, A, b, out);
    if (rc || n1 == 0 || n2 == 0) return rc;
    void* sc;
    if ((rc = pair_scratch(ctx, stream, &sc))) return rc;
    if (plp::launch_adjacent(n1 + n2, m_max, d, A, b, m, 0.0, thresh, nullptr, 0, (long long)n1 * n2, out,
                             (hipStream_t)stream, n1, sc))
        return fail(PLP_EUNSUPPORTED, "adjacent kernel: unsupported size");
    return check_launch("adjacent_r_kernel");
}

int plp_adjacent_pairs_range_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A,
                                 const double* b, const int32_t* m, double abs_tol, int64_t pair_lo,
                                 int64_t pair_hi, uint8_t* out) {
    int rc = check_pair_range(ctx, n, m_max, d, A, b, pair_lo, pair_hi, out, true);
    if (rc || pair_lo == pair_hi) return rc;
    void* sc;
    if ((rc = pair_scratch(ctx, stream, &sc))) return rc;
    if (plp::launch_adjacent(n, m_max, d, A, b, m, abs_tol, abs_tol / 10, nullptr, pair_lo, pair_hi, out,
                             (hipStream_t)stream, 0, sc))
        return fail(PLP_EUNSUPPORTED, "adjacent kernel: unsupported size");
    return check_launch("adjacent_r_kernel");
}

int plp_adjacent_pairs(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                       double abs_tol, uint8_t* adj) {
    int rc = check_pairs(ctx, n < 0, n == 0, m_max, d, A, b, adj);
    if (rc || n == 0) return rc;
    return pairs_host(ctx, n, m_max, d, A, b, m, adj, (size_t)n * n,
                      [&](hipStream_t st, const double* dA, const double* db, const int32_t* dm, uint8_t* dadj) {
                          return plp_adjacent_pairs_dev(ctx, st, n, m_max, d, dA, db, dm, abs_tol, dadj);
                      });
}

int plp_overlap_pairs(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                      double abs_tol, uint8_t* out) {
    int rc = check_pairs(ctx, n < 0, n == 0, m_max, d, A, b, out);
    if (rc || n == 0) return rc;
    return pairs_host(ctx, n, m_max, d, A, b, m, out, (size_t)n * n,
                      [&](hipStream_t st, const double* dA, const double* db, const int32_t* dm, uint8_t* dout) {
                          return plp_overlap_pairs_dev(ctx, st, n, m_max, d, dA, db, dm, abs_tol, dout);
                      });
}

int plp_overlap_cross(plp_ctx* ctx, int n1, int n2, int m_max, int d, const double* A, const double* b, const int32_t* m,
                      double thresh, uint8_t* out) {
    int rc = check_cross(ctx, n1, n2, m_max, d, A, b, out);
    if (rc || n1 == 0 || n2 == 0) return rc;
    return pairs_host(ctx, (size_t)n1 + n2, m_max, d, A, b, m, out, (size_t)n1 * n2,
                      [&](hipStream_t st, const double* dA, const double* db, const int32_t* dm, uint8_t* dout) {
                          return plp_overlap_cross_dev(ctx, st, n1, n2, m_max, d, dA, db, dm, thresh, dout);
                      });
}

int plp_adjacent_pairs_range(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b,
                             const int32_t* m, double abs_tol, int64_t pair_lo, int64_t pair_hi, uint8_t* out) {
    int rc = check_pair_range(ctx, n, m_max, d, A, b, pair_lo, pair_hi, out, false);
    if (rc || pair_lo == pair_hi) return rc;
    return pairs_host(ctx, n, m_max, d, A, b, m, out, (size_t)(pair_hi - pair_lo),
                      [&](hipStream_t st, const double* dA, const double* db, const int32_t* dm, uint8_t* dout) {
                          return plp_adjacent_pairs_range_dev(ctx, st, n, m_max, d, dA, db, dm, abs_tol, pair_lo, pair_hi,
                                                              dout);
                      });
}

// ------------------------------------------------------------------------------- listed pairs, box pairs
static int check_pair_list(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, int64_t K,
                           const int32_t* pairs, const uint8_t* out) {
    int rc = check_pairs(ctx, n < 0 || K < 0, K == 0, m_max, d, A, b, out);
    if (rc == PLP_OK && K > 0 && !pairs) return fail(PLP_EINVAL, "NULL pointer");
    return rc;
}

int plp_pair_list_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                      double inflate, double thresh, int64_t K, const int32_t* pairs, uint8_t* out) {
    int rc = check_pair_list(ctx, n, m_max, d, A, b, K, pairs, out);
    if (rc || K == 0) return rc;
    void* sc;
    if ((rc = pair_scratch(ctx, stream, &sc))) return rc;
    if (plp::launch_pair_list(n, m_max, d, A, b, m, inflate, thresh, K, pairs, out, (hipStream_t)stream, sc))
        return fail(PLP_EUNSUPPORTED, "adjacent kernel: unsupported size");
    return check_launch("adjacent_r_list_kernel");
}

int plp_pair_list(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m, double inflate,
                  double thresh, int64_t K, const int32_t* pairs, uint8_t* out) {
    int rc = check_pair_list(ctx, n, m_max, d, A, b, K, pairs, out);
    if (rc || K == 0) return rc;
    for (int64_t t = 0; t < K; ++t) {
        const int32_t i = pairs[2 * t], j = pairs[2 * t + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j)
            return fail(PLP_EINVAL, "pair %lld = (%d, %d): indices must be two different cells of [0, %d)", (long long)t, i, j, n);
    }
    double *dA, *db;
    int32_t *dm, *dpairs;
    uint8_t* dout;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)n * m_max * d);
    hc.in(db, b, (size_t)n * m_max);
    hc.in(dm, m, n);
    hc.in(dpairs, pairs, (size_t)K * 2);
    hc.out(dout, out, (size_t)K);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_pair_list_dev(ctx, hc.st, n, m_max, d, dA, db, dm, inflate, thresh, K, dpairs, dout);
    if (rc) return rc;
    return hc.download();
}

static int check_box_pairs(plp_ctx* ctx, int n, int d, const double* lb, const double* ub, double pad,
                           const plp_locate_grid* grid, const int32_t* cell_start, int n1, const void* out) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (n < 0 || d < 1 || n1 < 0 || n1 > n || !(pad >= 0.0)) return fail(PLP_EINVAL, "bad sizes");
    if (!out || (n > 0 && (!lb || !ub)) || (grid && n > 0 && !cell_start)) return fail(PLP_EINVAL, "NULL pointer");
    if (d > plp::MAX_D) return fail(PLP_EUNSUPPORTED, "d=%d > 16", d);
    if (grid && plp::loc::grid_bad(*grid, d)) return fail(PLP_EINVAL, "bad sizes (box pairs: grid descriptor)");
    return PLP_OK;
}

int plp_box_pairs_count_dev(plp_ctx* ctx, void* stream, int n, int d, const double* lb, const double* ub, double pad,
                            const plp_locate_grid* grid, const int32_t* cell_start, const int32_t* cell_items, int n1,
                            int64_t* per_cell) {
    int rc = check_box_pairs(ctx, n, d, lb, ub, pad, grid, cell_start, n1, per_cell);
    if (rc) return rc;
    const int lr = plp::launch_box_pairs_count(n, d, lb, ub, pad, grid, cell_start, cell_items, n1, (long long*)per_cell,
                                               (hipStream_t)stream);
    if (lr == 3) return fail(PLP_EHIP, "box pairs: hipMemsetAsync failed");
    if (lr) return fail(PLP_EINVAL, "bad sizes (box pairs)");
    return check_launch("box_pairs_kernel");
}

int plp_box_pairs_fill_dev(plp_ctx* ctx, void* stream, int n, int d, const double* lb, const double* ub, double pad,
                           const plp_locate_grid* grid, const int32_t* cell_start, const int32_t* cell_items, int n1,
                           const int64_t* per_cell, int cell_lo, int cell_hi, int32_t* pairs) {
    int rc = check_box_pairs(ctx, n, d, lb, ub, pad, grid, cell_start, n1, per_cell);
    if (rc) return rc;
    if (cell_lo < 0 || cell_hi > n || cell_lo > cell_hi) return fail(PLP_EINVAL, "bad sizes (box pairs: cell range)");
    if (cell_lo == cell_hi) return PLP_OK;
    if (!pairs) return fail(PLP_EINVAL, "NULL pointer");
    if (plp::launch_box_pairs_fill(n, d, lb, ub, pad, grid, cell_start, cell_items, n1, (const long long*)per_cell, cell_lo,
                                   cell_hi, pairs, (hipStream_t)stream))
        return fail(PLP_EINVAL, "bad sizes (box pairs)");
    return check_launch("box_pairs_kernel");
}

// (host-pointer forms: the lists are read up to cell_start[G], as plp_locate reads them)
int plp_box_pairs_count(plp_ctx* ctx, int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                        const int32_t* cell_start, const int32_t* cell_items, int n1, int64_t* per_cell) {
    int rc = check_box_pairs(ctx, n, d, lb, ub, pad, grid, cell_start, n1, per_cell);
    if (rc) return rc;
    const bool lists = grid && n > 0;
    const size_t G = lists ? (size_t)grid_cells(grid) : 0;
    const size_t items = lists ? (size_t)(cell_start[G] < 0 ? 0 : cell_start[G]) : 0;
    if (items && !cell_items) return fail(PLP_EINVAL, "NULL pointer");
    double *dlb, *dub;
    int32_t *dcs, *dci;
    int64_t* dpc;
    HostCall hc(ctx);
    hc.in(dlb, lb, (size_t)n * d);
    hc.in(dub, ub, (size_t)n * d);
    hc.in(dcs, lists ? cell_start : nullptr, G + 1);
    hc.in(dci, items ? cell_items : nullptr, items);
    hc.out(dpc, per_cell, (size_t)n + 1);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_box_pairs_count_dev(ctx, hc.st, n, d, dlb, dub, pad, grid, dcs, dci, n1, dpc);
    if (rc) return rc;
    return hc.download();
}

int plp_box_pairs_fill(plp_ctx* ctx, int n, int d, const double* lb, const double* ub, double pad, const plp_locate_grid* grid,
                       const int32_t* cell_start, const int32_t* cell_items, int n1, const int64_t* per_cell, int cell_lo,
                       int cell_hi, int32_t* pairs) {
    int rc = check_box_pairs(ctx, n, d, lb, ub, pad, grid, cell_start, n1, per_cell);
    if (rc) return rc;
    if (cell_lo < 0 || cell_hi > n || cell_lo > cell_hi) return fail(PLP_EINVAL, "bad sizes (box pairs: cell range)");
    const int64_t K = per_cell[cell_hi] - per_cell[cell_lo];
    if (K < 0) return fail(PLP_EINVAL, "bad sizes (box pairs: per_cell decreases)");
    if (K == 0) return PLP_OK;
    if (!pairs) return fail(PLP_EINVAL, "NULL pointer");
    const bool lists = grid != nullptr;
    const size_t G = lists ? (size_t)grid_cells(grid) : 0;
    const size_t items = lists ? (size_t)(cell_start[G] < 0 ? 0 : cell_start[G]) : 0;
    if (items && !cell_items) return fail(PLP_EINVAL, "NULL pointer");
    double *dlb, *dub;
    int32_t *dcs, *dci, *dpairs;
    int64_t* dpc;
    HostCall hc(ctx);
    hc.in(dlb, lb, (size_t)n * d);
    hc.in(dub, ub, (size_t)n * d);
    hc.in(dcs, lists ? cell_start : nullptr, G + 1);
    hc.in(dci, items ? cell_items : nullptr, items);
    hc.in(dpc, per_cell, (size_t)n + 1);
    hc.out(dpairs, pairs, (size_t)K * 2);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_box_pairs_fill_dev(ctx, hc.st, n, d, dlb, dub, pad, grid, dcs, dci, n1, dpc, cell_lo, cell_hi, dpairs);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- stacks and intersections of listed pairs
static int check_pair_stacks(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, int64_t K,
                             const int32_t* pairs, bool outs_ok) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (n < 0 || K < 0 || m_max < 1 || d < 1) return fail(PLP_EINVAL, "bad sizes");
    if (2 * m_max > plp::MAX_M || d > plp::MAX_D)   // (also for an empty list: the sizes are wrong whatever K is)
        return fail(PLP_EUNSUPPORTED, "m_max=%d d=%d outside envelope (2*m_max<=64, d<=16)", m_max, d);
    if (K == 0) return PLP_OK;
    if (!pairs || !outs_ok || (n > 0 && (!A || !b))) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}

static int check_listed(int n, int64_t K, const int32_t* pairs) {
    const long long t = plp::ps::host_first_bad(n, K, pairs);
    if (t >= 0)
        return fail(PLP_EINVAL, "pair %lld = (%d, %d): indices must be two different cells of [0, %d)", t, pairs[2 * t],
                    pairs[2 * t + 1], n);
    return PLP_OK;
}

int plp_pair_stacks_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                        int64_t K, const int32_t* pairs, double* A_s, double* b_s, int32_t* m_s) {
    int rc = check_pair_stacks(ctx, n, m_max, d, A, b, K, pairs, A_s && b_s && m_s);
    if (rc || K == 0) return rc;
    if (plp::launch_pair_stacks(n, m_max, d, A, b, m, K, pairs, A_s, b_s, m_s, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "pair stacks: unsupported size");
    return check_launch("pair_stack_kernel");
}

int plp_pair_stacks(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m, int64_t K,
                    const int32_t* pairs, double* A_s, double* b_s, int32_t* m_s) {
    int rc = check_pair_stacks(ctx, n, m_max, d, A, b, K, pairs, A_s && b_s && m_s);
    if (rc || K == 0) return rc;
    if ((rc = check_listed(n, K, pairs))) return rc;
    const size_t W = 2 * (size_t)m_max;
    double *dA, *db, *dAs, *dbs;
    int32_t *dm, *dpairs, *dms;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)n * m_max * d);
    hc.in(db, b, (size_t)n * m_max);
    hc.in(dm, m, n);
    hc.in(dpairs, pairs, (size_t)K * 2);
    hc.out(dAs, A_s, (size_t)K * W * d);
    hc.out(dbs, b_s, (size_t)K * W);
    hc.out(dms, m_s, (size_t)K);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_pair_stacks_dev(ctx, hc.st, n, m_max, d, dA, db, dm, K, dpairs, dAs, dbs, dms);
    if (rc) return rc;
    return hc.download();
}

// Pairs per chunk of plp_intersect_pairs_dev when the caller names none (the one statement of the rule; exported, so that
// the Python layer chunks its emission pass the same way): what keeps the chunk's stacks at 32 MiB (REASONED,
// NOT MEASURED -- DESIGN 4.21: some 50 000 stacks of two 8-row cells in d = 4, 3 800 of two 32-row cells in d = 16; the
// scratch stays in the tens of megabytes per stream).
int64_t plp_pair_chunk_default(int m_max, int d) {
    if (m_max < 1 || d < 1) return 1024;
    const size_t per = 2 * (size_t)m_max * ((size_t)d + 1) * 8;
    const size_t c = ((size_t)32 << 20) / per;
    return (int64_t)(c < 1024 ? 1024 : c);
}

int plp_intersect_pairs_dev(plp_ctx* ctx, void* stream, int n, int m_max, int d, const double* A, const double* b,
                            const int32_t* m, double abs_tol, int64_t K, const int32_t* pairs, int64_t chunk, uint64_t* keep,
                            int32_t* flags, double* r, double* xc, int32_t* nlp, int32_t* ms, int mo_max, double* A_out,
                            double* b_out, int32_t* m_out) {
    int rc = check_pair_stacks(ctx, n, m_max, d, A, b, K, pairs, keep && flags && r && xc && nlp && ms);
    if (rc) return rc;
    if (mo_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (K == 0) return PLP_OK;
    if (A_out && (!b_out || !m_out)) return fail(PLP_EINVAL, "NULL pointer");
    const int W = 2 * m_max;
    int64_t c = chunk > 0 ? chunk : plp_pair_chunk_default(m_max, d);
    c = c < K ? c : K;
    const size_t a_bytes = pad((size_t)c * W * d * 8), b_bytes = pad((size_t)c * W * 8);
    char* sc = static_cast<char*>(stream_buf(ctx->ps_scratch, stream, a_bytes + b_bytes));
    if (!sc) return fail(PLP_EHIP, "intersect_pairs: no device memory for the stacks of a chunk (%zu bytes)", a_bytes + b_bytes);
    double* As = reinterpret_cast<double*>(sc);
    double* bs = reinterpret_cast<double*>(sc + a_bytes);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t lo = 0; lo < K; lo += c) {
        const int64_t k = K - lo < c ? K - lo : c;
        const int32_t* pl = pairs + 2 * lo;
        // the rows that stay per stack are an output of the call and the row counts the reduce and the emission read
        if (plp::launch_pair_stacks(n, m_max, d, A, b, m, k, pl, As, bs, ms + lo, st))
            return fail(PLP_EUNSUPPORTED, "pair stacks: unsupported size");
        if ((rc = check_launch("pair_stack_kernel"))) return rc;
        rc = plp_reduce_batch_dev(ctx, stream, k, W, d, As, bs, ms + lo, abs_tol, keep + lo, flags + lo, r + lo,
                                  xc + (size_t)lo * d, nlp + lo);
        if (rc) return rc;
        if (A_out) {
            rc = plp_fm_emit_dev(ctx, stream, k, W, d, As, bs, ms + lo, keep + lo, 1, flags + lo, -1, 0, abs_tol, mo_max,
                                 A_out + (size_t)lo * mo_max * d, b_out + (size_t)lo * mo_max, m_out + lo);
            if (rc) return rc;
        }
        plp::launch_pair_bad(n, d, k, pl, reinterpret_cast<unsigned long long*>(keep + lo), flags + lo, r + lo,
                             xc + (size_t)lo * d, nlp + lo, ms + lo, A_out ? m_out + lo : nullptr, st);
        if ((rc = check_launch("pair_bad_kernel"))) return rc;
    }
    return PLP_OK;
}

int plp_intersect_pairs(plp_ctx* ctx, int n, int m_max, int d, const double* A, const double* b, const int32_t* m,
                        double abs_tol, int64_t K, const int32_t* pairs, int64_t chunk, uint64_t* keep, int32_t* flags, double* r,
                        double* xc, int32_t* nlp, int32_t* ms, int mo_max, double* A_out, double* b_out, int32_t* m_out) {
    int rc = check_pair_stacks(ctx, n, m_max, d, A, b, K, pairs, keep && flags && r && xc && nlp && ms);
    if (rc) return rc;
    if (mo_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (K == 0) return PLP_OK;
    if (A_out && (!b_out || !m_out)) return fail(PLP_EINVAL, "NULL pointer");
    if ((rc = check_listed(n, K, pairs))) return rc;
    const size_t mo = A_out ? (size_t)mo_max : 0;
    double *dA, *db, *dr, *dxc, *dAo, *dbo;
    int32_t *dm, *dpairs, *dhead;
    uint64_t* dkeep;
    // (flags, nlp, ms and m_out come back as one block: a call declares at most eight outputs)
    std::vector<int32_t> head((size_t)K * 4);
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)n * m_max * d);
    hc.in(db, b, (size_t)n * m_max);
    hc.in(dm, m, n);
    hc.in(dpairs, pairs, (size_t)K * 2);
    hc.out(dkeep, keep, (size_t)K);
    hc.out(dhead, head.data(), (size_t)K * 4);
    hc.out(dr, r, (size_t)K);
    hc.out(dxc, xc, (size_t)K * d);
    hc.out(dAo, A_out, (size_t)K * mo * d);
    hc.out(dbo, b_out, (size_t)K * mo);
    hc.direct_out = true;
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_intersect_pairs_dev(ctx, hc.st, n, m_max, d, dA, db, dm, abs_tol, K, dpairs, chunk, dkeep, dhead, dr, dxc, dhead + K,
                                 dhead + 2 * K, mo_max, A_out ? dAo : nullptr, dbo, dhead + 3 * K);
    if (rc) return rc;
    rc = hc.download();
    if (rc) return rc;
    memcpy(flags, head.data(), (size_t)K * 4);
    memcpy(nlp, head.data() + K, (size_t)K * 4);
    memcpy(ms, head.data() + 2 * K, (size_t)K * 4);
    if (A_out) memcpy(m_out, head.data() + 3 * K, (size_t)K * 4);
    return PLP_OK;
}

int plp_selftest(plp_ctx* ctx, int group_size, double* out_d, uint32_t* out_u) {
    if (!ctx || !out_d || !out_u) return fail(PLP_EINVAL, "NULL pointer");
    double* dd;
    uint32_t* du;
    HostCall hc(ctx);
    hc.out(dd, out_d, 128);
    hc.out(du, out_u, 128);
    int rc = hc.reserve();
    if (rc) return rc;
    if (plp::launch_selftest(group_size, dd, du, hc.st)) return fail(PLP_EINVAL, "group size must be 8/16/32/64");
    rc = check_launch("selftest_kernel");
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------------------- region_diff search
}  // extern "C"

// The search is host code of its own (plp_rdiff_search.hpp: the walk, radius memo, speculation); its batches of LPs
// are solved by the device backend (plp_rdiff_host.hpp: resident LP server or a launch per batch).
#include "plp_rdiff_host.hpp"

struct plp_rdiff_result : plp::rdiff::Result { long long n_lps = 0, n_batches = 0; };

extern "C" {

int plp_region_diff_search(plp_ctx* ctx, int d, int m, int N, const int32_t* mi, const double* A, const double* b,
                           double abs_tol, plp_rdiff_result** out) {
    if (!ctx || !mi || !A || !b || !out) return fail(PLP_EINVAL, "NULL pointer");
    if (d < 1 || d > plp::MAX_D || m < 0 || N < 1) return fail(PLP_EINVAL, "bad sizes d=%d m=%d N=%d", d, m, N);
    *out = nullptr;
    long long M = 0;
    for (int j = 0; j < N; ++j) {
        if (mi[j] < 1) return fail(PLP_EINVAL, "mi[%d] = %d (a cell without a new constraint covers the polytope)", j, mi[j]);
        M += mi[j];
    }
    HIP_TRY(hipSetDevice(ctx->device));
    RdiffBackend be;
    int rc = be.init(ctx, d, m + 2 * M, A, b);
    if (rc) { be.release(); return rc; }
    plp_rdiff_result* res = new plp_rdiff_result();
    plp::rdiff::Search<RdiffBackend> search(m, N, mi, abs_tol, be.env.spec, be, *res);
    const auto t_search0 = std::chrono::steady_clock::now();
    rc = search.run();
    res->n_lps = be.n_lps;
    res->n_batches = be.n_batches;
    if (be.env.stats)
        fprintf(stderr, "plp_region_diff_search: %lld LPs, %lld batches (%lld scan misses, %lld node misses), %lld requests, launch %.1f ms, device wait %.1f ms; beyond 64 rows: %lld LPs in %lld batches; resident server: %lld batches, %lld starts; search loop %.1f ms of which assembling the batches' lists %.1f ms, storing results %.1f ms\n",
                be.n_lps, be.n_batches, res->n_scan_miss, res->n_node_miss, res->n_requests, be.t_launch * 1e3, be.t_wait * 1e3,
                be.n_lps_long, be.n_batches_long, be.n_srv_batches, be.n_srv_starts,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_search0).count() * 1e3, search.t_spec * 1e3,
                search.R.t_store * 1e3);
    be.release();
    if (rc) { delete res; return rdiff_fail(rc, N, search.R.too_long); }
    *out = res;
    return PLP_OK;
}

int plp_rdiff_result_sizes(const plp_rdiff_result* r, int64_t* n_leaves, int64_t* n_rows, int64_t* n_lps, int64_t* n_batches) {
    if (!r) return fail(PLP_EINVAL, "NULL result");
    if (n_leaves) *n_leaves = (int64_t)r->kind.size();
    if (n_rows) *n_rows = (int64_t)r->rows.size();
    if (n_lps) *n_lps = r->n_lps;
    if (n_batches) *n_batches = r->n_batches;
    return PLP_OK;
}

int plp_rdiff_result_copy(const plp_rdiff_result* r, int32_t* kind, int32_t* off, int32_t* rows) {
    if (!r || !kind || !off || !rows) return fail(PLP_EINVAL, "NULL pointer");
    if (!r->kind.empty()) memcpy(kind, r->kind.data(), r->kind.size() * 4);
    memcpy(off, r->off.data(), r->off.size() * 4);
    if (!r->rows.empty()) memcpy(rows, r->rows.data(), r->rows.size() * 4);
    return PLP_OK;
}

int plp_rdiff_result_free(plp_rdiff_result* r) {
    delete r;
    return PLP_OK;
}

// ------------------------------------------------------------------------------- region_diff, many searches in one launch
static int rdiff_batch_check(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, int64_t Nc, int mc_max,
                             const double* CA, const double* Cb, const int32_t* cell_off, const int32_t* cell_idx, int max_lps,
                             int p_max, int r_max, int n_max, int M_max, const void* kind, const void* off, const void* rows,
                             const void* count, const void* nrows, const void* nlp, const void* status, const void* mi,
                             const void* src) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1 || Nc < 0 || mc_max < 0 || n_max < 0 || M_max < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (d > 4) return fail(PLP_EUNSUPPORTED, "region_diff_batch: d=%d outside the kernel (d<=4)", d);
    if (p_max < 1 || r_max < 1 || max_lps < 0)
        return fail(PLP_EINVAL, "region_diff_batch: p_max=%d r_max=%d max_lps=%d", p_max, r_max, max_lps);
    if (B > 2147483647ll || Nc > 2147483647ll || (long long)Nc * mc_max > 2147483647ll)
        return fail(PLP_EUNSUPPORTED, "region_diff_batch: B or the cell table exceeds 2^31 - 1");
    if (!cell_off || !kind || !off || !rows || !count || !nrows || !nlp || !status || (n_max > 0 && !mi) || (M_max > 0 && !src) ||
        (m_max > 0 && (!A || !b)) || (Nc > 0 && mc_max > 0 && (!CA || !Cb)) || (Nc > 0 && !cell_idx))
        return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}

int plp_region_diff_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, const double* A, const double* b,
                              const int32_t* m, int64_t Nc, int mc_max, const double* CA, const double* Cb, const int32_t* mc,
                              const int32_t* cell_off, const int32_t* cell_idx, double abs_tol, int max_lps, int p_max,
                              int r_max, int n_max, int M_max, int32_t* kind, int32_t* off, int32_t* rows, int32_t* count,
                              int32_t* nrows, int32_t* nlp, int32_t* status, int32_t* mi, int32_t* src) {
    int rc = rdiff_batch_check(ctx, B, m_max, d, A, b, Nc, mc_max, CA, Cb, cell_off, cell_idx, max_lps, p_max, r_max, n_max, M_max,
                               kind, off, rows, count, nrows, nlp, status, mi, src);
    if (rc || B == 0) return rc;
    if (plp::launch_rdiff_batch(B, m_max, d, A, b, m, Nc, mc_max, CA, Cb, mc, cell_off, cell_idx, abs_tol, max_lps, p_max, r_max,
                                n_max, M_max, kind, off, rows, count, nrows, nlp, status, mi, src, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "region_diff_batch: unsupported size");
    return check_launch("rdiff_batch_kernel");
}

int plp_region_diff_batch(plp_ctx* ctx, int64_t B, int m_max, int d, const double* A, const double* b, const int32_t* m,
                          int64_t Nc, int mc_max, const double* CA, const double* Cb, const int32_t* mc, const int32_t* cell_off,
                          const int32_t* cell_idx, double abs_tol, int max_lps, int p_max, int r_max, int n_max, int M_max,
                          int32_t* kind, int32_t* off, int32_t* rows, int32_t* count, int32_t* nrows, int32_t* nlp,
                          int32_t* status, int32_t* mi, int32_t* src) {
    int rc = rdiff_batch_check(ctx, B, m_max, d, A, b, Nc, mc_max, CA, Cb, cell_off, cell_idx, max_lps, p_max, r_max, n_max, M_max,
                               kind, off, rows, count, nrows, nlp, status, mi, src);
    if (rc || B == 0) return rc;
    if (cell_off[0] < 0) return fail(PLP_EINVAL, "region_diff_batch: cell_off[0] = %d", cell_off[0]);
    for (int64_t p = 0; p < B; ++p)   // (the upload of cell_idx is sized by cell_off[B]: every list must lie inside it)
        if (cell_off[p + 1] < cell_off[p])
            return fail(PLP_EINVAL, "region_diff_batch: cell_off decreases at %lld", (long long)p);
    double *dA, *db, *dCA, *dCb;
    int32_t *dm, *dmc, *dcoff, *dcidx, *dkind, *doff, *drows, *dhead, *dmi, *dsrc;
    // (count, nrows, nlp and status come back as one block: a call declares at most eight outputs)
    std::vector<int32_t> head((size_t)B * 4);
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d);
    hc.in(db, b, (size_t)B * m_max);
    hc.in(dm, m, B);
    hc.in(dCA, CA, (size_t)Nc * mc_max * d);
    hc.in(dCb, Cb, (size_t)Nc * mc_max);
    hc.in(dmc, mc, Nc);
    hc.in(dcoff, cell_off, (size_t)B + 1);
    hc.in(dcidx, cell_idx, (size_t)cell_off[B]);
    hc.out(dkind, kind, (size_t)B * p_max);
    hc.out(doff, off, (size_t)B * ((size_t)p_max + 1));
    hc.out(drows, rows, (size_t)B * r_max);
    hc.out(dhead, head.data(), (size_t)B * 4);
    hc.out(dmi, mi, (size_t)B * n_max);
    hc.out(dsrc, src, (size_t)B * M_max);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    // (a problem that ends early leaves its slots unwritten: the caller gets zeros there, not what the arena held)
    HIP_TRY(hipMemsetAsync(dkind, 0, (size_t)B * p_max * 4, hc.st));
    HIP_TRY(hipMemsetAsync(doff, 0, (size_t)B * ((size_t)p_max + 1) * 4, hc.st));
    HIP_TRY(hipMemsetAsync(drows, 0, (size_t)B * r_max * 4, hc.st));
    if (n_max > 0) HIP_TRY(hipMemsetAsync(dmi, 0, (size_t)B * n_max * 4, hc.st));
    if (M_max > 0) HIP_TRY(hipMemsetAsync(dsrc, 0, (size_t)B * M_max * 4, hc.st));
    rc = plp_region_diff_batch_dev(ctx, hc.st, B, m_max, d, dA, db, dm, Nc, mc_max, dCA, dCb, dmc, dcoff, dcidx, abs_tol, max_lps,
                                   p_max, r_max, n_max, M_max, dkind, doff, drows, dhead, dhead + B, dhead + 2 * B, dhead + 3 * B,
                                   dmi, dsrc);
    if (rc) return rc;
    rc = hc.download();
    if (rc) return rc;
    memcpy(count, head.data(), (size_t)B * 4);
    memcpy(nrows, head.data() + B, (size_t)B * 4);
    memcpy(nlp, head.data() + 2 * B, (size_t)B * 4);
    memcpy(status, head.data() + 3 * B, (size_t)B * 4);
    return PLP_OK;
}

// ------------------------------------------------------------------------------- envelope: the facet tests of many regions
static int envelope_check(plp_ctx* ctx, int64_t C, int mc_max, int d, const double* A, const double* b, int64_t B,
                          const int32_t* reg_off, int64_t L, const void* outer, const void* status, const void* nlp) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (C < 0 || mc_max < 0 || d < 1 || B < 0 || L < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0 || L == 0) return PLP_OK;
    if (d > 8) return fail(PLP_EUNSUPPORTED, "envelope_batch: d=%d outside the kernel (d<=8)", d);
    if (B > 2147483647ll || L > 2147483647ll || C > 2147483647ll || (long long)C * mc_max > 2147483647ll)
        return fail(PLP_EUNSUPPORTED, "envelope_batch: B, L or the member table exceeds 2^31 - 1");
    if (!reg_off || !outer || !status || !nlp || (C > 0 && mc_max > 0 && (!A || !b))) return fail(PLP_EINVAL, "NULL pointer");
    return PLP_OK;
}

int plp_envelope_batch_dev(plp_ctx* ctx, void* stream, int64_t C, int mc_max, int d, const double* A, const double* b,
                           const int32_t* mc, int64_t B, const int32_t* reg_off, int64_t L, const int32_t* mem_idx,
                           double abs_tol, uint64_t* outer, int32_t* status, int32_t* nlp) {
    int rc = envelope_check(ctx, C, mc_max, d, A, b, B, reg_off, L, outer, status, nlp);
    if (rc || B == 0 || L == 0) return rc;
    if (plp::launch_envelope_cross(C, mc_max, d, A, b, mc, B, reg_off, L, mem_idx, abs_tol, (unsigned long long*)outer, status,
                                   nlp, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "envelope_batch: unsupported size");
    return check_launch("envelope_cross_kernel");
}

int plp_envelope_batch(plp_ctx* ctx, int64_t C, int mc_max, int d, const double* A, const double* b, const int32_t* mc,
                       int64_t B, const int32_t* reg_off, int64_t L, const int32_t* mem_idx, double abs_tol, uint64_t* outer,
                       int32_t* status, int32_t* nlp) {
    int rc = envelope_check(ctx, C, mc_max, d, A, b, B, reg_off, L, outer, status, nlp);
    if (rc || B == 0 || L == 0) return rc;
    // (reg_off and mem_idx go up as they are: the kernel refuses an entry whose offsets or indices do not hold, and reads
    // neither mem_idx beyond L nor the table beyond C members)
    double *dA, *db;
    int32_t *dmc, *droff, *dmidx, *dstatus, *dnlp;
    uint64_t* douter;
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)C * mc_max * d);
    hc.in(db, b, (size_t)C * mc_max);
    hc.in(dmc, mc, C);
    hc.in(droff, reg_off, (size_t)B + 1);
    hc.in(dmidx, mem_idx, L);
    hc.out(douter, outer, L);
    hc.out(dstatus, status, L);
    hc.out(dnlp, nlp, L);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_envelope_batch_dev(ctx, hc.st, C, mc_max, d, dA, db, dmc, B, droff, L, dmidx, abs_tol, douter, dstatus, dnlp);
    if (rc) return rc;
    return hc.download();
}

// ------------------------------------------------------------------ projection by the iterative hull, one launch for B polytopes
static int projhull_check(plp_ctx* ctx, int64_t B, int m_max, int d, int k, const double* A, const double* b,
                          const int32_t* keep, const double* xc, int f_max, int max_lps, const void* Ao, const void* bo,
                          const void* on, const void* count, const void* V, const void* nv, const void* vmask, const void* nlp,
                          const void* status) {
    if (!ctx) return fail(PLP_EINVAL, "ctx is NULL");
    if (B < 0 || m_max < 0 || d < 1 || k < 1 || f_max < 1 || max_lps < 0) return fail(PLP_EINVAL, "bad sizes");
    if (B == 0) return PLP_OK;
    if (k > 3 || d < k || d > 16 || m_max > 64 || f_max > 128)
        return fail(PLP_EUNSUPPORTED, "project_hull_batch: m_max=%d d=%d k=%d f_max=%d outside the kernel (m<=64, k<=d<=16, k<=3, f_max<=128)",
                    m_max, d, k, f_max);
    if (B > 2147483647ll) return fail(PLP_EUNSUPPORTED, "project_hull_batch: B exceeds 2^31 - 1");
    if (!keep || !xc || !Ao || !bo || !on || !count || !V || !nv || !vmask || !nlp || !status || (m_max > 0 && (!A || !b)))
        return fail(PLP_EINVAL, "NULL pointer");
    for (int t = 0; t < k; ++t)
        if (keep[t] < 0 || keep[t] >= d || (t && keep[t] <= keep[t - 1]))
            return fail(PLP_EUNSUPPORTED, "project_hull_batch: keep must be increasing and inside 0 .. d - 1");
    return PLP_OK;
}

int plp_project_hull_batch_dev(plp_ctx* ctx, void* stream, int64_t B, int m_max, int d, int k, const double* A, const double* b,
                               const int32_t* m, const int32_t* keep, const double* xc, int f_max, int max_lps, double* Ao,
                               double* bo, uint64_t* on, int32_t* count, double* V, int32_t* nv, double* X, uint64_t* vmask,
                               int32_t* nlp, int32_t* status) {
    int rc = projhull_check(ctx, B, m_max, d, k, A, b, keep, xc, f_max, max_lps, Ao, bo, on, count, V, nv, vmask, nlp, status);
    if (rc || B == 0) return rc;
    if (plp::launch_projhull(B, m_max, d, k, A, b, m, keep, xc, f_max, max_lps, Ao, bo, (unsigned long long*)on, count, V, nv, X,
                             (unsigned long long*)vmask, nlp, status, (hipStream_t)stream))
        return fail(PLP_EUNSUPPORTED, "project_hull_batch: unsupported size");
    return check_launch("projhull_kernel");
}

int plp_project_hull_batch(plp_ctx* ctx, int64_t B, int m_max, int d, int k, const double* A, const double* b, const int32_t* m,
                           const int32_t* keep, const double* xc, int f_max, int max_lps, double* Ao, double* bo, uint64_t* on,
                           int32_t* count, double* V, int32_t* nv, double* X, uint64_t* vmask, int32_t* nlp, int32_t* status) {
    int rc = projhull_check(ctx, B, m_max, d, k, A, b, keep, xc, f_max, max_lps, Ao, bo, on, count, V, nv, vmask, nlp, status);
    if (rc || B == 0) return rc;
    double *dA, *db, *dxc, *dAo, *dbo, *dV, *dX = nullptr;
    int32_t *dm, *dhead;
    uint64_t *don, *dvmask;
    std::vector<int32_t> head((size_t)4 * B);   // count | nv | nlp | status: one copy back
    HostCall hc(ctx);
    hc.in(dA, A, (size_t)B * m_max * d);
    hc.in(db, b, (size_t)B * m_max);
    hc.in(dm, m, B);
    hc.in(dxc, xc, (size_t)B * d);
    hc.out(dAo, Ao, (size_t)B * f_max * k);
    hc.out(dbo, bo, (size_t)B * f_max);
    hc.out(don, on, (size_t)B * f_max);
    hc.out(dV, V, (size_t)B * PLP_PH_MAX_POINTS * k);
    if (X) hc.out(dX, X, (size_t)B * PLP_PH_MAX_POINTS * d);
    hc.out(dvmask, vmask, B);
    hc.out(dhead, head.data(), (size_t)4 * B);
    rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = plp_project_hull_batch_dev(ctx, hc.st, B, m_max, d, k, dA, db, dm, keep, dxc, f_max, max_lps, dAo, dbo, don, dhead, dV,
                                    dhead + B, dX, dvmask, dhead + 2 * B, dhead + 3 * B);
    if (rc) return rc;
    rc = hc.download();
    if (rc) return rc;
    memcpy(count, head.data(), (size_t)B * 4);
    memcpy(nv, head.data() + B, (size_t)B * 4);
    memcpy(nlp, head.data() + 2 * B, (size_t)B * 4);
    memcpy(status, head.data() + 3 * B, (size_t)B * 4);
    return PLP_OK;
}

}  // extern "C"
