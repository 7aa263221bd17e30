// plp_hostcall.hpp -- private to plp_capi.hip: the context, the error string, and what a host-pointer entry point is
// made of -- the grow-only arena, the small-call pinned mirror (copy_in / copy_out), the chunked upload of large batches
// (staged_run) and HostCall, which derives all of them from one declaration of the call's arrays.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <unordered_map>
#include <vector>

#include "../../include/plp.h"
#include "plp_kernels.hpp"
#include "plp_stage.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(PLP_EHIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

}  // namespace

struct plp_ctx {
    int device;
    hipStream_t stream;
    char* arena;
    size_t arena_bytes;
    char* pin;  // pinned host mirror of the first SMALL_XFER bytes of the arena (small calls: one copy each way)
    // region_diff search (kept across calls: a pinned allocation costs more than a small search)
    char* rd_pin = nullptr;      // host-mapped block [index block | radii | sequence word]
    char* rd_pin_dev = nullptr;
    double* rd_out = nullptr;    // radii of a batch (device)
    double* rd_tab = nullptr;    // the constraint table A | b (device)
    size_t rd_tab_bytes = 0;
    unsigned long long rd_seq = 0;
    // the search's resident LP server (plp_rdiff.hip: rdiff_server_kernel): host-mapped mailbox / records / results block,
    // its device view, the device-side state words, the sequence number of the last batch
    char* rd_srv = nullptr;
    char* rd_srv_dev = nullptr;
    unsigned long long* rd_srv_state = nullptr;
    unsigned long long rd_srv_seq = 0;    // batches issued so far
    unsigned long long rd_srv_word = 0;   // mailbox word of the last batch that was answered
    unsigned long long rd_srv_init[4] = {0, 0, 0, 0};
    // containment: per-row thresholds of the comparison form (plp_points.hip), a grow-only buffer
    void* mf_buf = nullptr;
    size_t mf_bytes = 0;
    hipEvent_t mf_ev = nullptr;  // recorded after every launch that uses mf_buf: the next user (any stream) waits on it
    bool mf_used = false;
    // device / pinned buffers of the last quickhull session that ended (plp_hull_destroy parks them here, plp_hull_create
    // takes them when they are large enough): hipMalloc / hipFree of five buffers cost more than a 100 000-point hull
    struct HullSpare {
        double* X = nullptr; int32_t* owner = nullptr; double* dist = nullptr; uint8_t* dead = nullptr;
        char* io = nullptr; char* pin = nullptr;
        size_t X_bytes = 0, owner_bytes = 0, dist_bytes = 0, dead_cap = 0, io_bytes = 0;
        bool full = false;
    } hull_spare;
    // large host-pointer batches (plp_stage.hpp): staging threads, pinned staging buffer, copy stream, one event per chunk
    plp::StagePool* pool = nullptr;
    char* stage = nullptr;
    size_t stage_bytes = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t stage_ev[16] = {};
    int stage_nev = 0;
    bool check_finite = false;  // plp_ctx_set_check_finite
    // plp_reduce_counters: device word the fused reduce kernels add their simplex-run count to (lazily allocated; the
    // kernels get nullptr until the first plp_reduce_counters call of the context, and then it costs one atomic per tile)
    unsigned long long* reduce_ctr = nullptr;
    // fused reduce: one word per call in flight (a ring of 64) that the fast kernels raise to the call's number when they
    // hand a polytope to the general kernel, so that its second pass can leave on one load (plp_reduce.hip)
    unsigned long long* retry_ring = nullptr;
    unsigned long long reduce_epoch = 0;
    // plp_assign_dev (few facets): the workgroups' (max, index) partials, one grow-only buffer PER STREAM -- calls on
    // different streams never share one, so nothing has to order them (a handful of streams per context in practice;
    // beyond 16 the table is emptied after a device synchronisation)
    struct StreamBuf { void* p = nullptr; size_t bytes = 0; unsigned calls = 0; };
    std::unordered_map<void*, StreamBuf> as_scratch;
    // the verifier behind the LP / Chebyshev / bounding-box batches (plp_verify.hip): fail list + the careful engine's
    // dictionaries, one grow-only buffer per stream like as_scratch; bounding boxes: the engines' bases and centres
    std::unordered_map<void*, StreamBuf> vf_scratch;
    std::unordered_map<void*, StreamBuf> vf_basis;
    // plp_intersect_pairs_dev: the stacks of one chunk of pairs (A_s | b_s; their row counts go to the caller's ms), per stream like the tables above
    std::unordered_map<void*, StreamBuf> ps_scratch;
};

namespace {

size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// a grow-only device buffer of this stream (see plp_ctx::as_scratch); nullptr: allocation failed
void* stream_buf(std::unordered_map<void*, plp_ctx::StreamBuf>& table, void* stream, size_t need) {
    if (table.size() >= 16 && !table.count(stream)) {
        (void)hipDeviceSynchronize();
        for (auto& kv : table) if (kv.second.p) (void)hipFree(kv.second.p);
        table.clear();
    }
    plp_ctx::StreamBuf& sb = table[stream];
    if (need > sb.bytes) {
        if (sb.p) { (void)hipStreamSynchronize((hipStream_t)stream); (void)hipFree(sb.p); }  // (its last user ran on this stream)
        sb.p = nullptr;
        sb.bytes = 0;
        if (hipMalloc(&sb.p, need + need / 4) == hipSuccess) {
            sb.bytes = need + need / 4;
            sb.calls = 0;
            (void)hipMemsetAsync(sb.p, 0, 256, (hipStream_t)stream);   // (the verifier's list counters start at zero)
        } else {
            (void)hipGetLastError();
        }
    }
    return sb.p;
}

int ensure_arena(plp_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->arena_bytes) return PLP_OK;
    if (ctx->arena) HIP_TRY(hipFree(ctx->arena));
    ctx->arena = nullptr;
    ctx->arena_bytes = 0;
    size_t want = bytes + bytes / 4;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->arena), want));
    ctx->arena_bytes = want;
    return PLP_OK;
}

// Host-pointer calls whose buffers fit SMALL_XFER move them through the pinned mirror: the inputs are
// gathered into it and cross PCIe as ONE copy, likewise the outputs.  A pageable hipMemcpyAsync of a few
// hundred bytes costs 10-20 us, and the set operations issue hundreds of small batches (region_diff: one
// per search level), so six copies per call were most of such a call.  Large calls copy each array directly.
constexpr size_t SMALL_XFER = 1u << 20;

struct Span {
    void* dev;
    const void* host_in;  // copy_in source (or nullptr)
    void* host_out;       // copy_out destination (or nullptr)
    size_t bytes;
};

// the few arrays of one call, kept on the stack (a small host-pointer call lasts 50 us: no heap traffic for its lists);
// one more than N is not stored and raises `overflow`
template <typename T, size_t N = 8>
struct Few {
    T v[N];
    size_t n = 0;
    bool overflow = false;
    void push_back(const T& x) {
        if (n < N) v[n++] = x;
        else overflow = true;
    }
    T* begin() { return v; }
    T* end() { return v + n; }
    const T* begin() const { return v; }
    const T* end() const { return v + n; }
    size_t size() const { return n; }
};

int ensure_pin(plp_ctx* ctx) {
    if (ctx->pin) return PLP_OK;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->pin), SMALL_XFER, hipHostMallocDefault));
    return PLP_OK;
}

bool fits_small(plp_ctx* ctx, const Few<Span>& spans) {
    for (const Span& sp : spans) {
        if (!sp.bytes) continue;
        const size_t end = (size_t)(static_cast<char*>(sp.dev) - ctx->arena) + sp.bytes;
        if (end > SMALL_XFER) return false;
    }
    return true;
}

int copy_in(plp_ctx* ctx, hipStream_t st, const Few<Span>& spans) {
    if (fits_small(ctx, spans) && ensure_pin(ctx) == PLP_OK) {
        size_t lo = SMALL_XFER, hi = 0;
        for (const Span& sp : spans) {
            if (!sp.bytes || !sp.host_in) continue;
            const size_t off = (size_t)(static_cast<char*>(sp.dev) - ctx->arena);
            memcpy(ctx->pin + off, sp.host_in, sp.bytes);
            lo = off < lo ? off : lo;
            hi = off + sp.bytes > hi ? off + sp.bytes : hi;
        }
        if (hi > lo) HIP_TRY(hipMemcpyAsync(ctx->arena + lo, ctx->pin + lo, hi - lo, hipMemcpyHostToDevice, st));
        return PLP_OK;
    }
    for (const Span& sp : spans)
        if (sp.bytes && sp.host_in) HIP_TRY(hipMemcpyAsync(sp.dev, sp.host_in, sp.bytes, hipMemcpyHostToDevice, st));
    return PLP_OK;
}

// Large host-pointer batch: the per-unit input arrays go to the device chunk by chunk (plp_stage.hpp) and `launch(lo, hi)`
// enqueues the kernels of units [lo, hi) on `st` behind the arrival of their chunk.  *staged = false: not applicable
// (small batch, PLP_STAGE=0, or a resource could not be had) and nothing was done -- the caller copies as before.
constexpr size_t STAGE_MIN_BYTES = 8u << 20;  // smaller batches go up as one copy

struct StageArray {
    const void* host;
    void* dev;
    size_t unit_bytes;
    bool f64 = false;  // doubles (checked for inf / nan when the context asks for it)
};

const char* const NONFINITE_MSG = "input must not contain values inf, nan, or None";

// plp_ctx_set_check_finite, inputs that are not staged chunk-wise: one pass over the array
int finite_or_fail(plp_ctx* ctx, const double* a, size_t count) {
    if (ctx->check_finite && a && count && plp::any_nonfinite_f64(reinterpret_cast<const char*>(a), count * 8))
        return fail(PLP_ENONFINITE, "%s", NONFINITE_MSG);
    return PLP_OK;
}

// The arrays' device regions (neighbours in the arena, `blk` .. `blk + blk_bytes`) are used as ONE block in which every
// chunk's pieces sit back to back -- the layout of the staging buffer -- so that a chunk crosses PCIe as one copy;
// `launch(lo, hi, ptrs)` gets the device address of each array's rows lo.. (ptrs[i] for arrays[i], NULL where host is).
template <typename F>
int staged_run(plp_ctx* ctx, hipStream_t st, int64_t B, int64_t align, const Few<StageArray>& arrays, char* blk,
               size_t blk_bytes, F launch, bool* staged) {
    *staged = false;
    size_t unit = 0;
    for (const StageArray& a : arrays)
        if (a.host) unit += a.unit_bytes;
    const size_t total = unit * (size_t)B;
    const char* off = getenv("PLP_STAGE");
    if ((off && off[0] == '0') || total < STAGE_MIN_BYTES || B < 4 * align || total > blk_bytes || arrays.size() > 8) return PLP_OK;
    if (!ctx->pool) {
        const char* nt = getenv("PLP_STAGE_THREADS");
        unsigned hw = std::thread::hardware_concurrency();
        int n = nt ? atoi(nt) : (hw >= 16 ? 7 : (hw >= 4 ? (int)hw / 2 - 1 : 1));
        if (n < 1) n = 1;
        if (n > 32) n = 32;
        try {
            ctx->pool = new plp::StagePool(n);
        } catch (...) {  // no threads to be had: the caller copies as before
            ctx->pool = nullptr;
            return PLP_OK;
        }
    }
    if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        ctx->copy_stream = nullptr;
        return PLP_OK;
    }
    while (ctx->stage_nev < 16) {
        if (hipEventCreateWithFlags(&ctx->stage_ev[ctx->stage_nev], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return PLP_OK;
        }
        ++ctx->stage_nev;
    }
    if (total > ctx->stage_bytes) {
        if (ctx->stage) (void)hipHostFree(ctx->stage);
        ctx->stage = nullptr;
        ctx->stage_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->stage), total + total / 4, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return PLP_OK;
        }
        ctx->stage_bytes = total + total / 4;
    }
    int64_t nch = (int64_t)(total / (4u << 20));
    nch = nch < 2 ? 2 : (nch > 16 ? 16 : nch);
    int64_t per = (B + nch - 1) / nch;
    per = (per + align - 1) / align * align;
    nch = (B + per - 1) / per;
    std::vector<std::vector<plp::StagePiece>> chunks;
    try {
        chunks.resize((size_t)nch);
        for (auto& c : chunks) c.reserve(arrays.size());
    } catch (...) {
        return PLP_OK;
    }
    size_t so = 0;  // (unit sizes are multiples of 4 and chunk lengths multiples of `align` >= 16: every piece 8-byte aligned)
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t lo = c * per, hi = lo + per < B ? lo + per : B;
        for (const StageArray& a : arrays) {
            if (!a.host) continue;
            const size_t bytes = (size_t)(hi - lo) * a.unit_bytes;
            chunks[(size_t)c].push_back({static_cast<const char*>(a.host) + (size_t)lo * a.unit_bytes, ctx->stage + so, blk + so,
                                         bytes, a.f64 && ctx->check_finite});
            so += bytes;
        }
    }
    // the copy stream must not overwrite device inputs an earlier call on `st` may still be reading
    HIP_TRY(hipEventRecord(ctx->stage_ev[15], st));
    HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, ctx->stage_ev[15], 0));
    const bool timing = getenv("PLP_STAGE_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    ctx->pool->start(chunks);
    *staged = true;
    int rc = PLP_OK;
    for (int64_t c = 0; c < nch && rc == PLP_OK; ++c) {
        ctx->pool->wait((int)c);
        if (timing) fprintf(stderr, "[stage] chunk %d staged at %.0f us\n", (int)c, us());
        if (ctx->pool->nonfinite()) break;  // (set only when the context checks its inputs)
        void* ptrs[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        {
            const std::vector<plp::StagePiece>& pc = chunks[(size_t)c];
            size_t bytes = 0, k = 0, i = 0;
            for (const StageArray& a : arrays) {
                if (a.host) { ptrs[i] = pc[k].dev; bytes += pc[k].bytes; ++k; }
                ++i;
            }
            const hipError_t e = hipMemcpyAsync(pc[0].dev, pc[0].dst, bytes, hipMemcpyHostToDevice, ctx->copy_stream);
            if (e != hipSuccess) rc = fail(PLP_EHIP, "staged upload: %s", hipGetErrorString(e));
        }
        if (rc == PLP_OK && (hipEventRecord(ctx->stage_ev[c % 15], ctx->copy_stream) != hipSuccess ||
                             hipStreamWaitEvent(st, ctx->stage_ev[c % 15], 0) != hipSuccess))
            rc = fail(PLP_EHIP, "staged upload: event");
        const int64_t lo = c * per, hi = lo + per < B ? lo + per : B;
        if (rc == PLP_OK) rc = launch(lo, hi, ptrs);
    }
    ctx->pool->finish();
    if (timing) {
        fprintf(stderr, "[stage] all enqueued at %.0f us\n", us());
        (void)hipStreamSynchronize(ctx->copy_stream);
        fprintf(stderr, "[stage] copies done at %.0f us\n", us());
        (void)hipStreamSynchronize(st);
        fprintf(stderr, "[stage] kernels done at %.0f us (%d chunks, %zu bytes)\n", us(), (int)nch, total);
    }
    if (rc == PLP_OK && ctx->pool->nonfinite()) rc = fail(PLP_ENONFINITE, "%s", NONFINITE_MSG);
    if (rc != PLP_OK) {  // nothing of this call may still be in flight when the caller sees the error
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(st);
    }
    return rc;
}

// copies the outputs to the host and synchronises the stream
int copy_out(plp_ctx* ctx, hipStream_t st, const Few<Span>& spans, bool via_stage) {
    // after a staged upload (plp_stage.hpp): the outputs (neighbours in the arena) come back as ONE copy into the pinned
    // staging buffer and the staging threads hand them out -- five pageable D2H copies of a C2 batch cost 1.5 ms
    // (`via_stage` = false: a call whose one or two large outputs measured faster as direct copies)
    if (via_stage && ctx->pool && ctx->stage) {
        size_t lo = ~(size_t)0, hi = 0;
        for (const Span& sp : spans) {
            if (!sp.bytes || !sp.host_out) continue;
            const size_t off = (size_t)(static_cast<char*>(sp.dev) - ctx->arena);
            lo = off < lo ? off : lo;
            hi = off + sp.bytes > hi ? off + sp.bytes : hi;
        }
        if (hi > lo && hi - lo >= SMALL_XFER && hi - lo <= ctx->stage_bytes) {
            HIP_TRY(hipMemcpyAsync(ctx->stage, ctx->arena + lo, hi - lo, hipMemcpyDeviceToHost, st));
            std::vector<std::vector<plp::StagePiece>> one(1);
            for (const Span& sp : spans)
                if (sp.bytes && sp.host_out)
                    one[0].push_back({ctx->stage + ((size_t)(static_cast<char*>(sp.dev) - ctx->arena) - lo),
                                      static_cast<char*>(sp.host_out), nullptr, sp.bytes});
            HIP_TRY(hipStreamSynchronize(st));
            ctx->pool->start(one);
            ctx->pool->wait(0);
            ctx->pool->finish();
            return PLP_OK;
        }
    }
    if (fits_small(ctx, spans) && ensure_pin(ctx) == PLP_OK) {
        size_t lo = SMALL_XFER, hi = 0;
        for (const Span& sp : spans) {
            if (!sp.bytes || !sp.host_out) continue;
            const size_t off = (size_t)(static_cast<char*>(sp.dev) - ctx->arena);
            lo = off < lo ? off : lo;
            hi = off + sp.bytes > hi ? off + sp.bytes : hi;
        }
        if (hi > lo) HIP_TRY(hipMemcpyAsync(ctx->pin + lo, ctx->arena + lo, hi - lo, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (const Span& sp : spans)
            if (sp.bytes && sp.host_out)
                memcpy(sp.host_out, ctx->pin + (size_t)(static_cast<char*>(sp.dev) - ctx->arena), sp.bytes);
        return PLP_OK;
    }
    for (const Span& sp : spans)
        if (sp.bytes && sp.host_out) HIP_TRY(hipMemcpyAsync(sp.host_out, sp.dev, sp.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PLP_OK;
}

// One host-pointer call.  Its arrays are declared once, in the order they take in the arena -- in(): the variable that
// receives the device pointer, the host pointer, the element count; out(): the same -- and everything else follows from
// the declarations: the arena size (256-byte padded slots), the device pointers (set by reserve(); NULL for an input
// whose host pointer is NULL, so an optional input needs no folding where it is used; an output always has its slot, a
// NULL host pointer only means it is not copied back), the upload and the download.
class HostCall {
  public:
    hipStream_t st;  // the context's stream: host-pointer calls run and synchronise on it
    // outputs of 1 MiB or more come back as one copy each, also when the context owns a staging buffer they could go
    // through (download; for the calls that have one or two large outputs: there the staging threads cost more than they save)
    bool direct_out = false;
    explicit HostCall(plp_ctx* c) : st(c->stream), ctx_(c) {}

    // `per_unit` > 0: the array holds that many elements per unit of the batch and may go up chunk by chunk
    // (upload_staged; such inputs are declared first).  `finite`: doubles checked for inf / nan when the context asks
    template <typename T>
    void in(T*& dev, const T* host, size_t count, size_t per_unit = 0, bool finite = false) {
        // (bytes = 0 when the host pointer is NULL: nothing to copy, and the slot does not count as in use)
        ins_.push_back({nullptr, host, nullptr, host ? count * sizeof(T) : 0});
        in_decl_.push_back({reinterpret_cast<void**>(&dev), off_, per_unit * sizeof(T), finite && std::is_same<T, double>::value});
        if (host) unit_bytes_ += per_unit * sizeof(T);
        off_ += pad(count * sizeof(T));
    }
    template <typename T>
    void out(T*& dev, T* host, size_t count) {
        outs_.push_back({nullptr, nullptr, host, host ? count * sizeof(T) : 0});
        out_decl_.push_back({reinterpret_cast<void**>(&dev), off_, 0, false});
        off_ += pad(count * sizeof(T));
    }

    // reserve / upload / download are forced inline: left to the compiler they stayed out of line, and a 60-80 us call
    // measured 0.7 us slower than with the same work written out in the entry point (profiles/hostcall_refactor_ab.json)
    // the arena holds the declared arrays (4096 bytes of headroom, as the calls always had); the device pointers are set
    __attribute__((always_inline)) int reserve() {
        if (ins_.overflow || outs_.overflow) return fail(PLP_EINVAL, "host call: more than 8 inputs or outputs");
        HIP_TRY(hipSetDevice(ctx_->device));
        int rc = ensure_arena(ctx_, off_ + 4096);
        if (rc) return rc;
        for (size_t i = 0; i < ins_.n; ++i) ins_.v[i].dev = ctx_->arena + in_decl_.v[i].off;
        for (size_t i = 0; i < outs_.n; ++i) *out_decl_.v[i].slot = outs_.v[i].dev = ctx_->arena + out_decl_.v[i].off;
        whole_inputs();
        return PLP_OK;
    }

    // the inputs, checked where flagged, go to the device (copy_in: one copy through the pinned mirror for a small call)
    __attribute__((always_inline)) int upload() {
        for (size_t i = 0; i < ins_.n; ++i) {
            if (!in_decl_.v[i].finite) continue;
            int rc = finite_or_fail(ctx_, static_cast<const double*>(ins_.v[i].host_in), ins_.v[i].bytes / 8);
            if (rc) return rc;
        }
        return copy_in(ctx_, st, ins_);
    }

    // Large batch of B units: the per-unit inputs go up chunk by chunk and `launch(lo, hi)` enqueues the kernels of units
    // [lo, hi) behind their chunk (staged_run) -- while it runs, the device pointers of those inputs point at the rows
    // of unit lo, so `launch` uses the declared variables as they are and offsets only its outputs.  *staged = false:
    // not applicable, nothing was done and the caller goes on with upload().
    template <typename F>
    int upload_staged(int64_t B, int64_t align, F launch, bool* staged) {
        *staged = false;
        if (unit_bytes_ * (size_t)B < STAGE_MIN_BYTES) return PLP_OK;  // (what staged_run would find: a small call stops here)
        Few<StageArray> arrays;
        char *lo = nullptr, *hi = nullptr;  // the block the per-unit inputs take in the arena (they are neighbours)
        for (size_t i = 0; i < ins_.n; ++i) {
            const Decl& d = in_decl_.v[i];
            if (!d.unit_bytes) continue;
            char* dev = static_cast<char*>(ins_.v[i].dev);
            arrays.push_back({ins_.v[i].host_in, dev, d.unit_bytes, d.finite});
            if (!lo) lo = dev;
            hi = dev + (size_t)B * d.unit_bytes;
        }
        int rc = staged_run(ctx_, st, B, align, arrays, lo, (size_t)(hi - lo),
                            [&](int64_t u0, int64_t u1, void* const* q) {
                                size_t k = 0;
                                for (const Decl& d : in_decl_)
                                    if (d.unit_bytes) *d.slot = q[k++];
                                return launch(u0, u1);
                            },
                            staged);
        whole_inputs();
        return rc;
    }

    // the outputs come back and the stream is synchronised (copy_out); may be called again after another launch
    __attribute__((always_inline)) int download() { return copy_out(ctx_, st, outs_, !direct_out); }

  private:
    struct Decl {
        void** slot;  // the caller's device-pointer variable
        size_t off;   // offset in the arena
        size_t unit_bytes;
        bool finite;
    };
    void whole_inputs() {
        for (size_t i = 0; i < ins_.n; ++i) *in_decl_.v[i].slot = ins_.v[i].host_in ? ins_.v[i].dev : nullptr;
    }
    plp_ctx* ctx_;
    size_t off_ = 0, unit_bytes_ = 0;
    Few<Span> ins_, outs_;        // what copy_in / copy_out take, built as the arrays are declared
    Few<Decl> in_decl_, out_decl_;
};

// the inputs cheby, bbox and reduce share, as the first arrays of their host-pointer calls
void declare_Abm(HostCall& hc, int64_t B, int m_max, int d, double*& dA, const double* A, double*& db, const double* b,
                 int32_t*& dm, const int32_t* m) {
    const size_t md = (size_t)m_max * d;
    hc.in(dA, A, (size_t)B * md, md, true);
    hc.in(db, b, (size_t)B * m_max, m_max, true);
    hc.in(dm, m, B, 1);
}

// reserve; the staged upload with `launch(lo, hi)` per chunk, or the plain upload and one launch(0, B); download
template <typename F>
int run_Abm(HostCall& hc, int64_t B, int64_t align, F launch) {
    int rc = hc.reserve();
    if (rc) return rc;
    bool staged = false;  // large batches: chunked upload, kernels of earlier chunks running meanwhile (plp_stage.hpp)
    rc = hc.upload_staged(B, align, launch, &staged);
    if (rc) return rc;
    if (!staged) {
        rc = hc.upload();
        if (rc) return rc;
        rc = launch(0, B);
        if (rc) return rc;
    }
    return hc.download();
}

// the outputs reduce and reduce_wide share (kw keep words per polytope), after their inputs
void declare_reduce_outs(HostCall& hc, int64_t B, int d, size_t kw, uint64_t*& dkeep, uint64_t* keep, int32_t*& dfl,
                         int32_t* flags, double*& dr, double* r, double*& dxc, double* xc, int32_t*& dnlp, int32_t* nlp) {
    hc.out(dkeep, keep, (size_t)B * kw);
    hc.out(dfl, flags, B);
    hc.out(dr, r, B);
    hc.out(dxc, xc, (size_t)B * d);
    hc.out(dnlp, nlp, B);
}


// the four pair operations (adjacency, overlap): a table of `cells` cells in, `nout` bytes out; `run(st, dA, db, dm, dout)`
// is the operation's device-pointer entry point on the uploaded table
template <typename F>
int pairs_host(plp_ctx* ctx, size_t cells, int m_max, int d, const double* A, const double* b, const int32_t* m, uint8_t* out,
               size_t nout, F run) {
    double *dA, *db;
    int32_t* dm;
    uint8_t* dout;
    HostCall hc(ctx);
    hc.in(dA, A, cells * m_max * d);
    hc.in(db, b, cells * m_max);
    hc.in(dm, m, cells);
    hc.out(dout, out, nout);
    hc.direct_out = true;
    int rc = hc.reserve();
    if (rc) return rc;
    rc = hc.upload();
    if (rc) return rc;
    rc = run(hc.st, dA, db, dm, dout);
    if (rc) return rc;
    return hc.download();
}

}  // namespace
