// Host-side pieces shared by the five training steps (farnn_train.hip): the carver that sizes and lays out a workspace with one
// piece of code, step profiling, the pinned error word, the handle every training context is and its life cycle, the driver
// every step entry point goes through, and the launches several steps make (DevBuf and launch: host_util.hip.h).  What the
// three steps over bucketed per-word blocks share beyond that is in train_bucketed.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "host_util.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"
#include "train_teacher.hip.h"

namespace farnn {

// One piece of code gives a workspace's size and its layout: a carve function calls take() once per array.  Run on a null base
// it only counts (`off` is the total); run on the buffer it hands out the pointers.  A sum cannot drift from its walk.
template <typename T>
struct Carver {
    T *base;
    size_t off = 0;
    explicit Carver(T *b) : base(b) {}
    T *take(size_t count) { T *r = base ? base + off : nullptr; off += count; return r; }
};

// Step timing with HIP event pairs (farnn_*_set_profiling / farnn_*_time).
struct StepProfile {
    int enabled = 0;
    double ms = 0.0;
    int64_t n = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // recorded pairs, not yet read
    hipEvent_t e0 = nullptr, e1 = nullptr;                    // the pair of the step under way
    struct Guard {                                            // a step that returns before end() leaves no pair behind
        StepProfile *prof;
        ~Guard() { prof->drop(); }
    };
    ~StepProfile() { drop(); drain(nullptr, nullptr); }
    Guard begin(hipStream_t s) {
        if (enabled && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) (void)hipEventRecord(e0, s);
        else drop();
        return Guard{this};
    }
    void end(hipStream_t s) {
        if (e0) { (void)hipEventRecord(e1, s); pending.emplace_back(e0, e1); }
        e0 = e1 = nullptr;
    }
    void drop() {                                             // destroys an unrecorded pair
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
    }
    // after a device synchronize: adds the pending pairs' times, reports and resets the totals (null arguments: only cleans up)
    void drain(double *total_ms, int64_t *steps) {
        for (auto &e : pending) {
            float t = 0.0f;
            if (total_ms && hipEventElapsedTime(&t, e.first, e.second) == hipSuccess) { ms += t; n++; }
            (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
        }
        pending.clear();
        if (total_ms) { *total_ms = ms; *steps = n; ms = 0.0; n = 0; }
    }
    int time(int device, double *total_ms, int64_t *steps) {      // train_ctx_time
        FARNN_HIP_TRY(hipSetDevice(device));
        FARNN_HIP_TRY(hipDeviceSynchronize());
        drain(total_ms, steps);
        return FARNN_OK;
    }
};

// One int in pinned, device-mapped host memory.  The kernels set its bits straight there (only on bad input is it touched);
// the next step reads it at its top without a synchronize.
struct ErrWord {
    volatile int *host = nullptr;
    int *dev = nullptr;               // the device's address of *host
    ~ErrWord() { if (host) (void)hipHostFree((void *)host); }
    bool create() {
        if (hipHostMalloc((void **)&host, sizeof(int), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void **)&dev, (void *)host, 0) != hipSuccess) return false;
        *host = 0;
        return true;
    }
    // *bits = what earlier steps' kernels set (0: nothing), cleared; the stream is synchronized only when something is set
    int take(hipStream_t s, int *bits) {
        if ((*bits = *host)) { FARNN_HIP_TRY(hipStreamSynchronize(s)); *bits = *host; *host = 0; }
        return FARNN_OK;
    }
};

// ---- the handle of a training step (farnn_*train_ctx) and its life cycle --------------------------------------------------
// `name` is the step's prefix in every message: "train", "onehot_train", "fst4_train", "ind1_train", "decomp_ind1_train".
struct TrainCtxBase {
    int device = 0;
    StepProfile prof;
    ErrWord err;                      // bit 0 a bad label, bit 1 a word outside 0..V-1 (the steps that bucket with it)
};
template <typename Ctx>
inline void train_ctx_destroy(Ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;                         // the buffers, the events and the error word free themselves
}
// the tail of every create, after the step's own checks of the dimensions
template <typename Ctx, typename Dims>
inline int train_ctx_create(const char *name, const Dims *d, int device, Ctx **out) {
    if (int rc = select_device(device)) return rc;
    Ctx *c = new Ctx();
    c->d = *d; c->device = device;
    if (!c->err.create()) { train_ctx_destroy(c); return fail(FARNN_ENOMEM, "%s_create: out of memory%s", name); }
    *out = c;
    return FARNN_OK;
}
inline int train_ctx_set_profiling(const char *name, TrainCtxBase *c, int32_t enable) {
    if (!c) return fail(FARNN_EINVAL, "%s_set_profiling: null context%s", name);
    c->prof.enabled = enable;
    return FARNN_OK;
}
inline int train_ctx_time(const char *name, TrainCtxBase *c, double *total_ms, int64_t *steps) {
    if (!c || !total_ms || !steps) return fail(FARNN_EINVAL, "%s_time: null argument%s", name);
    return c->prof.time(c->device, total_ms, steps);
}

// ---- one step, for every farnn_*_train_step ------------------------------------------------------------------------------
// A Step names itself (Step::name) and its label range (Step::label_range: "K" or "C"), holds c / w / o / s, and supplies
// validate() (its weights and outputs), plan(B, L) (host arithmetic only: every size the step refuses is refused there, before
// anything is enqueued), carve(...) (grow the buffers, lay the workspaces out, fill the kernels' parameters) and stages() (the
// launches, in order).  A step that returns before the end leaves no event pair behind (StepProfile::Guard).
// `more`: what an entry point hands its step beyond the common arguments (the teacher of farnn_decomp_ifst_teacher_train_step).
struct NoMore { template <typename Step> void operator()(Step &) const {} };
template <typename Step, typename Ctx, typename W, typename O, typename More = NoMore>
inline int run_train_step(Ctx *c, const W *w, const int64_t *x, const int64_t *lengths, const int64_t *labels, int B, int L,
                          int64_t valid_tokens, const O *o, void *stream, More more = More()) {
    if (!c || !w || !x || !lengths || !labels || !o) return fail(FARNN_EINVAL, "%s_step: null argument%s", Step::name);
    Step t = {};
    t.c = c; t.w = w; t.o = o; t.s = reinterpret_cast<hipStream_t>(stream);
    more(t);
    int rc, bad = 0;
    if ((rc = t.validate())) return rc;
    if (B <= 0 || L <= 0 || valid_tokens <= 0) return fail(FARNN_EINVAL, "%s_step: B, L and valid_tokens must be positive%s", Step::name);
    if ((rc = t.plan(B, L))) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->err.take(t.s, &bad))) return rc;
    if (bad & 2) return fail(FARNN_EINVAL, "%s_step: an earlier step saw a word outside 0..V-1 at a valid position (torch raises on it); that step clamped it%s", Step::name);
    if (bad) return fail(FARNN_EINVAL, "%s_step: an earlier step saw a label outside 0..%s-1 at a valid position (torch's CrossEntropyLoss raises on it); that step counted it as label 0", Step::name, Step::label_range);
    if ((rc = t.carve(x, lengths, labels, valid_tokens))) return rc;
    StepProfile::Guard timing = c->prof.begin(t.s);
    if ((rc = t.stages())) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    c->prof.end(t.s);
    return FARNN_OK;
}
// the two workspaces of the steps that bucket the positions (ws: floats, iws: ints)
template <typename Ctx>
inline int grow_workspaces(const char *name, Ctx *c, size_t need, size_t ineed) {
    if (int rc = c->ws.ensure(need, "%s_step: out of device memory for the workspace%s", name)) return rc;
    return c->iws.ensure(ineed, "%s_step: out of device memory for the index workspace%s", name);
}

// ---- the positions of a batch bucketed by word (onehot_train.hip.h) ------------------------------------------------------
struct Buckets {
    int *cnt, *wstart, *wcount, *itoff, *psoff, *list;   // [V][nch] counts per chunk, per-word tables, the sorted positions [B L]
};
inline int bucket_chunks(size_t N0) { return (int)((N0 + OT_CH - 1) / OT_CH); }
inline void carve_buckets(Carver<int> &a, Buckets &b, size_t V, size_t N0) {
    b.cnt = a.take(V * (size_t)bucket_chunks(N0));
    b.wstart = a.take(V); b.wcount = a.take(V); b.itoff = a.take(V + 1); b.psoff = a.take(V + 1);
    b.list = a.take(N0);
}
inline size_t carve_bucket_ints(int *base, Buckets &b, size_t V, size_t N0) { Carver<int> a(base); carve_buckets(a, b, V, N0); return a.off; }
inline int clear_bucket_counts(const Buckets &b, size_t V, size_t N0, hipStream_t s) {
    FARNN_HIP_TRY(hipMemsetAsync(b.cnt, 0, V * (size_t)bucket_chunks(N0) * sizeof(int), s));
    return FARNN_OK;
}
// count / scan (the counts in LDS when they fit) / fill; b.cnt is zero before.  err: the step's error word (bit 1: a word
// outside 0..V-1) or null.  all: every one of the B L positions is counted and listed, the pads included (the teacher's max step)
inline int launch_bucketing(const int64_t *x, const int64_t *len, int B, int L, int V, const Buckets &b, int *err, hipStream_t s,
                            bool all = false) {
    const int nch = bucket_chunks((size_t)B * L);
    const size_t lds_s = (size_t)V * nch * sizeof(int) <= 144 * 1024 ? (size_t)V * nch * sizeof(int) : 0;
    if (all) onehot_bucket_count_all_kernel<<<nch, OT_CH, 0, s>>>(x, B, L, V, nch, b.cnt, err);
    else onehot_bucket_count_kernel<<<nch, OT_CH, 0, s>>>(x, len, B, L, V, nch, b.cnt, err);
    if (int rc = launch(onehot_bucket_scan_kernel, 1, 1024, lds_s, s, b.cnt, V, nch, b.wstart, b.wcount, b.itoff, b.psoff,
                        lds_s ? V * nch : 0)) return rc;
    if (all) onehot_bucket_fill_all_kernel<<<nch, OT_CH, 0, s>>>(x, B, L, V, nch, b.cnt, b.list);
    else onehot_bucket_fill_kernel<<<nch, OT_CH, 0, s>>>(x, len, B, L, V, nch, b.cnt, b.list);
    return FARNN_OK;
}

// ---- train_loss_kernel<CLDS, PHASE> (train.hip.h): the scores, the loss, the decode and the adjoints of both chains' states ----
// Its LDS: the vectors of 8 wavefronts (a padded state row and 2 K scores each), and the score matrix [K][S+1] beside them
// (CLDS) when both fit 150 KiB -- else it is read through L2.
struct LossLds {
    size_t vec, mat;
    bool clds() const { return vec + mat <= 150 * 1024; }
    size_t bytes() const { return vec + (clds() ? mat : 0); }
};
inline LossLds train_loss_lds(size_t S, size_t K) {
    return {8 * (((S + 3) & ~(size_t)3) + 8 + 2 * K) * sizeof(float), ((K * (S + 1) + 3) & ~(size_t)3) * sizeof(float)};
}
template <int PHASE>
inline int launch_train_loss(const TrainParams &p, unsigned grid, hipStream_t s) {
    const LossLds l = train_loss_lds(p.S, p.K);
    return l.clds() ? launch(train_loss_kernel<true, PHASE>, grid, 512, l.bytes(), s, p)
                    : launch(train_loss_kernel<false, PHASE>, grid, 512, l.bytes(), s, p);
}

// train_teacher_loss_kernel<CLDS, PHASE> (train_teacher.hip.h): four score-wide vectors per wavefront instead of two
inline LossLds train_teacher_lds(size_t S, size_t K) {
    return {8 * (((S + 3) & ~(size_t)3) + 8 + 4 * K) * sizeof(float), ((K * (S + 1) + 3) & ~(size_t)3) * sizeof(float)};
}
template <int PHASE>
inline int launch_teacher_loss(const TrainParams &p, unsigned grid, hipStream_t s) {
    const LossLds l = train_teacher_lds(p.S, p.K);
    return l.clds() ? launch(train_teacher_loss_kernel<true, PHASE>, grid, 512, l.bytes(), s, p)
                    : launch(train_teacher_loss_kernel<false, PHASE>, grid, 512, l.bytes(), s, p);
}

// the loss of a step whose loss kernel leaves per-wavefront partials (8 per workgroup), added in order
inline void launch_loss_sum(const float *loss_part, unsigned lgrid, float *loss, hipStream_t s) {
    onehot_loss_sum_kernel<<<1, 64, 0, s>>>(loss_part, (int)lgrid * 8, loss);
}

// ---- the kernel forms picked by S: go(int_c<N>()) with the one instantiation that holds the size ------------------------------
// register slots per thread of the onehot chain kernels (sum and max semiring)
template <typename F>
inline int with_chain_slots(size_t S, F &&go) {
    return S <= 64 ? go(int_c<8>()) : S <= 72 ? go(int_c<18>()) : S <= 96 ? go(int_c<24>()) : go(int_c<32>());
}
// register rows per thread of the score kernels in bucket order and of decomp1_back_kernel (GW: row groups per wavefront)
template <typename F>
inline int with_rows_per_thread(size_t S, int GW, F &&go) {
    const int rows = (int)((S + 4 * GW - 1) / (4 * GW));
    return rows <= 4 ? go(int_c<4>()) : rows <= 6 ? go(int_c<6>()) : rows <= 8 ? go(int_c<8>()) : rows <= 12 ? go(int_c<12>()) : go(int_c<16>());
}

}  // namespace farnn
