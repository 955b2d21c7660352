// Host-side pieces shared by the training steps (farnn_train.hip): the carver that sizes and lays out a workspace with one piece
// of code, step profiling, the pinned error word, and the launches both steps make (DevBuf and launch: host_util.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include <vector>
#include "host_util.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

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
    int time(int device, double *total_ms, int64_t *steps) {      // farnn_train_time / farnn_onehot_train_time
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
// count / scan (the counts in LDS when they fit) / fill; b.cnt is zero before.  err: the step's error word (bit 1: a word
// outside 0..V-1) or null
inline int launch_bucketing(const int64_t *x, const int64_t *len, int B, int L, int V, const Buckets &b, int *err, hipStream_t s) {
    const int nch = bucket_chunks((size_t)B * L);
    const size_t lds_s = (size_t)V * nch * sizeof(int) <= 144 * 1024 ? (size_t)V * nch * sizeof(int) : 0;
    onehot_bucket_count_kernel<<<nch, OT_CH, 0, s>>>(x, len, B, L, V, nch, b.cnt, err);
    if (int rc = launch(onehot_bucket_scan_kernel, 1, 1024, lds_s, s, b.cnt, V, nch, b.wstart, b.wcount, b.itoff, b.psoff,
                        lds_s ? V * nch : 0)) return rc;
    onehot_bucket_fill_kernel<<<nch, OT_CH, 0, s>>>(x, len, B, L, V, nch, b.cnt, b.list);
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

}  // namespace farnn
