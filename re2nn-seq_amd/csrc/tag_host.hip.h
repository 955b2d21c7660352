// Host-side pieces of the tagging library's one translation unit (farnn_hip.hip): the handle, its workspace, the owner of a
// handle under construction, the scoped device temporaries and the upload helpers.  Included by farnn_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include <new>
#include <vector>

#include "common.hip.h"
#include "host_util.hip.h"
#include "chain.hip.h"
#include "layout.hip.h"
#include "decomp_chain.hip.h"
#include "decomp_rows.hip.h"
#include "decomp_vec.hip.h"
#include "chain_regs_params.hip.h"
#include "tag_plan.hip.h"

using namespace farnn;

enum { KIND_IFST = 2, KIND_IND1 = 1, KIND_FST4 = 0, KIND_DECOMP = 12, KIND_DECOMP1 = 11, KIND_DECOMP0 = 10 };
enum { KERN_CHAIN = 0, KERN_SCORE = 1, KERN_PREP = 2, KERN_TABLE = 3 /* token_table_kernel / token_blocks_kernel (farnn_tag_vectors) */, KERN_COUNT = 4 };

struct Prof {
    std::vector<hipEvent_t> ev[KERN_COUNT];   // (start, stop) pairs
    std::vector<hipEvent_t> pool;             // events created ahead of the timed region (farnn_set_profiling)
    double ms[KERN_COUNT] = {};
    long long n[KERN_COUNT] = {};
    hipEvent_t get() {
        hipEvent_t e = nullptr;
        if (!pool.empty()) { e = pool.back(); pool.pop_back(); return e; }
        return hipEventCreate(&e) == hipSuccess ? e : nullptr;
    }
};

// The per-handle workspace (farnn_reserve): it only grows, and every buffer is listed ONCE, in release().
struct Workspace {
    float *A = nullptr, *Bk = nullptr;      // the two chains' stashes [B][L+1][SP]
    int64_t *offs = nullptr;
    int *order = nullptr;
    unsigned long long *hs = nullptr;       // hand-off words of the register-fed kernels: progress [2][B], arrival [B] (64-bit each)
    size_t hs_bytes = 0;
    float *crf_scores = nullptr;
    float *d1_br = nullptr;                 // [B*L][MT][NT*16] per-row-tile partial output-rank vectors (decomposed independent=1)
    float *tt = nullptr;                    // [B*L][tvl] the call's token table (a vector-input handle: decomp_vec.hip.h)
    int64_t *ids = nullptr;                 // [B*L] ids[i] = i: the identity ids its recurrence runs on
    float *tbf = nullptr, *tbb = nullptr;   // [tokens][SR][SP] the call's token blocks and their transposes (a max-semiring vector-input handle)
    int B = 0, L = 0;                       // CAPACITY: sequences, positions
    void release() {
        for (void *p : {(void *)A, (void *)Bk, (void *)offs, (void *)order, (void *)hs, (void *)crf_scores, (void *)d1_br, (void *)tt, (void *)ids, (void *)tbf, (void *)tbb})
            if (p) (void)hipFree(p);
        *this = Workspace();
    }
};

struct farnn_model {
    Tunables tun;                           // the FARNN_* switches as they stood when the handle was created (host_util.hip.h)
    int kind = 0, device = 0;
    int V = 0, S = 0, SP = 0, C = 0, K = 0, Kp = 0, Kc = 0, R = 0, Rp = 0;
    int nl = 0, semiring = 0, o_idx = 0, use_crf = 0, farnn_gate = 0, mask_by_output = 0;
    float threshold = 0.5f, sig_k = 1.0f;
    // device-resident, library-owned weights
    float *Mf = nullptr, *Mb = nullptr;     // chain blocks [V][S][SP] (+ transposed)
    unsigned short *Mf16 = nullptr, *Mb16 = nullptr;   // their 16-bit image [V][SP][80] f16, when every entry is an f16 exactly (build_half_image)
    u64 *bmF = nullptr, *bmB = nullptr, *bmWF = nullptr, *bmWB = nullptr;   // compact form: bit-packed blocks (compact.hip.h)
    int bmNS = 0;                           // 64-bit words per bitmap row; 0: no compact form
    u64 *bmMF = nullptr, *bmMB = nullptr, *bmXF = nullptr, *bmXB = nullptr;   // K1t's planes: T | W, T & W (merge_planes_kernel; S <= 128)
    unsigned *bmTok = nullptr;              // [V] block offset | second-plane flag
    bool compact_on = false;                // farnn_set_compact: the recurrence walks the bitmaps instead of the dense blocks
    float *Ms = nullptr;                    // ind1: unmasked blocks for scoring
    float *A4 = nullptr;                    // fst4: [V][C][S][SP] premixed T4+W4
    float *Oten = nullptr;                  // ind1: [C][S][SP]
    float *o = nullptr, *h0 = nullptr, *hT = nullptr;
    bool o_ones = false;                    // every entry of o below S is exactly 1.0f (build_output_matrix: a device-side test at create)
    float *OT = nullptr, *P = nullptr, *tr = nullptr;
    float *OTm = nullptr; int c16 = 0;       // matrix-core image of OT for score_tiles (ot_to_mfma_kernel)
    LabelMap lm = {nullptr, 0, 0, -1, 0.0f, 0, 0, 0.0f}; // the output matrix as a label map, when it is one (label_map.hip.h)
    DecompWeights dw;                       // decomposed model weights
    DecompRowsPack rows;                    // packed rows of the K12 rows kernel (sum semiring)
    int RO = 0, ROp = 0;                    // decomposed independent=1: output factors
    float *d1_S1o = nullptr, *d1_S2o = nullptr, *d1_CoutT = nullptr;
    float *d1_BSSp = nullptr;               // [V][MT][KQ4][64][4] per-word bss = sum_r S1 S2 v + W in MFMA operand order
    float *d1_S1oP = nullptr;               // [MT][NT][64][4] S1o in MFMA accumulator order
    float *d1_S2oP = nullptr;               // [KQ4][NT][64][4] S2o in MFMA operand order
    int n_cu = 0;                           // compute units of the device (persistent launches)
    int RW = 0, RWp = 0;                    // decomposed independent=0: wildcard factors + label factor
    float *d0_Vgen = nullptr, *d0_CT = nullptr, *d0_S1w = nullptr, *d0_S2w = nullptr, *d0_CwT = nullptr;
    Workspace ws;
    ChainGeom geom;
    RegsGeom rgeom;                         // geometry of the register-fed recurrence kernel (chain_regs.hip.h); rgeom.ok: usable
    unsigned epoch_u = 0;                   // diagnostic FARNN_HOST_EPOCH=1: the round-3 host-side epoch
    TagPlan plan;                           // the plan of the last farnn_tag call (tag_plan.hip.h); plan.planned false: none yet
    // the one field remembered beside the plan: the last STAND-ALONE score launch was label_map_score_kernel (K2l).  A call that
    // launches no score kernel leaves it as it was, and farnn_kernel_name(KERN_SCORE) goes on reporting the older call's answer
    bool last_lm_score = false;
    int chain_ks = 3;
    bool dense_decomp = false;              // decomposed model served by dense per-word blocks + chain_kernel
    bool sf = false;                        // vector input (farnn_decomp_sf_create): no word table, V = 0; farnn_tag_vectors builds a token table per call
    // ... in the max semiring (farnn_decomp_sf_max_create): per call one S x S block per token (token_blocks_kernel) in front of the
    // dense chain kernels where sf_dense (farnn = 0 and the chain geometry holds the model), up to sf_block_tokens positions a call;
    // else the padded copy of v (token_table_kernel<false>) under decomp_chain_kernel
    bool sf_max = false, sf_dense = false;
    long long sf_block_tokens = 0;
    int profiling = 0;          // 0 off, N>0: time every N-th farnn_tag call
    long long calls = 0;
    int prof_this_call = 0;
    Prof prof;
    std::vector<void *> owned;              // everything to hipFree at destroy
    // host-buffer path (farnn_tag_host_*): pinned staging + device twins per in-flight batch, three streams
    struct HostSlot {
        int64_t *x_pin = nullptr, *flat_pin = nullptr;      // [x | lengths] staged together; flat predictions
        int64_t *x_dev = nullptr, *flat_dev = nullptr, *x_map = nullptr;   // device copy of x; device views of the pinned buffers
        size_t capN = 0, capB = 0;
        long long total = 0;
        hipEvent_t ev_out = nullptr;
        bool busy = false;
        unsigned gen = 0;                   // submits this slot has seen: a ticket = slot | gen << 8, so a stale ticket cannot consume a newer batch
    } hslot[FARNN_HOST_SLOTS];
    hipStream_t hs_run = nullptr;
    int hnext = 0;
    // stream ordering of the handle's ONE workspace (stash, hand-off words, launch order): a call on another stream than the
    // previous call's waits for that call's work first
    hipStream_t last_stream = nullptr;
    bool have_last = false, multi_stream = false;
    hipEvent_t ev_order = nullptr;
};

// A handle under construction: a create holds it here and releases it into *out on its last line, so every return in between
// (the ones inside FARNN_HIP_TRY included) destroys the handle and everything in m->owned.
struct DestroyModel { void operator()(farnn_model *m) const { farnn_destroy(m); } };
using ModelOwner = std::unique_ptr<farnn_model, DestroyModel>;

// The device temporaries of a create: whatever is taken here is freed when the scope ends, on every path.
struct DevTmp {
    std::vector<void *> held;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { for (void *p : held) (void)hipFree(p); }
    template <typename T>
    int raw(T **q, size_t count) {                       // uninitialised
        FARNN_HIP_TRY(hipMalloc((void **)q, count ? count * sizeof(T) : 4));
        held.push_back(*q);
        return FARNN_OK;
    }
    template <typename T>
    int zeros(T **q, size_t count) {
        if (int rc = raw(q, count)) return rc;
        FARNN_HIP_TRY(hipMemset(*q, 0, count * sizeof(T)));
        return FARNN_OK;
    }
    template <typename T>
    int copy(T **q, const T *src, size_t count, int on_device) {       // a copy of its own of a (host|device) array
        if (int rc = raw(q, count)) return rc;
        FARNN_HIP_TRY(hipMemcpy(*q, src, count * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        return FARNN_OK;
    }
    // a device view of a (host|device) array: a device pointer (and NULL) passes through, a host array is staged
    int view(const float **q, const float *src, size_t count, int on_device) {
        *q = src;
        if (on_device || !src) return FARNN_OK;
        float *dv = nullptr;
        if (int rc = copy(&dv, src, count, 0)) return rc;
        *q = dv;
        return FARNN_OK;
    }
};

// ---- uploads into memory the handle owns -------------------------------------------------------
static int dev_alloc(farnn_model *m, void **p, size_t bytes) {
    // +1 KiB slack: LDS-DMA moves whole 1 KiB pieces, the last piece of a table may run past its end
    FARNN_HIP_TRY(hipMalloc(p, bytes + 1024));
    m->owned.push_back(*p);
    return FARNN_OK;
}

// copy (host or device) floats into a fresh device buffer of `n_alloc` floats (zero padded)
static int dev_upload(farnn_model *m, float **dst, const float *src, size_t n, size_t n_alloc,
                      int on_device) {
    int rc = dev_alloc(m, (void **)dst, n_alloc * sizeof(float));
    if (rc) return rc;
    FARNN_HIP_TRY(hipMemset(*dst, 0, n_alloc * sizeof(float)));
    if (src && n)
        FARNN_HIP_TRY(hipMemcpy(*dst, src, n * sizeof(float),
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return FARNN_OK;
}

// rows x cols (row-major, host|device) -> device [rows_alloc][cols_p], zero padded
static int upload_padded(farnn_model *m, float **dst, const float *src, int rows, int cols,
                         int rows_alloc, int cols_p, int on_device) {
    int rc = dev_alloc(m, (void **)dst, (size_t)rows_alloc * cols_p * sizeof(float));
    if (rc) return rc;
    FARNN_HIP_TRY(hipMemset(*dst, 0, (size_t)rows_alloc * cols_p * sizeof(float)));
    if (src)
        FARNN_HIP_TRY(hipMemcpy2D(*dst, (size_t)cols_p * 4, src, (size_t)cols * 4, (size_t)cols * 4,
                                  rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return FARNN_OK;
}

// transposed upload: src [rows][cols] -> dst [cols][rows_p]
static int upload_transposed(farnn_model *m, float **dst, const float *src, int rows, int cols,
                             int rows_p, int on_device) {
    DevTmp tmp;
    const float *t = nullptr;
    int rc = tmp.view(&t, src, (size_t)rows * cols, on_device);
    if (rc) return rc;
    rc = dev_alloc(m, (void **)dst, (size_t)cols * rows_p * sizeof(float));
    if (rc) return rc;
    FARNN_HIP_TRY(hipMemset(*dst, 0, (size_t)cols * rows_p * sizeof(float)));
    int n = rows * cols;
    transpose_pad_kernel<<<(n + 255) / 256, 256>>>(t, *dst, rows, cols, rows_p);
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipDeviceSynchronize());
    return FARNN_OK;
}
