// libfarnn_hip.so -- float64 CP-ALS of a 3-way or 4-way tensor given as a coordinate list (farnn_cp_*; include/farnn.h, DESIGN.md
// rows f12, f13): the step from an automaton's tensor to the factors of IIID / IID / D.automata.*.pkl (reference
// wfa/tensor_func.py, which calls tensorly.parafac with init='random', normalize_factors=False).  The kernels are in cp_als.hip.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hip.h"
#include "cp_als.hip.h"
#include "host_util.hip.h"

using namespace farnn;

namespace {

constexpr int CP_MAX_ORDER = 4;

struct CpModeOrder {                 // the nonzeros grouped by this mode's index (stable: ties keep the canonical order)
    DevBuf<int> ints;                // chunk_beg | chunk_end | chunkptr | ia | ib [| ic]
    DevBuf<double> val;
    const int *chunk_beg = nullptr, *chunk_end = nullptr, *chunkptr = nullptr, *ia = nullptr, *ib = nullptr, *ic = nullptr;
    int nchunks = 0, panels = 0;
};

}  // namespace

struct farnn_cp_ctx {
    int device = 0;
    int order = 3;
    int dims[CP_MAX_ORDER] = {0, 0, 0, 0};
    long long nnz = 0;               // after repeated coordinates were added up
    int max_rank = 0;                // what the buffers hold: min(the caller's max_rank, CP_MAX_RANK)
    int asked_rank = 0;
    double normx2 = 0.0;
    CpModeOrder mode[CP_MAX_ORDER];
    DevBuf<double> part;             // [max chunks][R]
    DevBuf<double> gram[CP_MAX_ORDER];     // [panels][R][R] per mode
    DevBuf<double> H, L, Lt, M;      // [R][R] x 3, [max dim][R]
    DevBuf<double> F[CP_MAX_ORDER];  // the run's factors
    DevBuf<CpSlot> slot;
    CpSlot *host = nullptr;          // pinned
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int profiling = 0;
    double stage_ms[4] = {0, 0, 0, 0};     // normal matrix, MTTKRP, solve, error
    long long stage_n = 0;                 // timed sweeps
};

// the other modes of `mode`, ascending, into o[order - 1]
static void cp_others(int order, int mode, int *o) {
    for (int m = 0, k = 0; m < order; m++)
        if (m != mode) o[k++] = m;
}

static int cp_check_rank(const farnn_cp_ctx *c, int rank, const char *who) {
    if (rank < 1) return fail(FARNN_EINVAL, "%s: rank must be positive%s", who);
    if (rank > CP_MAX_RANK) return fail(FARNN_ERANGE, "%s: rank beyond the kernels' cap of 352%s", who);
    if (rank > c->asked_rank) return fail(FARNN_ERANGE, "%s: rank above the context's max_rank%s", who);
    return FARNN_OK;
}

static int cp_gram(farnn_cp_ctx *c, int m, const double *F, int R, hipStream_t s) {
    const int tiles = (R + 15) / 16;
    cp_gram_kernel<<<dim3(tiles, tiles, c->mode[m].panels), WAVE, 0, s>>>(F, c->dims[m], R, c->gram[m].p);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

static int cp_hadamard(farnn_cp_ctx *c, int mode, int R, double *H, hipStream_t s) {
    int o[CP_MAX_ORDER];
    cp_others(c->order, mode, o);
    const int a = o[0], b = o[1];
    const int blocks = (R * R + CP_THREADS - 1) / CP_THREADS;
    if (c->order == 3)
        cp_hadamard_kernel<2><<<blocks, CP_THREADS, 0, s>>>(c->gram[a].p, c->mode[a].panels, c->gram[b].p, c->mode[b].panels, nullptr, 0,
                                                            R, H);
    else
        cp_hadamard_kernel<3><<<blocks, CP_THREADS, 0, s>>>(c->gram[a].p, c->mode[a].panels, c->gram[b].p, c->mode[b].panels,
                                                            c->gram[o[2]].p, c->mode[o[2]].panels, R, H);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

static int cp_mttkrp(farnn_cp_ctx *c, int mode, int R, const double *const *f, double *out, hipStream_t s) {
    const CpModeOrder &o = c->mode[mode];
    int oth[CP_MAX_ORDER];
    cp_others(c->order, mode, oth);
    const double *Fa = f[oth[0]], *Fb = f[oth[1]];
    const dim3 block(64, 4), grid((o.nchunks + 3) / 4, (R + 63) / 64);
    if (c->order == 3)
        cp_mttkrp_chunk_kernel<3><<<grid, block, 0, s>>>(o.chunk_beg, o.chunk_end, o.nchunks, o.ia, o.ib, nullptr, o.val.p, Fa, Fb, nullptr,
                                                         R, c->part.p);
    else
        cp_mttkrp_chunk_kernel<4><<<grid, block, 0, s>>>(o.chunk_beg, o.chunk_end, o.nchunks, o.ia, o.ib, o.ic, o.val.p, Fa, Fb, f[oth[2]],
                                                         R, c->part.p);
    FARNN_HIP_TRY(hipGetLastError());
    cp_mttkrp_row_kernel<<<dim3((c->dims[mode] + 3) / 4, (R + 63) / 64), block, 0, s>>>(o.chunkptr, c->dims[mode], R, c->part.p, out);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

static int cp_solve(farnn_cp_ctx *c, int R, const double *H, const double *M, int rows, double *out, hipStream_t s) {
    int rc;
    if ((rc = launch(cp_cholesky_kernel, dim3(1), dim3(CP_THREADS), (size_t)2 * CP_NB * R * sizeof(double), s, H, R, c->L.p, c->Lt.p,
                     c->slot.p)))
        return rc;
    FARNN_HIP_TRY(hipGetLastError());
    if ((rc = launch(cp_trisolve_kernel, dim3((rows + CP_TILE - 1) / CP_TILE), dim3(CP_THREADS), (size_t)CP_TILE * R * sizeof(double), s,
                     (const double *)c->L.p, (const double *)c->Lt.p, R, M, rows, out)))
        return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// the slot behind everything enqueued on `s`; a set flag is cleared, so the context stays usable
static int cp_read_slot(farnn_cp_ctx *c, hipStream_t s, const char *who) {
    FARNN_HIP_TRY(hipMemcpyAsync(c->host, c->slot.p, sizeof(CpSlot), hipMemcpyDeviceToHost, s));
    FARNN_HIP_TRY(hipStreamSynchronize(s));
    if (c->host->flag) {
        FARNN_HIP_TRY(hipMemsetAsync(c->slot.p, 0, sizeof(CpSlot), s));
        return fail(FARNN_ENUMERIC, "%s: a Cholesky pivot of the normal matrix was not a positive finite number (singular system)%s", who);
    }
    return FARNN_OK;
}

// idx: `order` host arrays.  Repeated coordinates are found by comparing coordinate TUPLES (never a flattened index, which could
// pass 64 bits at order 4), and ||X||^2 is the merged values' sum of squares.
static int cp_create(int order, const int32_t *dims, int64_t nnz, const int32_t *const *idx, const double *val, int32_t max_rank,
                     int device, farnn_cp_ctx **out) {
    if (nnz <= 0) return fail(FARNN_EINVAL, "cp_create: the tensor has no nonzero%s%s");
    if (nnz >= (1ll << 30)) return fail(FARNN_ERANGE, "cp_create: more than 2^30 nonzeros%s%s");
    if (max_rank < 1) return fail(FARNN_EINVAL, "cp_create: max_rank must be positive%s%s");
    for (int m = 0; m < order; m++)
        if (dims[m] <= 0 || dims[m] >= (1 << 22)) return fail(FARNN_EINVAL, "cp_create: a dimension must lie in [1, 2^22)%s%s");
    for (int64_t e = 0; e < nnz; e++)
        for (int m = 0; m < order; m++)
            if (idx[m][e] < 0 || idx[m][e] >= dims[m]) return fail(FARNN_EINVAL, "cp_create: a coordinate lies outside its dimension%s%s");
    int rc;
    if ((rc = select_device(device))) return rc;

    // canonical order (lexicographic, stable), repeated coordinates added up in list order
    std::vector<int64_t> perm((size_t)nnz);
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
        for (int m = 0; m < order; m++)
            if (idx[m][a] != idx[m][b]) return idx[m][a] < idx[m][b];
        return false;
    });
    std::vector<int> ci[CP_MAX_ORDER];
    std::vector<double> cv;
    for (int64_t k = 0; k < nnz; k++) {
        const int64_t e = perm[(size_t)k];
        bool same = !cv.empty();
        for (int m = 0; m < order && same; m++) same = ci[m].back() == idx[m][e];
        if (same) {
            cv.back() += val[e];
            continue;
        }
        for (int m = 0; m < order; m++) ci[m].push_back(idx[m][e]);
        cv.push_back(val[e]);
    }
    const size_t n = cv.size();
    double normx2 = 0.0;
    for (size_t k = 0; k < n; k++) normx2 += cv[k] * cv[k];
    if (!(normx2 > 0.0) || !std::isfinite(normx2)) return fail(FARNN_EINVAL, "cp_create: the tensor's norm is not a positive finite number%s%s");

    farnn_cp_ctx *c = new farnn_cp_ctx();
    c->device = device;
    c->order = order;
    c->nnz = (long long)n;
    c->normx2 = normx2;
    c->asked_rank = max_rank;
    c->max_rank = std::min<int>(max_rank, CP_MAX_RANK);
    const size_t Rm = (size_t)c->max_rank;
    const char *oom = "cp_create: out of device memory%s%s";
    size_t max_chunks = 1, max_dim = 1;
    for (int m = 0; m < order && !rc; m++) {
        c->dims[m] = dims[m];
        max_dim = std::max(max_dim, (size_t)dims[m]);
        CpModeOrder &o = c->mode[m];
        o.panels = (dims[m] + CP_PANEL - 1) / CP_PANEL;
        std::vector<size_t> ord(n);
        std::iota(ord.begin(), ord.end(), (size_t)0);
        std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return ci[m][a] < ci[m][b]; });
        std::vector<int> chunk_beg, chunk_end, chunkptr((size_t)dims[m] + 1, 0);
        std::vector<double> v(n);
        int oth[CP_MAX_ORDER];
        cp_others(order, m, oth);
        size_t at = 0;
        for (int row = 0; row < dims[m]; row++) {
            chunkptr[(size_t)row] = (int)chunk_beg.size();
            size_t end = at;
            while (end < n && ci[m][ord[end]] == row) end++;
            for (size_t k = at; k < end; k += CP_CHUNK) {
                chunk_beg.push_back((int)k);
                chunk_end.push_back((int)std::min(end, k + CP_CHUNK));
            }
            at = end;
        }
        chunkptr[(size_t)dims[m]] = (int)chunk_beg.size();
        for (size_t k = 0; k < n; k++) v[k] = cv[ord[k]];
        o.nchunks = (int)chunk_beg.size();
        max_chunks = std::max(max_chunks, chunk_beg.size());
        std::vector<int> all;
        all.reserve(2 * chunk_beg.size() + chunkptr.size() + (size_t)(order - 1) * n);
        all.insert(all.end(), chunk_beg.begin(), chunk_beg.end());
        all.insert(all.end(), chunk_end.begin(), chunk_end.end());
        all.insert(all.end(), chunkptr.begin(), chunkptr.end());
        for (int j = 0; j < order - 1; j++)
            for (size_t k = 0; k < n; k++) all.push_back(ci[oth[j]][ord[k]]);
        if ((rc = o.ints.ensure(all.size(), oom)) || (rc = o.val.ensure(n, oom)) ||
            (rc = c->gram[m].ensure((size_t)o.panels * Rm * Rm, oom)) || (rc = c->F[m].ensure((size_t)dims[m] * Rm, oom)))
            break;
        o.chunk_beg = o.ints.p;
        o.chunk_end = o.chunk_beg + o.nchunks;
        o.chunkptr = o.chunk_end + o.nchunks;
        o.ia = o.chunkptr + dims[m] + 1;
        o.ib = o.ia + n;
        o.ic = order == 4 ? o.ib + n : nullptr;
        if (hipMemcpy(o.ints.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(o.val.p, v.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(FARNN_EIO, "cp_create: copying the coordinate lists to the device failed%s%s");
    }
    if (!rc) {
        (void)((rc = c->part.ensure(max_chunks * Rm, oom)) || (rc = c->H.ensure(Rm * Rm, oom)) || (rc = c->L.ensure(Rm * Rm, oom)) ||
               (rc = c->Lt.ensure(Rm * Rm, oom)) || (rc = c->M.ensure(max_dim * Rm, oom)) || (rc = c->slot.ensure(1, oom)));
    }
    if (!rc && hipHostMalloc((void **)&c->host, sizeof(CpSlot), hipHostMallocDefault) != hipSuccess) {
        c->host = nullptr;
        rc = fail(FARNN_ENOMEM, "cp_create: out of pinned host memory%s%s");
    }
    if (!rc && (hipMemset(c->slot.p, 0, sizeof(CpSlot)) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
        rc = fail(FARNN_EIO, "cp_create: clearing the flag on the device failed%s%s");
    for (int i = 0; i < 5 && !rc; i++)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) { c->ev[i] = nullptr; rc = fail(FARNN_EIO, "cp_create: hipEventCreate failed%s%s"); }
    if (rc) { farnn_cp_destroy(c); return rc; }
    *out = c;
    return FARNN_OK;
}

extern "C" int farnn_cp_create(const int32_t *dims, int64_t nnz, const int32_t *idx0, const int32_t *idx1, const int32_t *idx2,
                               const double *val, int32_t max_rank, int device, farnn_cp_ctx **out) {
    if (!out) return fail(FARNN_EINVAL, "cp_create: null argument%s%s");
    *out = nullptr;
    if (!dims || !idx0 || !idx1 || !idx2 || !val) return fail(FARNN_EINVAL, "cp_create: null argument%s%s");
    const int32_t *idx[3] = {idx0, idx1, idx2};
    return cp_create(3, dims, nnz, idx, val, max_rank, device, out);
}

extern "C" int farnn_cp_create_n(int32_t order, const int32_t *dims, int64_t nnz, const int32_t *const *idx, const double *val,
                                 int32_t max_rank, int device, farnn_cp_ctx **out) {
    if (!out) return fail(FARNN_EINVAL, "cp_create_n: null argument%s%s");
    *out = nullptr;
    if (order != 3 && order != 4) return fail(FARNN_EINVAL, "cp_create_n: order must be 3 or 4%s%s");
    if (!dims || !idx || !val) return fail(FARNN_EINVAL, "cp_create_n: null argument%s%s");
    for (int m = 0; m < order; m++)
        if (!idx[m]) return fail(FARNN_EINVAL, "cp_create_n: null argument%s%s");
    return cp_create(order, dims, nnz, idx, val, max_rank, device, out);
}

extern "C" void farnn_cp_destroy(farnn_cp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->host) (void)hipHostFree(c->host);
    delete c;
}

extern "C" int farnn_cp_order(const farnn_cp_ctx *c, int32_t *order) {
    if (!c || !order) return fail(FARNN_EINVAL, "cp_order: null argument%s%s");
    *order = c->order;
    return FARNN_OK;
}

// everything the two stage entries refuse, before any launch; f: the context's `order` device pointers
static int cp_check_stage(const farnn_cp_ctx *c, int mode, int rank, const double *const *f, const void *out, const char *who) {
    if (!c || !f || !out) return fail(FARNN_EINVAL, "%s: null argument%s", who);
    if (mode < 0 || mode >= c->order) return fail(FARNN_EINVAL, "%s: mode must be below the tensor's order%s", who);
    if (int rc = cp_check_rank(c, rank, who)) return rc;
    for (int m = 0; m < c->order; m++)
        if (m != mode && !f[m]) return fail(FARNN_EINVAL, "%s: a factor of another mode is null%s", who);
    return FARNN_OK;
}

static int cp_normal_matrix(farnn_cp_ctx *c, int mode, int rank, const double *const *f, double *H, hipStream_t s) {
    for (int m = 0; m < c->order; m++)
        if (m != mode)
            if (int rc = cp_gram(c, m, f[m], rank, s)) return rc;
    return cp_hadamard(c, mode, rank, H, s);
}

static int cp_order3_only(const farnn_cp_ctx *c, const char *who) {
    if (c && c->order != 3) return fail(FARNN_EINVAL, "%s: the context's tensor is not 3-way (use the _n entry)%s", who);
    return FARNN_OK;
}

extern "C" int farnn_cp_mttkrp(farnn_cp_ctx *c, int32_t mode, int32_t rank, const double *f0, const double *f1, const double *f2,
                               double *out, void *stream) {
    if (int rc = cp_order3_only(c, "cp_mttkrp")) return rc;
    const double *const f[3] = {f0, f1, f2};
    if (int rc = cp_check_stage(c, mode, rank, f, out, "cp_mttkrp")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    return cp_mttkrp(c, mode, rank, f, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int farnn_cp_mttkrp_n(farnn_cp_ctx *c, int32_t mode, int32_t rank, const double *const *f, double *out, void *stream) {
    if (int rc = cp_check_stage(c, mode, rank, f, out, "cp_mttkrp_n")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    return cp_mttkrp(c, mode, rank, f, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int farnn_cp_normal_matrix(farnn_cp_ctx *c, int32_t mode, int32_t rank, const double *f0, const double *f1, const double *f2,
                                      double *H, void *stream) {
    if (int rc = cp_order3_only(c, "cp_normal_matrix")) return rc;
    const double *const f[3] = {f0, f1, f2};
    if (int rc = cp_check_stage(c, mode, rank, f, H, "cp_normal_matrix")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    return cp_normal_matrix(c, mode, rank, f, H, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int farnn_cp_normal_matrix_n(farnn_cp_ctx *c, int32_t mode, int32_t rank, const double *const *f, double *H, void *stream) {
    if (int rc = cp_check_stage(c, mode, rank, f, H, "cp_normal_matrix_n")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    return cp_normal_matrix(c, mode, rank, f, H, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int farnn_cp_solve(farnn_cp_ctx *c, int32_t rank, const double *H, const double *M, int32_t rows, double *out, void *stream) {
    if (!c || !H || !M || !out) return fail(FARNN_EINVAL, "cp_solve: null argument%s%s");
    if (rows < 1) return fail(FARNN_EINVAL, "cp_solve: rows must be positive%s%s");
    if (int rc = cp_check_rank(c, rank, "cp_solve")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = cp_solve(c, rank, H, M, rows, out, s)) return rc;
    return cp_read_slot(c, s, "cp_solve");
}

// host_f: the context's `order` host arrays
static int cp_run(farnn_cp_ctx *c, int R, int n_iter_max, double tol, double *const *host_f, double *rec_errors, int32_t *n_sweeps,
                  hipStream_t s, const char *who) {
    const int order = c->order, last = order - 1;
    for (int m = 0; m < order; m++)
        FARNN_HIP_TRY(hipMemcpyAsync(c->F[m].p, host_f[m], (size_t)c->dims[m] * R * sizeof(double), hipMemcpyHostToDevice, s));
    const double *const f[CP_MAX_ORDER] = {c->F[0].p, c->F[1].p, c->F[2].p, c->F[3].p};
    bool fresh[CP_MAX_ORDER] = {false, false, false, false};     // the Gram panels of a factor stay good until that factor is solved for again
    const bool timed = c->profiling != 0;
    int rc = FARNN_OK;
    for (int sweep = 0; sweep < n_iter_max; sweep++) {
        float ms[4] = {0, 0, 0, 0};
        for (int n = 0; n < order; n++) {
            if (timed) FARNN_HIP_TRY(hipEventRecord(c->ev[0], s));
            for (int m = 0; m < order; m++) {
                if (m == n || fresh[m]) continue;
                if ((rc = cp_gram(c, m, f[m], R, s))) return rc;
                fresh[m] = true;
            }
            if ((rc = cp_hadamard(c, n, R, c->H.p, s))) return rc;
            if (timed) FARNN_HIP_TRY(hipEventRecord(c->ev[1], s));
            if ((rc = cp_mttkrp(c, n, R, f, c->M.p, s))) return rc;
            if (timed) FARNN_HIP_TRY(hipEventRecord(c->ev[2], s));
            if ((rc = cp_solve(c, R, c->H.p, c->M.p, c->dims[n], c->F[n].p, s))) return rc;
            fresh[n] = false;
            if (timed) {
                FARNN_HIP_TRY(hipEventRecord(c->ev[3], s));
                FARNN_HIP_TRY(hipEventSynchronize(c->ev[3]));
                for (int k = 0; k < 3; k++) {
                    float t = 0;
                    FARNN_HIP_TRY(hipEventElapsedTime(&t, c->ev[k], c->ev[k + 1]));
                    ms[k] += t;
                }
            }
        }
        if (timed) FARNN_HIP_TRY(hipEventRecord(c->ev[3], s));
        if ((rc = cp_gram(c, last, f[last], R, s))) return rc;
        fresh[last] = true;
        cp_error_kernel<<<1, CP_THREADS, 0, s>>>(c->H.p, c->gram[last].p, c->mode[last].panels, R, c->M.p, f[last], c->dims[last],
                                                 c->normx2, c->slot.p);
        FARNN_HIP_TRY(hipGetLastError());
        if (timed) FARNN_HIP_TRY(hipEventRecord(c->ev[4], s));
        if ((rc = cp_read_slot(c, s, who))) return rc;
        if (timed) {
            FARNN_HIP_TRY(hipEventElapsedTime(&ms[3], c->ev[3], c->ev[4]));
            for (int k = 0; k < 4; k++) c->stage_ms[k] += ms[k];
            c->stage_n += 1;
        }
        rec_errors[sweep] = c->host->err;
        *n_sweeps = sweep + 1;
        if (sweep >= 1 && fabs(rec_errors[sweep - 1] - rec_errors[sweep]) < tol) break;
    }
    for (int m = 0; m < order; m++)
        FARNN_HIP_TRY(hipMemcpyAsync(host_f[m], c->F[m].p, (size_t)c->dims[m] * R * sizeof(double), hipMemcpyDeviceToHost, s));
    FARNN_HIP_TRY(hipStreamSynchronize(s));
    return FARNN_OK;
}

extern "C" int farnn_cp_run(farnn_cp_ctx *c, int32_t rank, int32_t n_iter_max, double tol, double *f0, double *f1, double *f2,
                            double *rec_errors, int32_t *n_sweeps, void *stream) {
    if (!c || !f0 || !f1 || !f2 || !rec_errors || !n_sweeps) return fail(FARNN_EINVAL, "cp_run: null argument%s%s");
    *n_sweeps = 0;
    if (int rc = cp_order3_only(c, "cp_run")) return rc;
    if (n_iter_max < 1) return fail(FARNN_EINVAL, "cp_run: n_iter_max must be positive%s%s");
    if (int rc = cp_check_rank(c, rank, "cp_run")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    double *const host_f[3] = {f0, f1, f2};
    return cp_run(c, rank, n_iter_max, tol, host_f, rec_errors, n_sweeps, reinterpret_cast<hipStream_t>(stream), "cp_run");
}

extern "C" int farnn_cp_run_n(farnn_cp_ctx *c, int32_t rank, int32_t n_iter_max, double tol, double *const *f, double *rec_errors,
                              int32_t *n_sweeps, void *stream) {
    if (!c || !f || !rec_errors || !n_sweeps) return fail(FARNN_EINVAL, "cp_run_n: null argument%s%s");
    *n_sweeps = 0;
    for (int m = 0; m < c->order; m++)
        if (!f[m]) return fail(FARNN_EINVAL, "cp_run_n: null argument%s%s");
    if (n_iter_max < 1) return fail(FARNN_EINVAL, "cp_run_n: n_iter_max must be positive%s%s");
    if (int rc = cp_check_rank(c, rank, "cp_run_n")) return rc;
    FARNN_HIP_TRY(hipSetDevice(c->device));
    return cp_run(c, rank, n_iter_max, tol, f, rec_errors, n_sweeps, reinterpret_cast<hipStream_t>(stream), "cp_run_n");
}

extern "C" int farnn_cp_set_profiling(farnn_cp_ctx *c, int32_t enable) {
    if (!c) return fail(FARNN_EINVAL, "cp_set_profiling: null context%s%s");
    c->profiling = enable ? 1 : 0;
    for (double &v : c->stage_ms) v = 0.0;
    c->stage_n = 0;
    return FARNN_OK;
}

extern "C" int farnn_cp_time(farnn_cp_ctx *c, double *stage_ms, int64_t *sweeps) {
    if (!c || !stage_ms || !sweeps) return fail(FARNN_EINVAL, "cp_time: null argument%s%s");
    for (int k = 0; k < 4; k++) stage_ms[k] = c->stage_ms[k];
    *sweeps = c->stage_n;
    return FARNN_OK;
}

extern "C" int farnn_cp_norm2(const farnn_cp_ctx *c, double *normx2, int64_t *nnz) {
    if (!c || !normx2 || !nnz) return fail(FARNN_EINVAL, "cp_norm2: null argument%s%s");
    *normx2 = c->normx2;
    *nnz = c->nnz;
    return FARNN_OK;
}
