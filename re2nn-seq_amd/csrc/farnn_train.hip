// libfarnn_hip.so -- the training steps: the decomposed i-FST (farnn_train_*; include/farnn.h), the same on a dense
// input (farnn_decomp_sf_train_*), the decomposed FST on the same chains (farnn_decomp_fst_train_*), the onehot
// i-FST (farnn_onehot_train_*), the onehot FST (farnn_fst4_train_*), the onehot independent=1 model (farnn_ind1_train_*) and the
// decomposed independent=1 model (farnn_decomp_ind1_train_*), and the optimizer step that follows any of them (farnn_optim_*, at
// the end).  Their own translation unit: the training kernels (train.hip.h: the scores and the loss, shared by the first two
// steps; the headers below) compile once, beside the tagging path.  Each step is a struct whose member functions are its named
// stages, in the order they run; every entry point goes through run_train_step and every context is a TrainCtxBase
// (train_host.hip.h), and the last three steps are a BucketedStep each (train_bucketed.hip.h).
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <algorithm>
#include <vector>

#include "common.hip.h"
#include "host_util.hip.h"
#include "train_host.hip.h"
#include "train_teacher.hip.h"
#include "train_bucketed.hip.h"
#include "train_max.hip.h"
#include "onehot_train_max.hip.h"
#include "fst4_train.hip.h"
#include "ind1_train.hip.h"
#include "decomp1_train.hip.h"
#include "decomp0_train.hip.h"
#include "decomp0_train_max.hip.h"
#include "sf_train.hip.h"
#include "decomp1_gated_train.hip.h"
#include "decomp1_gated_max_train.hip.h"
#include "train_bucketed_crf.hip.h"
#include "optim.hip.h"

using namespace farnn;

// ---- training step (decomposed i-FST) ------------------------------------------
struct farnn_train_ctx : TrainCtxBase {     // (err: the kernels set bit 0 on a bad label)
    Tunables tun;                 // the FARNN_* switches as they stood when the context was created (host_util.hip.h)
    farnn_train_dims d;
    int n_cu = 256;               // compute units of the device
    int semiring = FARNN_SEMIRING_SUM;  // farnn_train_set_semiring
    DevBuf<float> fixed;          // create's block: the transposes and column sums below
    float *S1T = nullptr, *S2T = nullptr, *WT = nullptr, *Osum = nullptr, *dOsum = nullptr;
    float *Wss1T = nullptr, *Wss2T = nullptr, *Wrs1T = nullptr, *Wrs2T = nullptr;   // gate transposes (farnn > 0)
    DevBuf<float> VgenT, GV;      // [R][V] and 6 x [V][S]: the gates' input halves Vgen Wrs, their adjoints and those transposed (farnn > 0)
    DevBuf<float> ws;             // per-batch workspace (zeroed every step)
    DevBuf<float> part;           // partial products of the gate-input and the parameter-gradient reductions
    DevBuf<float> ones;           // 1.0f each: bias gradients as a product with a column of ones
    DevBuf<float> mws;            // max semiring only (train_max.hip.h): M, MT, dM, IN, GM; allocated on first use
    DevBuf<int> miws;             // max semiring only: IDX, the bucketing of the positions, the word slots
    // a vector-input context (farnn_decomp_sf_train_create, d.V = 0; sf_train.hip.h): nothing per word, and the position ids
    bool vector_input = false;
    DevBuf<int64_t> ids;          // [B L] 0, 1, 2, ...: the chains' token ids, written on the device when the buffer grows
};

// farnn_train_create (vec = false) and farnn_decomp_sf_train_create (vec = true: no vocabulary)
static int train_create(const farnn_train_dims *d, int device, farnn_train_ctx **out, bool vec) {
    if (!d || !out) return fail(FARNN_EINVAL, "train_create: null argument%s%s");
    *out = nullptr;
    if ((vec ? d->V != 0 : d->V <= 0) || d->S <= 0 || d->R <= 0 || d->K <= 0)
        return fail(FARNN_EINVAL, vec ? "decomp_sf_train_create: bad dimensions (a vector-input context has V = 0)%s%s" : "train_create: bad dimensions%s%s");
    if (d->nl < FARNN_NL_NONE || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "train_create: bad nonlinearity%s%s");
    // the CRF loss kernel keeps exp(transitions) in LDS: K = 190 is the hard limit (L = 4); at L = 64 it is K = 140
    // (checked per call, farnn_decomp_ifst_train_step returns FARNN_ERANGE before enqueuing anything)
    if (d->use_crf && (d->K < 4 || train_crf_lds_bytes(d->K, 4, true) > 160 * 1024))
        return fail(FARNN_ERANGE, "train_create: CRF needs 4..190 score columns%s%s");
    if (d->farnn < 0 || d->farnn > 2) return fail(FARNN_EINVAL, "train_create: farnn must be 0, 1 or 2%s%s");
    int rc;
    if ((rc = train_ctx_create("train", d, device, out))) return rc;
    farnn_train_ctx *c = *out;
    c->n_cu = device_cus(device);
    c->vector_input = vec;
    const size_t S = d->S, R = d->R, V = d->V;
    const char *oom = "train_create: out of device memory%s%s";
    if ((rc = c->fixed.ensure(2 * S * R + S * S + 2 * S + (d->farnn ? 2 * S * S + 2 * S * R : 0), oom)) ||
        (d->farnn && ((rc = c->VgenT.ensure(V * R, oom)) || (rc = c->GV.ensure(6 * V * S, oom))))) {
        train_ctx_destroy(c);
        *out = nullptr;
        return rc;
    }
    c->S1T = c->fixed.p; c->S2T = c->S1T + S * R; c->WT = c->S2T + S * R; c->Osum = c->WT + S * S; c->dOsum = c->Osum + S;
    if (d->farnn) { c->Wss1T = c->dOsum + S; c->Wss2T = c->Wss1T + S * S; c->Wrs1T = c->Wss2T + S * S; c->Wrs2T = c->Wrs1T + S * R; }
    return FARNN_OK;
}
extern "C" int farnn_train_create(const farnn_train_dims *d, int device, farnn_train_ctx **out) { return train_create(d, device, out, false); }
extern "C" int farnn_decomp_sf_train_create(const farnn_train_dims *d, int device, farnn_train_ctx **out) { return train_create(d, device, out, true); }
extern "C" void farnn_train_destroy(farnn_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_train_set_profiling(farnn_train_ctx *c, int32_t enable) { return train_ctx_set_profiling("train", c, enable); }
extern "C" int farnn_train_time(farnn_train_ctx *c, double *total_ms, int64_t *steps) { return train_ctx_time("train", c, total_ms, steps); }

extern "C" int farnn_train_set_semiring(farnn_train_ctx *c, int32_t semiring) {
    if (!c) return fail(FARNN_EINVAL, "train_set_semiring: null context%s%s");
    if (semiring != FARNN_SEMIRING_SUM && semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "train_set_semiring: semiring must be FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX%s%s");
    if (semiring == FARNN_SEMIRING_MAX && c->vector_input)
        return fail(FARNN_EINVAL, "train_set_semiring: a vector-input context exists in the sum semiring only (the max semiring needs an S x S block per token)%s%s");
    if (semiring == FARNN_SEMIRING_MAX && c->d.S > TM_MAX_S)
        return fail(FARNN_ERANGE, "train_set_semiring: the max-semiring step holds at most 192 states%s%s");
    c->semiring = semiring;
    return FARNN_OK;
}

static void atb_add(AtbJobs &jobs, const float *A, const float *Bm, float *out, long long N, int M, int J) {
    if (N <= 0) return;
    if (jobs.n >= ATB_MAX_JOBS) { jobs.total_wgs = -1; return; }       // checked by the caller: never drop a product silently
    AtbJob &j = jobs.j[jobs.n];
    j.A = A; j.B = Bm; j.out = out; j.N = N; j.M = M; j.J = J;
    j.tiles_m = (M + 63) / 64; j.tiles_j = (J + 63) / 64;
    j.nsplit = (int)((N + jobs.chunk - 1) / jobs.chunk);
    j.wg0 = jobs.total_wgs; j.out0 = jobs.total_out;
    j.part_off = jobs.n ? jobs.j[jobs.n - 1].part_off + (long long)jobs.j[jobs.n - 1].nsplit * jobs.j[jobs.n - 1].M * jobs.j[jobs.n - 1].J : 0;
    jobs.total_wgs += j.tiles_m * j.tiles_j * j.nsplit;
    jobs.total_out += M * J;
    jobs.n++;
}
static size_t atb_partial_floats(const AtbJobs &jobs) {
    if (!jobs.n) return 0;
    const AtbJob &l = jobs.j[jobs.n - 1];
    return (size_t)(l.part_off + (long long)l.nsplit * l.M * l.J);
}
static void atb_launch(const AtbJobs &jobs, hipStream_t s) {
    atb_partial_kernel<<<jobs.total_wgs, 256, 0, s>>>(jobs);
    atb_reduce_kernel<<<(jobs.total_out + 255) / 256, 256, 0, s>>>(jobs);
}
static void prep_add(PrepJobs &pj, int kind, const float *src, float *dst, size_t rows, size_t cols) {
    if (pj.n >= PREP_MAX_JOBS) { pj.total = -1; return; }
    PrepJob &j = pj.j[pj.n++];
    j.kind = kind; j.src = src; j.dst = dst; j.rows = (int)rows; j.cols = (int)cols; j.e0 = pj.total;
    // every job starts on a 256-thread block boundary; a transpose takes one block per 32x32 tile
    const size_t ne = kind == 1 ? ((rows + 31) / 32) * ((cols + 31) / 32) * 256
                                : (((kind == 2 ? cols : rows * cols) + 255) / 256) * 256;
    if (pj.total < 0 || ne > (size_t)0x7fffffff - (size_t)pj.total) { pj.total = -1; return; }   // 32-bit element index
    pj.total += (int)ne;
}


// What a step needs, from the dimensions alone (train_plan)
struct TrainPlan {
    bool crf, mx;
    bool teacher;                       // a KD / PR step: both chains of every sequence run L steps, the loss walks every position
    int farnn, B, L;
    size_t S, R, K, V, N1, N0, nwmax;   // N1 = B (L+1) stash rows, N0 = B L positions, nwmax: bound on the batch's distinct words
    size_t need, mneed, mineed;         // floats of ws and of mws, ints of miws: the totals of the carve functions below
    bool ldsw_f, ldsw_b;                // chain kernels: the weights in LDS, or read through L2
    int ns_f, ns_b, nss_f, nss_b;       // sequences per workgroup; S x S matrices a through-L2 kernel still keeps in LDS (0..3)
    size_t lds_f, lds_b, lds_tok, lds_m, lds_w;   // LDS bytes of the chain kernels (sum; max), of the max semiring's dM and weight gradients,
    size_t lds_c;                       // and of the CRF kernel,
    bool crf_big;                       // which keeps transitions, expected counts and emissions in global memory for large tag sets
    unsigned lgrid;                     // workgroups of the loss kernel
};
// the max semiring's workspaces (train_max.hip.h): blocks of the batch's distinct words (at most min(V, B L)), the per-step
// argmax and dTr entries, the bucketing of the positions by word
struct MaxWs { float *M, *MT, *dM; int *wslot, *wlist, *nwords; Buckets bk; TrainMaxParams mp; };

// the three workspaces: size (null base) and layout (the buffer) from the same code
static size_t carve_train_ws(float *base, TrainParams &p, const TrainPlan &pl) {
    Carver<float> a(base);
    const size_t nS = pl.N1 * pl.S, nR = pl.N1 * pl.R;
    p.A = a.take(nS); p.Bk = a.take(nS); p.GA = a.take(nS); p.GB = a.take(nS);
    p.Zf = a.take(nS); p.Zb = a.take(nS); p.BBAR = a.take(nS); p.PRE = a.take(nS);
    p.D1f = a.take(nR); p.D1b = a.take(nR); p.Tf = a.take(nR); p.Tb = a.take(nR);
    p.DS = a.take(pl.N0 * pl.K); p.AB = a.take(pl.N0 * pl.S);
    if (pl.crf) { p.SC = a.take(pl.N0 * pl.K); p.dtrans_part = a.take((size_t)pl.B * pl.K * pl.K); }
    if (pl.teacher) p.loss_part = a.take((size_t)pl.lgrid * 8);      // one loss partial per wavefront of the teacher's loss kernel
    if (pl.farnn) {
        p.ZGf = a.take(nS); p.ZGb = a.take(nS); p.RGf = a.take(nS); p.RGb = a.take(nS); p.CDf = a.take(nS); p.CDb = a.take(nS);
        p.DAZf = a.take(nS); p.DAZb = a.take(nS); p.DARf = a.take(nS); p.DARb = a.take(nS); p.HBARf = a.take(nS);
        p.VRf = a.take(nR); p.VRb = a.take(nR);
    }
    return a.off;
}
static size_t carve_max_floats(float *base, MaxWs &m, const TrainPlan &pl) {
    Carver<float> a(base);
    const size_t blocks = pl.nwmax * pl.S * pl.S, nS = pl.N1 * pl.S;
    m.mp.M = m.M = a.take(blocks); m.mp.MT = m.MT = a.take(blocks); m.dM = a.take(blocks);
    m.mp.INf = a.take(nS); m.mp.INb = a.take(nS); m.mp.GMf = a.take(nS); m.mp.GMb = a.take(nS);
    return a.off;
}
static size_t carve_max_ints(int *base, MaxWs &m, const TrainPlan &pl) {
    Carver<int> a(base);
    m.mp.IDXf = a.take(pl.N1 * pl.S); m.mp.IDXb = a.take(pl.N1 * pl.S);
    carve_buckets(a, m.bk, pl.V, pl.N0);
    m.mp.wslot = m.wslot = a.take(pl.V); m.mp.wlist = m.wlist = a.take(pl.nwmax); m.mp.nwords = m.nwords = a.take(1);
    a.take(pl.V);      // (unused: the sum this carve replaced counted V ints more than its walk took; the allocation stays what it was)
    return a.off;
}
// Stage 1: the arguments
static int train_validate(const farnn_train_ctx *c, const farnn_train_weights *w, const farnn_train_outputs *o) {
    if (!w->Vgen || !w->S1 || !w->S2 || !w->W || !w->C || !w->h0 || !w->hT) return fail(FARNN_EINVAL, "train_step: null weight%s%s");
    if (!o->loss || !o->dVgen || !o->dS1 || !o->dS2 || !o->dW || !o->dC || !o->dh0 || !o->dhT || !o->tags)
        return fail(FARNN_EINVAL, "train_step: null output%s%s");
    if (c->d.use_crf && (!w->crf_trans || !o->dtrans)) return fail(FARNN_EINVAL, "train_step: CRF transitions / their gradient missing%s%s");
    if (c->d.farnn >= 1 && (!w->Wss1 || !w->Wrs1 || !w->bs1 || !o->dWss1 || !o->dWrs1 || !o->dbs1))
        return fail(FARNN_EINVAL, "train_step: update-gate weights / gradients missing%s%s");
    if (c->d.farnn == 2 && (!w->Wss2 || !w->Wrs2 || !w->bs2 || !o->dWss2 || !o->dWrs2 || !o->dbs2))
        return fail(FARNN_EINVAL, "train_step: reset-gate weights / gradients missing%s%s");
    return FARNN_OK;
}
// Stage 2: host arithmetic only, no HIP call -- the workspace sizes, the kernel forms and the LDS bytes of every launch, from the
// dimensions, the semiring, B, L, the device's CU count and the FARNN_TRAIN_* switches.  Every size the step refuses is refused
// here, the launches above 160 KiB of LDS included: a refused step has enqueued nothing and has not touched the caller's outputs.
template <typename Ctx>      // (farnn_train_ctx, and the decomposed FST's context: the same chains)
static int train_plan(const Ctx *c, int B, int L, bool teacher, TrainPlan &pl) {
    const size_t S = c->d.S, R = c->d.R, K = c->d.K, V = c->d.V, SR = S > R ? S : R;
    const int farnn = c->d.farnn;
    const bool crf = c->d.use_crf != 0;
    // the CRF kernel keeps exp(transitions) [K][K+1] and two message tables [L][K] in LDS (K = 130 at L = 64: 144 KiB; K = 140
    // is the limit at L = 64, K = 190 at L = 4)
    if (crf && train_crf_lds_bytes(K, L, true) > 160 * 1024)
        return fail(FARNN_ERANGE, "train_step: CRF tag set too large for this sequence length (K(K+1)*4 + 9*L*K + ... bytes of LDS must fit 160 KiB)%s%s");
    if (SR > (size_t)TR_VPT * TR_THREADS / TR_NSEQ) return fail(FARNN_ERANGE, "train_step: more than 512 states or rank above 512%s%s");
    // the chain kernels address their per-step arrays [B (L+1)][S | R] and the per-word tables [V][S | R] by 32-bit element
    // offsets against scalar base pointers (train.hip.h)
    if ((unsigned long long)B * (L + 1) * SR >= (1ull << 30) || (unsigned long long)V * SR >= (1ull << 30))
        return fail(FARNN_ERANGE, "train_step: B (L+1) max(S, R) and V max(S, R) must stay below 2^30 elements%s%s");
    pl.crf = crf; pl.mx = c->semiring == FARNN_SEMIRING_MAX; pl.teacher = teacher; pl.farnn = farnn; pl.B = B; pl.L = L;
    pl.S = S; pl.R = R; pl.K = K; pl.V = V;
    pl.N1 = (size_t)B * (L + 1); pl.N0 = (size_t)B * L; pl.nwmax = std::min(V, pl.N0);
    pl.lgrid = (unsigned)std::min<size_t>(c->n_cu, (pl.N0 + 7) / 8);
    TrainParams p0; MaxWs m0;
    pl.need = carve_train_ws(nullptr, p0, pl); pl.mneed = carve_max_floats(nullptr, m0, pl); pl.mineed = carve_max_ints(nullptr, m0, pl);

    const size_t nwv = TR_THREADS / 64;
    const size_t SPd = ((S + 3) & ~(size_t)3) + 8, RPd = ((R + 3) & ~(size_t)3) + 8;
    // LDS of the vectors, partial sums and token lists of a chain workgroup with ns sequences
    auto vecf = [&](size_t ns) { return (ns * SPd + ns * RPd + ns * nwv * SR + ns * nwv * S + ns * (size_t)L +
                                         (farnn ? ns * SPd + 2 * ns * nwv * S : 0)) * sizeof(float); };
    auto vecb = [&](size_t ns) { return (2 * ns * SPd + ns * RPd + 2 * ns * nwv * SR + ns * nwv * S + ns * (size_t)L +
                                         (farnn ? 2 * ns * SPd : 0)) * sizeof(float); };
    const size_t mat_f = ((2 * S * R + S * S + 3) & ~(size_t)3) * sizeof(float), mat_b = ((3 * S * R + S * S + 3) & ~(size_t)3) * sizeof(float);
    pl.ldsw_f = vecf(TR_NSEQ) + mat_f <= 160 * 1024 && !tun(TUN_TRAIN_NOLDS);
    pl.ldsw_b = vecb(TR_NSEQ) + mat_b <= 160 * 1024 && !tun(TUN_TRAIN_NOLDS);
    // sequences per workgroup: two with the matrices in LDS; four when they are read through L2 every step (that mode
    // is bound by the L2 rate, and every element read then feeds four sequences) if the batch still fills the chip
    const size_t lds_cap = 156 * 1024;
    auto pick_ns = [&](bool ldsw, size_t vec4) -> int {
        const int forced = tun(TUN_TRAIN_NSEQ);
        if (ldsw) return TR_NSEQ;
        const bool fits = TR_NSEQ_L2 * SR <= (size_t)TR_VPT * TR_THREADS && vec4 + 16 <= lds_cap;
        if (forced == 2 || !fits) return TR_NSEQ;
        // (rounds 2-3 kept the gated four-sequence kernels with two register slots per thread -- 4 R or 4 S above 512, e.g. the
        // shipped rank 250 -- away: they spilled 80-320 bytes per lane.  Round 4 retired the scratch (train.hip.h: 32-bit offsets,
        // no hoisted per-call-site addresses): at B = 1024, rank 250, farnn 2 four sequences per workgroup run 5.3 ms against 7.1)
        // measured at rank 250: with 256 sequences four per workgroup leave half the CUs idle (2.98 vs 2.63 ms per step),
        // with 1024 they win (6.5 vs 8.3 ms): four once two-sequence workgroups would outnumber the CUs two to one
        return (forced == 4 || (size_t)B >= 2 * (size_t)c->n_cu) ? TR_NSEQ_L2 : TR_NSEQ;
    };
    pl.ns_f = pick_ns(pl.ldsw_f, vecf(TR_NSEQ_L2)); pl.ns_b = pick_ns(pl.ldsw_b, vecb(TR_NSEQ_L2));
    const size_t vec_f = vecf(pl.ns_f), vec_b = vecb(pl.ns_b);
    // through-L2 kernels keep as many of their S x S matrices in LDS as fit (wildcard matrix, then the gates' Wss)
    const size_t ssb = S * S * sizeof(float);
    const size_t want_ss = farnn == 2 ? 3 : (farnn == 1 ? 2 : 1);
    pl.nss_f = pl.ldsw_f || vec_f + 16 > lds_cap ? 0 : (int)std::min(want_ss, (lds_cap - vec_f - 16) / ssb);
    pl.nss_b = pl.ldsw_b || vec_b + 16 > lds_cap ? 0 : (int)std::min(want_ss, (lds_cap - vec_b - 16) / ssb);
    if (tun(TUN_TRAIN_NOLDS) > 1) pl.nss_f = pl.nss_b = 0;
    pl.lds_f = vec_f + (pl.ldsw_f ? mat_f : 16 + pl.nss_f * ssb); pl.lds_b = vec_b + (pl.ldsw_b ? mat_b : 16 + pl.nss_b * ssb);
    pl.lds_tok = (size_t)L * sizeof(int); pl.lds_m = ssb; pl.lds_w = tmax_wgrad_lds_bytes(S);
    pl.crf_big = train_crf_lds_bytes(K, L, false) > 160 * 1024;
    pl.lds_c = crf ? train_crf_lds_bytes(K, L, pl.crf_big) : 0;
    int rc;
    if ((rc = lds_fits(train_loss_lds(S, K).bytes())) || (rc = lds_fits(pl.lds_c))) return rc;
    if (teacher && (rc = lds_fits(train_teacher_lds(S, K).bytes()))) return rc;
    if (pl.mx) return (rc = lds_fits(pl.lds_tok)) || (rc = lds_fits(pl.lds_m)) ? rc : lds_fits(pl.lds_w);
    return (rc = lds_fits(pl.lds_f)) ? rc : lds_fits(pl.lds_b);
}
// One step: its plan and what its stages hand on.  The stages are the member functions, below in the order they run.
struct TrainStep : TrainPlan {
    static constexpr const char *name = "train", *label_range = "K";
    farnn_train_ctx *c; const farnn_train_weights *w; const farnn_train_outputs *o; hipStream_t s;
    TrainParams p; MaxWs m; PrepJobs prep; AtbJobs gate_jobs, grad_jobs;
    float *dGVT;                        // dGV^T ([S][V]) as the A operand of dVgen += dGV Wrs^T
    const float *re; const farnn_teacher *tch;      // the teacher's scores [B][L][K] and parameters; null: the plain step
    bool tch_max;                       // the entry is farnn_decomp_ifst_teacher_max_train_step: the context must be in the max semiring
    int validate() { return train_validate(c, w, o); }
    int plan(int B_, int L_) {
        if (int rc = teacher_check()) return rc;
        return train_plan(c, B_, L_, tch != nullptr, *this);
    }
    int teacher_check() const; int teacher_loss();
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prep_jobs(); int product_jobs();
    int prepare(); int forward(); int max_forward(); int loss(); int backward(); int max_weight_gradients(); int gradients();
    int max_backward() { return launch(tmax_backward_kernel<>, dim3(B, 2), TM_THREADS, lds_tok, s, p, m.mp); }
    int stages() {
        int rc;
        if ((rc = prepare()) || (rc = mx ? max_forward() : forward()) || (rc = loss())) return rc;
        return (rc = mx ? max_backward() : backward()) ? rc : gradients();
    }
};

// Stage 3: grow the buffers, lay the workspaces out, fill the kernels' parameters and the job lists.  Nothing is enqueued yet.
int TrainStep::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens) {
    int rc;
    if ((rc = c->ws.ensure(need, "train_step: out of device memory for the workspace%s%s"))) return rc;
    if (farnn && c->ones.n < N1) {
        if ((rc = c->ones.ensure(N1, "train_step: out of device memory for the column of ones%s%s"))) return rc;
        std::vector<float> hones(N1, 1.0f);
        FARNN_HIP_TRY(hipMemcpy(c->ones.p, hones.data(), N1 * sizeof(float), hipMemcpyHostToDevice));
    }
    if (mx && ((rc = c->mws.ensure(mneed, "train_step: out of device memory for the max-semiring workspace%s%s")) ||
               (rc = c->miws.ensure(mineed, "train_step: out of device memory for the max-semiring index workspace%s%s")))) return rc;
    [[maybe_unused]] const size_t carved = carve_train_ws(c->ws.p, p, *this);
    [[maybe_unused]] const size_t mcarved = mx ? carve_max_floats(c->mws.p, m, *this) : mneed, micarved = mx ? carve_max_ints(c->miws.p, m, *this) : mineed;
    assert(carved == need && mcarved == mneed && micarved == mineed);     // the sizing pass and the carving pass agree
    p.Vgen = w->Vgen; p.S1 = w->S1; p.S2 = w->S2; p.W = w->W; p.C = w->C; p.h0 = w->h0; p.hT = w->hT; p.P = w->P;
    p.S1T = c->S1T; p.S2T = c->S2T; p.WT = c->WT; p.Osum = c->Osum;
    p.x = x; p.len = lengths; p.labels = labels; p.err = c->err.dev;
    if (crf) p.trans = w->crf_trans;
    p.farnn = farnn; p.sig_k = c->d.sigmoid_exponent;
    if (farnn) {
        p.Wss1 = w->Wss1; p.Wrs1 = w->Wrs1; p.bs1 = w->bs1; p.Wss2 = w->Wss2; p.Wrs2 = w->Wrs2; p.bs2 = w->bs2;
        p.Wss1T = c->Wss1T; p.Wss2T = c->Wss2T; p.Wrs1T = c->Wrs1T; p.Wrs2T = c->Wrs2T;
        p.GV1 = c->GV.p; p.GV2 = c->GV.p + V * S; p.dGV1 = c->GV.p + 2 * V * S; p.dGV2 = c->GV.p + 3 * V * S;
        dGVT = c->GV.p + 4 * V * S;
    }
    p.nss_f = nss_f; p.nss_b = nss_b;
    p.dVgen = o->dVgen; p.dOsum = c->dOsum; p.dh0 = o->dh0; p.dhT = o->dhT; p.loss = o->loss; p.tags = o->tags;
    p.B = B; p.L = L; p.V = (int)V; p.S = (int)S; p.R = (int)R; p.K = (int)K; p.nl = c->d.nl; p.o_idx = c->d.o_idx;
    p.threshold = c->d.threshold; p.inv_tokens = 1.0f / (float)valid_tokens;
    if (teacher) {
        p.full_chain = 1; p.re = re; p.t_mode = tch->mode; p.t_c1 = tch->c1; p.t_pi = tch->pi;
        p.t_inv_n = (float)(1.0 / ((double)B * (double)L * (double)K));      // KLDivLoss(): the mean over ALL elements (KD.py:6,:17)
    }
    if ((rc = prep_jobs()) || (rc = product_jobs())) return rc;
    // one buffer serves both reductions, one after the other on the stream
    if ((rc = c->part.ensure(std::max(atb_partial_floats(gate_jobs), atb_partial_floats(grad_jobs)),
                             "train_step: out of device memory for the partial products%s%s"))) return rc;
    gate_jobs.partial = grad_jobs.partial = c->part.p;
    return FARNN_OK;
}
// the preparation jobs of stage 4: the outputs and accumulators to zero, the transposes, the column sum of C
int TrainStep::prep_jobs() {
    PrepJobs &pj = prep;
    prep_add(pj, 0, nullptr, o->loss, 1, 1); prep_add(pj, 0, nullptr, o->dVgen, V, R); prep_add(pj, 0, nullptr, o->dS1, S, R);
    prep_add(pj, 0, nullptr, o->dS2, S, R); prep_add(pj, 0, nullptr, o->dW, S, S); prep_add(pj, 0, nullptr, o->dC, K, S);
    prep_add(pj, 0, nullptr, o->dh0, 1, S); prep_add(pj, 0, nullptr, o->dhT, 1, S); prep_add(pj, 0, nullptr, c->dOsum, 1, S);
    prep_add(pj, 1, w->S1, c->S1T, S, R); prep_add(pj, 1, w->S2, c->S2T, S, R); prep_add(pj, 1, w->W, c->WT, S, S);
    prep_add(pj, 2, w->C, c->Osum, K, S);
    if (farnn) {
        prep_add(pj, 0, nullptr, o->dWss1, S, S); prep_add(pj, 0, nullptr, o->dWrs1, R, S); prep_add(pj, 0, nullptr, o->dbs1, 1, S);
        prep_add(pj, 1, w->Wss1, c->Wss1T, S, S); prep_add(pj, 1, w->Wrs1, c->Wrs1T, R, S);
        prep_add(pj, 1, w->Vgen, c->VgenT.p, V, R); prep_add(pj, 0, nullptr, c->GV.p, 4 * V, S);      // GV1 | GV2 | dGV1 | dGV2
        if (farnn == 2) {
            prep_add(pj, 0, nullptr, o->dWss2, S, S); prep_add(pj, 0, nullptr, o->dWrs2, R, S); prep_add(pj, 0, nullptr, o->dbs2, 1, S);
            prep_add(pj, 1, w->Wss2, c->Wss2T, S, S); prep_add(pj, 1, w->Wrs2, c->Wrs2T, R, S);
        }
    }
    return pj.total < 0 ? fail(FARNN_ERANGE, "train_step: too many preparation jobs%s%s") : FARNN_OK;
}
// the products of stage 4 (the gates' input halves) and of stage 8 (the parameter gradients), as job lists
int TrainStep::product_jobs() {
    const int S = (int)this->S, R = (int)this->R, K = (int)this->K, V = (int)this->V;      // as the job fields hold them
    const long long N1 = (long long)this->N1, N0 = (long long)this->N0;
    const size_t VS = this->V * this->S;
    gate_jobs.chunk = grad_jobs.chunk = 128;
    if (farnn) {
        // GV = Vgen Wrs as A^T B with the rank as the reduction index: A = Vgen^T [R][V], B = Wrs [R][S]
        atb_add(gate_jobs, c->VgenT.p, w->Wrs1, c->GV.p, R, V, S);
        if (farnn == 2) atb_add(gate_jobs, c->VgenT.p, w->Wrs2, c->GV.p + VS, R, V, S);
    }
    // parameter gradients = tall-skinny products over the per-token rows (rows of non-tokens are zero)
    AtbJobs &jobs = grad_jobs;
    if (!mx) {
        atb_add(jobs, p.Zf, p.Tf, o->dS2, N1, S, R);                 // dS2 += Zf^T (v*rr)
        if (!farnn) {
            atb_add(jobs, p.A, p.D1f + R, o->dS1, N1 - 1, S, R);     // dS1 += f_{t-1}^T (u*v)
            atb_add(jobs, p.A, p.Zf + S, o->dW, N1 - 1, S, S);       // dW  += f_{t-1}^T z
        } else {                                                     // the chain input is hbar_t, stored per row
            atb_add(jobs, p.HBARf, p.D1f, o->dS1, N1, S, R);
            atb_add(jobs, p.HBARf, p.Zf, o->dW, N1, S, S);
        }
        atb_add(jobs, p.Zb, p.Tb, o->dS1, N1, S, R);                 // backward chain: roles of S1, S2 swap
        atb_add(jobs, p.BBAR, p.D1b, o->dS2, N1, S, R);
        atb_add(jobs, p.Zb, p.BBAR, o->dW, N1, S, S);                // pre_j += sum_s bbar_s W[j][s]
    }
    atb_add(jobs, p.DS, p.AB, o->dC, N0, K, S);                      // dC += ds^T (alpha*beta)
    if (farnn) {
        // gates read the raw previous state (stash shifted by one row) and v_t: dWss = h_{t-1}^T da, dWrs = v^T da, dbs = 1^T da
        atb_add(jobs, p.A, p.DAZf + S, o->dWss1, N1 - 1, S, S);
        atb_add(jobs, p.Bk, p.DAZb + S, o->dWss1, N1 - 1, S, S);
        atb_add(jobs, w->Vgen, p.dGV1, o->dWrs1, V, R, S);           // dWrs = Vgen^T dGV
        atb_add(jobs, dGVT, c->Wrs1T, o->dVgen, S, V, R);            // dVgen += dGV Wrs^T
        atb_add(jobs, c->ones.p, p.DAZf, o->dbs1, N1, 1, S);
        atb_add(jobs, c->ones.p, p.DAZb, o->dbs1, N1, 1, S);
        if (farnn == 2) {
            atb_add(jobs, p.A, p.DARf + S, o->dWss2, N1 - 1, S, S);
            atb_add(jobs, p.Bk, p.DARb + S, o->dWss2, N1 - 1, S, S);
            atb_add(jobs, w->Vgen, p.dGV2, o->dWrs2, V, R, S);
            atb_add(jobs, dGVT + VS, c->Wrs2T, o->dVgen, S, V, R);
            atb_add(jobs, c->ones.p, p.DARf, o->dbs2, N1, 1, S);
            atb_add(jobs, c->ones.p, p.DARb, o->dbs2, N1, 1, S);
        }
    }
    return jobs.total_wgs < 0 ? fail(FARNN_ERANGE, "train_step: too many gradient products for one launch%s%s") : FARNN_OK;
}
// Stage 4: zero the workspace, the outputs and the accumulators, transpose the weights; the gates' input halves
int TrainStep::prepare() {
    FARNN_HIP_TRY(hipMemsetAsync(c->ws.p, 0, need * sizeof(float), s));
    train_prep_kernel<<<(prep.total + 255) / 256, 256, 0, s>>>(prep);
    if (farnn) atb_launch(gate_jobs, s);
    return FARNN_OK;
}
// The one instantiation of a chain kernel for (ldsw, gated, ns) at these sizes: f(LDSW, GATED, VPS, VPR, NS) as integral
// constants -- weights in LDS or through L2, with or without the gate state, slots per thread for the states and the rank,
// sequences per workgroup.  The weights-in-LDS forms exist with TR_NSEQ sequences per workgroup only.
template <typename F>
static int with_chain_form(const TrainPlan &pl, bool ldsw, int ns, F &&f) {
    auto slots = [&](auto LDSW, auto GATED, auto NS) {
        if (NS() * pl.S > (size_t)TR_THREADS) return f(LDSW, GATED, int_c<2>(), int_c<2>(), NS);
        if (NS() * pl.R > (size_t)TR_THREADS) return f(LDSW, GATED, int_c<1>(), int_c<2>(), NS);
        return f(LDSW, GATED, int_c<1>(), int_c<1>(), NS);
    };
    auto gates = [&](auto LDSW, auto NS) { return pl.farnn ? slots(LDSW, std::true_type(), NS) : slots(LDSW, std::false_type(), NS); };
    if (ldsw) return gates(std::true_type(), int_c<TR_NSEQ>());
    return ns == TR_NSEQ ? gates(std::false_type(), int_c<TR_NSEQ>()) : gates(std::false_type(), int_c<TR_NSEQ_L2>());
}
// Stage 5: both chains with the state stash
int TrainStep::forward() {
    return with_chain_form(*this, ldsw_f, ns_f, [&](auto LDSW, auto GATED, auto VPS, auto VPR, auto NS) {
        return launch(train_forward_kernel<LDSW(), GATED(), VPS(), VPR(), NS()>, dim3((B + NS() - 1) / NS(), 2), TR_THREADS, lds_f, s, p);
    });
}
// Stage 5, max semiring: the positions bucketed by word (onehot_train.hip.h), the distinct words' slots, their blocks, both chains
int TrainStep::max_forward() {
    int rc;
    // (with a teacher every position is bucketed: the chains run through the pad tokens, whose words need their blocks too)
    if ((rc = clear_bucket_counts(m.bk, V, N0, s)) || (rc = launch_bucketing(p.x, p.len, B, L, (int)V, m.bk, nullptr, s, teacher))) return rc;
    tmax_slots_kernel<<<1, 1024, 0, s>>>(m.bk.wcount, (int)V, m.wslot, m.wlist, m.nwords);
    const unsigned nt = (unsigned)((S + 31) / 32);
    tmax_premix_kernel<<<dim3((unsigned)nwmax, nt * nt), 256, 0, s>>>(w->Vgen, w->S1, w->S2, w->W, m.wlist, m.nwords, m.M, m.MT, (int)S, (int)R);
    return launch(tmax_forward_kernel, dim3(B, 2), TM_THREADS, lds_tok, s, p, m.mp);
}
// Stage 6: the scores, the loss (cross-entropy or CRF), the decode, the adjoints of both chains' states
int TrainStep::loss() {
    int rc;
    if (teacher) return teacher_loss();
    if (!crf) return launch_train_loss<0>(p, lgrid, s);
    // emissions -> CRF forward-backward (loss, d loss / d emissions, transition counts, Viterbi tags) -> adjoints
    if ((rc = launch_train_loss<1>(p, lgrid, s))) return rc;
    // (large tag sets: transitions, expected counts and emissions stay in global memory)
    if ((rc = crf_big ? launch(train_crf_kernel<true>, B, 256, lds_c, s, p) : launch(train_crf_kernel<false>, B, 256, lds_c, s, p))) return rc;
    crf_reduce_kernel<<<(unsigned)((K * K + 255) / 256), 256, 0, s>>>(p.dtrans_part, o->dtrans, B, (int)(K * K));
    return launch_train_loss<2>(p, lgrid, s);
}
// The teacher's refusals (stage 2: nothing is enqueued, the outputs stay untouched)
int TrainStep::teacher_check() const {
    if (!tch) return FARNN_OK;
    if (!re) return fail(FARNN_EINVAL, "teacher_train_step: null teacher scores%s%s");
    if (tch->mode != FARNN_TEACHER_KD && tch->mode != FARNN_TEACHER_PR)
        return fail(FARNN_EINVAL, "teacher_train_step: mode must be FARNN_TEACHER_KD or FARNN_TEACHER_PR%s%s");
    if (!(tch->c1 >= 1.0f) || !std::isfinite(tch->c1)) return fail(FARNN_EINVAL, "teacher_train_step: c1 must be at least 1 (main.py asserts it)%s%s");
    if (!(tch->pi >= 0.0f && tch->pi <= 1.0f)) return fail(FARNN_EINVAL, "teacher_train_step: pi must lie in [0, 1]%s%s");
    if (!tch_max && c->semiring == FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "teacher_train_step: the max semiring has no KD / PR teacher (its kernels walk the valid positions only)%s%s");
    if (tch_max && c->semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "teacher_max_train_step: the context is in the sum semiring (farnn_train_set_semiring, or farnn_decomp_ifst_teacher_train_step)%s%s");
    return FARNN_OK;
}
// Stage 6 with a teacher (train_teacher.hip.h): the same split around the CRF kernel, every position walked, then the loss
// from the wavefronts' partials (and pi times the CRF's sum and transition gradient)
int TrainStep::teacher_loss() {
    int rc;
    if (!crf) {
        if ((rc = launch_teacher_loss<0>(p, lgrid, s))) return rc;
    } else {
        if ((rc = launch_teacher_loss<1>(p, lgrid, s))) return rc;
        if ((rc = crf_big ? launch(train_crf_kernel<true>, B, 256, lds_c, s, p) : launch(train_crf_kernel<false>, B, 256, lds_c, s, p))) return rc;
        crf_reduce_kernel<<<(unsigned)((K * K + 255) / 256), 256, 0, s>>>(p.dtrans_part, o->dtrans, B, (int)(K * K));
        if ((rc = launch_teacher_loss<2>(p, lgrid, s))) return rc;
    }
    const int KK = crf ? (int)(K * K) : 0;
    teacher_finish_kernel<<<(unsigned)std::max(1, (KK + 255) / 256), 256, 0, s>>>(p.loss_part, (int)lgrid * 8, o->loss, p.t_pi, crf ? 1 : 0,
                                                                               crf ? o->dtrans : nullptr, KK);
    return FARNN_OK;
}
// Stage 7: back-propagation through time (max semiring: max_backward)
int TrainStep::backward() {
    return with_chain_form(*this, ldsw_b, ns_b, [&](auto LDSW, auto GATED, auto VPS, auto VPR, auto NS) {
        return launch(train_backward_kernel<LDSW(), GATED(), VPS(), VPR(), NS()>, dim3((B + NS() - 1) / NS(), 2), TR_THREADS, lds_b, s, p);
    });
}
// Stage 8a, max semiring: dM per distinct word, then dS1 (+ dVgen, dW) and dS2 from it
int TrainStep::max_weight_gradients() {
    int rc;
    if ((rc = launch(tmax_dM_kernel, (unsigned)nwmax, TM_THREADS, lds_m, s, p, m.mp, m.bk.list, m.bk.wstart, m.bk.wcount, m.dM))) return rc;
    const dim3 wgrid((unsigned)((R + 63) / 64), (unsigned)((S + 31) / 32), TM_WCH);
    if ((rc = launch(tmax_wgrad_kernel<false>, wgrid, 256, lds_w, s, p, m.mp, m.dM, o->dS1, o->dW))) return rc;
    return launch(tmax_wgrad_kernel<true>, wgrid, 256, lds_w, s, p, m.mp, m.dM, o->dS2, o->dW);
}
// Stage 8: the parameter gradients as products over the per-token rows
int TrainStep::gradients() {
    if (farnn) {                                       // dGV^T for dVgen += dGV Wrs^T
        PrepJobs tj = {};
        for (int gsel = 0; gsel < farnn; gsel++) prep_add(tj, 1, c->GV.p + (2 + gsel) * V * S, dGVT + gsel * S * V, V, S);
        train_prep_kernel<<<(tj.total + 255) / 256, 256, 0, s>>>(tj);
    }
    if (mx) { if (int rc = max_weight_gradients()) return rc; }
    atb_launch(grad_jobs, s);
    add_row_to_all_kernel<<<(unsigned)((K * S + 255) / 256), 256, 0, s>>>(o->dC, c->dOsum, (int)K, (int)S);
    return FARNN_OK;
}

extern "C" int farnn_decomp_ifst_train_step(farnn_train_ctx *c, const farnn_train_weights *w, const int64_t *x,
                                            const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                            int64_t valid_tokens, const farnn_train_outputs *o, void *stream) {
    TunScope tun_scope(c ? &c->tun : nullptr);     // (a null context: run_train_step refuses it)
    if (c && c->vector_input) return fail(FARNN_EINVAL, "train_step: a vector-input context takes farnn_decomp_sf_train_step%s%s");
    return run_train_step<TrainStep>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}

extern "C" int farnn_decomp_ifst_teacher_train_step(farnn_train_ctx *c, const farnn_train_weights *w, const int64_t *x,
                                                    const int64_t *lengths, const int64_t *labels, const float *re_scores,
                                                    const farnn_teacher *teacher, int32_t B, int32_t L, int64_t valid_tokens,
                                                    const farnn_train_outputs *o, void *stream) {
    TunScope tun_scope(c ? &c->tun : nullptr);
    if (!re_scores || !teacher) return fail(FARNN_EINVAL, "teacher_train_step: null teacher argument%s%s");
    if (c && c->vector_input) return fail(FARNN_EINVAL, "teacher_train_step: a vector-input context has no teacher (the KL term reads the scores at the pad positions)%s%s");
    return run_train_step<TrainStep>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream,
                                     [&](TrainStep &t) { t.re = re_scores; t.tch = teacher; });
}

// The same step on a context in the max semiring (--train_mode max --marryup_type kd | pr): the tmax_* chains run L steps for
// every sequence, every position is bucketed, and the loss kernels are the sum step's -- only the recurrences are max-times.
extern "C" int farnn_decomp_ifst_teacher_max_train_step(farnn_train_ctx *c, const farnn_train_weights *w, const int64_t *x,
                                                        const int64_t *lengths, const int64_t *labels, const float *re_scores,
                                                        const farnn_teacher *teacher, int32_t B, int32_t L, int64_t valid_tokens,
                                                        const farnn_train_outputs *o, void *stream) {
    TunScope tun_scope(c ? &c->tun : nullptr);
    if (!re_scores || !teacher) return fail(FARNN_EINVAL, "teacher_max_train_step: null teacher argument%s%s");
    if (c && c->vector_input) return fail(FARNN_EINVAL, "teacher_max_train_step: a vector-input context has no teacher (the KL term reads the scores at the pad positions)%s%s");
    return run_train_step<TrainStep>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream,
                                     [&](TrainStep &t) { t.re = re_scores; t.tch = teacher; t.tch_max = true; });
}

// ---- training step of the vector-input i-FST (FARNN_S_SF; sf_train.hip.h) ---------------------------------
// The decomposed i-FST's step with v [B][L][R] as the chains' table and the ids b L + t as their tokens (p.V = B L): the plan,
// the chains, the loss and the job lists' shared part are TrainStep's; what was per word (the gate halves, their adjoints,
// dWrs, dVgen) is per token here.  Sum semiring, no teacher.
struct SfStep : TrainStep {
    static constexpr const char *name = "decomp_sf_train";
    const float *v; float *dv;
    SfGateParams gp; SfDvParams dp;
    size_t need_sf; unsigned tgrid;
    float *GV1, *GV2, *dG1, *dG2, *VM;       // VM [B L][R]: v at the valid positions, zero at the pads (dWrs is reduced from it)

    int validate() {
        if (!c->vector_input) return fail(FARNN_EINVAL, "decomp_sf_train_step: the context was made by farnn_train_create (word ids): farnn_decomp_ifst_train_step is its step%s%s");
        if (w->Vgen || o->dVgen) return fail(FARNN_EINVAL, "decomp_sf_train_step: Vgen and dVgen must be NULL (the input is v, its gradient dv)%s%s");
        if (!w->S1 || !w->S2 || !w->W || !w->C || !w->h0 || !w->hT) return fail(FARNN_EINVAL, "decomp_sf_train_step: null weight%s%s");
        if (!o->loss || !o->dS1 || !o->dS2 || !o->dW || !o->dC || !o->dh0 || !o->dhT || !o->tags)
            return fail(FARNN_EINVAL, "decomp_sf_train_step: null output%s%s");
        if (c->d.use_crf && (!w->crf_trans || !o->dtrans)) return fail(FARNN_EINVAL, "decomp_sf_train_step: CRF transitions / their gradient missing%s%s");
        if (c->d.farnn >= 1 && (!w->Wss1 || !w->Wrs1 || !w->bs1 || !o->dWss1 || !o->dWrs1 || !o->dbs1))
            return fail(FARNN_EINVAL, "decomp_sf_train_step: update-gate weights / gradients missing%s%s");
        if (c->d.farnn == 2 && (!w->Wss2 || !w->Wrs2 || !w->bs2 || !o->dWss2 || !o->dWrs2 || !o->dbs2))
            return fail(FARNN_EINVAL, "decomp_sf_train_step: reset-gate weights / gradients missing%s%s");
        return FARNN_OK;
    }
    // the step's own arrays, behind everything the chains lay out (none of them needs the step's memset: every element read is written first)
    size_t carve_sf(float *base) {
        Carver<float> a(base);
        p.DVf = a.take(N1 * R); p.DVb = a.take(N1 * R); p.HP = a.take((size_t)B * 2 * S); p.OP = a.take((size_t)B * 2 * S);
        if (crf) p.crf_loss_part = a.take((size_t)B); else p.loss_part = a.take((size_t)lgrid * 8);
        if (farnn) { GV1 = a.take(N0 * S); GV2 = a.take(N0 * S); dG1 = a.take(N0 * S); dG2 = a.take(N0 * S); VM = a.take(N0 * R); }
        return a.off;
    }
    int plan(int B_, int L_) {
        if (int rc = train_plan(c, B_, L_, false, *this)) return rc;       // (the sum semiring: farnn_train_set_semiring refuses the other)
        V = N0;                                                            // the "vocabulary" of the chains: one row per position
        need_sf = carve_sf(nullptr);
        tgrid = (unsigned)std::min<size_t>(4 * (size_t)c->n_cu, (N0 + SF_TP - 1) / SF_TP);
        int rc;
        return (farnn && (rc = lds_fits(sf_gate_lds_bytes(R)))) ? rc : lds_fits(sf_dv_lds_bytes(S, farnn));
    }
    int carve(const int64_t *, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prepare(); int sf_loss(); int backward(); int gradients();
    int stages() {
        int rc;
        if ((rc = prepare()) || (rc = forward()) || (rc = sf_loss())) return rc;
        return (rc = backward()) ? rc : gradients();
    }
};

int SfStep::carve(const int64_t *, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens) {
    int rc;
    if ((rc = c->ws.ensure(need + need_sf, "decomp_sf_train_step: out of device memory for the workspace%s%s"))) return rc;
    if (farnn && c->ones.n < N1) {
        if ((rc = c->ones.ensure(N1, "decomp_sf_train_step: out of device memory for the column of ones%s%s"))) return rc;
        std::vector<float> hones(N1, 1.0f);
        FARNN_HIP_TRY(hipMemcpy(c->ones.p, hones.data(), N1 * sizeof(float), hipMemcpyHostToDevice));
    }
    if (c->ids.n < N0) {
        // growth only (like the column of ones): filled on the device and awaited here, so that a later step on any stream finds them
        if ((rc = c->ids.ensure(N0, "decomp_sf_train_step: out of device memory for the position ids%s%s"))) return rc;
        sf_iota_kernel<<<(unsigned)((c->ids.n + 255) / 256), 256, 0, s>>>(c->ids.p, c->ids.n);
        FARNN_HIP_TRY(hipStreamSynchronize(s));
    }
    [[maybe_unused]] const size_t carved = carve_train_ws(c->ws.p, p, *this), carved_sf = carve_sf(c->ws.p + need);
    assert(carved == need && carved_sf == need_sf);
    p.Vgen = v; p.S1 = w->S1; p.S2 = w->S2; p.W = w->W; p.C = w->C; p.h0 = w->h0; p.hT = w->hT; p.P = w->P;
    p.S1T = c->S1T; p.S2T = c->S2T; p.WT = c->WT; p.Osum = c->Osum;
    p.x = c->ids.p; p.len = lengths; p.labels = labels; p.err = c->err.dev;
    if (crf) p.trans = w->crf_trans;
    p.farnn = farnn; p.sig_k = c->d.sigmoid_exponent;
    if (farnn) {
        p.Wss1 = w->Wss1; p.Wrs1 = w->Wrs1; p.bs1 = w->bs1; p.Wss2 = w->Wss2; p.Wrs2 = w->Wrs2; p.bs2 = w->bs2;
        p.Wss1T = c->Wss1T; p.Wss2T = c->Wss2T; p.Wrs1T = c->Wrs1T; p.Wrs2T = c->Wrs2T;
        p.GV1 = GV1; p.GV2 = GV2;
    }
    p.nss_f = nss_f; p.nss_b = nss_b;
    p.dOsum = c->dOsum; p.dh0 = o->dh0; p.dhT = o->dhT; p.loss = o->loss; p.tags = o->tags;
    p.B = B; p.L = L; p.V = (int)N0; p.S = (int)S; p.R = (int)R; p.K = (int)K; p.nl = c->d.nl; p.o_idx = c->d.o_idx;
    p.threshold = c->d.threshold; p.inv_tokens = 1.0f / (float)valid_tokens;
    gp = {v, lengths, w->Wrs1, w->Wrs2, GV1, GV2, VM, B, L, (int)S, (int)R, farnn};
    dp = {lengths, p.DVf, p.DVb, p.DAZf, p.DAZb, p.DARf, p.DARb, c->Wrs1T, c->Wrs2T, dv, dG1, dG2, B, L, (int)S, (int)R, farnn};
    // the preparation jobs: the outputs and accumulators to zero, the transposes, the column sum of C
    PrepJobs &pj = prep;
    prep_add(pj, 0, nullptr, o->loss, 1, 1); prep_add(pj, 0, nullptr, o->dS1, S, R);
    prep_add(pj, 0, nullptr, o->dS2, S, R); prep_add(pj, 0, nullptr, o->dW, S, S); prep_add(pj, 0, nullptr, o->dC, K, S);
    prep_add(pj, 0, nullptr, o->dh0, 1, S); prep_add(pj, 0, nullptr, o->dhT, 1, S); prep_add(pj, 0, nullptr, c->dOsum, 1, S);
    prep_add(pj, 1, w->S1, c->S1T, S, R); prep_add(pj, 1, w->S2, c->S2T, S, R); prep_add(pj, 1, w->W, c->WT, S, S);
    prep_add(pj, 2, w->C, c->Osum, K, S);
    if (farnn) {
        prep_add(pj, 0, nullptr, o->dWss1, S, S); prep_add(pj, 0, nullptr, o->dWrs1, R, S); prep_add(pj, 0, nullptr, o->dbs1, 1, S);
        prep_add(pj, 1, w->Wss1, c->Wss1T, S, S); prep_add(pj, 1, w->Wrs1, c->Wrs1T, R, S);
        if (farnn == 2) {
            prep_add(pj, 0, nullptr, o->dWss2, S, S); prep_add(pj, 0, nullptr, o->dWrs2, R, S); prep_add(pj, 0, nullptr, o->dbs2, 1, S);
            prep_add(pj, 1, w->Wss2, c->Wss2T, S, S); prep_add(pj, 1, w->Wrs2, c->Wrs2T, R, S);
        }
    }
    if (pj.total < 0) return fail(FARNN_ERANGE, "decomp_sf_train_step: too many preparation jobs%s%s");
    // the parameter gradients: the id step's products over the per-token rows; dWrs = sum over the valid positions of
    // v_t^T (the position's gate adjoints), from the masked copy of v and sf_dv_kernel's per-position sums (zero rows at the pads)
    const int iS = (int)S, iR = (int)R, iK = (int)K;
    const long long n1 = (long long)N1, n0 = (long long)N0;
    AtbJobs &jobs = grad_jobs;
    jobs.chunk = 128;
    atb_add(jobs, p.Zf, p.Tf, o->dS2, n1, iS, iR);
    if (!farnn) {
        atb_add(jobs, p.A, p.D1f + R, o->dS1, n1 - 1, iS, iR);
        atb_add(jobs, p.A, p.Zf + S, o->dW, n1 - 1, iS, iS);
    } else {
        atb_add(jobs, p.HBARf, p.D1f, o->dS1, n1, iS, iR);
        atb_add(jobs, p.HBARf, p.Zf, o->dW, n1, iS, iS);
    }
    atb_add(jobs, p.Zb, p.Tb, o->dS1, n1, iS, iR);
    atb_add(jobs, p.BBAR, p.D1b, o->dS2, n1, iS, iR);
    atb_add(jobs, p.Zb, p.BBAR, o->dW, n1, iS, iS);
    atb_add(jobs, p.DS, p.AB, o->dC, n0, iK, iS);
    if (farnn) {
        atb_add(jobs, p.A, p.DAZf + S, o->dWss1, n1 - 1, iS, iS);
        atb_add(jobs, p.Bk, p.DAZb + S, o->dWss1, n1 - 1, iS, iS);
        atb_add(jobs, VM, dG1, o->dWrs1, n0, iR, iS);
        atb_add(jobs, c->ones.p, p.DAZf, o->dbs1, n1, 1, iS);
        atb_add(jobs, c->ones.p, p.DAZb, o->dbs1, n1, 1, iS);
        if (farnn == 2) {
            atb_add(jobs, p.A, p.DARf + S, o->dWss2, n1 - 1, iS, iS);
            atb_add(jobs, p.Bk, p.DARb + S, o->dWss2, n1 - 1, iS, iS);
            atb_add(jobs, VM, dG2, o->dWrs2, n0, iR, iS);
            atb_add(jobs, c->ones.p, p.DARf, o->dbs2, n1, 1, iS);
            atb_add(jobs, c->ones.p, p.DARb, o->dbs2, n1, 1, iS);
        }
    }
    if (jobs.total_wgs < 0) return fail(FARNN_ERANGE, "decomp_sf_train_step: too many gradient products for one launch%s%s");
    if ((rc = c->part.ensure(atb_partial_floats(jobs), "decomp_sf_train_step: out of device memory for the partial products%s%s"))) return rc;
    jobs.partial = c->part.p;
    return FARNN_OK;
}
// Stage 4: zero the chains' workspace, the outputs and the accumulators, transpose the weights; the gates' input halves of the
// valid positions
int SfStep::prepare() {
    FARNN_HIP_TRY(hipMemsetAsync(c->ws.p, 0, need * sizeof(float), s));
    train_prep_kernel<<<(prep.total + 255) / 256, 256, 0, s>>>(prep);
    return farnn ? launch(sf_gate_kernel, tgrid, SF_THREADS, sf_gate_lds_bytes(R), s, gp) : FARNN_OK;
}
// Stage 6: TrainStep's, with the loss summed from partials in index order (per wavefront of the loss kernel, or per sequence
// of the CRF kernel) in place of the float atomics
int SfStep::sf_loss() {
    if (int rc = loss()) return rc;
    if (crf) onehot_loss_sum_kernel<<<1, 64, 0, s>>>(p.crf_loss_part, B, o->loss);
    else launch_loss_sum(p.loss_part, lgrid, o->loss, s);
    return FARNN_OK;
}
// Stage 7: back-propagation through time: d v_t and the gates' input adjoints stay in their per-step rows (the DET form)
int SfStep::backward() {
    return with_chain_form(*this, ldsw_b, ns_b, [&](auto LDSW, auto GATED, auto VPS, auto VPR, auto NS) {
        return launch(train_backward_kernel<LDSW(), GATED(), VPS(), VPR(), NS(), true, true>, dim3((B + NS() - 1) / NS(), 2), TR_THREADS, lds_b, s, p);
    });
}
// Stage 8: dv assembled per position, then the parameter gradients as products over the per-token rows
int SfStep::gradients() {
    if (int rc = launch(sf_dv_kernel, tgrid, SF_THREADS, sf_dv_lds_bytes(S, farnn), s, dp)) return rc;
    sf_seq_sum_kernel<<<(unsigned)((3 * S + 255) / 256), 256, 0, s>>>(p.HP, p.OP, o->dh0, o->dhT, c->dOsum, B, (int)S);
    atb_launch(grad_jobs, s);
    add_row_to_all_kernel<<<(unsigned)((K * S + 255) / 256), 256, 0, s>>>(o->dC, c->dOsum, (int)K, (int)S);
    return FARNN_OK;
}

extern "C" int farnn_decomp_sf_train_step(farnn_train_ctx *c, const farnn_train_weights *w, const float *v, const int64_t *lengths,
                                          const int64_t *labels, int32_t B, int32_t L, int64_t valid_tokens,
                                          const farnn_train_outputs *o, float *dv, void *stream) {
    TunScope tun_scope(c ? &c->tun : nullptr);
    if (!v || !dv) return fail(FARNN_EINVAL, "decomp_sf_train_step: null v or dv%s%s");
    // (the chains' token ids are the context's own: the driver's x argument only has to be non-null)
    return run_train_step<SfStep>(c, w, lengths, lengths, labels, B, L, valid_tokens, o, stream,
                                  [&](SfStep &t) { t.v = v; t.dv = dv; });
}

// ---- training step of the decomposed FST (FARNN_S_D_W; decomp0_train.hip.h) ------------------------------
struct farnn_decomp_fst_train_ctx : TrainCtxBase {
    Tunables tun;
    farnn_decomp_fst_train_dims d;
    int n_cu = 256;
    int semiring = FARNN_SEMIRING_SUM;  // farnn_decomp_fst_train_set_semiring
    DevBuf<float> fixed;          // create's block: what depends on the dimensions only (Decomp0Step::carve_fixed)
    DevBuf<float> ws;             // per-batch workspace (zeroed every step)
    DevBuf<int> iws;              // the bucketing of the positions by word
    DevBuf<float> part;           // partial products of the parameter-gradient reductions
    DevBuf<float> ones;           // 1.0f each: the chains' output mask and the bias gradients' column of ones
    size_t ones_filled = 0;       // how many of them a step has written (the buffer grows with the batch)
    DevBuf<float> mws;            // max semiring only (Decomp0Step::carve_max_floats): M, MT, dM, IN, GM, the chunks' partial sums;
    DevBuf<int> miws;             // IDX, the word slots -- allocated on first use
};
// what create's block holds
struct D0Fixed {
    float *S1T, *S2T, *Wm, *WT, *S1wT, *S2wT, *csum, *cwsum, *dOsum, *Rtab, *dRt, *dVs, *dS1s, *dS2s, *X1, *X2;
    float *Wss1T, *Wss2T, *GV1, *GV2, *dGV1, *dGV2, *dRg1, *dRg2;      // farnn > 0
};
static size_t carve_d0_fixed(float *base, D0Fixed &f, const farnn_decomp_fst_train_dims &d) {
    Carver<float> a(base);
    const size_t S = d.S, R = d.R, Q = d.Q, V = d.V;
    f.S1T = a.take(S * R); f.S2T = a.take(S * R); f.Wm = a.take(S * S); f.WT = a.take(S * S);
    f.S1wT = a.take(S * Q); f.S2wT = a.take(S * Q); f.csum = a.take(R); f.cwsum = a.take(Q); f.dOsum = a.take(S);
    f.Rtab = a.take(V * R); f.dRt = a.take(V * R); f.dVs = a.take(V * R); f.dS1s = a.take(S * R); f.dS2s = a.take(S * R);
    f.X1 = a.take(S * Q); f.X2 = a.take(S * Q);
    if (d.farnn) {
        f.Wss1T = a.take(S * S); f.Wss2T = a.take(S * S);
        f.GV1 = a.take(V * S); f.GV2 = a.take(V * S); f.dGV1 = a.take(V * S); f.dGV2 = a.take(V * S);
        f.dRg1 = a.take(V * R); f.dRg2 = a.take(V * R);
    }
    return a.off;
}

extern "C" int farnn_decomp_fst_train_create(const farnn_decomp_fst_train_dims *d, int device, farnn_decomp_fst_train_ctx **out) {
    if (!d || !out) return fail(FARNN_EINVAL, "decomp_fst_train_create: null argument%s%s");
    *out = nullptr;
    if (d->V <= 0 || d->S <= 0 || d->R <= 0 || d->Q <= 0 || d->K <= 0) return fail(FARNN_EINVAL, "decomp_fst_train_create: bad dimensions%s%s");
    if (d->nl < FARNN_NL_NONE || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "decomp_fst_train_create: bad nonlinearity%s%s");
    if (d->use_crf && (d->K < 4 || train_crf_lds_bytes(d->K, 4, true) > 160 * 1024))
        return fail(FARNN_ERANGE, "decomp_fst_train_create: CRF needs 4..190 score columns%s%s");
    if (d->farnn < 0 || d->farnn > 2) return fail(FARNN_EINVAL, "decomp_fst_train_create: farnn must be 0, 1 or 2%s%s");
    int rc;
    if ((rc = train_ctx_create("decomp_fst_train", d, device, out))) return rc;
    farnn_decomp_fst_train_ctx *c = *out;
    c->n_cu = device_cus(device);
    D0Fixed f;
    if ((rc = c->fixed.ensure(carve_d0_fixed(nullptr, f, *d), "decomp_fst_train_create: out of device memory%s%s"))) {
        train_ctx_destroy(c);
        *out = nullptr;
        return rc;
    }
    return FARNN_OK;
}
extern "C" void farnn_decomp_fst_train_destroy(farnn_decomp_fst_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_decomp_fst_train_set_profiling(farnn_decomp_fst_train_ctx *c, int32_t enable) { return train_ctx_set_profiling("decomp_fst_train", c, enable); }
extern "C" int farnn_decomp_fst_train_time(farnn_decomp_fst_train_ctx *c, double *total_ms, int64_t *steps) { return train_ctx_time("decomp_fst_train", c, total_ms, steps); }

extern "C" int farnn_decomp_fst_train_set_semiring(farnn_decomp_fst_train_ctx *c, int32_t semiring) {
    if (!c) return fail(FARNN_EINVAL, "decomp_fst_train_set_semiring: null context%s%s");
    if (semiring != FARNN_SEMIRING_SUM && semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "decomp_fst_train_set_semiring: semiring must be FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX%s%s");
    if (semiring == FARNN_SEMIRING_MAX && c->d.S > TM_MAX_S)
        return fail(FARNN_ERANGE, "decomp_fst_train_set_semiring: the max-semiring step holds at most 192 states%s%s");
    c->semiring = semiring;
    return FARNN_OK;
}

// C = A B, k ascending, every element one owner (decomp1_gemm_kernel): A element (m, k) at A[m am + k ak], B (k, n) at B[k bk + n bn]
static void d0_gemm(hipStream_t s, const float *A, size_t am, size_t ak, const float *Bm, size_t bk, size_t bn, float *Cm, int M, int N, int K) {
    const D1Gemm g = {A, Bm, nullptr, nullptr, Cm, M, N, K, am, ak, bk, bn, (size_t)N};
    decomp1_gemm_kernel<<<dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64)), 256, 0, s>>>(g);
}

// One step.  The chains and their back-propagation are the decomposed i-FST's (TrainPlan, with_chain_form) on the word table
// Rtab, the matrix W and a mask of ones; the stages are the member functions, in the order they run.  In the max semiring (mx) the
// chains are the i-FST's max chains on the same inputs, and the chain inputs' gradients come from the per-word dM_w
// (decomp0_train_max.hip.h) in place of the five chain products.
struct Decomp0Step : TrainPlan {
    static constexpr const char *name = "decomp_fst_train", *label_range = "K";
    farnn_decomp_fst_train_ctx *c; const farnn_decomp_fst_train_weights *w; const farnn_decomp_fst_train_outputs *o; hipStream_t s;
    TrainParams p; D0Params q; D0Fixed f; PrepJobs prep; AtbJobs jobs; Buckets bk; BucketedCrf crfst;
    D0Lds lds0; unsigned grid0; size_t Q, need0, ineed;
    float *DVS, *U, *UW, *DP, *DQ, *DPW, *DQW, *loss_part;
    MaxWs m; D0MaxWgrad mg; size_t mneed0, mineed0, lds_mw;      // max semiring only

    int validate() {
        if (!w->Vgen || !w->Ce || !w->S1 || !w->S2 || !w->Cw || !w->S1w || !w->S2w || !w->WW || !w->h0 || !w->hT)
            return fail(FARNN_EINVAL, "decomp_fst_train_step: null weight%s%s");
        if (!o->loss || !o->dVgen || !o->dCe || !o->dS1 || !o->dS2 || !o->dCw || !o->dS1w || !o->dS2w || !o->dWW || !o->dh0 || !o->dhT || !o->tags)
            return fail(FARNN_EINVAL, "decomp_fst_train_step: null output%s%s");
        if (c->d.use_crf && (!w->crf_trans || !o->dtrans)) return fail(FARNN_EINVAL, "decomp_fst_train_step: CRF transitions / their gradient missing%s%s");
        if (c->d.farnn >= 1 && (!w->Wss1 || !w->Wrs1 || !w->bs1 || !o->dWss1 || !o->dWrs1 || !o->dbs1))
            return fail(FARNN_EINVAL, "decomp_fst_train_step: update-gate weights / gradients missing%s%s");
        if (c->d.farnn == 2 && (!w->Wss2 || !w->Wrs2 || !w->bs2 || !o->dWss2 || !o->dWrs2 || !o->dbs2))
            return fail(FARNN_EINVAL, "decomp_fst_train_step: reset-gate weights / gradients missing%s%s");
        return FARNN_OK;
    }
    // the step's own arrays, behind everything the chains lay out (carve_train_ws)
    size_t carve_ws(float *base) {
        const size_t off0 = carve_train_ws(base, p, *this);
        Carver<float> a(base ? base + off0 : nullptr);
        p.DVf = a.take(N1 * R); p.DVb = a.take(N1 * R); p.HP = a.take((size_t)B * 2 * S);
        U = a.take(N0 * R); UW = a.take(N0 * Q); DVS = a.take(N0 * R);
        DP = a.take(N1 * R); DQ = a.take(N1 * R); DPW = a.take(N1 * Q); DQW = a.take(N1 * Q);
        loss_part = a.take((size_t)grid0 * D0_WAVES);
        if (crf) crfst.carve(a, (size_t)B, (size_t)L, K, false);
        return off0 + a.off;
    }
    // the max semiring's workspaces: the i-FST's blocks and per-step arrays, the chunks' partial sums behind them; the argmax
    // of every step and the word slots (the bucketing is the step's own, iws)
    size_t carve_max_floats0(float *base) {
        const size_t off0 = carve_max_floats(base, m, *this);
        Carver<float> a(base ? base + off0 : nullptr);
        const size_t nch = d0max_chunks(nwmax);
        mg.PS1 = a.take(nch * S * R); mg.PS2 = a.take(nch * S * R); mg.PW = a.take(nch * S * S);
        return off0 + a.off;
    }
    size_t carve_max_ints0(int *base) {
        Carver<int> a(base);
        m.mp.IDXf = a.take(N1 * S); m.mp.IDXb = a.take(N1 * S);
        m.mp.wslot = m.wslot = a.take(V); m.mp.wlist = m.wlist = a.take(nwmax); m.mp.nwords = m.nwords = a.take(1);
        return a.off;
    }
    // every size the step refuses, before anything is enqueued
    int plan(int B_, int L_) {
        Q = (size_t)c->d.Q;
        if (Q > (size_t)TR_VPT * TR_THREADS / TR_NSEQ) return fail(FARNN_ERANGE, "decomp_fst_train_step: wildcard rank above 512%s%s");
        if ((unsigned long long)B_ * (L_ + 1) * Q >= (1ull << 30))
            return fail(FARNN_ERANGE, "decomp_fst_train_step: B (L+1) Q must stay below 2^30 elements%s%s");
        if (int rc = train_plan(c, B_, L_, false, *this)) return rc;
        lds0 = decomp0_loss_lds(S, R, Q, K);
        if (int rc = lds_fits(lds0.bytes())) return rc;
        grid0 = (unsigned)std::min<size_t>(c->n_cu, (N0 + D0_TP - 1) / D0_TP);
        need0 = carve_ws(nullptr);
        ineed = carve_bucket_ints(nullptr, bk, V, N0);
        if (mx) {
            lds_mw = d0max_wgrad_lds_bytes(S);
            if (int rc = lds_fits(lds_mw)) return rc;
            mneed0 = carve_max_floats0(nullptr); mineed0 = carve_max_ints0(nullptr);
        }
        return FARNN_OK;
    }
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prepare(); int forward(); int max_forward(); int loss(); int backward(); int gradients(); int max_gradients();
    int max_backward() { return launch(tmax_backward_kernel<true>, dim3(B, 2), TM_THREADS, lds_tok, s, p, m.mp); }
    int stages() {
        int rc;
        if ((rc = prepare()) || (rc = mx ? max_forward() : forward()) || (rc = loss())) return rc;
        if (mx) return (rc = max_backward()) ? rc : max_gradients();
        return (rc = backward()) ? rc : gradients();
    }
    template <int PHASE>
    int launch_loss() {
        return lds0.clds() ? launch(decomp0_loss_kernel<true, PHASE>, grid0, D0_THREADS, lds0.bytes(), s, q)
                           : launch(decomp0_loss_kernel<false, PHASE>, grid0, D0_THREADS, lds0.bytes(), s, q);
    }
};

// Stage 3: grow the buffers, lay the workspaces out, fill the kernels' parameters and the job lists.  Nothing is enqueued yet.
int Decomp0Step::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens) {
    int rc;
    if ((rc = c->ws.ensure(need0, "decomp_fst_train_step: out of device memory for the workspace%s%s")) ||
        (rc = c->iws.ensure(ineed, "decomp_fst_train_step: out of device memory for the index workspace%s%s"))) return rc;
    const size_t nones = std::max(N1, S);
    if (c->ones.n < nones) {                                   // (filled on the step's stream, in prepare())
        if ((rc = c->ones.ensure(nones, "decomp_fst_train_step: out of device memory for the column of ones%s%s"))) return rc;
        c->ones_filled = 0;
    }
    if (mx && ((rc = c->mws.ensure(mneed0, "decomp_fst_train_step: out of device memory for the max-semiring workspace%s%s")) ||
               (rc = c->miws.ensure(mineed0, "decomp_fst_train_step: out of device memory for the max-semiring index workspace%s%s")))) return rc;
    [[maybe_unused]] const size_t carved = carve_ws(c->ws.p), icarved = carve_bucket_ints(c->iws.p, bk, V, N0);
    assert(carved == need0 && icarved == ineed);
    if (mx) {
        [[maybe_unused]] const size_t mcarved = carve_max_floats0(c->mws.p), micarved = carve_max_ints0(c->miws.p);
        assert(mcarved == mneed0 && micarved == mineed0);
    }
    carve_d0_fixed(c->fixed.p, f, c->d);
    // the chains: the i-FST's kernels on (Rtab, S1, S2, W, gates), no output mask
    p.Vgen = f.Rtab; p.S1 = w->S1; p.S2 = w->S2; p.W = f.Wm; p.C = nullptr; p.h0 = w->h0; p.hT = w->hT; p.P = w->P;
    p.S1T = f.S1T; p.S2T = f.S2T; p.WT = f.WT; p.Osum = c->ones.p;
    p.x = x; p.len = lengths; p.labels = labels; p.err = c->err.dev;
    p.farnn = farnn; p.sig_k = c->d.sigmoid_exponent;
    if (farnn) {
        p.Wss1 = w->Wss1; p.Wrs1 = w->Wrs1; p.bs1 = w->bs1; p.Wss2 = w->Wss2; p.Wrs2 = w->Wrs2; p.bs2 = w->bs2;
        p.Wss1T = f.Wss1T; p.Wss2T = f.Wss2T;
        p.GV1 = f.GV1; p.GV2 = f.GV2; p.dGV1 = f.dGV1; p.dGV2 = f.dGV2;
    }
    p.nss_f = nss_f; p.nss_b = nss_b;
    p.dOsum = f.dOsum; p.loss = o->loss; p.tags = o->tags;
    p.B = B; p.L = L; p.V = (int)V; p.S = (int)S; p.R = (int)R; p.K = (int)K; p.nl = c->d.nl; p.o_idx = c->d.o_idx;
    p.threshold = c->d.threshold; p.inv_tokens = 1.0f / (float)valid_tokens;
    // the score head
    q.Vgen = w->Vgen; q.Ce = w->Ce; q.Cw = w->Cw; q.S1 = w->S1; q.S2 = w->S2; q.S1w = w->S1w; q.S2w = w->S2w; q.P = w->P;
    q.S1T = f.S1T; q.S2T = f.S2T; q.S1wT = f.S1wT; q.S2wT = f.S2wT;
    q.A = p.A; q.Bk = p.Bk; q.GA = p.GA; q.GB = p.GB; q.x = x; q.len = lengths; q.labels = labels;
    q.SC = p.SC; q.DS = p.DS; q.U = U; q.UW = UW; q.DVS = DVS; q.DP = DP; q.DQ = DQ; q.DPW = DPW; q.DQW = DQW;
    q.loss_part = loss_part; q.tags = o->tags; q.err = c->err.dev;
    q.B = B; q.L = L; q.V = (int)V; q.S = (int)S; q.R = (int)R; q.Q = (int)Q; q.K = (int)K; q.o_idx = c->d.o_idx;
    q.threshold = c->d.threshold; q.inv_tokens = p.inv_tokens;
    if (crf) crfst.fill(w->crf_trans, nullptr, p.SC, p.DS, lengths, labels, o->tags, c->err.dev, B, L, K, c->d.o_idx, c->d.threshold);
    // the preparation jobs: the outputs the products add into and the score's shares to zero, the transposes, the column sums
    PrepJobs &pj = prep;
    prep_add(pj, 0, nullptr, o->loss, 1, 1); prep_add(pj, 0, nullptr, o->dS1, S, R); prep_add(pj, 0, nullptr, o->dS2, S, R);
    prep_add(pj, 0, nullptr, o->dWW, S, S); prep_add(pj, 0, nullptr, o->dCe, K, R); prep_add(pj, 0, nullptr, o->dCw, K, Q);
    prep_add(pj, 0, nullptr, o->dS1w, S, Q); prep_add(pj, 0, nullptr, o->dS2w, S, Q);
    prep_add(pj, 0, nullptr, f.dS1s, S, R); prep_add(pj, 0, nullptr, f.dS2s, S, R);
    prep_add(pj, 1, w->S1, f.S1T, S, R); prep_add(pj, 1, w->S2, f.S2T, S, R);
    prep_add(pj, 1, w->S1w, f.S1wT, S, Q); prep_add(pj, 1, w->S2w, f.S2wT, S, Q);
    prep_add(pj, 2, w->Ce, f.csum, K, R); prep_add(pj, 2, w->Cw, f.cwsum, K, Q);
    if (farnn) {
        prep_add(pj, 0, nullptr, o->dWss1, S, S); prep_add(pj, 0, nullptr, o->dbs1, 1, S); prep_add(pj, 1, w->Wss1, f.Wss1T, S, S);
        if (farnn == 2) { prep_add(pj, 0, nullptr, o->dWss2, S, S); prep_add(pj, 0, nullptr, o->dbs2, 1, S); prep_add(pj, 1, w->Wss2, f.Wss2T, S, S); }
    }
    if (pj.total < 0) return fail(FARNN_ERANGE, "decomp_fst_train_step: too many preparation jobs%s%s");
    // the products over the per-token rows.  Every output has at most two addends: the two chains' shares (a + b = b + a in
    // floating point, whichever atomic lands first); the score's shares of dS1 / dS2 go to a buffer of their own
    const int iS = (int)S, iR = (int)R, iQ = (int)Q, iK = (int)K;
    const long long n1 = (long long)N1, n0 = (long long)N0;
    jobs.chunk = 128;
    if (!mx) {
        atb_add(jobs, p.Zf, p.Tf, o->dS2, n1, iS, iR);
        if (!farnn) {
            atb_add(jobs, p.A, p.D1f + R, o->dS1, n1 - 1, iS, iR);
            atb_add(jobs, p.A, p.Zf + S, o->dWW, n1 - 1, iS, iS);
        } else {
            atb_add(jobs, p.HBARf, p.D1f, o->dS1, n1, iS, iR);
            atb_add(jobs, p.HBARf, p.Zf, o->dWW, n1, iS, iS);
        }
        atb_add(jobs, p.Zb, p.Tb, o->dS1, n1, iS, iR);
        atb_add(jobs, p.BBAR, p.D1b, o->dS2, n1, iS, iR);
        atb_add(jobs, p.Zb, p.BBAR, o->dWW, n1, iS, iS);
    } else {                                                         // dS1, dS2 and dWW are d0max_reduce_kernel's
        mg.dM = m.dM; mg.S1 = w->S1; mg.S2 = w->S2; mg.Rtab = f.Rtab; mg.wlist = m.wlist; mg.nwords = m.nwords; mg.dRt = f.dRt;
        mg.S = iS; mg.R = iR;
    }
    atb_add(jobs, p.DS, U, o->dCe, n0, iK, iR);                      // dC_embed += ds x u
    atb_add(jobs, p.DS, UW, o->dCw, n0, iK, iQ);                     // dC_wildcard += ds x uw
    atb_add(jobs, p.A, DP, f.dS1s, n1, iS, iR);                      // alpha x dp
    atb_add(jobs, p.Bk, DQ, f.dS2s, n1, iS, iR);                     // beta x dq
    atb_add(jobs, p.A, DPW, o->dS1w, n1, iS, iQ);                    // alpha x dpw
    atb_add(jobs, p.Bk, DQW, o->dS2w, n1, iS, iQ);                   // beta x dqw
    if (farnn) {
        atb_add(jobs, p.A, p.DAZf + S, o->dWss1, n1 - 1, iS, iS);
        atb_add(jobs, p.Bk, p.DAZb + S, o->dWss1, n1 - 1, iS, iS);
        atb_add(jobs, c->ones.p, p.DAZf, o->dbs1, n1, 1, iS);
        atb_add(jobs, c->ones.p, p.DAZb, o->dbs1, n1, 1, iS);
        if (farnn == 2) {
            atb_add(jobs, p.A, p.DARf + S, o->dWss2, n1 - 1, iS, iS);
            atb_add(jobs, p.Bk, p.DARb + S, o->dWss2, n1 - 1, iS, iS);
            atb_add(jobs, c->ones.p, p.DARf, o->dbs2, n1, 1, iS);
            atb_add(jobs, c->ones.p, p.DARb, o->dbs2, n1, 1, iS);
        }
    }
    if (jobs.total_wgs < 0) return fail(FARNN_ERANGE, "decomp_fst_train_step: too many gradient products for one launch%s%s");
    if ((rc = c->part.ensure(atb_partial_floats(jobs), "decomp_fst_train_step: out of device memory for the partial products%s%s"))) return rc;
    jobs.partial = c->part.p;
    return FARNN_OK;
}
// Stage 4 (prep): zero the workspace and the outputs, transpose, the column sums; Rtab, W, W^T; the gates' input halves; the buckets
int Decomp0Step::prepare() {
    int rc;
    FARNN_HIP_TRY(hipMemsetAsync(c->ws.p, 0, need0 * sizeof(float), s));
    if ((rc = clear_bucket_counts(bk, V, N0, s))) return rc;
    if (c->ones_filled < c->ones.n) {
        decomp0_fill_kernel<<<(unsigned)((c->ones.n + 255) / 256), 256, 0, s>>>(c->ones.p, c->ones.n, 1.0f);
        c->ones_filled = c->ones.n;
    }
    train_prep_kernel<<<(prep.total + 255) / 256, 256, 0, s>>>(prep);
    const size_t ne = std::max(V * R, S * S);
    decomp0_prep_kernel<<<(unsigned)((ne + 255) / 256), 256, 0, s>>>(w->Vgen, f.csum, f.Rtab, V * R, (int)R, w->S1w, w->S2w, f.cwsum, w->WW,
                                                                    f.Wm, f.WT, (int)S, (int)Q);
    if (farnn) {                                               // GV = Rtab Wrs (:259-262: the gates read _R, not V_vec)
        d0_gemm(s, f.Rtab, R, 1, w->Wrs1, S, 1, f.GV1, (int)V, (int)S, (int)R);
        if (farnn == 2) d0_gemm(s, f.Rtab, R, 1, w->Wrs2, S, 1, f.GV2, (int)V, (int)S, (int)R);
    }
    return launch_bucketing(p.x, p.len, B, L, (int)V, bk, c->err.dev, s);
}
// Stage 5: both chains with the state stash (the i-FST's kernels)
int Decomp0Step::forward() {
    return with_chain_form(*this, ldsw_f, ns_f, [&](auto LDSW, auto GATED, auto VPS, auto VPR, auto NS) {
        return launch(train_forward_kernel<LDSW(), GATED(), VPS(), VPR(), NS()>, dim3((B + NS() - 1) / NS(), 2), TR_THREADS, lds_f, s, p);
    });
}
// Stage 6: the score head, the loss (cross-entropy, or the CRF between the emissions and the adjoints), the decode
int Decomp0Step::loss() {
    int rc;
    if (!crf) {
        if ((rc = launch_loss<0>())) return rc;
        onehot_loss_sum_kernel<<<1, 64, 0, s>>>(loss_part, (int)grid0 * D0_WAVES, o->loss);
        return FARNN_OK;
    }
    if ((rc = launch_loss<1>()) || (rc = crfst.run(p.SC, grid0, o->dtrans, o->loss, s))) return rc;
    return launch_loss<2>();
}
// Stage 7: back-propagation through time, the i-FST's kernel in its DET form
int Decomp0Step::backward() {
    return with_chain_form(*this, ldsw_b, ns_b, [&](auto LDSW, auto GATED, auto VPS, auto VPR, auto NS) {
        return launch(train_backward_kernel<LDSW(), GATED(), VPS(), VPR(), NS(), true>, dim3((B + NS() - 1) / NS(), 2), TR_THREADS, lds_b, s, p);
    });
}
// Stage 5, max semiring: the distinct words' slots (the positions are bucketed by prepare()), their blocks Tr_w, both chains
int Decomp0Step::max_forward() {
    tmax_slots_kernel<<<1, 1024, 0, s>>>(bk.wcount, (int)V, m.wslot, m.wlist, m.nwords);
    const unsigned nt = (unsigned)((S + 31) / 32);
    tmax_premix_kernel<<<dim3((unsigned)nwmax, nt * nt), 256, 0, s>>>(f.Rtab, w->S1, w->S2, f.Wm, m.wlist, m.nwords, m.M, m.MT, (int)S, (int)R);
    return launch(tmax_forward_kernel, dim3(B, 2), TM_THREADS, lds_tok, s, p, m.mp);
}
// Stage 8, max semiring: dM per distinct word; dS1, dS2, dWW and the words' rows of dRtab from it, the chunks in order; then
// the sum step's reductions
int Decomp0Step::max_gradients() {
    int rc;
    if ((rc = launch(tmax_dM_kernel, (unsigned)nwmax, TM_THREADS, lds_m, s, p, m.mp, bk.list, bk.wstart, bk.wcount, m.dM))) return rc;
    if ((rc = launch(d0max_wgrad_kernel, dim3((unsigned)d0max_chunks(nwmax), (unsigned)((R + D0M_RB - 1) / D0M_RB)), D0_THREADS, lds_mw, s, mg))) return rc;
    const size_t ne = std::max(S * R, S * S);
    d0max_reduce_kernel<<<(unsigned)((ne + 255) / 256), 256, 0, s>>>(mg.PS1, mg.PS2, mg.PW, m.nwords, o->dS1, o->dS2, o->dWW, S * R, S * S);
    return gradients();
}
// Stage 8: the reductions, all in a fixed order
int Decomp0Step::gradients() {
    const int iV = (int)V, iS = (int)S, iR = (int)R, iQ = (int)Q;
    const D0WordSum ws = {bk.list, bk.wstart, bk.wcount, p.len, DVS, p.DVf, p.DVb, p.DAZf, p.DAZb, p.DARf, p.DARb,
                          f.dVs, f.dRt, f.dGV1, f.dGV2, L, iS, iR, farnn};
    if (mx) decomp0_word_sum_kernel<true><<<(unsigned)V, 256, 0, s>>>(ws);
    else decomp0_word_sum_kernel<false><<<(unsigned)V, 256, 0, s>>>(ws);
    if (farnn) {                                               // dRtab += dGV Wrs^T, dWrs = Rtab^T dGV
        d0_gemm(s, f.dGV1, S, 1, w->Wrs1, 1, S, f.dRg1, iV, iR, iS);
        d0_gemm(s, f.Rtab, 1, R, f.dGV1, S, 1, o->dWrs1, iR, iS, iV);
        if (farnn == 2) {
            d0_gemm(s, f.dGV2, S, 1, w->Wrs2, 1, S, f.dRg2, iV, iR, iS);
            d0_gemm(s, f.Rtab, 1, R, f.dGV2, S, 1, o->dWrs2, iR, iS, iV);
        }
    }
    atb_launch(jobs, s);
    d0_gemm(s, o->dWW, S, 1, w->S2w, Q, 1, f.X1, iS, iQ, iS);      // X1 = dW S2w
    d0_gemm(s, o->dWW, 1, S, w->S1w, Q, 1, f.X2, iS, iQ, iS);      // X2 = dW^T S1w
    const D0Fold fo = {f.dVs, farnn ? f.dRg1 : nullptr, farnn == 2 ? f.dRg2 : nullptr, f.csum, f.cwsum, f.dS1s, f.dS2s, f.X1, f.X2,
                       f.dRt, o->dVgen, o->dS1, o->dS2, o->dS1w, o->dS2w, V * R, S * R, S * Q, iR, iQ};
    const size_t ne = std::max(V * R, std::max(S * R, S * Q));
    decomp0_fold_kernel<<<(unsigned)((ne + 255) / 256), 256, 0, s>>>(fo);
    const D0SumAdj sa = {f.dRt, w->Vgen, w->S1w, f.X1, p.HP, o->dCe, o->dCw, o->dh0, o->dhT, iV, iR, iQ, iS, (int)K, B};
    decomp0_sum_adj_kernel<<<(unsigned)((R + Q + 2 * S + 255) / 256), 256, 0, s>>>(sa);
    return FARNN_OK;
}

extern "C" int farnn_decomp_fst_train_step(farnn_decomp_fst_train_ctx *c, const farnn_decomp_fst_train_weights *w, const int64_t *x,
                                           const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                           int64_t valid_tokens, const farnn_decomp_fst_train_outputs *o, void *stream) {
    TunScope tun_scope(c ? &c->tun : nullptr);
    return run_train_step<Decomp0Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}

// ---- training step of the onehot i-FST (FARNN_S_O_I_S; onehot_train.hip.h) -------------------------------
struct farnn_onehot_train_ctx : TrainCtxBase {
    farnn_onehot_train_dims d;
    int n_cu = 256;
    int semiring = FARNN_SEMIRING_SUM;  // farnn_onehot_train_set_semiring
    DevBuf<float> ws;             // per-batch float workspace: stashes, adjoints, MT, o, loss partials, dT partial tiles; the max
                                  // semiring's index and winning-entry stashes behind them (grown by the first max step)
    DevBuf<int> iws;              // per-batch int workspace: bucket counts / offsets, per-word tables, the sorted positions
};

extern "C" int farnn_onehot_train_create(const farnn_onehot_train_dims *d, int device, farnn_onehot_train_ctx **out) {
    if (!d || !out) return fail(FARNN_EINVAL, "onehot_train_create: null argument%s%s");
    *out = nullptr;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0) return fail(FARNN_EINVAL, "onehot_train_create: bad dimensions%s%s");
    if (d->nl < FARNN_NL_NONE || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "onehot_train_create: bad nonlinearity%s%s");
    if (d->S > OT_MAX_S) return fail(FARNN_ERANGE, "onehot_train_create: more than 128 states%s%s");
    // the loss kernel keeps output_mat or reads it through L2; its per-wavefront vectors must fit
    if (train_loss_lds(d->S, d->C).vec > 150 * 1024) return fail(FARNN_ERANGE, "onehot_train_create: too many score columns%s%s");
    if (int rc = train_ctx_create("onehot_train", d, device, out)) return rc;
    (*out)->n_cu = device_cus(device);
    return FARNN_OK;
}
extern "C" void farnn_onehot_train_destroy(farnn_onehot_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_onehot_train_set_profiling(farnn_onehot_train_ctx *c, int32_t enable) {
    return train_ctx_set_profiling("onehot_train", c, enable);
}
extern "C" int farnn_onehot_train_time(farnn_onehot_train_ctx *c, double *total_ms, int64_t *steps) {
    return train_ctx_time("onehot_train", c, total_ms, steps);
}

extern "C" int farnn_onehot_train_set_semiring(farnn_onehot_train_ctx *c, int32_t semiring) {
    if (!c) return fail(FARNN_EINVAL, "onehot_train_set_semiring: null context%s%s");
    if (semiring != FARNN_SEMIRING_SUM && semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "onehot_train_set_semiring: semiring must be FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX%s%s");
    c->semiring = semiring;
    return FARNN_OK;
}
// One step: the plan (sizes from the dimensions alone) and what the stages hand on
struct OhStep {
    static constexpr const char *name = "onehot_train", *label_range = "C";
    bool mx;                      // the max semiring (onehot_train_max.hip.h): its own chain, BPTT and dT stages
    int B, L;
    size_t S, K, V, N1, N0;
    unsigned lgrid;               // workgroups of the loss kernel
    size_t need, ineed;           // floats of ws, ints of iws: the totals of carve_ws / carve_bucket_ints
    size_t lds_tok, lds_mdt;      // LDS bytes of the chain kernels and of the max semiring's dT kernel
    farnn_onehot_train_ctx *c; const farnn_onehot_train_weights *w; const farnn_onehot_train_outputs *o; hipStream_t s;
    OhTrainParams q;
    OhMaxParams mq;
    TrainParams p;                // of the loss kernel
    float *DS, *AB, *M, *MT, *osum, *loss_part, *partial;
    Buckets bk;
    size_t carve_ws(float *base);
    int validate(); int plan(int B, int L);
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prepare(); int loss(); int max_chains(); int max_dT(); int stages();
    template <bool BPTT> int chains() { return launch_onehot_chains<BPTT>(q, lds_tok, s); }
    int max_bptt() { return launch(onehot_max_bptt_kernel, dim3(B, 2), OT_THREADS, 0, s, q, mq); }
    int dT() { return launch_onehot_dT(q, bk, o->dT, partial, s); }
};

size_t OhStep::carve_ws(float *base) {
    Carver<float> a(base);
    const size_t nS = N1 * S, SS = S * S;
    q.A = a.take(nS); q.Bk = a.take(nS); q.GA = a.take(nS); q.GB = a.take(nS); q.UF = a.take(nS); q.DQ = a.take(nS);
    DS = a.take(N0 * K); AB = a.take(N0 * S);
    M = a.take(V * SS); MT = a.take(V * SS);
    osum = a.take((S + 3) & ~(size_t)3);
    loss_part = a.take((size_t)lgrid * 8);
    partial = a.take((2 * ((N0 + OT_G - 1) / OT_G) + 1) * SS);      // partial tiles of the words with several runs
    if (mx) {
        // the max semiring, behind everything the sum step lays out: the winning entries, and the indices as bytes.  The
        // per-step dM entries take the rows the sum step's BPTT writes (UF, DQ), which the max step does not use.
        mq.WINf = a.take(nS); mq.WINb = a.take(nS);
        mq.IDXf = (uint8_t *)a.take((nS + 3) / 4); mq.IDXb = (uint8_t *)a.take((nS + 3) / 4);
        mq.GMf = q.UF; mq.GMb = q.DQ;
    }
    return a.off;
}
// Stage 1: the arguments
int OhStep::validate() {
    if (!w->T || !w->W || !w->O || !w->h0 || !w->hT) return fail(FARNN_EINVAL, "onehot_train_step: null weight%s%s");
    if (!o->loss || !o->dT || !o->tags) return fail(FARNN_EINVAL, "onehot_train_step: null output%s%s");
    return FARNN_OK;
}
// Stage 2: host arithmetic only; every size the step refuses is refused here, before anything is enqueued
int OhStep::plan(int B_, int L_) {
    // positions are 32-bit flat indices b L + i in the bucketing and dT kernels
    if ((unsigned long long)B_ * (L_ + 1) >= (1ull << 30)) return fail(FARNN_ERANGE, "onehot_train_step: B (L+1) must stay below 2^30%s%s");
    mx = c->semiring == FARNN_SEMIRING_MAX;
    B = B_; L = L_; S = c->d.S; K = c->d.C; V = c->d.V;
    N1 = (size_t)B * (L + 1); N0 = (size_t)B * L;
    // the loss kernel's persistent workgroups: three per compute unit (48 KiB of LDS each at ATIS size; one per unit left
    // the position loop latency-bound: 127 us)
    lgrid = (unsigned)std::min<size_t>(3 * (size_t)c->n_cu, (N0 + 7) / 8);
    lds_tok = (size_t)(L + 1) * sizeof(int); lds_mdt = onehot_max_dT_lds_bytes(S);
    need = carve_ws(nullptr); ineed = carve_bucket_ints(nullptr, bk, V, N0);
    if (int rc = lds_fits(lds_tok)) return rc;
    return mx ? lds_fits(lds_mdt) : FARNN_OK;
}
// Stage 3: grow the buffers, lay the workspaces out, fill the chain and the loss kernels' parameters (the loss kernel is the
// decomposed step's, PHASE 0, with output_mat in C_output_mat's place and the loss as per-wavefront partials)
int OhStep::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens) {
    if (int rc = grow_workspaces(name, c, need, ineed)) return rc;
    [[maybe_unused]] const size_t carved = carve_ws(c->ws.p), icarved = carve_bucket_ints(c->iws.p, bk, V, N0);
    assert(carved == need && icarved == ineed);     // the sizing pass and the carving pass agree
    q.M = M; q.MT = MT; q.o = osum; q.h0 = w->h0; q.hT = w->hT; q.x = x; q.len = lengths;
    q.B = B; q.L = L; q.V = (int)V; q.S = (int)S; q.nl = c->d.nl;
    p.C = w->O; p.P = w->P; p.len = q.len; p.labels = labels; p.err = c->err.dev;
    p.A = q.A; p.Bk = q.Bk; p.GA = q.GA; p.GB = q.GB; p.DS = DS; p.AB = AB;
    p.loss = o->loss; p.loss_part = loss_part; p.tags = o->tags;
    p.B = B; p.L = L; p.V = (int)V; p.S = (int)S; p.K = (int)K; p.nl = c->d.nl; p.o_idx = c->d.o_idx;
    p.threshold = c->d.threshold; p.inv_tokens = 1.0f / (float)valid_tokens;
    return FARNN_OK;
}
// Stages 4 and 5: o = output_mat.sum(0), M_w = T[w] + W and its transpose, the positions bucketed by word.  Every workspace
// entry a kernel reads is written by an earlier kernel of this step (the chains write the stash rows 0..len, the loss kernel
// the adjoint rows of every valid position): only the bucket counts are zeroed
int OhStep::prepare() {
    if (int rc = clear_bucket_counts(bk, V, N0, s)) return rc;
    PrepJobs pj = {};
    prep_add(pj, 2, w->O, osum, K, S);              // o = output_mat.sum(0)
    train_prep_kernel<<<(pj.total + 255) / 256, 256, 0, s>>>(pj);
    const unsigned nt = (unsigned)((S + 31) / 32);
    onehot_premix_kernel<<<(unsigned)V * nt * nt, 256, 0, s>>>(w->T, w->W, M, MT, (int)S);
    return launch_bucketing(q.x, q.len, B, L, (int)V, bk, c->err.dev, s);
}
// Stage 6, max semiring: both chains with the state, arg-max index and winning-entry stash (the sum kernel's register slots by S)
int OhStep::max_chains() {
    return with_chain_slots(S, [&](auto RS) { return launch(onehot_max_chain_kernel<RS()>, dim3(B, 2), OT_THREADS, lds_tok, s, q, mq); });
}
// Stage 7: scores, cross-entropy, decode, d loss / d alpha, d loss / d beta
int OhStep::loss() {
    if (int rc = launch_train_loss<0>(p, lgrid, s)) return rc;
    launch_loss_sum(loss_part, lgrid, o->loss, s);
    return FARNN_OK;
}
// Stage 9, max semiring: the per-step dM entries added per word in bucket order, the sum step's runs and its reduction
int OhStep::max_dT() {
    const unsigned ngrid = (unsigned)(V + (N0 + OT_G - 1) / OT_G);
    if (int rc = launch(onehot_max_dT_kernel, ngrid, 256, lds_mdt, s, q, mq, bk.list, bk.wstart, bk.wcount, bk.itoff, bk.psoff,
                        o->dT, partial)) return rc;
    onehot_dT_reduce_kernel<<<dim3((unsigned)V, (unsigned)((S * S + 255) / 256)), 256, 0, s>>>(bk.itoff, bk.psoff, partial, o->dT, (int)S);
    return FARNN_OK;
}
// Stages 4 to 9 (6 and 8: both chains, with the state stash, then back-propagation through time; 9: d loss / d language_tensor)
int OhStep::stages() {
    int rc;
    if ((rc = prepare()) || (rc = mx ? max_chains() : chains<false>()) || (rc = loss())) return rc;
    return (rc = mx ? max_bptt() : chains<true>()) ? rc : mx ? max_dT() : dT();
}

extern "C" int farnn_onehot_ifst_train_step(farnn_onehot_train_ctx *c, const farnn_onehot_train_weights *w, const int64_t *x,
                                            const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                            int64_t valid_tokens, const farnn_onehot_train_outputs *o, void *stream) {
    return run_train_step<OhStep>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}

// ---- training step of the onehot FST (FARNN_S_O; fst4_train.hip.h) ----------------------------------------
struct farnn_fst4_train_ctx : TrainCtxBase {
    farnn_fst4_train_dims d;
    int semiring = FARNN_SEMIRING_SUM;  // farnn_fst4_train_set_semiring
    DevBuf<float> ws;             // per-batch float workspace: stashes, adjoints, scores, M / MT / dM, the partials
    DevBuf<int> iws;              // per-batch int workspace: the bucketing of the positions by word
};

extern "C" int farnn_fst4_train_create(const farnn_fst4_train_dims *d, int device, farnn_fst4_train_ctx **out) {
    if (!d || !out) return fail(FARNN_EINVAL, "fst4_train_create: null argument%s%s");
    *out = nullptr;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0) return fail(FARNN_EINVAL, "fst4_train_create: bad dimensions%s%s");
    if (d->S > OT_MAX_S) return fail(FARNN_ERANGE, "fst4_train_create: more than 128 states%s%s");
    // fst4_loss_kernel keeps two score vectors per wavefront in LDS (fst4_loss_lds_bytes): C <= 2400
    if (fst4_loss_lds_bytes(d->C) > 150 * 1024) return fail(FARNN_ERANGE, "fst4_train_create: too many score columns%s%s");
    // byte offsets into [V][C][S][S] stay inside 63 bits
    if ((unsigned long long)d->V * (unsigned long long)d->C > (1ull << 47))
        return fail(FARNN_ERANGE, "fst4_train_create: V C S S is not addressable%s%s");
    return train_ctx_create("fst4_train", d, device, out);
}
extern "C" void farnn_fst4_train_destroy(farnn_fst4_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_fst4_train_set_profiling(farnn_fst4_train_ctx *c, int32_t enable) {
    return train_ctx_set_profiling("fst4_train", c, enable);
}
extern "C" int farnn_fst4_train_time(farnn_fst4_train_ctx *c, double *total_ms, int64_t *steps) {
    return train_ctx_time("fst4_train", c, total_ms, steps);
}
extern "C" int farnn_fst4_train_set_semiring(farnn_fst4_train_ctx *c, int32_t semiring) {
    return bucketed_set_semiring("fst4_train", c, semiring);
}

// One step (BucketedStep, train_bucketed.hip.h); the groups of its score kernels divide the label columns
struct Fst4Step : BucketedStep<farnn_fst4_train_ctx, farnn_fst4_train_weights, farnn_fst4_train_outputs, Fst4TrainParams> {
    static constexpr const char *name = "fst4_train", *label_range = "C";
    float *Wsum;
    size_t carve_ws(float *base);
    int validate(); int plan(int B, int L);
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prepare(); int wildcard(); int stages();
    template <int MODE> int scores();
};

size_t Fst4Step::carve_ws(float *base) {
    Carver<float> a(base);
    const size_t SS = S * S;
    carve_head(a);
    SC = a.take(N0 * K); DS = a.take(N0 * K);
    M = a.take(V * SS); MT = a.take(V * SS); dM = a.take(V * SS);
    Wsum = a.take((SS + 3) & ~(size_t)3);
    carve_tail(a);
    carve_max(a);
    return a.off;
}
// Stage 1: the arguments
int Fst4Step::validate() {
    if (!w->T4 || !w->W4 || !w->h0 || !w->hT) return fail(FARNN_EINVAL, "fst4_train_step: null weight%s%s");
    if (!o->loss || !o->dT4 || !o->tags) return fail(FARNN_EINVAL, "fst4_train_step: null output%s%s");
    return FARNN_OK;
}
int Fst4Step::plan(int B_, int L_) {
    if (int rc = plan_bucketed(name, B_, L_, c->d.C, fst4_train_lds_floats)) return rc;
    need = carve_ws(nullptr);
    return FARNN_OK;
}
// Stage 3: grow the buffers, lay the workspaces out, fill the kernels' parameters
int Fst4Step::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels_, int64_t valid_tokens) {
    if (int rc = grow_workspaces(name, c, need, ineed)) return rc;
    [[maybe_unused]] const size_t carved = carve_ws(c->ws.p);
    assert(carved == need);     // the sizing pass and the carving pass agree
    // the chains always use relu and have no output mask (model_onehot.py:93-94, :100-101)
    carve_bucketed(x, lengths, labels_, valid_tokens, FARNN_NL_RELU);
    f.T4 = w->T4; f.W4 = w->W4; f.A = q.A; f.Bk = q.Bk; f.len = lengths;
    f.list = bk.list; f.wstart = bk.wstart; f.wcount = bk.wcount;
    f.SC = SC; f.DS = DS; f.part = part; f.dM = dM; f.dT4 = o->dT4;
    f.L = L; f.S = (int)S; f.C = (int)K; f.cpg = cpg; f.ngrp = ngrp;
    return FARNN_OK;
}
// Stages 4 and 5: the positions bucketed by word; W4.sum(0); M[w] = T4[w].sum(0) + W4.sum(0) and its transpose for the words of
// the batch only (the bucket counts say which: the blocks of the other words are never read)
int Fst4Step::prepare() {
    int rc;
    if ((rc = clear_bucket_counts(bk, V, N0, s)) || (rc = bucket_and_fill())) return rc;
    const unsigned nt = (unsigned)((S + 31) / 32);
    fst4_premix_kernel<<<dim3(1, nt * nt), 256, 0, s>>>(w->W4, nullptr, nullptr, Wsum, nullptr, (int)S, (int)K);
    fst4_premix_kernel<<<dim3((unsigned)V, nt * nt), 256, 0, s>>>(w->T4, Wsum, bk.wcount, M, MT, (int)S, (int)K);
    return FARNN_OK;
}
// Stages 7, 9 and 12: the score kernels in bucket order (MODE 0: the scores, 1: the partials of d alpha / d beta, 2: dT4);
// register rows per thread by S
template <int MODE>
int Fst4Step::scores() {
    return with_rows_per_thread(S, f.GW, [&](auto RPT) {
        return launch(fst4_train_kernel<RPT(), MODE>, dim3((unsigned)V, ngrp), F4_THREADS, lds_sc, s, f);
    });
}
// Stage 13 (asked for): d loss / d wildcard_tensor
int Fst4Step::wildcard() {
    if (!o->dW4) return FARNN_OK;
    const size_t CSS = K * S * S;
    fst4_dW_kernel<<<(unsigned)((CSS + 255) / 256), 256, 0, s>>>(o->dT4, bk.wcount, o->dW4, (int)V, CSS);
    return FARNN_OK;
}
// Stages 4 to 13 (6 and 10: both chains, with the state stash, then back-propagation through time)
int Fst4Step::stages() {
    int rc;
    if ((rc = prepare()) || (rc = chains<false>()) || (rc = scores<0>()) || (rc = loss_on_scores()) ||
        (rc = adjoints([&] { return scores<1>(); })) || (rc = chains<true>()) || (rc = dM_words()) || (rc = scores<2>())) return rc;
    return wildcard();
}

extern "C" int farnn_fst4_train_step(farnn_fst4_train_ctx *c, const farnn_fst4_train_weights *w, const int64_t *x,
                                     const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                     int64_t valid_tokens, const farnn_fst4_train_outputs *o, void *stream) {
    return run_train_step<Fst4Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}

// ---- training step of the onehot independent=1 model (FARNN_S_O_I; ind1_train.hip.h) ----------------------
struct farnn_ind1_train_ctx : TrainCtxBase {
    farnn_ind1_train_dims d;
    int semiring = FARNN_SEMIRING_SUM;  // farnn_ind1_train_set_semiring
    DevBuf<float> ws;             // per-batch float workspace: stashes, adjoints, scores, Mc / McT / dMc, the partials
    DevBuf<int> iws;              // per-batch int workspace: the bucketing of the positions by word
};

extern "C" int farnn_ind1_train_create(const farnn_ind1_train_dims *d, int device, farnn_ind1_train_ctx **out) {
    if (!d || !out) return fail(FARNN_EINVAL, "ind1_train_create: null argument%s%s");
    *out = nullptr;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0) return fail(FARNN_EINVAL, "ind1_train_create: bad dimensions%s%s");
    if (d->S > OT_MAX_S) return fail(FARNN_ERANGE, "ind1_train_create: more than 128 states%s%s");
    // fst4_loss_kernel keeps two score vectors per wavefront in LDS (fst4_loss_lds_bytes): C <= 2400
    if (fst4_loss_lds_bytes(d->C) > 150 * 1024) return fail(FARNN_ERANGE, "ind1_train_create: too many score columns%s%s");
    return train_ctx_create("ind1_train", d, device, out);
}
extern "C" void farnn_ind1_train_destroy(farnn_ind1_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_ind1_train_set_profiling(farnn_ind1_train_ctx *c, int32_t enable) {
    return train_ctx_set_profiling("ind1_train", c, enable);
}
extern "C" int farnn_ind1_train_time(farnn_ind1_train_ctx *c, double *total_ms, int64_t *steps) {
    return train_ctx_time("ind1_train", c, total_ms, steps);
}
extern "C" int farnn_ind1_train_set_semiring(farnn_ind1_train_ctx *c, int32_t semiring) {
    return bucketed_set_semiring("ind1_train", c, semiring);
}

// One step (BucketedStep); the groups of its score kernel's MODE 0 and 1 divide the label columns
struct Ind1Step : BucketedStep<farnn_ind1_train_ctx, farnn_ind1_train_weights, farnn_ind1_train_outputs, Ind1TrainParams> {
    static constexpr const char *name = "ind1_train", *label_range = "C";
    float *Osum;
    size_t carve_ws(float *base);
    int validate(); int plan(int B, int L);
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int prepare(); int stages();
    template <int MODE> int scores();
};

size_t Ind1Step::carve_ws(float *base) {
    Carver<float> a(base);
    const size_t SS = S * S;
    carve_head(a);
    SC = a.take(N0 * K); DS = a.take(N0 * K);
    M = a.take(V * SS); MT = a.take(V * SS); dM = a.take(V * SS);
    Osum = a.take((SS + 3) & ~(size_t)3);
    carve_tail(a);
    carve_max(a);
    return a.off;
}
// Stage 1: the arguments
int Ind1Step::validate() {
    if (!w->T || !w->W || !w->O || !w->h0 || !w->hT) return fail(FARNN_EINVAL, "ind1_train_step: null weight%s%s");
    if (!o->loss || !o->dT || !o->tags) return fail(FARNN_EINVAL, "ind1_train_step: null output%s%s");
    return FARNN_OK;
}
int Ind1Step::plan(int B_, int L_) {
    if (int rc = plan_bucketed(name, B_, L_, c->d.C, ind1_train_lds_floats)) return rc;
    need = carve_ws(nullptr);
    return FARNN_OK;
}
// Stage 3: grow the buffers, lay the workspaces out, fill the kernels' parameters
int Ind1Step::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels_, int64_t valid_tokens) {
    if (int rc = grow_workspaces(name, c, need, ineed)) return rc;
    [[maybe_unused]] const size_t carved = carve_ws(c->ws.p);
    assert(carved == need);     // the sizing pass and the carving pass agree
    // the chains always use relu (model_onehot.py:266, :278); the output mask is premixed into Mc
    carve_bucketed(x, lengths, labels_, valid_tokens, FARNN_NL_RELU);
    f.T = w->T; f.W = w->W; f.O = w->O; f.A = q.A; f.Bk = q.Bk; f.len = lengths;
    f.list = bk.list; f.wstart = bk.wstart; f.wcount = bk.wcount;
    f.SC = SC; f.DS = DS; f.part = part; f.dMc = dM; f.Osum = Osum; f.dT = o->dT;
    f.L = L; f.S = (int)S; f.C = (int)K; f.cpg = cpg; f.ngrp = ngrp; f.mask = c->d.mask_by_output != 0;
    return FARNN_OK;
}
// Stages 4 and 5: the positions bucketed by word; with the mask Osum = output_tensor.sum(0); Mc[w] = (T[w] + W) (* Osum) and its
// transpose for the words of the batch only (the bucket counts say which: the blocks of the other words are never read)
int Ind1Step::prepare() {
    int rc;
    if ((rc = clear_bucket_counts(bk, V, N0, s)) || (rc = bucket_and_fill())) return rc;
    const unsigned nt = (unsigned)((S + 31) / 32);
    if (f.mask) fst4_premix_kernel<<<dim3(1, nt * nt), 256, 0, s>>>(w->O, nullptr, nullptr, Osum, nullptr, (int)S, (int)K);
    ind1_premix_kernel<<<dim3((unsigned)V, nt * nt), 256, 0, s>>>(w->T, w->W, f.mask ? Osum : nullptr, bk.wcount, M, MT, (int)S);
    return FARNN_OK;
}
// Stages 7, 9 and 12: the score kernel in bucket order (MODE 0: the scores, 1: the partials of d alpha / d beta, 2: dT, all the
// labels of a word in one workgroup); register rows per thread by S
template <int MODE>
int Ind1Step::scores() {
    return with_rows_per_thread(S, f.GW, [&](auto RPT) {
        return launch(ind1_train_kernel<RPT(), MODE>, dim3((unsigned)V, MODE == 2 ? 1 : ngrp), I1_THREADS, lds_sc, s, f);
    });
}
// Stages 4 to 12 (6 and 10: both chains, with the state stash, then back-propagation through time)
int Ind1Step::stages() {
    int rc;
    if ((rc = prepare()) || (rc = chains<false>()) || (rc = scores<0>()) || (rc = loss_on_scores()) ||
        (rc = adjoints([&] { return scores<1>(); })) || (rc = chains<true>()) || (rc = dM_words())) return rc;
    return scores<2>();
}

extern "C" int farnn_ind1_train_step(farnn_ind1_train_ctx *c, const farnn_ind1_train_weights *w, const int64_t *x,
                                     const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                     int64_t valid_tokens, const farnn_ind1_train_outputs *o, void *stream) {
    return run_train_step<Ind1Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}

// ---- training step of the decomposed independent=1 model (FARNN_S_D_W_I; decomp1_train.hip.h) --------------
struct farnn_decomp_ind1_train_ctx : TrainCtxBase {
    farnn_decomp_ind1_train_dims d;
    int semiring = FARNN_SEMIRING_SUM;  // farnn_decomp_ind1_train_set_semiring
    DevBuf<float> ws;             // per-batch float workspace: stashes, adjoints, br / scores, N / Mc / McT / dMc / dN, the factor
                                  // products Kfac / Ofac / E, the partials
    DevBuf<int> iws;              // per-batch int workspace: the bucketing of the positions by word
};

extern "C" int farnn_decomp_ind1_train_create(const farnn_decomp_ind1_train_dims *d, int device, farnn_decomp_ind1_train_ctx **out) {
    if (!d || !out) return fail(FARNN_EINVAL, "decomp_ind1_train_create: null argument%s%s");
    *out = nullptr;
    if (d->V <= 0 || d->S <= 0 || d->R <= 0 || d->RO <= 0 || d->C <= 0) return fail(FARNN_EINVAL, "decomp_ind1_train_create: bad dimensions%s%s");
    if (d->nl < FARNN_NL_NONE || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "decomp_ind1_train_create: bad nonlinearity%s%s");
    if (d->S > OT_MAX_S) return fail(FARNN_ERANGE, "decomp_ind1_train_create: more than 128 states%s%s");
    // fst4_loss_kernel keeps two score vectors per wavefront in LDS (fst4_loss_lds_bytes): C <= 2400
    if (fst4_loss_lds_bytes(d->C) > 150 * 1024) return fail(FARNN_ERANGE, "decomp_ind1_train_create: too many score columns%s%s");
    // element offsets into Kfac [R][S][S] and Ofac [R_O][S][S] are computed in 32 bits by the kernels that fill them
    if ((unsigned long long)d->R * d->S * d->S >= (1ull << 31))
        return fail(FARNN_ERANGE, "decomp_ind1_train_create: rank R too large (R S S must stay below 2^31)%s%s");
    if ((unsigned long long)d->RO * d->S * d->S >= (1ull << 31))
        return fail(FARNN_ERANGE, "decomp_ind1_train_create: output rank R_O too large (R_O S S must stay below 2^31)%s%s");
    return train_ctx_create("decomp_ind1_train", d, device, out);
}
extern "C" void farnn_decomp_ind1_train_destroy(farnn_decomp_ind1_train_ctx *c) { train_ctx_destroy(c); }
extern "C" int farnn_decomp_ind1_train_set_profiling(farnn_decomp_ind1_train_ctx *c, int32_t enable) {
    return train_ctx_set_profiling("decomp_ind1_train", c, enable);
}
extern "C" int farnn_decomp_ind1_train_time(farnn_decomp_ind1_train_ctx *c, double *total_ms, int64_t *steps) {
    return train_ctx_time("decomp_ind1_train", c, total_ms, steps);
}
extern "C" int farnn_decomp_ind1_train_set_semiring(farnn_decomp_ind1_train_ctx *c, int32_t semiring) {
    return bucketed_set_semiring("decomp_ind1_train", c, semiring);
}

// One step (BucketedStep); the groups of its score kernel's MODE 0 and 1 divide the output ranks
struct Decomp1Step : BucketedStep<farnn_decomp_ind1_train_ctx, farnn_decomp_ind1_train_weights, farnn_decomp_ind1_train_outputs,
                                  Ind1TrainParams> {
    static constexpr const char *name = "decomp_ind1_train", *label_range = "C";
    size_t R, RO;
    D1BackParams bp;
    // farnn_decomp_ind1_crf_train_step: the CRF stage in loss_on_scores' place (train_bucketed_crf.hip.h)
    bool crf;
    const float *crf_trans; float *dtrans;
    BucketedCrf cs;
    // farnn_decomp_ind1_gated_train_step: the gated chains, their back-propagation and the gates' gradients in the plain stages'
    // place (decomp1_gated_train.hip.h); null for every other entry
    const farnn_decomp_ind1_gate_weights *gw; const farnn_decomp_ind1_gate_outputs *go;
    // farnn_decomp_ind1_gated_max_train_step: the same on a max context, the chains and their back-propagation those of
    // decomp1_gated_max_train.hip.h, dM_words the plain max step's
    bool gmx;
    D1GateParams gp;
    size_t lds_gate;
    float *GV1, *GV2, *dGV1, *dGV2, *GT1, *GT2;
    float *BR, *DBR, *Nw, *dN, *Kfac, *Ofac, *E, *Osum, *dOsum, *zero, *csum, *dcsum, *fpart, *HP;
    size_t carve_ws(float *base);
    void carve_gates(Carver<float> &a);
    int gated_chains(); int gated_bptt(); int gated_dM_words(); int gate_gradients();
    int gated_max_chains(); int gated_max_bptt();
    int validate(); int plan(int B, int L);
    int carve(const int64_t *x, const int64_t *lengths, const int64_t *labels, int64_t valid_tokens);
    int gemm(const float *A, size_t am, size_t ak, const float *Bm, size_t bk_, size_t bn, float *Cm, size_t ldc, size_t M_, size_t N_,
             size_t K_, const float *add = nullptr, const int *rows = nullptr);
    int prepare(); int loss(); int back(); int factors(); int stages();
    template <int MODE> int scores();
};

size_t Decomp1Step::carve_ws(float *base) {
    Carver<float> a(base);
    const size_t SS = S * S, SS4 = (SS + 3) & ~(size_t)3, RO4 = (RO + 3) & ~(size_t)3;
    carve_head(a);
    BR = a.take(N0 * RO); DS = a.take(N0 * K);             // (neighbours: cleared by one memset)
    DBR = a.take(N0 * RO); SC = a.take(N0 * K);
    Nw = a.take(V * SS); M = a.take(V * SS); MT = a.take(V * SS); dM = a.take(V * SS); dN = a.take(V * SS);
    Kfac = a.take(R * SS); E = a.take(R * SS); Ofac = a.take(RO * SS);
    Osum = a.take(SS4); dOsum = a.take(SS4); zero = a.take(SS4);
    csum = a.take(RO4); dcsum = a.take(RO4);
    carve_tail(a);
    fpart = a.take(V * RO * 2 * S);                             // the words' shares of dS1_output / dS2_output
    HP = a.take((size_t)B * 2 * S);                               // the sequences' shares of dh0 / dhT
    if (!gw) carve_max(a);
    if (crf) cs.carve(a, B, L, K, w->P != nullptr);               // (behind everything the plain step lays out)
    if (gw) carve_gates(a);                                       // (and so is the gated step's)
    if (gw) carve_max(a);                                         // (the gated max step's WIN / IDX: behind all of the above)
    return a.off;
}
// the gated step's own arrays: the chains' stash of z, r, y and hbar, the gates' pre-activation adjoints, the input halves
// GV = Vgen Wrs + bs and their adjoints per word, the gates' share of dVgen
void Decomp1Step::carve_gates(Carver<float> &a) {
    const size_t nS2 = 2 * N1 * S, two = gw->farnn == 2;
    gp.Z = a.take(nS2); gp.Y = a.take(nS2); gp.DAZ = a.take(nS2);
    gp.Rg = a.take(two * nS2); gp.HB = a.take(two * nS2); gp.DAR = a.take(two * nS2);
    GV1 = a.take(V * S); dGV1 = a.take(V * S); GT1 = a.take(V * R);
    GV2 = a.take(two * V * S); dGV2 = a.take(two * V * S); GT2 = a.take(two * V * R);
}
// Stage 1: the arguments
int Decomp1Step::validate() {
    if (!w->Vgen || !w->S1 || !w->S2 || !w->W || !w->C || !w->S1o || !w->S2o || !w->h0 || !w->hT)
        return fail(FARNN_EINVAL, "decomp_ind1_train_step: null weight%s%s");
    if (!o->loss || !o->dVgen || !o->dS1 || !o->dS2 || !o->tags) return fail(FARNN_EINVAL, "decomp_ind1_train_step: null output%s%s");
    return FARNN_OK;
}
int Decomp1Step::plan(int B_, int L_) {
    R = c->d.R; RO = c->d.RO;
    if (int rc = plan_bucketed(name, B_, L_, RO, ind1_train_lds_floats)) return rc;
    if (crf)
        if (int rc = BucketedCrf::plan_check(name, K, L)) return rc;
    if (gw) {
        const char *entry = gmx ? "decomp_ind1_gated_max_train_step" : "decomp_ind1_gated_train_step";
        if (gw->farnn != 1 && gw->farnn != 2) return fail(FARNN_EINVAL, "%s: farnn must be 1 or 2%s", entry);
        if (!gw->Wss1 || !gw->Wrs1 || !gw->bs1 || !go->dWss1 || !go->dWrs1 || !go->dbs1 ||
            (gw->farnn == 2 && (!gw->Wss2 || !gw->Wrs2 || !gw->bs2 || !go->dWss2 || !go->dWrs2 || !go->dbs2)))
            return fail(FARNN_EINVAL, "%s: a gate weight or gate gradient of this farnn is null%s", entry);
        if (!(gw->sigmoid_exponent > 0.0f)) return fail(FARNN_EINVAL, "%s: sigmoid_exponent must be positive%s", entry);
        if (mx && !gmx) return fail(FARNN_EINVAL, "decomp_ind1_gated_train_step: the context is in the max semiring; the gated chains are built for the sum semiring only%s%s");
        if (!mx && gmx) return fail(FARNN_EINVAL, "decomp_ind1_gated_max_train_step: the context is in the sum semiring; this entry runs the gated chains of the max semiring only%s%s");
        lds_gate = decomp1_gated_lds_bytes(S, gw->farnn, L);
        if (lds_gate + D1G_STATIC_LDS > 160 * 1024)
            return fail(FARNN_ERANGE, "%s: the gate matrices (farnn S S floats) and a sequence's L + 1 tokens need more than 160 KiB of LDS%s", entry);
    }
    need = carve_ws(nullptr);
    return FARNN_OK;
}
// Stage 3: grow the buffers, lay the workspaces out, fill the kernels' parameters
int Decomp1Step::carve(const int64_t *x, const int64_t *lengths, const int64_t *labels_, int64_t valid_tokens) {
    if (int rc = grow_workspaces(name, c, need, ineed)) return rc;
    [[maybe_unused]] const size_t carved = carve_ws(c->ws.p);
    assert(carved == need);     // the sizing pass and the carving pass agree
    // the chains use args.update_nonlinear (model_decompose_independent.py:181-188); the output mask is premixed into Mc
    carve_bucketed(x, lengths, labels_, valid_tokens, c->d.nl);
    // the score kernel in factor space: N (wildcard_mat already in it) in T's place beside a zero W, Ofac in O's, br in the scores'
    f.T = Nw; f.W = zero; f.O = Ofac; f.A = q.A; f.Bk = q.Bk; f.len = lengths;
    f.list = bk.list; f.wstart = bk.wstart; f.wcount = bk.wcount;
    f.SC = BR; f.DS = DBR; f.part = part; f.dMc = dM; f.Osum = Osum; f.dT = dN;
    f.L = L; f.S = (int)S; f.C = (int)RO; f.cpg = cpg; f.ngrp = ngrp; f.mask = 1;
    bp.N = Nw; bp.Ofac = Ofac; bp.S1o = w->S1o; bp.S2o = w->S2o; bp.A = q.A; bp.Bk = q.Bk; bp.len = lengths;
    bp.list = bk.list; bp.wstart = bk.wstart; bp.wcount = bk.wcount; bp.DBR = DBR; bp.dMc = dM; bp.Osum = Osum;
    bp.dN = dN; bp.fpart = fpart; bp.L = L; bp.S = (int)S; bp.SP = f.SP; bp.RO = (int)RO; bp.CPR = f.CPR; bp.GW = f.GW;
    // max semiring: UF / DQ hold dM entries, not adjoint rows -- BPTT itself carries on into row 0 (onehot_max_bptt_carry_kernel)
    if (mx && (o->dh0 || o->dhT)) carry0 = HP;
    if (crf) cs.fill(crf_trans, w->P, SC, DS, lengths, labels_, o->tags, c->err.dev, B, L, K, c->d.o_idx, c->d.threshold);
    if (gw) {
        gp.Wss1 = gw->Wss1; gp.Wss2 = gw->Wss2; gp.GV1 = GV1; gp.GV2 = GV2; gp.HP = HP;
        gp.farnn = gw->farnn; gp.k = gw->sigmoid_exponent;
    }
    return FARNN_OK;
}
// C[m][n] = sum_k A[m am + k ak] B[k bk + n bn] (+ add[n]); rows: the rows read as zero (decomp1_gemm_kernel)
int Decomp1Step::gemm(const float *A, size_t am, size_t ak, const float *Bm, size_t bk_, size_t bn, float *Cm, size_t ldc, size_t M_,
                      size_t N_, size_t K_, const float *add, const int *rows) {
    D1Gemm g = {A, Bm, add, rows, Cm, (int)M_, (int)N_, (int)K_, am, ak, bk_, bn, ldc};
    return launch(decomp1_gemm_kernel, dim3((unsigned)((M_ + D1_TM - 1) / D1_TM), (unsigned)((N_ + D1_TM - 1) / D1_TM)), 256, 0, s, g);
}
// Stages 4 and 5: the positions bucketed by word; the factor products Kfac and Ofac; Osum; N[w] = Vgen[w] Kfac + wildcard_mat
// for the words of the batch (the bucket counts say which), Mc[w] = N[w] * Osum and its transpose.  br and d score are cleared:
// their rows at pad positions enter the products over the positions (dC_output) as zeros
int Decomp1Step::prepare() {
    int rc;
    if ((rc = clear_bucket_counts(bk, V, N0, s))) return rc;
    FARNN_HIP_TRY(hipMemsetAsync(BR, 0, N0 * (RO + K) * sizeof(float), s));
    FARNN_HIP_TRY(hipMemsetAsync(zero, 0, S * S * sizeof(float), s));
    if ((rc = bucket_and_fill())) return rc;
    const size_t SS = S * S;
    decomp1_outer_kernel<<<(unsigned)((R * SS + 255) / 256), 256, 0, s>>>(w->S1, w->S2, Kfac, (int)S, (int)R);
    decomp1_outer_kernel<<<(unsigned)((RO * SS + 255) / 256), 256, 0, s>>>(w->S1o, w->S2o, Ofac, (int)S, (int)RO);
    decomp1_csum_kernel<<<(unsigned)((RO + 255) / 256), 256, 0, s>>>(w->C, csum, (int)K, (int)RO);
    decomp1_osum_kernel<<<(unsigned)((SS + 255) / 256), 256, 0, s>>>(csum, Ofac, Osum, (int)SS, (int)RO);
    if ((rc = gemm(w->Vgen, R, 1, Kfac, SS, 1, Nw, SS, V, SS, R, w->W, bk.wcount))) return rc;
    const unsigned nt = (unsigned)((S + 31) / 32);
    ind1_premix_kernel<<<dim3((unsigned)V, nt * nt), 256, 0, s>>>(Nw, zero, Osum, bk.wcount, M, MT, (int)S);
    if (!gw) return FARNN_OK;
    // the gated step: the gates' input halves GV = Vgen Wrs + bs for the batch's words; the gates' adjoint rows cleared (row 0
    // and the pad rows stay zero: the products over every row read them)
    const size_t nS2 = 2 * N1 * S;
    FARNN_HIP_TRY(hipMemsetAsync(gp.DAZ, 0, nS2 * sizeof(float), s));
    if (gw->farnn == 2) FARNN_HIP_TRY(hipMemsetAsync(gp.DAR, 0, nS2 * sizeof(float), s));
    if ((rc = gemm(w->Vgen, R, 1, gw->Wrs1, S, 1, GV1, S, V, S, R, gw->bs1, bk.wcount))) return rc;
    if (gw->farnn == 2 && (rc = gemm(w->Vgen, R, 1, gw->Wrs2, S, 1, GV2, S, V, S, R, gw->bs2, bk.wcount))) return rc;
    return FARNN_OK;
}
// Stages 6 and 10 of the gated step: decomp1_gated_chain_kernel / decomp1_gated_bptt_kernel in launch_onehot_chains' place
int Decomp1Step::gated_chains() {
    return with_chain_slots(S, [&](auto RS) { return launch(decomp1_gated_chain_kernel<RS()>, dim3(B, 2), OT_THREADS, lds_gate, s, q, gp); });
}
int Decomp1Step::gated_bptt() {
    return with_chain_slots(S, [&](auto RS) { return launch(decomp1_gated_bptt_kernel<RS()>, dim3(B, 2), OT_THREADS, lds_gate, s, q, gp); });
}
// The same two stages on a max context: the index and winning-entry stash beside the gated stash, back-propagation to the
// winning index only (it writes the steps' dMc entries for dM_words and HP itself)
int Decomp1Step::gated_max_chains() {
    return with_chain_slots(S, [&](auto RS) { return launch(decomp1_gated_max_chain_kernel<RS()>, dim3(B, 2), OT_THREADS, lds_gate, s, q, gp, mq); });
}
int Decomp1Step::gated_max_bptt() {
    return launch(decomp1_gated_max_bptt_kernel, dim3(B, 2), OT_THREADS, lds_gate, s, q, gp, mq);
}
// Stage 11 of the gated step: dMc[w] with hbar as the row factor (farnn 2: its stash in the state stash's place; farnn 1: hbar
// is the state) and back-propagation's u in UF / DQ as the column factor
int Decomp1Step::gated_dM_words() {
    OhTrainParams qd = q;
    if (gw->farnn == 2) { qd.A = gp.HB; qd.Bk = gp.HB + N1 * S; }
    return launch_onehot_dT(qd, bk, dM, partial, s);
}
// The gates stage, behind factors(): the words' dGV in bucket order, dWrs = Vgen^T dGV, dbs = sum_w dGV[w], dVgen += dGV Wrs^T,
// dWss = H^T DAZ over every row of both chains' state stash (A and Bk are neighbours; DAZ shifted by one row)
int Decomp1Step::gate_gradients() {
    int rc;
    const size_t nS = N1 * S;
    const bool two = gw->farnn == 2;
    assert(q.Bk == q.A + nS);
    decomp1_gate_word_kernel<<<dim3((unsigned)V, two ? 2 : 1), 128, 0, s>>>(gp.DAZ, gp.DAR, q.len, bk.list, bk.wstart, bk.wcount, dGV1,
                                                                             dGV2, L, (int)S, nS);
    decomp1_gate_bias_kernel<<<two ? 2 : 1, 128, 0, s>>>(dGV1, dGV2, go->dbs1, go->dbs2, (int)V, (int)S);
    if ((rc = gemm(w->Vgen, 1, R, dGV1, S, 1, go->dWrs1, S, R, S, V)) ||
        (rc = gemm(dGV1, S, 1, gw->Wrs1, 1, S, GT1, R, V, R, S)) ||
        (rc = gemm(q.A, 1, S, gp.DAZ + S, S, 1, go->dWss1, S, S, S, 2 * N1 - 1))) return rc;
    if (two && ((rc = gemm(w->Vgen, 1, R, dGV2, S, 1, go->dWrs2, S, R, S, V)) ||
                (rc = gemm(dGV2, S, 1, gw->Wrs2, 1, S, GT2, R, V, R, S)) ||
                (rc = gemm(q.A, 1, S, gp.DAR + S, S, 1, go->dWss2, S, S, S, 2 * N1 - 1)))) return rc;
    decomp1_gate_add_kernel<<<(unsigned)((V * R + 255) / 256), 256, 0, s>>>(o->dVgen, GT1, two ? GT2 : nullptr, V * R);
    return FARNN_OK;
}
// Stages 7 and 9: ind1_train_kernel in bucket order over the output ranks (MODE 0: br, 1: the partials of d alpha / d beta)
template <int MODE>
int Decomp1Step::scores() {
    return with_rows_per_thread(S, f.GW, [&](auto RPT) {
        return launch(ind1_train_kernel<RPT(), MODE>, dim3((unsigned)V, ngrp), I1_THREADS, lds_sc, s, f);
    });
}
// Stage 8: score = br C_output^T (:206); the loss on the scores (CRF: the negative log-likelihood of the emissions, a sum over
// the sequences, :293); d br = d score C_output
int Decomp1Step::loss() {
    int rc;
    if ((rc = gemm(BR, RO, 1, w->C, 1, RO, SC, K, N0, K, RO)) ||
        (rc = crf ? cs.run(SC, lgrid, dtrans, o->loss, s) : loss_on_scores())) return rc;
    return gemm(DS, K, 1, w->C, RO, 1, DBR, RO, N0, RO, K);
}
// Stage 12: dN[w] and the words' shares of dS1_output / dS2_output, one workgroup per word over all output ranks
int Decomp1Step::back() {
    return with_rows_per_thread(S, f.GW, [&](auto RPT) { return launch(decomp1_back_kernel<RPT()>, (unsigned)V, I1_THREADS, lds_sc, s, bp); });
}
// Stage 13: the dense adjoints contracted onto the factors, every sum over the words in id order and over the sequences in order
int Decomp1Step::factors() {
    int rc;
    const size_t SS = S * S;
    decomp1_word_sum_kernel<<<(unsigned)((SS + 255) / 256), 256, 0, s>>>(dN, dM, Nw, bk.wcount, o->dW, dOsum, (int)V, SS);
    decomp1_out_factors_kernel<<<(unsigned)RO, 128, 0, s>>>(fpart, bk.wcount, dOsum, w->S1o, w->S2o, csum, o->dS1o, o->dS2o, dcsum,
                                                           (int)V, (int)S, (int)RO);
    // dC_output[c,r] = sum_pos d score[pos,c] br[pos,r] (positions in order) + dcsum[r] (every row: csum = C_output.sum(0))
    if (o->dC && (rc = gemm(DS, 1, K, BR, RO, 1, o->dC, RO, K, RO, N0, dcsum))) return rc;
    if ((rc = gemm(dN, SS, 1, Kfac, 1, SS, o->dVgen, R, V, R, SS, nullptr, bk.wcount)) ||      // dv_r = sum_ij dN[w]_ij S1[i,r] S2[j,r]
        (rc = gemm(w->Vgen, 1, R, dN, SS, 1, E, SS, R, SS, V))) return rc;                     // E[r] = sum_w v_r[w] dN[w]
    decomp1_in_factors_kernel<<<(unsigned)R, 128, 0, s>>>(E, w->S1, w->S2, o->dS1, o->dS2, (int)S, (int)R);
    if (o->dh0 || o->dhT) {
        if (!mx && !gw) decomp1_init_adj_kernel<<<(unsigned)B, 128, 0, s>>>(q, HP);      // (the gated BPTT wrote HP itself)
        decomp1_init_sum_kernel<<<1, 128, 0, s>>>(HP, o->dh0, o->dhT, B, (int)S);
    }
    return FARNN_OK;
}
// Stages 4 to 13 (6 and 10: both chains, with the state stash, then back-propagation through time)
int Decomp1Step::stages() {
    int rc;
    if (gw) {
        if ((rc = prepare()) || (rc = mx ? gated_max_chains() : gated_chains()) || (rc = scores<0>()) || (rc = loss()) ||
            (rc = adjoints([&] { return scores<1>(); })) || (rc = mx ? gated_max_bptt() : gated_bptt()) ||
            (rc = mx ? dM_words() : gated_dM_words()) || (rc = back()) || (rc = factors())) return rc;
        return gate_gradients();
    }
    if ((rc = prepare()) || (rc = chains<false>()) || (rc = scores<0>()) || (rc = loss()) ||
        (rc = adjoints([&] { return scores<1>(); })) || (rc = chains<true>()) || (rc = dM_words()) || (rc = back())) return rc;
    return factors();
}

extern "C" int farnn_decomp_ind1_train_step(farnn_decomp_ind1_train_ctx *c, const farnn_decomp_ind1_train_weights *w, const int64_t *x,
                                            const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                            int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *o, void *stream) {
    return run_train_step<Decomp1Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream);
}
extern "C" int farnn_decomp_ind1_crf_train_step(farnn_decomp_ind1_train_ctx *c, const farnn_decomp_ind1_train_weights *w,
                                                const float *crf_trans, const int64_t *x, const int64_t *lengths,
                                                const int64_t *labels, int32_t B, int32_t L, int64_t valid_tokens,
                                                const farnn_decomp_ind1_train_outputs *o, float *dtrans, void *stream) {
    if (!crf_trans || !dtrans) return fail(FARNN_EINVAL, "decomp_ind1_train_crf_step: CRF transitions / their gradient missing%s%s");
    return run_train_step<Decomp1Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream,
                                       [&](Decomp1Step &t) { t.crf = true; t.crf_trans = crf_trans; t.dtrans = dtrans; });
}
extern "C" int farnn_decomp_ind1_gated_train_step(farnn_decomp_ind1_train_ctx *c, const farnn_decomp_ind1_train_weights *w,
                                                  const farnn_decomp_ind1_gate_weights *g, const float *crf_trans, const int64_t *x,
                                                  const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                                  int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *o,
                                                  const farnn_decomp_ind1_gate_outputs *go, float *dtrans, void *stream) {
    if (!g || !go) return fail(FARNN_EINVAL, "decomp_ind1_gated_train_step: null gate weights / gate outputs%s%s");
    if ((crf_trans == nullptr) != (dtrans == nullptr))
        return fail(FARNN_EINVAL, "decomp_ind1_gated_train_step: CRF transitions and their gradient go together (both or neither)%s%s");
    return run_train_step<Decomp1Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream, [&](Decomp1Step &t) {
        t.gw = g; t.go = go;
        if (crf_trans) { t.crf = true; t.crf_trans = crf_trans; t.dtrans = dtrans; }
    });
}
extern "C" int farnn_decomp_ind1_gated_max_train_step(farnn_decomp_ind1_train_ctx *c, const farnn_decomp_ind1_train_weights *w,
                                                      const farnn_decomp_ind1_gate_weights *g, const float *crf_trans, const int64_t *x,
                                                      const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                                      int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *o,
                                                      const farnn_decomp_ind1_gate_outputs *go, float *dtrans, void *stream) {
    if (!g || !go) return fail(FARNN_EINVAL, "decomp_ind1_gated_max_train_step: null gate weights / gate outputs%s%s");
    if ((crf_trans == nullptr) != (dtrans == nullptr))
        return fail(FARNN_EINVAL, "decomp_ind1_gated_max_train_step: CRF transitions and their gradient go together (both or neither)%s%s");
    return run_train_step<Decomp1Step>(c, w, x, lengths, labels, B, L, valid_tokens, o, stream, [&](Decomp1Step &t) {
        t.gw = g; t.go = go; t.gmx = true;
        if (crf_trans) { t.crf = true; t.crf_trans = crf_trans; t.dtrans = dtrans; }
    });
}

// ---- the optimizer step (farnn_optim_*; optim.hip.h) -------------------------------------------------------------------
struct farnn_optim {
    farnn_optim_desc d;
    int device = 0;
    std::vector<int64_t> numel, steps;        // per tensor: elements; the steps in which it had a gradient
    struct Launch { int t0, nt; size_t c0; unsigned nchunks; };   // tensors t0 .. t0 + nt - 1, their chunks in the table
    std::vector<Launch> launches;
    DevBuf<OptChunk> chunks;                  // the chunk table, written once by create
};

static int optim_check_desc(const farnn_optim_desc *d) {
    if (d->kind != FARNN_OPTIM_SGD && d->kind != FARNN_OPTIM_ADAM) return fail(FARNN_EINVAL, "optim_create: kind must be FARNN_OPTIM_SGD or FARNN_OPTIM_ADAM%s%s");
    if (!(d->lr >= 0.0) || d->lr > 3.0e38) return fail(FARNN_EINVAL, "optim_create: lr must be a finite number >= 0%s%s");
    if (d->kind == FARNN_OPTIM_ADAM && (!(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) ||
                                        !(d->eps >= 0.0) || d->eps > 3.0e38))
        return fail(FARNN_EINVAL, "optim_create: betas must lie in [0, 1) and eps must be a finite number >= 0%s%s");
    return FARNN_OK;
}

extern "C" int farnn_optim_create(const farnn_optim_desc *desc, const int64_t *numel, int32_t n, int device, farnn_optim **out) {
    if (!desc || !numel || !out) return fail(FARNN_EINVAL, "optim_create: null argument%s%s");
    *out = nullptr;
    int rc;
    if ((rc = optim_check_desc(desc))) return rc;
    if (n <= 0) return fail(FARNN_EINVAL, "optim_create: no tensors%s%s");
    for (int i = 0; i < n; i++)
        if (numel[i] <= 0) return fail(FARNN_EINVAL, "optim_create: every numel must be positive%s%s");
    // the chunk table: OPT_MAX_TENSORS tensors per launch, one workgroup per chunk
    std::vector<OptChunk> table;
    std::vector<farnn_optim::Launch> launches;
    for (int t0 = 0; t0 < n; t0 += OPT_MAX_TENSORS) {
        farnn_optim::Launch l = {t0, std::min<int>(OPT_MAX_TENSORS, n - t0), table.size(), 0u};
        size_t nchunks = 0;
        for (int t = 0; t < l.nt; t++) nchunks += (size_t)((numel[t0 + t] + OPT_CHUNK - 1) / OPT_CHUNK);
        if (nchunks > (size_t)0x7fffffff) return fail(FARNN_ERANGE, "optim_create: more than 2^31 chunks in one launch%s%s");
        for (int t = 0; t < l.nt; t++)
            for (int64_t off = 0; off < numel[t0 + t]; off += OPT_CHUNK)
                table.push_back({t, (int32_t)std::min<int64_t>(OPT_CHUNK, numel[t0 + t] - off), off});
        l.nchunks = (unsigned)nchunks;
        launches.push_back(l);
    }
    if ((rc = select_device(device))) return rc;
    farnn_optim *o = new farnn_optim();
    o->d = *desc; o->device = device;
    o->numel.assign(numel, numel + n); o->steps.assign(n, 0);
    o->launches = launches;
    if ((rc = o->chunks.ensure(table.size(), "optim_create: out of device memory for the chunk table%s%s"))) { delete o; return rc; }
    if (hipMemcpy(o->chunks.p, table.data(), table.size() * sizeof(OptChunk), hipMemcpyHostToDevice) != hipSuccess) {
        delete o;
        return fail(FARNN_EIO, "optim_create: copying the chunk table to the device failed%s%s");
    }
    *out = o;
    return FARNN_OK;
}

extern "C" void farnn_optim_destroy(farnn_optim *o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    delete o;
}

extern "C" int farnn_optim_set_lr(farnn_optim *o, double lr) {
    if (!o) return fail(FARNN_EINVAL, "optim_set_lr: null handle%s%s");
    if (!(lr >= 0.0) || lr > 3.0e38) return fail(FARNN_EINVAL, "optim_set_lr: lr must be a finite number >= 0%s%s");
    o->d.lr = lr;
    return FARNN_OK;
}

extern "C" int farnn_optim_steps(const farnn_optim *o, int32_t i, int64_t *out) {
    if (!o || !out) return fail(FARNN_EINVAL, "optim_steps: null argument%s%s");
    if (i < 0 || (size_t)i >= o->steps.size()) return fail(FARNN_EINVAL, "optim_steps: tensor index out of range%s%s");
    *out = o->steps[i];
    return FARNN_OK;
}

extern "C" int farnn_optim_set_steps(farnn_optim *o, int32_t i, int64_t steps) {
    if (!o) return fail(FARNN_EINVAL, "optim_set_steps: null handle%s%s");
    if (i < 0 || (size_t)i >= o->steps.size()) return fail(FARNN_EINVAL, "optim_set_steps: tensor index out of range%s%s");
    if (steps < 0) return fail(FARNN_EINVAL, "optim_set_steps: a step count cannot be negative%s%s");
    o->steps[i] = steps;
    return FARNN_OK;
}

extern "C" int farnn_optim_step(farnn_optim *o, float *const *params, const float *const *grads, float *const *exp_avg,
                                float *const *exp_avg_sq, void *stream) {
    if (!o || !params || !grads) return fail(FARNN_EINVAL, "optim_step: null argument%s%s");
    const bool adam = o->d.kind == FARNN_OPTIM_ADAM;
    if (adam && (!exp_avg || !exp_avg_sq)) return fail(FARNN_EINVAL, "optim_step: Adam needs exp_avg and exp_avg_sq%s%s");
    const int n = (int)o->numel.size();
    // everything is checked before anything is enqueued or counted
    for (int i = 0; i < n; i++) {
        if (!grads[i]) continue;
        if (!params[i]) return fail(FARNN_EINVAL, "optim_step: a tensor with a gradient has no parameter pointer%s%s");
        if (adam && (!exp_avg[i] || !exp_avg_sq[i])) return fail(FARNN_EINVAL, "optim_step: a tensor with a gradient has no exp_avg / exp_avg_sq (Adam)%s%s");
    }
    FARNN_HIP_TRY(hipSetDevice(o->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (const farnn_optim::Launch &l : o->launches) {
        OptArgs a = {};
        bool any = false;
        for (int t = 0; t < l.nt; t++) {
            const int i = l.t0 + t;
            if (!grads[i]) continue;          // a.g[t] stays null: the kernel leaves the tensor's chunks alone
            any = true;
            a.p[t] = params[i]; a.g[t] = grads[i];
            if (adam) {
                const double step = (double)++o->steps[i];
                a.m[t] = exp_avg[i]; a.v[t] = exp_avg_sq[i];
                a.step_size[t] = (float)(o->d.lr / (1.0 - pow(o->d.beta1, step)));
                a.bc2_sqrt[t] = (float)sqrt(1.0 - pow(o->d.beta2, step));
            } else {
                ++o->steps[i];
                a.step_size[t] = (float)o->d.lr;
            }
        }
        if (!any) continue;
        a.w1 = (float)(1.0 - o->d.beta1); a.beta2 = (float)o->d.beta2; a.w2 = (float)(1.0 - o->d.beta2); a.eps = (float)o->d.eps;
        if (adam) optim_step_kernel<true><<<l.nchunks, OPT_THREADS, 0, s>>>(o->chunks.p + l.c0, a);
        else optim_step_kernel<false><<<l.nchunks, OPT_THREADS, 0, s>>>(o->chunks.p + l.c0, a);
    }
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}
