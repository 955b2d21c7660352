// The CRF loss stage of a step over bucketed per-word blocks (BucketedStep, train_bucketed.hip.h): what stands in
// loss_on_scores' place under --use_crf 1 (reference model_decompose_independent.py:277-298, baselines/crf.py:48-99, 202-260).
//   bucketed_crf_emit_kernel      emissions = scores . P                         (:277-278; fst4_loss_kernel's first half)
//   bucketed_crf_kernel<BIG>      one workgroup per sequence, train_crf_kernel's method: log Z - gold into the sequence's
//                                 own loss slot, d loss / d emissions = marginals - gold one-hot, expected - gold transition
//                                 counts into the sequence's slice, the Viterbi path with column K-3 clamped (:293, :298)
//   bucketed_crf_adjoint_kernel   d scores = d emissions . P^T, in place             (fst4_loss_kernel's last part)
// and the launches every such step makes behind them: crf_reduce_kernel (the slices in sequence order) and
// onehot_loss_sum_kernel (the sequences' losses in index order).  Without a priority matrix the scores are the emissions and
// d emissions is d scores: only the CRF kernel and the two sums run.
// No float atomics: two steps on the same inputs are bit-identical.
#pragma once
#include "train_host.hip.h"
#include "fst4_train.hip.h"

namespace farnn {

struct BucketedCrfParams {          // (the names TrainParams gives the same things)
    const float *trans;             // [K][K] transitions
    const float *SC;                // [B L][K] emissions
    float *DS;                      // [B L][K] d loss / d emissions (valid positions; the pads are the caller's)
    float *dtrans_part;             // [B][K][K]
    const int64_t *len, *labels;
    int32_t *tags;
    int *err;
    float *loss;                    // [B] log Z - gold per sequence
    int K, L, o_idx;
    float threshold;
};

// One workgroup per sequence: train_crf_kernel's method (train.hip.h, whose comments record what each choice cost to find) on
// this stage's parameters -- scaled exp-domain messages, four independent chains per LDS dot product, the expected counts in
// registers when a thread owns at most 32 rows (K <= 84), BIG for the tag sets whose three tables do not fit LDS -- with the
// loss in the sequence's own slot instead of an atomic, and an empty sequence's slot and tags written here.  A kernel of its
// own and not a function shared with train_crf_kernel: sharing the body moved that kernel's register allocation.
// LDS (train_crf_lds_bytes): tr, etr, ex [K][K+1]; al[L][K] log-messages; ea[L][K] = exp(al - amax_t); am[L]; bt[2][K]; eb[K];
//      red[8]; vit[2][K]; fl[L][K] emissions; bp[L][K] bytes
template <bool BIG>
__global__ void __launch_bounds__(256)
bucketed_crf_kernel(const BucketedCrfParams p) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x;
    const int K = p.K, K1 = K + 1, START = K - 2, STOP = K - 1;
    const int n = clamp_len(p.len[b], p.L);
    const int TS = BIG ? K : K1;                                               // row stride of tr / ex
    float *etr = smem, *lds_tr = etr + K * K1, *lds_ex = lds_tr + (BIG ? 0 : K * K1);
    float *al = lds_ex + (BIG ? 0 : K * K1), *ea = al + (long long)p.L * K;
    float *am = ea + (long long)p.L * K, *bt = am + p.L, *eb = bt + 2 * K, *red = eb + K, *vit = red + 8;
    float *fl = vit + 2 * K;                                                   // [L][K] this sequence's emissions (!BIG)
    unsigned char *bp = (unsigned char *)(fl + (BIG ? 0 : (long long)p.L * K));
    float *dpart = p.dtrans_part + (long long)b * K * K;
    const float *tr;
    float *ex;
    if constexpr (BIG) { tr = p.trans; ex = dpart; } else { tr = lds_tr; ex = lds_ex; }
    for (int e = tid; e < K * K; e += nt) {
        const int o = (e / K) * K1 + e % K;
        const float t = p.trans[e];
        etr[o] = __expf(t);
        if constexpr (BIG) { dpart[e] = 0.0f; } else { lds_tr[o] = t; lds_ex[o] = 0.0f; }
    }
    __syncthreads();
    if (n == 0) {                                                              // nothing to the loss, to dtrans or to DS
        if constexpr (!BIG)
            for (int e = tid; e < K * K; e += nt) dpart[e] = 0.0f;
        if (tid == 0) p.loss[b] = 0.0f;
        for (int t = tid; t < p.L; t += nt) p.tags[(long long)b * p.L + t] = -1;
        return;
    }
    const float *F;
    if constexpr (BIG) {
        F = p.SC + (long long)b * p.L * K;
    } else {
        const float *Fg = p.SC + (long long)b * p.L * K;
        for (int e = tid; e < n * K; e += nt) fl[e] = Fg[e];
        F = fl;
    }
    __syncthreads();
    const int64_t *y = p.labels + (long long)b * p.L;
    // forward messages and the Viterbi recursion on the clamped emissions (association as in crf.py:123, :145)
    // red[4..7]: per-wavefront maxima of the newest forward (later backward) message
    const int wv = tid >> 6, lane_ = tid & 63;
    {
        float vmax = -INFINITY;
        for (int j = tid; j < K; j += nt) {
            const float f0 = F[j], a0 = f0 + tr[START * TS + j];
            al[j] = a0;
            vit[j] = (j == K - 3 ? fminf(f0, p.threshold) : f0) + tr[START * TS + j];
            vmax = fmaxf(vmax, a0);
        }
        for (int o = 32; o; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, WAVE));
        if (lane_ == 0) red[4 + wv] = vmax;
    }
    __syncthreads();
    for (int t = 0; t < n; t++) {
        // scale of step t: amax_t (from the wavefront maxima) and ea_t = exp(al_t - amax_t)
        const float *at = al + (long long)t * K;
        const float mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        for (int j = tid; j < K; j += nt) ea[(long long)t * K + j] = __expf(at[j] - mx);
        if (tid == 0) am[t] = mx;
        __syncthreads();
        if (t + 1 < n) {
            // threads 0..127 do the sum recursion, 128..255 the max recursion (Viterbi); four independent chains per loop
            const float *et = ea + (long long)t * K, *vp = vit + (t & 1) * K;
            const int half = tid >> 7, lt = tid & 127;
            float vmax = -INFINITY;
            if (half == 0) {
                for (int j = lt; j < K; j += 128) {
                    float s4[4] = {0.f, 0.f, 0.f, 0.f};
                    int i = 0;
#pragma unroll 4
                    for (; i + 4 <= K; i += 4) {
#pragma unroll
                        for (int u = 0; u < 4; u++) s4[u] = fmaf(et[i + u], etr[(i + u) * K1 + j], s4[u]);
                    }
                    for (; i < K; i++) s4[0] = fmaf(et[i], etr[i * K1 + j], s4[0]);
                    const float an = mx + __logf((s4[0] + s4[1]) + (s4[2] + s4[3])) + F[(long long)(t + 1) * K + j];
                    al[(long long)(t + 1) * K + j] = an;
                    vmax = fmaxf(vmax, an);
                }
            } else {
                for (int j = lt; j < K; j += 128) {
                    const float ft = F[(long long)(t + 1) * K + j], fc = j == K - 3 ? fminf(ft, p.threshold) : ft;
                    float b4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    int i4[4] = {0, 0, 0, 0};
                    int i = 0;
#pragma unroll 4
                    for (; i + 4 <= K; i += 4) {
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const float cand = (fc + tr[(i + u) * TS + j]) + vp[i + u];
                            if (cand > b4[u]) { b4[u] = cand; i4[u] = i + u; }
                        }
                    }
                    for (; i < K; i++) {
                        const float cand = (fc + tr[i * TS + j]) + vp[i];
                        if (cand > b4[0]) { b4[0] = cand; i4[0] = i; }
                    }
                    float bv = b4[0];
                    int bi = i4[0];
#pragma unroll
                    for (int u = 1; u < 4; u++)                              // first maximum over i, like torch.max (crf.py:148)
                        if (b4[u] > bv || (b4[u] == bv && i4[u] < bi)) { bv = b4[u]; bi = i4[u]; }
                    vit[((t + 1) & 1) * K + j] = bv;
                    bp[(long long)(t + 1) * K + j] = (unsigned char)bi;
                }
            }
            for (int o = 32; o; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, WAVE));
            if (lane_ == 0) red[4 + wv] = vmax;                               // -inf from the Viterbi wavefronts
            __syncthreads();
        }
    }
    // log Z, the gold score and the Viterbi backtrace (one thread: n steps)
    if (tid == 0) {
        const float *et = ea + (long long)(n - 1) * K, *vp = vit + ((n - 1) & 1) * K;
        float se = 0.0f;
        for (int i = 0; i < K; i++) se = fmaf(et[i], etr[i * K1 + STOP], se);
        const float logZ = am[n - 1] + logf(se);
        int prev = START;
        float gold = 0.0f;
        for (int t = 0; t < n; t++) {
            int yt = (int)y[t];
            if (y[t] < 0 || y[t] >= K) { yt = 0; atomicOr(p.err, 1); }         // same clamp as the marginals below
            gold += F[(long long)t * K + yt] + tr[prev * TS + yt];
            ex[prev * TS + yt] -= 1.0f;                                         // gold transition counts
            prev = yt;
        }
        gold += tr[prev * TS + STOP];
        ex[prev * TS + STOP] -= 1.0f;
        red[0] = logZ;
        p.loss[b] = logZ - gold;                                                // the sequence's own slot: no atomic
        float bv = -INFINITY; int ptr = 0;
        for (int i = 0; i < K; i++) { const float c = vp[i] + tr[i * TS + STOP]; if (c > bv) { bv = c; ptr = i; } }
        for (int t = n - 1; t >= 0; t--) {
            p.tags[(long long)b * p.L + t] = ptr == K - 3 ? p.o_idx : ptr;
            if (t > 0) ptr = bp[(long long)t * K + ptr];
        }
    }
    for (int t = n + tid; t < p.L; t += nt) p.tags[(long long)b * p.L + t] = -1;
    {
        float vmax = -INFINITY;
        for (int i = tid; i < K; i += nt) {
            const float bv = tr[i * TS + STOP];
            bt[((n - 1) & 1) * K + i] = bv;                                      // backward message at the last token
            vmax = fmaxf(vmax, F[(long long)(n - 1) * K + i] + bv);
        }
        for (int o = 32; o; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, WAVE));
        __syncthreads();                                                         // the forward loop's last reads of red[4..7]
        if (lane_ == 0) red[4 + wv] = vmax;
    }
    __syncthreads();
    const float logZ = red[0];
    // expected transition counts: thread (row group r0, column cj) owns rows r0, r0 + rstep, ... of column cj.  When that
    // is at most CRF_XR rows, its counts and its exp(transition) entries live in registers for the whole backward pass
    constexpr int CRF_XR = 32;
    const int xcj = tid % K1, xr0 = tid / K1, xrstep = nt / K1 > 0 ? nt / K1 : 1;
    const bool xreg = K1 <= nt && (K + xrstep - 1) / xrstep <= CRF_XR;
    const bool xmine = xreg && xcj < K && xr0 < xrstep;
    float exr[CRF_XR], etrr[CRF_XR];
#pragma unroll
    for (int u = 0; u < CRF_XR; u++) {
        const int i = xr0 + u * xrstep;
        exr[u] = 0.0f;
        etrr[u] = (xmine && i < K) ? etr[i * K1 + xcj] : 0.0f;
    }
    // backward messages, marginals and expected transition counts
    for (int t = n - 1; t >= 0; t--) {
        const float *bc = bt + (t & 1) * K;
        float *bn = bt + ((t + 1) & 1) * K;                                     // becomes beta_{t-1}
        const float *at = al + (long long)t * K;
        // scale of the backward side at step t: bmax over f_t + beta_t, eb = exp(f_t + beta_t - bmax)
        const float bmx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        for (int j = tid; j < K; j += nt) {
            eb[j] = __expf(F[(long long)t * K + j] + bc[j] - bmx);
            const float m = __expf(at[j] + bc[j] - logZ);
            int yt = (int)y[t];
            yt = yt < 0 || yt >= K ? 0 : yt;
            p.DS[((long long)b * p.L + t) * K + j] = m - (j == yt ? 1.0f : 0.0f);
            if (t == 0) ex[START * TS + j] += m;
            if (t == n - 1) ex[j * TS + STOP] += m;
        }
        __syncthreads();                                                        // eb ready; START row / STOP column settled
        if (t > 0) {
            const float *ep = ea + (long long)(t - 1) * K;
            const float scale = __expf(am[t - 1] + bmx - logZ);                 // xi_{t-1}(i,j) = ea[i] etr[i][j] eb[j] scale
            if (xreg) {
                if (xmine) {
                    const float se = scale * eb[xcj];
#pragma unroll
                    for (int u = 0; u < CRF_XR; u++) {
                        const int i = xr0 + u * xrstep;
                        exr[u] = fmaf(ep[i < K ? i : 0] * se, etrr[u], exr[u]);          // etrr is 0 past the last row
                    }
                }
            } else if (K1 <= nt) {
                const int cj = tid % K1, r0 = tid / K1, rstep = nt / K1;        // K1 columns per row in LDS (the pad column is skipped)
                if (cj < K && r0 < rstep) {
                    const float ebj = eb[cj];
#pragma unroll 4
                    for (int i = r0; i < K; i += rstep)
                        ex[i * TS + cj] = fmaf(ep[i] * scale, etr[i * K1 + cj] * ebj, ex[i * TS + cj]);
                }
            } else {
                for (int e = tid; e < K * K; e += nt) {
                    const int i = e / K, j = e - i * K;
                    ex[i * TS + j] = fmaf(ep[i] * scale, etr[i * K1 + j] * eb[j], ex[i * TS + j]);
                }
            }
            float vmax = -INFINITY;
            for (int i = tid; i < K; i += nt) {                                 // beta_{t-1}[i] = bmax + log sum_j etr[i][j] eb[j]
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                int j = 0;
#pragma unroll 4
                for (; j + 4 <= K; j += 4) {
                    s0 = fmaf(etr[i * K1 + j], eb[j], s0); s1 = fmaf(etr[i * K1 + j + 1], eb[j + 1], s1);
                    s2 = fmaf(etr[i * K1 + j + 2], eb[j + 2], s2); s3 = fmaf(etr[i * K1 + j + 3], eb[j + 3], s3);
                }
                for (; j < K; j++) s0 = fmaf(etr[i * K1 + j], eb[j], s0);
                const float se = (s0 + s1) + (s2 + s3);
                const float bnew = bmx + __logf(se);
                bn[i] = bnew;
                vmax = fmaxf(vmax, F[(long long)(t - 1) * K + i] + bnew);
            }
            for (int o = 32; o; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, WAVE));
            if (lane_ == 0) red[4 + wv] = vmax;                                   // read after the barrier below
        }
        __syncthreads();
    }
    if (xmine) {
#pragma unroll
        for (int u = 0; u < CRF_XR; u++) {
            const int i = xr0 + u * xrstep;
            if (i < K) ex[i * TS + xcj] += exr[u];                              // each element has exactly one owner
        }
    }
    __syncthreads();
    for (int e = tid; e < K * K; e += nt) dpart[e] = ex[(e / K) * TS + e % K];
}

// EM[pos] = SC[pos] . P at the valid positions (:277-278), a wavefront per position, k ascending as fst4_loss_kernel.
// LDS: 8 wavefronts, sc[K] each
__global__ void __launch_bounds__(512)
bucketed_crf_emit_kernel(const float *__restrict__ SC, const float *__restrict__ P, const int64_t *__restrict__ len,
                         float *__restrict__ EM, int B, int L, int K) {
    extern __shared__ __align__(16) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    float *sc = sm + (size_t)w * K;
    for (long long pos = (long long)blockIdx.x * nw + w; pos < (long long)B * L; pos += (long long)gridDim.x * nw) {
        const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
        if (i >= clamp_len(len[b], L)) continue;
        for (int c = lane; c < K; c += WAVE) sc[c] = SC[pos * K + c];
        for (int d = lane; d < K; d += WAVE) {
            float a = 0.0f;
            for (int c = 0; c < K; c++) a = fmaf(sc[c], P[(long long)c * K + d], a);
            EM[pos * K + d] = a;
        }
    }
}

// DS[pos][c] = sum_d DS[pos][d] P[c][d] at the valid positions, in place: the wavefront that owns the row stages it first
__global__ void __launch_bounds__(512)
bucketed_crf_adjoint_kernel(float *DS, const float *__restrict__ P, const int64_t *__restrict__ len, int B, int L, int K) {
    extern __shared__ __align__(16) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    float *ds = sm + (size_t)w * K;
    for (long long pos = (long long)blockIdx.x * nw + w; pos < (long long)B * L; pos += (long long)gridDim.x * nw) {
        const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
        if (i >= clamp_len(len[b], L)) continue;
        for (int d = lane; d < K; d += WAVE) ds[d] = DS[pos * K + d];
        for (int c = lane; c < K; c += WAVE) {
            float a = 0.0f;
            for (int d = 0; d < K; d++) a = fmaf(ds[d], P[(long long)c * K + d], a);
            DS[pos * K + c] = a;
        }
    }
}

// The host side: what a step plans, carves and launches for the stage
struct BucketedCrf {
    BucketedCrfParams p;
    const float *P;                 // the priority matrix or null
    float *EM, *loss_seq;           // [B L][K] emissions (with P only), [B]
    bool big;
    size_t lds;
    int B;

    // every size the stage refuses, before anything is enqueued
    static int plan_check(const char *name, size_t K, size_t L) {
        if (K < 4) return fail(FARNN_EINVAL, "%s_crf_step: the CRF needs at least 4 score columns (2 labels, START, STOP)%s", name);
        if (train_crf_lds_bytes(K, L, true) > 160 * 1024)
            return fail(FARNN_ERANGE, "%s_crf_step: CRF tag set too large for this sequence length (C(C+1)*4 + 9*L*C + ... bytes of LDS must fit 160 KiB)%s", name);
        return FARNN_OK;
    }
    // behind everything else of the step's float workspace
    void carve(Carver<float> &a, size_t B_, size_t L, size_t K, bool priority) {
        EM = priority ? a.take(B_ * L * K) : nullptr;
        p.dtrans_part = a.take(B_ * K * K);
        loss_seq = a.take(B_);
    }
    // SC: the scores before the priority layer; DS: where d loss / d SC goes (zero at the pads before the call)
    void fill(const float *trans, const float *P_, const float *SC, float *DS, const int64_t *len, const int64_t *labels,
              int32_t *tags, int *err, int B_, int L, size_t K, int o_idx, float threshold) {
        P = P_; B = B_;
        p.trans = trans; p.SC = P ? EM : SC; p.DS = DS; p.len = len; p.labels = labels; p.tags = tags; p.err = err;
        p.loss = loss_seq; p.K = (int)K; p.L = L; p.o_idx = o_idx; p.threshold = threshold;
        big = train_crf_lds_bytes(K, L, false) > 160 * 1024;
        lds = train_crf_lds_bytes(K, L, big);
    }
    int run(const float *SC, unsigned lgrid, float *dtrans, float *loss, hipStream_t s) {
        int rc;
        const size_t lds_row = 8 * (size_t)p.K * sizeof(float);
        if (P && (rc = launch(bucketed_crf_emit_kernel, lgrid, 512, lds_row, s, SC, P, p.len, EM, B, p.L, p.K))) return rc;
        if ((rc = big ? launch(bucketed_crf_kernel<true>, B, 256, lds, s, p) : launch(bucketed_crf_kernel<false>, B, 256, lds, s, p))) return rc;
        if (P && (rc = launch(bucketed_crf_adjoint_kernel, lgrid, 512, lds_row, s, p.DS, P, p.len, B, p.L, p.K))) return rc;
        const int KK = p.K * p.K;
        crf_reduce_kernel<<<(unsigned)((KK + 255) / 256), 256, 0, s>>>(p.dtrans_part, dtrans, B, KK);
        onehot_loss_sum_kernel<<<1, 64, 0, s>>>(loss_seq, B, loss);
        return FARNN_OK;
    }
};

}  // namespace farnn
