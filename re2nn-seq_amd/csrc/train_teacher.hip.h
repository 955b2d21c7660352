// The regular-expression teacher of the decomposed i-FST's training step (--marryup_type kd | pr).
//
// Reference: FARNN_S_D_W_I_S.forward_local(train=True, re_tags=...) (model_decompose_single.py:291-300) and baselines/KD.py:
//   KD   KL = KLDivLoss()(log_softmax(scores / T), softmax(re / T)) T^2,                T = c1_kdpr          (KD.py:3-7)
//   PR   KL = KLDivLoss()(log_softmax(scores), q),  q = softmax(softmax(scores) * exp(re - 1) * c1_kdpr)     (KD.py:10-18)
//   loss = pi * original + (1 - pi) * KL
// KLDivLoss() has torch's default reduction 'mean': the sum over ALL B L K elements over B L K, the pad positions included.  The
// scores of a pad position i >= len are C (f_{i+1} * b_{i+1}) of the chains continued through the pad tokens (train.hip.h:
// full_chain), so this kernel walks every position of the batch, and its adjoints reach every step of both chains.  The PR
// teacher q is a function of the scores and is NOT detached (KD.py:15-17): the adjoint flows through it as well.
#pragma once
#include "train.hip.h"

namespace farnn {

__device__ __forceinline__ float tt_wave_sum(float v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ float tt_wave_max(float v) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}

// ---- scores, the original loss, the KL term and the adjoints of alpha / beta at EVERY position ----------------------------
// Shaped like train_loss_kernel: persistent workgroups of 8 wavefronts, a wavefront per position, C_output_mat staged in LDS
// (row stride S+1) when it fits.  LDS: [Cs[K][S+1]] then per wavefront ab[mv_pad(S)], sc[K], ds[K], tg[K], uu[K].
// PHASE 0: fused (cross-entropy + KL).  CRF mode splits it around train_crf_kernel: PHASE 1 writes the emissions SC and
// alpha*beta of every position, PHASE 2 reads the emissions and the CRF's d loss / d emissions (DS: zero at the pads) back.
// A valid position reads alpha row i+1 and backward row len-1-i as train_loss_kernel does; a pad position reads row i+1 of
// both (reverse(ht_backward_score, lengths + 1) flips the first len+1 rows only, :261): backward row len is read by nobody.
// The loss leaves as one partial per wavefront (loss_part[gridDim.x * 8], added in index order by teacher_finish_kernel):
// no float atomic, so two steps give the same KL bit for bit.
template <bool CLDS, int PHASE>
__global__ void __launch_bounds__(512)
train_teacher_loss_kernel(const TrainParams p) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int S = p.S, K = p.K, SP = mv_pad(S), ldc = CLDS ? S + 1 : S;
    float *Cs = smem;
    float *ab = smem + (CLDS ? ((K * (S + 1) + 3) & ~3) : 0) + w * (SP + 4 * K), *sc = ab + SP, *ds = sc + K, *tg = ds + K, *uu = tg + K;
    if (CLDS) {
        for (int e = tid; e < K * S; e += blockDim.x) { const int c = e / S, s_ = e - c * S; Cs[c * (S + 1) + s_] = p.C[e]; }
        __syncthreads();
    }
    const float *Cm = CLDS ? Cs : p.C;
    const float pi = p.t_pi, wkl = (1.0f - p.t_pi) * p.t_inv_n;           // weights of the original loss and of one KL element
    float loss_acc = 0.0f;
    for (long long pos = (long long)blockIdx.x * nw + w; pos < (long long)p.B * p.L; pos += (long long)gridDim.x * nw) {
        const int b = (int)(pos / p.L), i = (int)(pos - (long long)b * p.L);
        const int len = clamp_len(p.len[b], p.L);
        const bool valid = i < len;                                        // (wave-uniform)
        const int brow = valid ? len - 1 - i : i + 1;
        const float *al = p.A + ((long long)b * (p.L + 1) + i + 1) * S;
        const float *be = p.Bk + ((long long)b * (p.L + 1) + brow) * S;
        if (PHASE != 2) {
            for (int s = lane; s < S; s += WAVE) {
                const float v = al[s] * be[s];
                ab[s] = v;
                p.AB[pos * S + s] = v;
            }
            for (int c = lane; c < K; c += WAVE) {                                        // get_final_score (:200-203)
                const float *cr = Cm + (long long)c * ldc;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                int s = 0;
                for (; s + 8 <= S; s += 8) {
                    float cv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) cv[u] = cr[s + u];
                    const v4f x0 = *(const v4f *)(ab + s), x1 = *(const v4f *)(ab + s + 4);
                    a0 = fmaf(x0[0], cv[0], a0); a1 = fmaf(x0[1], cv[1], a1); a2 = fmaf(x0[2], cv[2], a2); a3 = fmaf(x0[3], cv[3], a3);
                    a0 = fmaf(x1[0], cv[4], a0); a1 = fmaf(x1[1], cv[5], a1); a2 = fmaf(x1[2], cv[6], a2); a3 = fmaf(x1[3], cv[7], a3);
                }
                for (; s < S; s++) a0 = fmaf(ab[s], cr[s], a0);
                sc[c] = (a0 + a1) + (a2 + a3);
            }
            if (p.P) {                                                                     // priority layer
                for (int d = lane; d < K; d += WAVE) {
                    float a = 0.0f;
                    for (int c = 0; c < K; c++) a = fmaf(sc[c], p.P[(long long)c * K + d], a);
                    ds[d] = a;
                }
                for (int d = lane; d < K; d += WAVE) sc[d] = ds[d];
            }
        }
        if (PHASE == 1) {
            if (!valid && lane == 0) p.tags[pos] = -1;         // (train_crf_kernel writes no tag for a sequence of length 0)
            for (int c = lane; c < K; c += WAVE) p.SC[pos * K + c] = sc[c];
            continue;
        }
        if (PHASE == 2)
            for (int c = lane; c < K; c += WAVE) sc[c] = p.SC[pos * K + c];
        for (int c = lane; c < K; c += WAVE) tg[c] = p.re[pos * K + c];
        // log-sum-exp of the scores: the cross-entropy's and PR's softmax (KD takes its own, at temperature T)
        float mx = -INFINITY;
        for (int c = lane; c < K; c += WAVE) mx = fmaxf(mx, sc[c]);
        mx = tt_wave_max(mx);
        float se = 0.0f;
        for (int c = lane; c < K; c += WAVE) se += expf(sc[c] - mx);
        const float lse = mx + logf(tt_wave_sum(se));
        // ds = pi * d original / d scores
        if (PHASE == 0) {
            if (valid) {
                // softmax cross-entropy (mean over the batch's valid tokens) and the prediction, as train_loss_kernel
                const long long lab64 = p.labels[pos];
                const int lab = (lab64 < 0 || lab64 >= K) ? 0 : (int)lab64;
                if (lane == 0 && lab64 != lab) atomicOr(p.err, 1);
                loss_acc += pi * ((lse - sc[lab]) * p.inv_tokens);
                float bv = -INFINITY; int bi = 0x7ffffffe;
                for (int c = lane; c < K; c += WAVE) {
                    float vv = sc[c] + 0.0f;
                    if (c == K - 1) vv = fminf(vv, p.threshold);
                    if (vv > bv) { bv = vv; bi = c; }
                }
                bi = wave_argmax_dpp(bv, bi);
                if (lane == 0) p.tags[pos] = (bi >= K) ? 0 : (bi == K - 1 ? p.o_idx : bi);
                for (int c = lane; c < K; c += WAVE) ds[c] = pi * ((expf(sc[c] - lse) - (c == lab ? 1.0f : 0.0f)) * p.inv_tokens);
            } else {
                if (lane == 0) p.tags[pos] = -1;
                for (int c = lane; c < K; c += WAVE) ds[c] = 0.0f;
            }
        } else {
            for (int c = lane; c < K; c += WAVE) ds[c] = pi * p.DS[pos * K + c];          // d CRF loss / d emissions (zero at the pads)
        }
        // the KL term of this position (its K elements) and (1 - pi) / (B L K) * d KL / d scores, added to ds
        float kl;
        if (p.t_mode == FARNN_TEACHER_KD) {
            const float T = p.t_c1, it = 1.0f / T;
            float m1 = -INFINITY, m2 = -INFINITY;
            for (int c = lane; c < K; c += WAVE) { m1 = fmaxf(m1, sc[c] * it); m2 = fmaxf(m2, tg[c] * it); }
            m1 = tt_wave_max(m1); m2 = tt_wave_max(m2);
            float s1 = 0.0f, s2 = 0.0f;
            for (int c = lane; c < K; c += WAVE) { s1 += expf(sc[c] * it - m1); s2 += expf(tg[c] * it - m2); }
            const float l1 = m1 + logf(tt_wave_sum(s1)), l2 = m2 + logf(tt_wave_sum(s2));
            float kls = 0.0f;
            for (int c = lane; c < K; c += WAVE) {
                const float lq = sc[c] * it - l1, lt = tg[c] * it - l2, pt = expf(lt);      // student's and teacher's log-probabilities
                kls = fmaf(pt, lt - lq, kls);
                ds[c] = fmaf(wkl * T, expf(lq) - pt, ds[c]);                                 // T^2 (softmax(scores / T) - teacher) / T
            }
            kl = tt_wave_sum(kls) * (T * T);
        } else {
            const float c1 = p.t_c1;
            // u = softmax(scores) * exp(re - 1) * c1, q = softmax(u)
            float mu = -INFINITY;
            for (int c = lane; c < K; c += WAVE) {
                const float e = expf(tg[c] - 1.0f) * c1, u = expf(sc[c] - lse) * e;
                tg[c] = e; uu[c] = u;
                mu = fmaxf(mu, u);
            }
            mu = tt_wave_max(mu);
            float su = 0.0f;
            for (int c = lane; c < K; c += WAVE) su += expf(uu[c] - mu);
            const float lu = mu + logf(tt_wave_sum(su));
            // KL = sum q (log q - lp); d KL / d q = g = log q + 1 - lp; through q = softmax(u): du = q (g - sum q g)
            float kls = 0.0f, G = 0.0f;
            for (int c = lane; c < K; c += WAVE) {
                const float lq = uu[c] - lu, q = expf(lq), lp = sc[c] - lse;
                kls = fmaf(q, lq - lp, kls);
                G = fmaf(q, lq + 1.0f - lp, G);
            }
            kl = tt_wave_sum(kls); G = tt_wave_sum(G);
            // through u = s e: dsm = du e; through s = softmax(scores): s (dsm - sum s dsm); through lp: s - q
            float D = 0.0f;
            for (int c = lane; c < K; c += WAVE) {
                const float lq = uu[c] - lu, q = expf(lq), lp = sc[c] - lse;
                const float dsm = q * (lq + 1.0f - lp - G) * tg[c];
                uu[c] = dsm;
                D = fmaf(expf(lp), dsm, D);
                tg[c] = q;
            }
            D = tt_wave_sum(D);
            for (int c = lane; c < K; c += WAVE) {
                const float s_ = expf(sc[c] - lse);
                ds[c] = fmaf(wkl, s_ * (uu[c] - D) + (s_ - tg[c]), ds[c]);
            }
        }
        loss_acc = fmaf(wkl, kl, loss_acc);
        if (p.P) {                                                                         // back through scores . P
            for (int c = lane; c < K; c += WAVE) {
                float a = 0.0f;
                for (int d = 0; d < K; d++) a = fmaf(ds[d], p.P[(long long)c * K + d], a);
                sc[c] = a;
            }
            for (int c = lane; c < K; c += WAVE) ds[c] = sc[c];
        }
        for (int c = lane; c < K; c += WAVE) p.DS[pos * K + c] = ds[c];
        float *ga = p.GA + ((long long)b * (p.L + 1) + i + 1) * S;
        float *gb = p.GB + ((long long)b * (p.L + 1) + brow) * S;
        for (int s = lane; s < S; s += WAVE) {
            float d0 = 0.0f, d1 = 0.0f;
            int c = 0;
            for (; c + 8 <= K; c += 8) {
                float cv[8], dv[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { cv[u] = Cm[(long long)(c + u) * ldc + s]; dv[u] = ds[c + u]; }
#pragma unroll
                for (int u = 0; u < 8; u += 2) { d0 = fmaf(dv[u], cv[u], d0); d1 = fmaf(dv[u + 1], cv[u + 1], d1); }
            }
            for (; c < K; c++) d0 = fmaf(ds[c], Cm[(long long)c * ldc + s], d0);           // d(alpha*beta)
            const float d = d0 + d1;
            ga[s] = d * be[s];
            gb[s] = d * al[s];
        }
    }
    if (PHASE != 1 && lane == 0) p.loss_part[blockIdx.x * nw + w] = loss_acc;
}

// loss = [pi * the CRF's sum, which train_crf_kernel left there] + the wavefronts' partials in index order; dtrans *= pi
__global__ void __launch_bounds__(256)
teacher_finish_kernel(const float *__restrict__ part, int n, float *loss, float pi, int crf, float *dtrans, int KK) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < KK) dtrans[idx] *= pi;
    if (blockIdx.x == 0 && threadIdx.x < WAVE) {
        const int lane = threadIdx.x;
        float s = 0.0f;
        for (int k = lane; k < n; k += WAVE) s += part[k];
        s = tt_wave_sum(s);
        if (lane == 0) loss[0] = crf ? fmaf(pi, loss[0], s) : s;
    }
}

}  // namespace farnn
