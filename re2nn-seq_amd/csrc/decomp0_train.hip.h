// Training step of the decomposed FST tagger (FARNN_S_D_W, --method decompose --independent 0): the CE1 loss
// or the CRF negative log-likelihood, and the gradients of Vgen, C_embed, S1, S2, C_wildcard, S1_wildcard, S2_wildcard,
// wildcard_wildcard, h0, hT, the gates and the CRF's transitions.
//
// Reference: FARNN_S_D_W.forward_local(train=True) (model_decompose.py:373-456) followed by loss.backward().  With v = Vgen[w]:
//   csum = C_embed.sum(0), cwsum = C_wildcard.sum(0)                                                           (:328, :394)
//   Rtab[w] = v * csum;  W = S1w diag(cwsum) S2w^T + WW                                                        (:253, :327-332)
//   chains: the decomposed i-FST's recurrence (train.hip.h) on (Rtab, S1, S2, W, gates) with an output mask of ones  (:243-308)
//   score_i[c] = sum_r v_r C_embed[c,r] (alpha_i S1)_r (beta_i S2)_r + sum_q C_wildcard[c,q] (alpha_i S1w)_q (beta_i S2w)_q
//                alpha_i = the forward state BEFORE token i, beta_i = the backward state behind it              (:310-325, :426-427)
// The chains with their stash and the back-propagation through time are train.hip.h's kernels, unchanged for the i-FST; this
// step launches train_backward_kernel's DET form, which stores what the plain form adds with float atomics (the word table's
// and the gates' per-step adjoints, the sequences' dh0 / dhT).  The max semiring's chains and their weight gradients are
// decomp0_train_max.hip.h's; the rest of that step is this header's, unchanged.  This header adds
//   decomp0_prep_kernel      Rtab, W and W^T from the column sums
//   decomp0_loss_kernel      the score head and its adjoint: a tile of 16 positions per workgroup round, the four state-by-rank
//                            products, the two label-by-rank products and all their transposes on the f32 matrix cores
//   decomp0_word_sum_kernel  the per-position rows of dVgen, dRtab and the gates' input adjoints summed per word in bucket order
//   decomp0_fold_kernel / decomp0_sum_adj_kernel   the chain inputs folded back into the model's tensors
// No float atomic adds two values of one step in an order that can change: every output of atb_reduce_kernel here has at most
// two addends (a + b = b + a bit for bit), everything else has one owner and a fixed order.  Two steps are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

namespace farnn {

constexpr int D0_TP = 16;           // positions per tile: the M of v_mfma_f32_16x16x4_f32
constexpr int D0_THREADS = 256;     // four wavefronts: each takes every fourth block of 16 output columns
constexpr int D0_WAVES = D0_THREADS / 64;

// row stride of a tile operand in LDS: a multiple of 4 with an odd quarter, so that the 16 rows x 4 k of an MFMA A operand
// (lane l reads row l & 15, column k + (l >> 4)) fall into 64 different banks; at least 3 zero columns behind n
__host__ __device__ __forceinline__ int d0_pad(int n) { return ((((n + 3) >> 2) + 1) | 1) << 2; }

struct D0Params {
    const float *Vgen, *Ce, *Cw, *S1, *S2, *S1w, *S2w, *P;   // [V][R], [K][R], [K][Q], [S][R] x2, [S][Q] x2, [K][K] or null
    const float *S1T, *S2T, *S1wT, *S2wT;                    // [R][S] x2, [Q][S] x2
    const float *A, *Bk;                                     // stash [B][L+1][S]
    float *GA, *GB;                                          // adjoint rows of the stash, read by train_backward_kernel
    const int64_t *x, *len, *labels;
    float *SC, *DS;                                          // [B L][K] emissions (CRF), d loss / d scores
    float *U, *UW, *DVS;                                     // [B L][R] v p q, [B L][Q] pw qw, [B L][R] the score's share of dVgen[w]
    float *DP, *DQ, *DPW, *DQW;                              // [B (L+1)][R | Q]: dp, dpw at alpha's stash row, dq, dqw at beta's
    float *loss_part;                                        // [gridDim.x * D0_WAVES]
    int32_t *tags;
    int *err;
    int B, L, V, S, R, Q, K, o_idx;
    float threshold, inv_tokens;
};

// LDS floats of decomp0_loss_kernel: al be [16][d0_pad(S)], p q g [16][d0_pad(R)], pw qw gw [16][d0_pad(Q)], sc ds
// [16][d0_pad(K)], 64 ints; the label factors [K][d0_pad(R)] + [K][d0_pad(Q)] behind them when CLDS
struct D0Lds {
    size_t tile, mat;
    bool clds() const { return tile + mat <= 150 * 1024; }
    size_t bytes() const { return tile + (clds() ? mat : 0); }
};
inline D0Lds decomp0_loss_lds(size_t S, size_t R, size_t Q, size_t K) {
    const size_t t = D0_TP * (2 * (size_t)d0_pad((int)S) + 3 * (size_t)d0_pad((int)R) + 3 * (size_t)d0_pad((int)Q) + 2 * (size_t)d0_pad((int)K)) + 64;
    return {t * sizeof(float), K * ((size_t)d0_pad((int)R) + (size_t)d0_pad((int)Q)) * sizeof(float)};
}

// out(m, n, acc) for the 16 x N product  in1[16][K1] B1[K1][N] + in2[16][K2] B2[K2][N]  (K2 = 0: one product).  in: LDS tiles,
// zero behind K (d0_pad); B element (k, n) at B[k bk + n bn], in global memory or LDS.  The wavefront takes the column blocks
// wave, wave + 4, ...; k ascends: a fixed order.
template <typename Out>
__device__ __forceinline__ void d0_mma(const float *in1, int ld1, const float *B1, size_t bk1, size_t bn1, int K1,
                                       const float *in2, int ld2, const float *B2, size_t bk2, size_t bn2, int K2,
                                       int N, int wave, int lane, Out &&out) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const int lr = lane & 15, lk = lane >> 4;
    for (int n0 = wave * 16; n0 < N; n0 += 16 * D0_WAVES) {
        f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
        const int n = n0 + lr;
        const bool nok = n < N;
        const float *b1 = B1 + (size_t)(nok ? n : 0) * bn1;
        for (int k0 = 0; k0 < K1; k0 += 4) {
            const int k = k0 + lk;
            const float a = in1[lr * ld1 + k];
            const float b = (nok && k < K1) ? b1[(size_t)k * bk1] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        if (K2 > 0) {
            const float *b2 = B2 + (size_t)(nok ? n : 0) * bn2;
            for (int k0 = 0; k0 < K2; k0 += 4) {
                const int k = k0 + lk;
                const float a = in2[lr * ld2 + k];
                const float b = (nok && k < K2) ? b2[(size_t)k * bk2] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
        }
        if (nok) {
#pragma unroll
            for (int r = 0; r < 4; r++) out(lk * 4 + r, n, acc[r]);      // D: row lk * 4 + r, column lr of the block
        }
    }
}

__global__ void __launch_bounds__(256)
decomp0_fill_kernel(float *__restrict__ dst, size_t n, float v) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = v;
}

// Rtab[w][r] = Vgen[w][r] csum[r];  W[i][j] = WW[i][j] + sum_q S1w[i][q] cwsum[q] S2w[j][q] and its transpose (q ascending)
__global__ void __launch_bounds__(256)
decomp0_prep_kernel(const float *__restrict__ Vgen, const float *__restrict__ csum, float *__restrict__ Rtab, size_t VR, int R,
                    const float *__restrict__ S1w, const float *__restrict__ S2w, const float *__restrict__ cwsum,
                    const float *__restrict__ WW, float *__restrict__ Wm, float *__restrict__ WT, int S, int Q) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < VR) Rtab[e] = Vgen[e] * csum[e % R];
    if (e < (size_t)S * S) {
        const int i = (int)(e / S), j = (int)(e - (size_t)i * S);
        float a = 0.0f;
        for (int q = 0; q < Q; q++) a = fmaf(S1w[(size_t)i * Q + q] * cwsum[q], S2w[(size_t)j * Q + q], a);
        a += WW[e];
        Wm[e] = a;
        WT[(size_t)j * S + i] = a;
    }
}

// ---- the score head, the loss and the adjoints ----------------------------------------------------------------------------------
// Persistent workgroups; a round takes the 16 positions pos0 .. pos0 + 15 of the flattened [B][L] grid (a pad position is a zero
// row).  PHASE as train_loss_kernel: 0 the fused cross-entropy, 1 the emissions SC for the CRF kernel, 2 the adjoints from DS.
// CLDS: C_embed and C_wildcard staged once per workgroup behind the tile.
template <bool CLDS, int PHASE>
__global__ void __launch_bounds__(D0_THREADS)
decomp0_loss_kernel(const D0Params p) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.S, R = p.R, Q = p.Q, K = p.K, L = p.L;
    const int SP = d0_pad(S), RP = d0_pad(R), QP = d0_pad(Q), KP = d0_pad(K);
    float *al = smem, *be = al + D0_TP * SP, *pp = be + D0_TP * SP, *qq = pp + D0_TP * RP, *gg = qq + D0_TP * RP;
    float *pw = gg + D0_TP * RP, *qw = pw + D0_TP * QP, *gw = qw + D0_TP * QP, *sc = gw + D0_TP * QP, *ds = sc + D0_TP * KP;
    int *meta = (int *)(ds + D0_TP * KP);                       // [4][16]: valid, alpha's stash row, beta's stash row, word
    int *m_ok = meta, *m_ra = meta + 16, *m_rb = meta + 32, *m_w = meta + 48;
    float *Cel = (float *)(meta + 64), *Cwl = Cel + K * RP;
    if (CLDS) {
        for (int e = tid; e < K * R; e += D0_THREADS) { const int c = e / R, r = e - c * R; Cel[c * RP + r] = p.Ce[e]; }
        for (int e = tid; e < K * Q; e += D0_THREADS) { const int c = e / Q, q = e - c * Q; Cwl[c * QP + q] = p.Cw[e]; }
    }
    const float *Ce = CLDS ? Cel : p.Ce, *Cw = CLDS ? Cwl : p.Cw;
    const size_t ldce = CLDS ? RP : R, ldcw = CLDS ? QP : Q;
    const long long N0 = (long long)p.B * L;
    float loss_acc = 0.0f;
    for (long long pos0 = (long long)blockIdx.x * D0_TP; pos0 < N0; pos0 += (long long)gridDim.x * D0_TP) {
        __syncthreads();                                        // the last round's readers are done; CLDS staging is visible
        if (tid < D0_TP) {
            const long long pos = pos0 + tid;
            int ok = 0, ra = 0, rb = 0, w = 0;
            if (pos < N0) {
                const int b = (int)(pos / L), i = (int)(pos - (long long)b * L), len = clamp_len(p.len[b], L);
                if (i < len) {
                    ok = 1; ra = b * (L + 1) + i; rb = b * (L + 1) + (len - 1 - i);
                    w = clamp_tok(p.x[pos], p.V);
                } else if (PHASE != 1) p.tags[pos] = -1;         // (under the CRF the CRF kernel writes the pads' tags)
            }
            m_ok[tid] = ok; m_ra[tid] = ra; m_rb[tid] = rb; m_w[tid] = w;
        }
        __syncthreads();
        for (int e = tid; e < D0_TP * SP; e += D0_THREADS) {
            const int m = e / SP, s = e - m * SP;
            const bool ok = m_ok[m] && s < S;
            al[e] = ok ? p.A[(size_t)m_ra[m] * S + s] : 0.0f;
            be[e] = ok ? p.Bk[(size_t)m_rb[m] * S + s] : 0.0f;
        }
        // every column below R / Q / K of these tiles is written before it is read; only the pad columns an MFMA operand reads
        // need zeros, and the rows of ds that belong to no position
        for (int e = tid; e < D0_TP * (RP - R); e += D0_THREADS) {
            const int o = (e / (RP - R)) * RP + R + e % (RP - R);
            pp[o] = 0.0f; qq[o] = 0.0f; gg[o] = 0.0f;
        }
        for (int e = tid; e < D0_TP * (QP - Q); e += D0_THREADS) {
            const int o = (e / (QP - Q)) * QP + Q + e % (QP - Q);
            pw[o] = 0.0f; qw[o] = 0.0f; gw[o] = 0.0f;
        }
        for (int e = tid; e < D0_TP * KP; e += D0_THREADS) ds[e] = 0.0f;
        __syncthreads();
        // p = alpha S1, q = beta S2, pw = alpha S1w, qw = beta S2w: the factors are read once per tile
        d0_mma(al, SP, p.S1, R, 1, S, nullptr, 0, nullptr, 0, 0, 0, R, wave, lane, [&](int m, int n, float v) { pp[m * RP + n] = v; });
        d0_mma(be, SP, p.S2, R, 1, S, nullptr, 0, nullptr, 0, 0, 0, R, wave, lane, [&](int m, int n, float v) { qq[m * RP + n] = v; });
        d0_mma(al, SP, p.S1w, Q, 1, S, nullptr, 0, nullptr, 0, 0, 0, Q, wave, lane, [&](int m, int n, float v) { pw[m * QP + n] = v; });
        d0_mma(be, SP, p.S2w, Q, 1, S, nullptr, 0, nullptr, 0, 0, 0, Q, wave, lane, [&](int m, int n, float v) { qw[m * QP + n] = v; });
        __syncthreads();
        if (PHASE != 2) {
            for (int e = tid; e < D0_TP * R; e += D0_THREADS) {          // u = v p q
                const int m = e / R, r = e - m * R;
                float u = 0.0f;
                if (m_ok[m]) {
                    u = p.Vgen[(size_t)m_w[m] * R + r] * pp[m * RP + r] * qq[m * RP + r];
                    p.U[(size_t)(pos0 + m) * R + r] = u;
                }
                gg[m * RP + r] = u;
            }
            for (int e = tid; e < D0_TP * Q; e += D0_THREADS) {          // uw = pw qw
                const int m = e / Q, q = e - m * Q;
                float u = 0.0f;
                if (m_ok[m]) {
                    u = pw[m * QP + q] * qw[m * QP + q];
                    p.UW[(size_t)(pos0 + m) * Q + q] = u;
                }
                gw[m * QP + q] = u;
            }
            __syncthreads();
            // score = u C_embed^T + uw C_wildcard^T                                                      (:314-323)
            d0_mma(gg, RP, Ce, 1, ldce, R, gw, QP, Cw, 1, ldcw, Q, K, wave, lane, [&](int m, int n, float v) { sc[m * KP + n] = v; });
            __syncthreads();
            if (p.P) {                                                   // the priority layer
                for (int e = tid; e < D0_TP * K; e += D0_THREADS) {
                    const int m = e / K, d = e - m * K;
                    float a = 0.0f;
                    for (int c = 0; c < K; c++) a = fmaf(sc[m * KP + c], p.P[(size_t)c * K + d], a);
                    ds[m * KP + d] = a;
                }
                __syncthreads();
                for (int e = tid; e < D0_TP * K; e += D0_THREADS) { const int m = e / K, d = e - m * K; sc[m * KP + d] = ds[m * KP + d]; }
                __syncthreads();
            }
        }
        if (PHASE == 1) {
            for (int e = tid; e < D0_TP * K; e += D0_THREADS) {
                const int m = e / K, c = e - m * K;
                if (m_ok[m]) p.SC[(size_t)(pos0 + m) * K + c] = sc[m * KP + c];
            }
            continue;
        }
        if (PHASE == 0) {
            // softmax cross-entropy and the argmax decode, a wavefront per position (train_loss_kernel's arithmetic)
            for (int m = wave; m < D0_TP; m += D0_WAVES) {
                if (!m_ok[m]) continue;                                  // (wave-uniform)
                const long long pos = pos0 + m;
                const float *s_ = sc + m * KP;
                float *d_ = ds + m * KP;
                float mx = -INFINITY;
                for (int c = lane; c < K; c += WAVE) mx = fmaxf(mx, s_[c]);
                for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
                float se = 0.0f;
                for (int c = lane; c < K; c += WAVE) se += expf(s_[c] - mx);
                for (int o = 32; o; o >>= 1) se += __shfl_xor(se, o, WAVE);
                const long long lab64 = p.labels[pos];
                const int lab = (lab64 < 0 || lab64 >= K) ? 0 : (int)lab64;
                if (lane == 0 && lab64 != lab) atomicOr(p.err, 1);
                const float lse = mx + logf(se);
                loss_acc += lse - s_[lab];
                float bv = -INFINITY; int bi = 0x7ffffffe;
                for (int c = lane; c < K; c += WAVE) {
                    float vv = s_[c] + 0.0f;
                    if (c == K - 1) vv = fminf(vv, p.threshold);
                    if (vv > bv) { bv = vv; bi = c; }
                }
                bi = wave_argmax_dpp(bv, bi);
                if (lane == 0) p.tags[pos] = (bi >= K) ? 0 : (bi == K - 1 ? p.o_idx : bi);
                for (int c = lane; c < K; c += WAVE) d_[c] = (expf(s_[c] - lse) - (c == lab ? 1.0f : 0.0f)) * p.inv_tokens;
            }
        } else {
            for (int e = tid; e < D0_TP * K; e += D0_THREADS) {
                const int m = e / K, c = e - m * K;
                ds[m * KP + c] = m_ok[m] ? p.DS[(size_t)(pos0 + m) * K + c] : 0.0f;       // d loss / d emissions (CRF)
            }
        }
        __syncthreads();
        if (p.P) {                                                       // back through scores . P
            for (int e = tid; e < D0_TP * K; e += D0_THREADS) {
                const int m = e / K, c = e - m * K;
                float a = 0.0f;
                for (int d = 0; d < K; d++) a = fmaf(ds[m * KP + d], p.P[(size_t)c * K + d], a);
                sc[m * KP + c] = a;
            }
            __syncthreads();
            for (int e = tid; e < D0_TP * K; e += D0_THREADS) { const int m = e / K, c = e - m * K; ds[m * KP + c] = sc[m * KP + c]; }
            __syncthreads();
        }
        for (int e = tid; e < D0_TP * K; e += D0_THREADS) {
            const int m = e / K, c = e - m * K;
            if (m_ok[m]) p.DS[(size_t)(pos0 + m) * K + c] = ds[m * KP + c];
        }
        // du = ds C_embed, duw = ds C_wildcard
        d0_mma(ds, KP, Ce, ldce, 1, K, nullptr, 0, nullptr, 0, 0, 0, R, wave, lane, [&](int m, int n, float v) { gg[m * RP + n] = v; });
        d0_mma(ds, KP, Cw, ldcw, 1, K, nullptr, 0, nullptr, 0, 0, 0, Q, wave, lane, [&](int m, int n, float v) { gw[m * QP + n] = v; });
        __syncthreads();
        for (int e = tid; e < D0_TP * R; e += D0_THREADS) {              // dp = du v q, dq = du v p, dv = du p q
            const int m = e / R, r = e - m * R;
            float dp = 0.0f, dq = 0.0f;
            if (m_ok[m]) {
                const float v = p.Vgen[(size_t)m_w[m] * R + r], g = gg[m * RP + r], a = pp[m * RP + r], b = qq[m * RP + r];
                dp = g * v * b; dq = g * v * a;
                p.DP[(size_t)m_ra[m] * R + r] = dp;
                p.DQ[(size_t)m_rb[m] * R + r] = dq;
                p.DVS[(size_t)(pos0 + m) * R + r] = g * a * b;
            }
            pp[m * RP + r] = dp; qq[m * RP + r] = dq;
        }
        for (int e = tid; e < D0_TP * Q; e += D0_THREADS) {              // dpw = duw qw, dqw = duw pw
            const int m = e / Q, q = e - m * Q;
            float dp = 0.0f, dq = 0.0f;
            if (m_ok[m]) {
                const float g = gw[m * QP + q];
                dp = g * qw[m * QP + q]; dq = g * pw[m * QP + q];
                p.DPW[(size_t)m_ra[m] * Q + q] = dp;
                p.DQW[(size_t)m_rb[m] * Q + q] = dq;
            }
            pw[m * QP + q] = dp; qw[m * QP + q] = dq;
        }
        __syncthreads();
        // GA = dp S1^T + dpw S1w^T at alpha's stash row, GB = dq S2^T + dqw S2w^T at beta's
        d0_mma(pp, RP, p.S1T, S, 1, R, pw, QP, p.S1wT, S, 1, Q, S, wave, lane,
               [&](int m, int n, float v) { if (m_ok[m]) p.GA[(size_t)m_ra[m] * S + n] = v; });
        d0_mma(qq, RP, p.S2T, S, 1, R, qw, QP, p.S2wT, S, 1, Q, S, wave, lane,
               [&](int m, int n, float v) { if (m_ok[m]) p.GB[(size_t)m_rb[m] * S + n] = v; });
    }
    if (PHASE == 0 && lane == 0) p.loss_part[blockIdx.x * D0_WAVES + wave] = loss_acc * p.inv_tokens;
}

// ---- per word, in bucket order: the rows the loss kernel and the back-propagation left per position ------------------------------
// dVs[w] = sum DVS[pos]; dRt[w] = sum DVf[row of the forward step that read pos] + DVb[row of the backward step];
// dGV1[w] / dGV2[w] likewise from DAZ / DAR (farnn >= 1 / 2).  Zero rows for a word that does not occur.  grid (V).
// MX (the max semiring, decomp0_train_max.hip.h): dRt of the batch's words comes from dM_w and is left alone; the other rows are zeroed.
struct D0WordSum {
    const int *list, *wstart, *wcount;
    const int64_t *len;
    const float *DVS, *DVf, *DVb, *DAZf, *DAZb, *DARf, *DARb;
    float *dVs, *dRt, *dGV1, *dGV2;
    int L, S, R, farnn;
};
template <bool MX = false>
__global__ void __launch_bounds__(256)
decomp0_word_sum_kernel(const D0WordSum p) {
    const int w = blockIdx.x, n = p.wcount[w], first = p.wstart[w], L = p.L;
    for (int r = threadIdx.x; r < p.R; r += 256) {
        float a = 0.0f, c = 0.0f;
        for (int k = 0; k < n; k++) {
            const int pos = p.list[first + k], b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
            const size_t row0 = (size_t)b * (L + 1);
            a += p.DVS[(size_t)pos * p.R + r];
            if constexpr (!MX) c += p.DVf[(row0 + i + 1) * p.R + r] + p.DVb[(row0 + len - i) * p.R + r];
        }
        p.dVs[(size_t)w * p.R + r] = a;
        if (!MX || n == 0) p.dRt[(size_t)w * p.R + r] = c;
    }
    if (!p.farnn) return;
    for (int s = threadIdx.x; s < p.S; s += 256) {
        float a = 0.0f, c = 0.0f;
        for (int k = 0; k < n; k++) {
            const int pos = p.list[first + k], b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
            const size_t rf = ((size_t)b * (L + 1) + i + 1) * p.S + s, rb = ((size_t)b * (L + 1) + len - i) * p.S + s;
            a += p.DAZf[rf] + p.DAZb[rb];
            if (p.farnn == 2) c += p.DARf[rf] + p.DARb[rb];
        }
        p.dGV1[(size_t)w * p.S + s] = a;
        if (p.farnn == 2) p.dGV2[(size_t)w * p.S + s] = c;
    }
}

// ---- the chain's inputs folded back, one owner per element -------------------------------------------------------------------------
// dRt += dRg1 + dRg2 (the gates' share, null without gates); dVgen = dVs + dRt csum; dS1 += dS1s, dS2 += dS2s (the score's
// share); dS1w += (dW S2w) cwsum, dS2w += (dW^T S1w) cwsum
struct D0Fold {
    const float *dVs, *dRg1, *dRg2, *csum, *cwsum, *dS1s, *dS2s, *X1, *X2;
    float *dRt, *dVgen, *dS1, *dS2, *dS1w, *dS2w;
    size_t VR, SR, SQ;
    int R, Q;
};
__global__ void __launch_bounds__(256)
decomp0_fold_kernel(const D0Fold p) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < p.VR) {
        float t = p.dRt[e];
        if (p.dRg1) t += p.dRg1[e];
        if (p.dRg2) t += p.dRg2[e];
        p.dRt[e] = t;
        p.dVgen[e] = fmaf(t, p.csum[e % p.R], p.dVs[e]);
    }
    if (e < p.SR) { p.dS1[e] += p.dS1s[e]; p.dS2[e] += p.dS2s[e]; }
    if (e < p.SQ) {
        const float c = p.cwsum[e % p.Q];
        p.dS1w[e] = fmaf(p.X1[e], c, p.dS1w[e]);
        p.dS2w[e] = fmaf(p.X2[e], c, p.dS2w[e]);
    }
}

// thread r < R: dcsum[r] = sum_w dRt[w][r] Vgen[w][r] (words in id order), added to every row of dC_embed; thread R + q:
// dcwsum[q] = sum_i S1w[i][q] X1[i][q] (X1 = dW S2w), added to every row of dC_wildcard; thread R + Q + s: dh0[s] = the sum of
// the sequences' shares HP[b][0][s] in order, thread R + Q + S + s: dhT[s] likewise
struct D0SumAdj {
    const float *dRt, *Vgen, *S1w, *X1, *HP;
    float *dCe, *dCw, *dh0, *dhT;
    int V, R, Q, S, K, B;
};
__global__ void __launch_bounds__(256)
decomp0_sum_adj_kernel(const D0SumAdj p) {
    int t = blockIdx.x * 256 + threadIdx.x;
    if (t < p.R) {
        float a = 0.0f;
        for (int w = 0; w < p.V; w++) a = fmaf(p.dRt[(size_t)w * p.R + t], p.Vgen[(size_t)w * p.R + t], a);
        for (int c = 0; c < p.K; c++) p.dCe[(size_t)c * p.R + t] += a;
        return;
    }
    t -= p.R;
    if (t < p.Q) {
        float a = 0.0f;
        for (int i = 0; i < p.S; i++) a = fmaf(p.S1w[(size_t)i * p.Q + t], p.X1[(size_t)i * p.Q + t], a);
        for (int c = 0; c < p.K; c++) p.dCw[(size_t)c * p.Q + t] += a;
        return;
    }
    t -= p.Q;
    if (t < 2 * p.S) {
        const int dir = t / p.S, s = t - dir * p.S;
        float a = 0.0f;
        for (int b = 0; b < p.B; b++) a += p.HP[((size_t)b * 2 + dir) * p.S + s];
        (dir == 0 ? p.dh0 : p.dhT)[s] = a;
    }
}

}  // namespace farnn
