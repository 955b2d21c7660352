// Training step of the onehot FST tagger (FARNN_S_O, --method onehot --independent 0): the CE1 loss and the gradients of
// language_tensor [V][C][S][S] and (asked for) wildcard_tensor [C][S][S].
//
// Reference: FARNN_S_O.forward_local(train=True) (model_onehot.py:66-146; sum semiring, CE1) followed by loss.backward()
// (train_onehot.py:156-206).  With A[w,c] = T4[w,c] + W4[c] (:87) and M[w] = sum_c T4[w,c] + sum_c W4[c] (:82):
//   chains   alpha_{i+1} = relu(alpha_i M[x_i]), alpha_0 = h0;  beta_i = relu(M[x_i] beta_{i+1}), beta_n = hT      (:89-102)
//   score_i[c] = sum_{s,j} relu(A[x_i,c,s,j] alpha_i[s] beta_{i+1}[j]) [. P]                                  (:115-127)
// The chains, their back-propagation through time and dM[w] are the onehot i-FST step's kernels (onehot_train.hip.h) on
// the premixed M with a mask of ones and relu: the stash row A[b][t] is alpha_t, Bk[b][t] is beta_{len-t}, and the adjoint
// of a state sits in the row of that state, so nothing is shifted.  This header adds the premix of the batch's words, the
// scores from the stashed states, the loss on given scores, and the backward of the scores.
//
// The score kernels (fst4_train_kernel) walk the positions in bucket (word) order: a workgroup takes one word and one
// group of label columns, holds one label's S x S block of A in registers (T4 + W4 read once per word and pass, 16 bytes
// per lane along j, rows past S and the last partial chunk predicated) and runs over the word's positions, staged in LDS
// F4_G at a time.  MODE 0 writes the scores; MODE 1 the contributions to d alpha_i and d beta_{i+1} as one partial per
// label group (fst4_adj_reduce_kernel adds the groups in order); MODE 2, after the chains' back-propagation, accumulates
// dA_score in registers over the whole run and writes dT4[w,c] = dA_score + dM[w] once (zeros for an absent word).
// No float atomics: every sum has one owner and a fixed order, two steps on the same inputs are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

namespace farnn {

constexpr int F4_THREADS = 256;   // score kernels: 4 wavefronts
constexpr int F4_G = 32;          // positions staged per round
constexpr int F4_MAX_GROUPS = 16; // label groups per word at most (the d alpha / d beta partials are [B L][groups][2][S])

struct Fst4TrainParams {
    const float *T4, *W4;            // [V][C][S][S], [C][S][S]
    const float *A, *Bk;             // stash [B][L+1][S]
    const int64_t *len;
    const int *list, *wstart, *wcount;   // the positions bucketed by word
    float *SC;                       // [B L][C] scores before the priority layer (MODE 0)
    const float *DS;                 // [B L][C] d loss / d SC (MODE 1, 2)
    float *part;                     // [B L, bucket order][ngrp][2][S] (MODE 1)
    const float *dM;                 // [V][S][S] (MODE 2)
    float *dT4;                      // [V][C][S][S] (MODE 2)
    int L, S, SP, C, cpg, ngrp;      // SP = S rounded up to 4; label columns per group; groups
    int CPR, GW;                     // 16-byte chunks per row; rows a wavefront takes at a time (GW CPR <= 64 lanes)
};

// LDS floats of fst4_train_kernel: alpha, beta [F4_G][SP]; g, position [F4_G]; the wavefronts' score shares [4][F4_G];
// MODE 1: two buffers of a position's d alpha [SP] and d beta shares [4 GW][4 CPR], and the chunk's sums [F4_G][2][SP]
inline size_t fst4_train_lds_floats(int SP, int CPR, int GW) {
    return (size_t)2 * F4_G * SP + 2 * F4_G + 4 * F4_G + 2 * ((size_t)SP + 16 * (size_t)GW * CPR) + (size_t)2 * F4_G * SP;
}

// LDS bytes of fst4_loss_kernel: 8 wavefronts, sc[K] and ds[K] each
inline size_t fst4_loss_lds_bytes(size_t K) { return 8 * 2 * K * sizeof(float); }

// four floats of a row at column j0 (4-byte aligned, unpadded rows): one 16-byte load inside the row, single loads at its end
__device__ __forceinline__ v4f f4_load(const float *q, int j0, int S) {
    v4f v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j0 + 3 < S) {
        __builtin_memcpy(&v, q, 16);
    } else {
        v[0] = q[0];
        if (j0 + 1 < S) v[1] = q[1];
        if (j0 + 2 < S) v[2] = q[2];
    }
    return v;
}
__device__ __forceinline__ void f4_store(float *q, int j0, int S, v4f v) {
    if (j0 + 3 < S) {
        __builtin_memcpy(q, &v, 16);
    } else {
        q[0] = v[0];
        if (j0 + 1 < S) q[1] = v[1];
        if (j0 + 2 < S) q[2] = v[2];
    }
}

// grid (V, ngrp).  RPT: register rows per thread (row s = g + 4 GW k, k < RPT, covers S).
template <int RPT, int MODE>
__global__ void __launch_bounds__(F4_THREADS)
fst4_train_kernel(const Fst4TrainParams p) {
    extern __shared__ __align__(16) float sm[];
    const int w = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int S = p.S, SP = p.SP, C = p.C, L = p.L, CPR = p.CPR;
    const int c0 = grp * p.cpg, c1 = min(C, c0 + p.cpg);
    const int nw = p.wcount[w], first = p.wstart[w];
    if (MODE != 2 && nw == 0) return;
    const int gw = lane / CPR, lr = lane - gw * CPR;
    const bool active = gw < p.GW;
    const int G = 4 * p.GW, g = wave * p.GW + (active ? gw : 0);
    const int j0 = 4 * lr;
    const size_t SS = (size_t)S * S;
    float *al = sm, *be = al + F4_G * SP, *gs = be + F4_G * SP;
    int *pl = (int *)(gs + F4_G);
    float *red = gs + 2 * F4_G;                                   // [4][F4_G]
    float *dal = red + 4 * F4_G, *dbl = dal + 2 * SP;             // [2][SP], [2][G][4 CPR]
    float *acc = dbl + 2 * 4 * G * CPR;                           // [F4_G][2][SP]
    const int nbuf = 4 * G * CPR;

    if (MODE == 2 && nw == 0) {                                   // an absent word: its rows are zero
        const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active)
            for (int c = c0; c < c1; c++) {
                float *ob = p.dT4 + ((size_t)w * C + c) * SS;
                for (int s = g; s < S; s += G) f4_store(ob + (size_t)s * S + j0, j0, S, z);
            }
        return;
    }
    // positions n0 .. n0 + n - 1 of the word: alpha_i, beta_{i+1} and the flat position
    auto stage = [&](int n0, int n) {
        for (int e = tid; e < n * SP; e += F4_THREADS) {
            const int q = e / SP, s = e - q * SP;
            const int pos = p.list[first + n0 + q];
            const int b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
            const size_t row0 = (size_t)b * (L + 1);
            al[e] = s < S ? p.A[(row0 + i) * S + s] : 0.0f;
            be[e] = s < S ? p.Bk[(row0 + len - 1 - i) * S + s] : 0.0f;
            if (s == 0) pl[q] = pos;
        }
    };
    const bool one_round = nw <= F4_G;
    if (one_round) stage(0, nw);                                  // (the barrier at the top of the first round follows)

    for (int c = c0; c < c1; c++) {
        v4f a[RPT], d[MODE == 2 ? RPT : 1];
        const float *tb = p.T4 + ((size_t)w * C + c) * SS, *wb = p.W4 + (size_t)c * SS;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int s = g + G * k;
            a[k] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
            if (active && s < S) a[k] = f4_load(tb + (size_t)s * S + j0, j0, S) + f4_load(wb + (size_t)s * S + j0, j0, S);
            if (MODE == 2) d[k] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        }
        for (int n0 = 0; n0 < nw; n0 += F4_G) {
            const int n = min(F4_G, nw - n0);
            __syncthreads();
            if (!one_round) { stage(n0, n); __syncthreads(); }
            if (MODE != 0) {
                if (tid < n) gs[tid] = p.DS[(size_t)pl[tid] * C + c];
                __syncthreads();
            }
            for (int q = 0; q < n; q++) {
                const v4f b4 = *(const v4f *)(be + q * SP + j0);
                const float *aq = al + q * SP;
                if (MODE == 0) {
                    float sum = 0.0f;
#pragma unroll
                    for (int k = 0; k < RPT; k++) {
                        const float av = aq[min(g + G * k, S - 1)];          // (rows past S hold zero blocks)
#pragma unroll
                        for (int e = 0; e < 4; e++) sum += fmaxf((a[k][e] * av) * b4[e], 0.0f);      // :119-122
                    }
                    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
                    if (lane == 0) red[wave * F4_G + q] = sum;
                } else if (MODE == 1) {
                    const float gq = gs[q];
                    const int buf = q & 1;
                    v4f db = {0.0f, 0.0f, 0.0f, 0.0f};
                    float da[RPT];
#pragma unroll
                    for (int k = 0; k < RPT; k++) {
                        const float av = aq[min(g + G * k, S - 1)];
                        float t = 0.0f;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float ga = (a[k][e] * av) * b4[e] > 0.0f ? gq * a[k][e] : 0.0f;
                            t = fmaf(ga, b4[e], t);
                            db[e] = fmaf(ga, av, db[e]);
                        }
                        da[k] = t;
                    }
                    // a row's chunks sit in CPR neighbouring lanes of one wavefront: lane lr = 0 ends with their sum
                    for (int o = 1; o < CPR; o <<= 1)
#pragma unroll
                        for (int k = 0; k < RPT; k++) {
                            const float v = __shfl_down(da[k], o, WAVE);
                            if (lr + o < CPR) da[k] += v;
                        }
                    if (active) {
                        if (lr == 0)
#pragma unroll
                            for (int k = 0; k < RPT; k++)
                                if (g + G * k < S) dal[buf * SP + g + G * k] = da[k];
                        *(v4f *)(dbl + buf * nbuf + (g * CPR + lr) * 4) = db;
                    }
                    __syncthreads();
                    if (tid < S) {                                // thread s owns d alpha[s] and d beta[s]: row groups in order
                        float y = 0.0f;
                        const float *src = dbl + buf * nbuf + tid;
                        for (int k = 0; k < G; k++) y += src[k * CPR * 4];
                        acc[(q * 2) * SP + tid] = dal[buf * SP + tid];
                        acc[(q * 2 + 1) * SP + tid] = y;
                    }
                } else {
                    const float gq = gs[q];
#pragma unroll
                    for (int k = 0; k < RPT; k++) {
                        const float av = aq[min(g + G * k, S - 1)];
                        const float ga = gq * av;
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if ((a[k][e] * av) * b4[e] > 0.0f) d[k][e] = fmaf(ga, b4[e], d[k][e]);
                    }
                }
            }
            if (MODE == 0) {
                __syncthreads();
                if (tid < n)
                    p.SC[(size_t)pl[tid] * C + c] = (red[tid] + red[F4_G + tid]) + (red[2 * F4_G + tid] + red[3 * F4_G + tid]);
            }
            if (MODE == 1) {                                      // this label's sums join the group's partial
                __syncthreads();
                for (int e = tid; e < n * 2 * S; e += F4_THREADS) {
                    const int r = e / S, s = e - r * S;           // r = 2 q + (0: d alpha, 1: d beta)
                    float *dst = p.part + (((size_t)(first + n0 + (r >> 1)) * p.ngrp + grp) * 2 + (r & 1)) * S + s;
                    const float v = acc[r * SP + s];
                    *dst = c == c0 ? v : *dst + v;
                }
            }
        }
        if (MODE == 2 && active) {
            float *ob = p.dT4 + ((size_t)w * C + c) * SS;
            const float *mb = p.dM + (size_t)w * SS;
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                const int s = g + G * k;
                if (s < S) f4_store(ob + (size_t)s * S + j0, j0, S, d[k] + f4_load(mb + (size_t)s * S + j0, j0, S));
            }
        }
    }
}

// GA[b][i] = d loss / d alpha_i, GB[b][len-1-i] = d loss / d beta_{i+1}: the label groups' partials added in group order, one
// workgroup per position of the bucket list; alpha_len feeds no score: its adjoint row is zero
__global__ void __launch_bounds__(128)
fst4_adj_reduce_kernel(const float *__restrict__ part, const int *__restrict__ list, const int *__restrict__ wstart,
                       const int *__restrict__ wcount, const int64_t *__restrict__ len, float *GA, float *GB, int V, int L,
                       int S, int ngrp) {
    const int k = blockIdx.x, t = threadIdx.x;
    if (k >= wstart[V - 1] + wcount[V - 1] || t >= S) return;
    const int pos = list[k], b = pos / L, i = pos - b * L, n = clamp_len(len[b], L);
    const float *src = part + (size_t)k * ngrp * 2 * S + t;
    float da = 0.0f, db = 0.0f;
    for (int g = 0; g < ngrp; g++) { da += src[(size_t)g * 2 * S]; db += src[(size_t)g * 2 * S + S]; }
    const size_t row0 = (size_t)b * (L + 1);
    GA[(row0 + i) * S + t] = da;
    GB[(row0 + n - 1 - i) * S + t] = db;
    if (i == n - 1) GA[(row0 + n) * S + t] = 0.0f;
    // GB row n (the adjoint of beta_0) is never written and the workspace is not cleared: beta_0 feeds no score, and nothing
    // reads that row only because onehot_train_chain_kernel<., true> walks the backward chain over t = 1 .. n-1 and
    // onehot_dT_kernel skips the backward term at i = 0.  A change to either must write the row here first.
}

// out[w] = sum_c src[w][c] (+ add), and its transpose: one 32 x 32 tile per workgroup of 256 threads; grid (words, tiles).
// present: only the words of the batch (wcount[w] > 0) are mixed -- the others' blocks are never gathered.
// First with src = W4 as one word (Wsum, no transpose), then with src = T4, add = Wsum: M[w] = T4[w].sum(0) + W4.sum(0) (:82)
__global__ void __launch_bounds__(256)
fst4_premix_kernel(const float *__restrict__ src, const float *__restrict__ add, const int *__restrict__ present,
                   float *__restrict__ M, float *__restrict__ MT, int S, int C) {
    __shared__ float tile[32][33];
    const int w = blockIdx.x;
    if (present && present[w] == 0) return;
    const int nt = (S + 31) >> 5, tt = blockIdx.y;
    const int r0 = (tt / nt) * 32, q0 = (tt % nt) * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t SS = (size_t)S * S, base = (size_t)w * SS;
    const float *sb = src + (size_t)w * C * SS;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = r0 + ty + 8 * k, q = q0 + tx;
        float v = 0.0f;
        if (r < S && q < S) {
            const float *e = sb + r * S + q;
            for (int c = 0; c < C; c++) v += e[(size_t)c * SS];
            if (add) v += add[r * S + q];
            M[base + r * S + q] = v;
        }
        tile[ty + 8 * k][tx] = v;
    }
    if (!MT) return;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = q0 + ty + 8 * k, r = r0 + tx;
        if (r < S && q < S) MT[base + q * S + r] = tile[tx][ty + 8 * k];
    }
}

__global__ void __launch_bounds__(256)
fst4_fill_kernel(float *dst, float v, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = v;
}

// The priority layer, the cross-entropy, the decode and d loss / d scores on given scores: what train_loss_kernel<., 0>
// (train.hip.h) does behind its own score product.  A wavefront per position; LDS: per wavefront sc[K], ds[K].
__global__ void __launch_bounds__(512)
fst4_loss_kernel(const float *__restrict__ SC, const float *__restrict__ P, const int64_t *__restrict__ len,
                 const int64_t *__restrict__ labels, int *err, float *DS, int32_t *tags, float *loss_part, int B, int L, int K,
                 int o_idx, float threshold, float inv_tokens) {
    extern __shared__ __align__(16) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    float *sc = sm + (size_t)w * 2 * K, *ds = sc + K;
    float loss_acc = 0.0f;
    for (long long pos = (long long)blockIdx.x * nw + w; pos < (long long)B * L; pos += (long long)gridDim.x * nw) {
        const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
        if (i >= clamp_len(len[b], L)) {
            if (lane == 0) tags[pos] = -1;
            continue;
        }
        for (int c = lane; c < K; c += WAVE) sc[c] = SC[pos * K + c];
        if (P) {                                                                       // priority layer (:124-125)
            for (int d = lane; d < K; d += WAVE) {
                float a = 0.0f;
                for (int c = 0; c < K; c++) a = fmaf(sc[c], P[(long long)c * K + d], a);
                ds[d] = a;
            }
            for (int d = lane; d < K; d += WAVE) sc[d] = ds[d];
        }
        float mx = -INFINITY;
        for (int c = lane; c < K; c += WAVE) mx = fmaxf(mx, sc[c]);
        for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
        float se = 0.0f;
        for (int c = lane; c < K; c += WAVE) se += expf(sc[c] - mx);
        for (int o = 32; o; o >>= 1) se += __shfl_xor(se, o, WAVE);
        // a label outside 0..K-1: counted as label 0 in the loss and in the gradient, reported through the sticky flag
        const long long lab64 = labels[pos];
        const int lab = (lab64 < 0 || lab64 >= K) ? 0 : (int)lab64;
        if (lane == 0 && lab64 != lab) atomicOr(err, 1);
        const float lse = mx + logf(se);
        loss_acc += lse - sc[lab];
        {
            float bv = -INFINITY; int bi = 0x7ffffffe;                                 // local_decode (:172-176)
            for (int c = lane; c < K; c += WAVE) {
                float vv = sc[c] + 0.0f;
                if (c == K - 1) vv = fminf(vv, threshold);
                if (vv > bv) { bv = vv; bi = c; }
            }
            bi = wave_argmax_dpp(bv, bi);
            if (lane == 0) tags[pos] = (bi >= K) ? 0 : (bi == K - 1 ? o_idx : bi);
        }
        for (int c = lane; c < K; c += WAVE) ds[c] = (expf(sc[c] - lse) - (c == lab ? 1.0f : 0.0f)) * inv_tokens;
        if (P) {                                                                       // back through scores . P
            for (int c = lane; c < K; c += WAVE) {
                float a = 0.0f;
                for (int d = 0; d < K; d++) a = fmaf(ds[d], P[(long long)c * K + d], a);
                sc[c] = a;
            }
            for (int c = lane; c < K; c += WAVE) ds[c] = sc[c];
        }
        for (int c = lane; c < K; c += WAVE) DS[pos * K + c] = ds[c];
    }
    if (lane == 0) loss_part[blockIdx.x * nw + w] = loss_acc * inv_tokens;
}

// dW4[c] = sum over the batch's words, in word order, of dT4[w][c] (the absent words' rows are zero)
__global__ void __launch_bounds__(256)
fst4_dW_kernel(const float *__restrict__ dT4, const int *__restrict__ wcount, float *__restrict__ dW4, int V, size_t CSS) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= CSS) return;
    float s = 0.0f;
    for (int w = 0; w < V; w++)
        if (wcount[w] > 0) s += dT4[(size_t)w * CSS + e];
    dW4[e] = s;
}

}  // namespace farnn
