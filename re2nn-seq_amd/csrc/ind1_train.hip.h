// Training step of the onehot independent=1 tagger (FARNN_S_O_I, --method onehot --independent 1): the CE1 loss and the
// gradient of language_tensor [V][S][S], the only tensor the reference trains (model_onehot.py:213-223).
//
// Reference: FARNN_S_O_I.forward_local(train=True) (model_onehot.py:184-306; sum semiring, CE1) followed by loss.backward()
// (train_onehot.py:156-206).  With N[w] = T[w] + W (:250), Osum = output_tensor.sum(0) (:252) and Mc[w] = N[w], or
// N[w] * Osum under args.independent == 2 (:260, :272):
//   chains   alpha_{i+1} = relu(alpha_i Mc[x_i]), alpha_0 = h0;  beta_i = relu(Mc[x_i] beta_{i+1}), beta_n = hT     (:256-279)
//   score_i[c] = sum_{s,j} O[c,s,j] alpha_i[s] beta_{i+1}[j] N[x_i][s,j] [. P]      (:229-233, :293-304; N, not Mc; no relu)
// The chains, their back-propagation through time and dMc[w] are the onehot i-FST step's kernels (onehot_train.hip.h) on
// the premixed Mc with a mask of ones and relu, exactly as the onehot FST's step (fst4_train.hip.h) runs them; the loss on
// given scores and the ordered reduction of the d alpha / d beta partials are that step's kernels too.  This header adds
// the premix of the batch's words, the scores from the stashed states and the backward of the scores.
//
// The score kernel (ind1_train_kernel) walks the positions in bucket (word) order like fst4_train_kernel: a workgroup takes
// one word and one group of label columns, keeps N[w] in registers for the whole run (16 bytes per lane along j, rows past S
// and the last partial chunk predicated), streams the O[c] blocks (shared by every workgroup: they stay in L2) and runs over
// the word's positions, staged in LDS I1_G at a time.  MODE 0 writes the scores; MODE 1 the contributions to d alpha_i and
// d beta_{i+1} as one partial per label group (fst4_adj_reduce_kernel adds the groups in order; there is no relu mask);
// MODE 2, after the chains' back-propagation, loops over ALL labels in one workgroup per word (grid (V, 1): the sum over the
// labels has one owner and the order c = 0 .. C-1), accumulating per label D_c = sum_pos dscore[pos,c] alpha beta^T and
// then dT[w] = sum_c O[c] * D_c + dMc[w] (* Osum), written once (zeros for an absent word).
// No float atomics: every sum has one owner and a fixed order, two steps on the same inputs are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"
#include "fst4_train.hip.h"

namespace farnn {

// __launch_bounds__(I1_THREADS): 4 wavefronts, one per SIMD, so a wavefront may use the whole 512-register file -- MODE 0 / 1
// hold N and N * O[c] (2 x 4 RPT registers, 128 at S = 128), MODE 2 the label's D_c and the running sum (the same count).
// LDS: ind1_train_lds_floats, 75.5 KiB at S = 128 (of 160 KiB per workgroup).
constexpr int I1_THREADS = 256;   // score kernels: 4 wavefronts
constexpr int I1_G = 32;          // positions staged per round

struct Ind1TrainParams {
    const float *T, *W, *O;          // [V][S][S], [S][S], [C][S][S]
    const float *A, *Bk;             // stash [B][L+1][S]
    const int64_t *len;
    const int *list, *wstart, *wcount;   // the positions bucketed by word
    float *SC;                       // [B L][C] scores before the priority layer (MODE 0)
    const float *DS;                 // [B L][C] d loss / d SC (MODE 1, 2)
    float *part;                     // [B L, bucket order][ngrp][2][S] (MODE 1)
    const float *dMc, *Osum;         // [V][S][S], [S][S] (MODE 2; Osum is read only with the mask)
    float *dT;                       // [V][S][S] (MODE 2)
    int L, S, SP, C, cpg, ngrp;      // SP = S rounded up to 4; label columns per group; groups (MODE 0, 1)
    int CPR, GW;                     // 16-byte chunks per row; rows a wavefront takes at a time (GW CPR <= 64 lanes)
    int mask;                        // args.independent == 2: Mc = N * Osum
};

// LDS floats of ind1_train_kernel (the layout of fst4_train_kernel): alpha, beta [I1_G][SP]; g, position [I1_G]; the
// wavefronts' score shares [4][I1_G]; MODE 1: two buffers of a position's d alpha [SP] and d beta shares [4 GW][4 CPR], and
// the chunk's sums [I1_G][2][SP].  Every carve offset is a multiple of 16 bytes (SP is a multiple of 4).
inline size_t ind1_train_lds_floats(int SP, int CPR, int GW) {
    return (size_t)2 * I1_G * SP + 2 * I1_G + 4 * I1_G + 2 * ((size_t)SP + 16 * (size_t)GW * CPR) + (size_t)2 * I1_G * SP;
}

// grid (V, ngrp) for MODE 0 and 1, (V, 1) for MODE 2.  RPT: register rows per thread (row s = g + 4 GW k, k < RPT, covers S).
template <int RPT, int MODE>
__global__ void __launch_bounds__(I1_THREADS)
ind1_train_kernel(const Ind1TrainParams p) {
    extern __shared__ __align__(16) float sm[];
    const int w = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int S = p.S, SP = p.SP, C = p.C, L = p.L, CPR = p.CPR;
    const int c0 = MODE == 2 ? 0 : grp * p.cpg, c1 = MODE == 2 ? C : min(C, c0 + p.cpg);
    const int nw = p.wcount[w], first = p.wstart[w];
    if (MODE != 2 && nw == 0) return;
    const int gw = lane / CPR, lr = lane - gw * CPR;
    const bool active = gw < p.GW;
    const int G = 4 * p.GW, g = wave * p.GW + (active ? gw : 0);
    const int j0 = 4 * lr;
    const size_t SS = (size_t)S * S;
    float *al = sm, *be = al + I1_G * SP, *gs = be + I1_G * SP;
    int *pl = (int *)(gs + I1_G);
    float *red = gs + 2 * I1_G;                                   // [4][I1_G]
    float *dal = red + 4 * I1_G, *dbl = dal + 2 * SP;             // [2][SP], [2][G][4 CPR]
    float *acc = dbl + 2 * 4 * G * CPR;                           // [I1_G][2][SP]
    const int nbuf = 4 * G * CPR;
    const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};

    if (MODE == 2 && nw == 0) {                                   // an absent word: its block is zero
        if (active)
            for (int s = g; s < S; s += G) f4_store(p.dT + (size_t)w * SS + (size_t)s * S + j0, j0, S, z);
        return;
    }
    // positions n0 .. n0 + n - 1 of the word: alpha_i, beta_{i+1} and the flat position
    auto stage = [&](int n0, int n) {
        for (int e = tid; e < n * SP; e += I1_THREADS) {
            const int q = e / SP, s = e - q * SP;
            const int pos = p.list[first + n0 + q];
            const int b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
            const size_t row0 = (size_t)b * (L + 1);
            al[e] = s < S ? p.A[(row0 + i) * S + s] : 0.0f;
            be[e] = s < S ? p.Bk[(row0 + len - 1 - i) * S + s] : 0.0f;
            if (s == 0) pl[q] = pos;
        }
    };
    const bool one_round = nw <= I1_G;
    if (one_round) stage(0, nw);                                  // (the barrier at the top of the first round follows)

    // MODE 0, 1: nt = N[w], kept for the whole run; MODE 2: the running sum_c O[c] * D_c
    v4f nt[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int s = g + G * k;
        nt[k] = z;
        if (MODE != 2 && active && s < S)
            nt[k] = f4_load(p.T + (size_t)w * SS + (size_t)s * S + j0, j0, S) + f4_load(p.W + (size_t)s * S + j0, j0, S);   // :250
    }

    for (int c = c0; c < c1; c++) {
        const float *ob = p.O + (size_t)c * SS;
        v4f a[RPT];                                               // MODE 0, 1: N[w] * O[c]; MODE 2: D_c
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int s = g + G * k;
            a[k] = z;
            if (MODE != 2 && active && s < S) a[k] = nt[k] * f4_load(ob + (size_t)s * S + j0, j0, S);
        }
        for (int n0 = 0; n0 < nw; n0 += I1_G) {
            const int n = min(I1_G, nw - n0);
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
                        for (int e = 0; e < 4; e++) sum = fmaf(a[k][e] * av, b4[e], sum);            // :230-232, no relu
                    }
                    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
                    if (lane == 0) red[wave * I1_G + q] = sum;
                } else if (MODE == 1) {
                    const float gq = gs[q];
                    const int buf = q & 1;
                    v4f db = z;
                    float da[RPT];
#pragma unroll
                    for (int k = 0; k < RPT; k++) {
                        const float av = aq[min(g + G * k, S - 1)];
                        float t = 0.0f;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float ga = gq * a[k][e];
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
                        const float ga = gq * aq[min(g + G * k, S - 1)];
#pragma unroll
                        for (int e = 0; e < 4; e++) a[k][e] = fmaf(ga, b4[e], a[k][e]);
                    }
                }
            }
            if (MODE == 0) {
                __syncthreads();
                if (tid < n)
                    p.SC[(size_t)pl[tid] * C + c] = (red[tid] + red[I1_G + tid]) + (red[2 * I1_G + tid] + red[3 * I1_G + tid]);
            }
            if (MODE == 1) {                                      // this label's sums join the group's partial
                __syncthreads();
                for (int e = tid; e < n * 2 * S; e += I1_THREADS) {
                    const int r = e / S, s = e - r * S;           // r = 2 q + (0: d alpha, 1: d beta)
                    float *dst = p.part + (((size_t)(first + n0 + (r >> 1)) * p.ngrp + grp) * 2 + (r & 1)) * S + s;
                    const float v = acc[r * SP + s];
                    *dst = c == c0 ? v : *dst + v;
                }
            }
        }
        if (MODE == 2) {                                          // labels in order: the sum over c has this one owner
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                const int s = g + G * k;
                if (active && s < S) {
                    const v4f o4 = f4_load(ob + (size_t)s * S + j0, j0, S);
#pragma unroll
                    for (int e = 0; e < 4; e++) nt[k][e] = fmaf(o4[e], a[k][e], nt[k][e]);
                }
            }
        }
    }
    if (MODE == 2 && active) {
        float *out = p.dT + (size_t)w * SS;
        const float *mb = p.dMc + (size_t)w * SS;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int s = g + G * k;
            if (s < S) {
                v4f dm = f4_load(mb + (size_t)s * S + j0, j0, S);
                if (p.mask) dm = dm * f4_load(p.Osum + (size_t)s * S + j0, j0, S);     // Mc = N * Osum (:260)
                f4_store(out + (size_t)s * S + j0, j0, S, nt[k] + dm);
            }
        }
    }
}

// Mc[w] = T[w] + W (* Osum with the mask: :250, :260) and its transpose for the words of the batch only (present[w] > 0: the
// blocks of the other words are never read by the chains); one 32 x 32 tile per workgroup of 256 threads; grid (V, tiles)
__global__ void __launch_bounds__(256)
ind1_premix_kernel(const float *__restrict__ T, const float *__restrict__ W, const float *__restrict__ Osum,
                   const int *__restrict__ present, float *__restrict__ M, float *__restrict__ MT, int S) {
    __shared__ float tile[32][33];
    const int w = blockIdx.x;
    if (present[w] == 0) return;
    const int nt = (S + 31) >> 5, tt = blockIdx.y;
    const int r0 = (tt / nt) * 32, q0 = (tt % nt) * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t base = (size_t)w * S * S;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = r0 + ty + 8 * k, q = q0 + tx;
        float v = 0.0f;
        if (r < S && q < S) {
            v = T[base + r * S + q] + W[r * S + q];
            if (Osum) v *= Osum[r * S + q];
            M[base + r * S + q] = v;
        }
        tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = q0 + ty + 8 * k, r = r0 + tx;
        if (r < S && q < S) MT[base + q * S + r] = tile[tx][ty + 8 * k];
    }
}

}  // namespace farnn
