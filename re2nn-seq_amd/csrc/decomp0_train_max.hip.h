// Training step of the decomposed FST tagger (FARNN_S_D_W) in the max semiring (--train_mode max): what the
// step adds to the decomposed i-FST's max chains (train_max.hip.h) so that two steps stay bit-identical.
//
// Reference: FARNN_S_D_W.get_forward_score with train_mode = 'max' (model_decompose.py:269-276) and utils._maxmul
// (utils.py:192-195).  Only the two recurrences go through _maxmul; the score head, the priority layer, the CE1 / CRF loss and
// the decode stay sum-times (decomp0_train.hip.h, unchanged).  With _R = Rtab[w] = Vgen[w] * C_embed.sum(0) (:253):
//   Tr_w = S2 . (_R o S1) + W          (:270-272) -- tmax_premix_kernel's association on (Rtab, S1, S2, W)
//   forward chain  n[s] = max_j hbar[j] Tr_w[j, s],   backward chain  n[s] = max_j hbar[j] Tr_w[s, j]       (:274, :276)
// The chains (tmax_slots / premix / forward), their back-propagation (tmax_backward_kernel's DET form: no float atomics) and
// the per-word dM_w (tmax_dM_kernel) are train_max.hip.h's.  This header adds the weight gradients from dM without atomics.
// With v_w = Rtab[w] over the batch's distinct words in slot (vocabulary) order:
//   X_w = dM_w S2,  Y_w = dM_w^T S1                         [S][R] each, on v_mfma_f32_16x16x4_f32
//   dS1[j, r] = sum_w v_w[r] X_w[j, r]      dS2[s, r] = sum_w v_w[r] Y_w[s, r]
//   dRtab[w, r] = sum_j S1[j, r] X_w[j, r]  dW = sum_w dM_w
//   d0max_wgrad_kernel   a chunk of D0M_WCH words and a block of D0M_RB ranks per workgroup: the chunk's partial sums of dS1, dS2
//                        and dW (words ascending) and the rows of dRtab of its words
//   d0max_reduce_kernel  the chunks' partial sums added in chunk order
// A chunk's boundaries depend on the word count and D0M_WCH only; every element has one owner and a fixed addition order.
#pragma once
#include "common.hip.h"
#include "train_max.hip.h"
#include "decomp0_train.hip.h"

namespace farnn {

constexpr int D0M_WCH = 16;         // distinct words per chunk
constexpr int D0M_RB = 64;          // ranks per workgroup: one block of 16 MFMA columns per wavefront
static_assert(D0M_RB == 16 * D0_WAVES, "d0_mma gives every wavefront one block of 16 columns");

struct D0MaxWgrad {
    const float *dM;                // [slots][S][S]
    const float *S1, *S2, *Rtab;    // [S][R] x2, [V][R]
    const int *wlist, *nwords;      // word of every slot, their count
    float *PS1, *PS2, *PW;          // [chunks][S][R] x2, [chunks][S][S]
    float *dRt;                     // [V][R]: the rows of the batch's words (decomp0_word_sum_kernel<true> zeroes the others)
    int S, R;
};

// chunks of a batch with at most nwmax distinct words
inline size_t d0max_chunks(size_t nwmax) { return (nwmax + D0M_WCH - 1) / D0M_WCH; }
inline size_t d0max_partial_floats(size_t nwmax, size_t S, size_t R) { return d0max_chunks(nwmax) * (2 * S * R + S * S); }
// LDS floats: the S1 and S2 panels [D0M_RB][d0_pad(S)] (rank major: the MFMA B operand's 16 columns x 4 k fall into 64 banks),
// the row and the column tile of dM_w and the dW tile [16][d0_pad(S)], v and dRtab of the chunk's words [D0M_WCH][D0M_RB]
inline size_t d0max_wgrad_lds_bytes(size_t S) {
    return ((2 * D0M_RB + 3 * D0_TP) * (size_t)d0_pad((int)S) + 2 * D0M_WCH * D0M_RB) * sizeof(float);
}

// grid (chunks, ceil(R / D0M_RB)).  A tile is 16 rows of X_w and Y_w: rows t0 .. t0 + 15 of dM_w against S2, columns t0 .. t0 + 15
// against S1.  Tiles outside, the chunk's words inside: a lane keeps its 4 + 4 elements of the partial sums in registers over
// the words and stores them once.  The rank block 0 also sums the row tiles into the chunk's share of dW.
__global__ void __launch_bounds__(D0_THREADS)
d0max_wgrad_kernel(const D0MaxWgrad p) {
    extern __shared__ __align__(16) float smem[];
    const int S = p.S, R = p.R, SP = d0_pad(S), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, r0 = blockIdx.y * D0M_RB, nw = *p.nwords;
    const int w0 = chunk * D0M_WCH;
    if (w0 >= nw) return;                                       // (uniform: the whole workgroup leaves)
    const int nk = min(D0M_WCH, nw - w0);
    float *P1 = smem, *P2 = P1 + D0M_RB * SP, *A1 = P2 + D0M_RB * SP, *A2 = A1 + D0_TP * SP, *DW = A2 + D0_TP * SP;
    float *vv = DW + D0_TP * SP, *dv = vv + D0M_WCH * D0M_RB;
    const bool dwo = blockIdx.y == 0;
    const size_t SS = (size_t)S * S, SR = (size_t)S * R;
    for (int e = tid; e < D0M_RB * SP; e += D0_THREADS) {       // (global reads along the rank; zero behind S and behind R)
        const int k = e / D0M_RB, n = e - k * D0M_RB;
        const bool ok = k < S && r0 + n < R;
        P1[n * SP + k] = ok ? p.S1[(size_t)k * R + r0 + n] : 0.0f;
        P2[n * SP + k] = ok ? p.S2[(size_t)k * R + r0 + n] : 0.0f;
    }
    for (int e = tid; e < D0M_WCH * D0M_RB; e += D0_THREADS) {
        const int k = e / D0M_RB, n = e - k * D0M_RB;
        vv[e] = (k < nk && r0 + n < R) ? p.Rtab[(size_t)p.wlist[w0 + k] * R + r0 + n] : 0.0f;
        dv[e] = 0.0f;
    }
    __syncthreads();
    const int lr = lane & 15, lk = lane >> 4, n = wave * 16 + lr;          // the lane's column of the rank block, rows lk * 4 ..
    for (int t0 = 0; t0 < S; t0 += D0_TP) {
        float acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float s1r[4];                                           // S1 at the lane's elements of X
#pragma unroll
        for (int i = 0; i < 4; i++) { const int j = t0 + lk * 4 + i; s1r[i] = j < S ? P1[n * SP + j] : 0.0f; }
        for (int k = 0; k < nk; k++) {
            __syncthreads();                                    // the last word's tiles are consumed
            const float *D = p.dM + (size_t)(w0 + k) * SS;
            for (int e = tid; e < D0_TP * SP; e += D0_THREADS) {          // rows t0 .. of dM_w
                const int m = e / SP, j = e - m * SP;
                A1[e] = (t0 + m < S && j < S) ? D[(size_t)(t0 + m) * S + j] : 0.0f;
            }
            for (int e = tid; e < D0_TP * SP; e += D0_THREADS) {          // columns t0 .. of dM_w, transposed
                const int j = e / D0_TP, m = e - j * D0_TP;
                A2[m * SP + j] = (t0 + m < S && j < S) ? D[(size_t)j * S + t0 + m] : 0.0f;
            }
            __syncthreads();
            const float v = vv[k * D0M_RB + n];
            float x[4];
            // X = dM_w S2: rows t0 .., this rank block
            d0_mma(A1, SP, P2, 1, SP, S, nullptr, 0, nullptr, 0, 0, 0, D0M_RB, wave, lane, [&](int m, int, float a) { x[m & 3] = a; });
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) { acc1[i] = fmaf(v, x[i], acc1[i]); d = fmaf(s1r[i], x[i], d); }
            // dRtab[w, r]: the tile's 16 rows -- the lane's four, then the four lanes of the column, a fixed tree
            d += __shfl_xor(d, 16, WAVE);
            d += __shfl_xor(d, 32, WAVE);
            if (lk == 0) dv[k * D0M_RB + n] += d;               // (one owner; tiles ascending)
            // Y = dM_w^T S1
            d0_mma(A2, SP, P1, 1, SP, S, nullptr, 0, nullptr, 0, 0, 0, D0M_RB, wave, lane, [&](int m, int, float a) { x[m & 3] = a; });
#pragma unroll
            for (int i = 0; i < 4; i++) acc2[i] = fmaf(v, x[i], acc2[i]);
            if (dwo)                                            // (element e has one owner over the words)
                for (int e = tid; e < D0_TP * SP; e += D0_THREADS) DW[e] = k ? DW[e] + A1[e] : A1[e];
        }
        if (r0 + n < R) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int j = t0 + lk * 4 + i;
                if (j < S) {
                    p.PS1[(size_t)chunk * SR + (size_t)j * R + r0 + n] = acc1[i];
                    p.PS2[(size_t)chunk * SR + (size_t)j * R + r0 + n] = acc2[i];
                }
            }
        }
        if (dwo)
            for (int e = tid; e < D0_TP * SP; e += D0_THREADS) {
                const int m = e / SP, j = e - m * SP;
                if (t0 + m < S && j < S) p.PW[(size_t)chunk * SS + (size_t)(t0 + m) * S + j] = DW[e];
            }
    }
    __syncthreads();
    for (int e = tid; e < nk * D0M_RB; e += D0_THREADS) {
        const int k = e / D0M_RB, c = e - k * D0M_RB;
        if (r0 + c < R) p.dRt[(size_t)p.wlist[w0 + k] * R + r0 + c] = dv[e];
    }
}

// dS1, dS2 [S][R] and dW [S][S]: the chunks' shares in chunk order, one thread per element
__global__ void __launch_bounds__(256)
d0max_reduce_kernel(const float *__restrict__ PS1, const float *__restrict__ PS2, const float *__restrict__ PW,
                    const int *__restrict__ nwords, float *__restrict__ dS1, float *__restrict__ dS2, float *__restrict__ dW,
                    size_t SR, size_t SS) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int nch = (*nwords + D0M_WCH - 1) / D0M_WCH;
    if (e < SR) {
        float a = 0.0f, b = 0.0f;
        for (int c = 0; c < nch; c++) { a += PS1[(size_t)c * SR + e]; b += PS2[(size_t)c * SR + e]; }
        dS1[e] = a; dS2[e] = b;
    }
    if (e < SS) {
        float a = 0.0f;
        for (int c = 0; c < nch; c++) a += PW[(size_t)c * SS + e];
        dW[e] = a;
    }
}

}  // namespace farnn
