// Training step of the decomposed independent=1 tagger (FARNN_S_D_W_I, --method decompose --independent 1): the CE1 loss and
// the gradients of S1, S2, Vgen, wildcard_mat, C_output, S1_output, S2_output, h0 and hT.
//
// Reference: FARNN_S_D_W_I.forward_local(train=True) (model_decompose_independent.py:148-300; farnn = 0, sum semiring, CE1)
// followed by loss.backward() (train_decompose.py:161-221).  With v = Vgen[w] (model_decompose.py:222-241):
//   N[w][i][j] = sum_r v_r S1[i,r] S2[j,r] + wildcard_mat[i,j]                                              (:171-173)
//   Osum[i][j] = sum_r (sum_c C_output[c,r]) S1_output[i,r] S2_output[j,r]     (:210-214: einsum 'sr,jr->js' of S2_output
//                                                     [s,r] and csum_r S1_output[j,r] -- the FIRST index is S1_output's)
//   Mc[w] = N[w] * Osum                                                                                      (:174)
//   chains   alpha_{t+1} = nl(alpha_t Mc[x_t]), alpha_0 = h0;  beta_t = nl(Mc[x_t] beta_{t+1}), beta_n = hT  (:176-188, :239-252)
//   br_i[r] = sum_{ij} alpha_i[i] beta_{i+1}[j] N[x_i][i,j] S1_output[i,r] S2_output[j,r];  score_i = br_i C_output^T [. P]
//                                                                                                            (:199-208, :260-278)
// Everything the chains need is the onehot steps' code on the premixed Mc with a mask of ones and the model's nl
// (onehot_train.hip.h: chains, BPTT, bucketing, per-word dMc); the loss on given scores and the ordered adjoint reduction are
// fst4_train.hip.h's.  The scores are taken in FACTOR SPACE through ind1_train_kernel (ind1_train.hip.h): with
// Ofac[r] = S1_output[:,r] S2_output[:,r]^T materialised once per step ([R_O][S][S], smaller than O[c] = sum_r C[c,r] Ofac[r]
// whenever R_O < C), its MODE 0 with Ofac in output_tensor's place writes br [B L][R_O] and its MODE 1 the d alpha / d beta
// partials from d br = d score C_output; score = br C_output^T, d br and the score path of dC_output are small products.
// This header adds what makes the model decomposed:
//   decomp1_outer_kernel    Kfac[r] = S1[:,r] S2[:,r]^T and Ofac[r], once per step
//   decomp1_gemm_kernel     one ordered float32 product C = A B (+ a row vector) with free strides: N = Vgen Kfac + W for the
//                           batch's words, dVgen = dN Kfac^T, E[r] = sum_w Vgen[w,r] dN[w] (words in id order), score, d br,
//                           dC_output.  A 64 x 64 tile per workgroup, k ascending: every output element has one owner.
//   decomp1_back_kernel     per word (bucket order, N-sized register tiles as ind1_train_kernel's MODE 2): F_r = sum_pos d br[pos,r]
//                           alpha beta^T per output rank r, dN[w] = sum_r Ofac[r] * F_r + dMc[w] * Osum, and the word's share
//                           of dS1_output[:,r] / dS2_output[:,r] (the row / column sums of N[w] * F_r against the other factor)
//                           as one partial per word: [V][R_O][2][S], never [words][C][S][S]
//   decomp1_word_sum_kernel dW = sum_w dN[w], dOsum = sum_w dMc[w] * N[w], the batch's words in id order
//   decomp1_out_factors_kernel  dS1_output, dS2_output (the words' partials in id order + the Osum path) and dcsum
//   decomp1_in_factors_kernel   dS1[i,r] = sum_j E[r][i,j] S2[j,r], dS2 likewise
//   decomp1_init_adj_kernel / _sum_kernel   dh0, dhT: the score adjoint of row 0 plus what BPTT's first step carries into it
//                           (onehot_train_chain_kernel<., true> stops at step 1: its UF / DQ row 1 is read here), sequences in order
// No float atomics: every sum has one owner and a fixed order, two steps on the same inputs are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"
#include "fst4_train.hip.h"
#include "ind1_train.hip.h"

namespace farnn {

// out[r][i][j] = A[i][r] B[j][r]  (A, B: [S][R] row-major); one element per thread
__global__ void __launch_bounds__(256)
decomp1_outer_kernel(const float *__restrict__ A, const float *__restrict__ Bm, float *__restrict__ out, int S, int R) {
    const size_t SS = (size_t)S * S, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= SS * R) return;
    const int r = (int)(e / SS), ij = (int)(e - (size_t)r * SS), i = ij / S, j = ij - i * S;
    out[e] = A[(size_t)i * R + r] * Bm[(size_t)j * R + r];
}

// csum[r] = sum_c C_output[c][r] (:211), labels in order
__global__ void __launch_bounds__(256)
decomp1_csum_kernel(const float *__restrict__ Cout, float *__restrict__ csum, int C, int RO) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= RO) return;
    float s = 0.0f;
    for (int c = 0; c < C; c++) s += Cout[(size_t)c * RO + r];
    csum[r] = s;
}

// Osum[e] = sum_r csum[r] Ofac[r][e] (:212-214), ranks in order
__global__ void __launch_bounds__(256)
decomp1_osum_kernel(const float *__restrict__ csum, const float *__restrict__ Ofac, float *__restrict__ Osum, int SS, int RO) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= SS) return;
    float s = 0.0f;
    for (int r = 0; r < RO; r++) s = fmaf(csum[r], Ofac[(size_t)r * SS + e], s);
    Osum[e] = s;
}

// C[m][n] = sum_{k < K} A[m am + k ak] B[k bk + n bn] (+ add[n]), k ascending: a 64 x 64 tile per workgroup of 256 threads,
// a 4 x 4 block per thread, 16 k at a time through LDS.  rows: when given, a row m with rows[m] == 0 reads A as zero (its
// output is add[n] or zero: the words absent from the batch).  grid (ceil(M / 64), ceil(N / 64)): M, the side
// that grows with the batch, along x.
struct D1Gemm {
    const float *A, *Bm, *add;
    const int *rows;
    float *Cm;
    int M, N, K;
    size_t am, ak, bk, bn, ldc;
};
constexpr int D1_TM = 64, D1_TK = 16;

__global__ void __launch_bounds__(256)
decomp1_gemm_kernel(const D1Gemm g) {
    __shared__ __align__(16) float As[D1_TK][D1_TM + 4];
    __shared__ __align__(16) float Bs[D1_TK][D1_TM + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * D1_TM, n0 = blockIdx.y * D1_TM;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.0f;
    // the staging walk follows the operand's unit stride: along the tile's 64 rows / columns, or along k
    const bool a_mfast = g.am <= g.ak, b_nfast = g.bn <= g.bk;
    for (int k0 = 0; k0 < g.K; k0 += D1_TK) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = tid + 256 * u;
            {
                const int mm = a_mfast ? (idx & 63) : (idx >> 4), kk = a_mfast ? (idx >> 6) : (idx & 15);
                const int m = m0 + mm, k = k0 + kk;
                float v = 0.0f;
                if (m < g.M && k < g.K && (!g.rows || g.rows[m] != 0)) v = g.A[(size_t)m * g.am + (size_t)k * g.ak];
                As[kk][mm] = v;
            }
            {
                const int nn = b_nfast ? (idx & 63) : (idx >> 4), kk = b_nfast ? (idx >> 6) : (idx & 15);
                const int n = n0 + nn, k = k0 + kk;
                float v = 0.0f;
                if (n < g.N && k < g.K) v = g.Bm[(size_t)k * g.bk + (size_t)n * g.bn];
                Bs[kk][nn] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < D1_TK; kk++) {
            const v4f a4 = *(const v4f *)&As[kk][4 * ty], b4 = *(const v4f *)&Bs[kk][4 * tx];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] = fmaf(a4[a], b4[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int m = m0 + 4 * ty + a;
        if (m >= g.M) continue;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int n = n0 + 4 * tx + b;
            if (n < g.N) g.Cm[(size_t)m * g.ldc + n] = acc[a][b] + (g.add ? g.add[n] : 0.0f);
        }
    }
}

struct D1BackParams {
    const float *N, *Ofac, *S1o, *S2o;   // [V][S][S], [RO][S][S], [S][RO], [S][RO]
    const float *A, *Bk;                 // stash [B][L+1][S]
    const int64_t *len;
    const int *list, *wstart, *wcount;   // the positions bucketed by word
    const float *DBR;                    // [B L][RO] d loss / d br
    const float *dMc, *Osum;             // [V][S][S], [S][S]
    float *dN;                           // [V][S][S] (zero for an absent word)
    float *fpart;                        // [V][RO][2][S]: the word's share of dS1_output[:,r], dS2_output[:,r] (present words only)
    int L, S, SP, RO, CPR, GW;           // as Ind1TrainParams
};

// grid (V); the thread layout, the staging and the LDS carve of ind1_train_kernel (ind1_train_lds_floats).  Registers: the
// running dN and F_r (2 x 4 RPT, 128 at S = 128) as its MODE 2.
template <int RPT>
__global__ void __launch_bounds__(I1_THREADS)
decomp1_back_kernel(const D1BackParams p) {
    extern __shared__ __align__(16) float sm[];
    const int w = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int S = p.S, SP = p.SP, RO = p.RO, L = p.L, CPR = p.CPR;
    const int nw = p.wcount[w], first = p.wstart[w];
    const int gw = lane / CPR, lr = lane - gw * CPR;
    const bool active = gw < p.GW;
    const int G = 4 * p.GW, g = wave * p.GW + (active ? gw : 0);
    const int j0 = 4 * lr;
    const size_t SS = (size_t)S * S;
    float *al = sm, *be = al + I1_G * SP, *gs = be + I1_G * SP;
    int *pl = (int *)(gs + I1_G);
    float *dal = gs + 2 * I1_G + 4 * I1_G, *dbl = dal + 2 * SP;      // [SP], [G][4 CPR] (the first of ind1's two buffers)
    const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};

    if (nw == 0) {                                                // an absent word: its block is zero
        if (active)
            for (int s = g; s < S; s += G) f4_store(p.dN + (size_t)w * SS + (size_t)s * S + j0, j0, S, z);
        return;
    }
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

    v4f nt[RPT];                                                  // the running sum_r Ofac[r] * F_r
#pragma unroll
    for (int k = 0; k < RPT; k++) nt[k] = z;
    const float *nb = p.N + (size_t)w * SS;

    for (int r = 0; r < RO; r++) {
        v4f a[RPT];                                               // F_r
#pragma unroll
        for (int k = 0; k < RPT; k++) a[k] = z;
        for (int n0 = 0; n0 < nw; n0 += I1_G) {
            const int n = min(I1_G, nw - n0);
            __syncthreads();
            if (!one_round) { stage(n0, n); __syncthreads(); }
            if (tid < n) gs[tid] = p.DBR[(size_t)pl[tid] * RO + r];
            __syncthreads();
            for (int q = 0; q < n; q++) {
                const v4f b4 = *(const v4f *)(be + q * SP + j0);
                const float *aq = al + q * SP;
                const float gq = gs[q];
#pragma unroll
                for (int k = 0; k < RPT; k++) {
                    const float ga = gq * aq[min(g + G * k, S - 1)];
#pragma unroll
                    for (int e = 0; e < 4; e++) a[k][e] = fmaf(ga, b4[e], a[k][e]);
                }
            }
        }
        // dN += Ofac[r] * F_r; with P = N[w] * F_r: u1[i] = sum_j P_ij S2_output[j,r], u2[j] = sum_i P_ij S1_output[i,r]
        const float *ob = p.Ofac + (size_t)r * SS;
        v4f s2 = z;
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (active && j0 + e < S) s2[e] = p.S2o[(size_t)(j0 + e) * RO + r];
        v4f db = z;
        float da[RPT];
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int s = g + G * k;
            da[k] = 0.0f;
            if (active && s < S) {
                const v4f o4 = f4_load(ob + (size_t)s * S + j0, j0, S);
                const v4f pn = f4_load(nb + (size_t)s * S + j0, j0, S) * a[k];
                const float s1 = p.S1o[(size_t)s * RO + r];
                float t = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    nt[k][e] = fmaf(o4[e], a[k][e], nt[k][e]);
                    t = fmaf(pn[e], s2[e], t);
                    db[e] = fmaf(pn[e], s1, db[e]);
                }
                da[k] = t;
            }
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
                    if (g + G * k < S) dal[g + G * k] = da[k];
            *(v4f *)(dbl + (g * CPR + lr) * 4) = db;
        }
        __syncthreads();
        if (tid < S) {                                            // thread s owns u1[s] and u2[s]: row groups in order
            float y = 0.0f;
            const float *src = dbl + tid;
            for (int k = 0; k < G; k++) y += src[k * CPR * 4];
            float *dst = p.fpart + ((size_t)w * RO + r) * 2 * S;
            dst[tid] = dal[tid];
            dst[S + tid] = y;
        }
        // (dal / dbl are written again only behind the barriers of the next rank's first round)
    }
    if (active) {
        float *out = p.dN + (size_t)w * SS;
        const float *mb = p.dMc + (size_t)w * SS;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int s = g + G * k;
            if (s < S) {
                const v4f dm = f4_load(mb + (size_t)s * S + j0, j0, S) * f4_load(p.Osum + (size_t)s * S + j0, j0, S);   // Mc = N * Osum (:174)
                f4_store(out + (size_t)s * S + j0, j0, S, nt[k] + dm);
            }
        }
    }
}

// dW[e] = sum_w dN[w][e] and dOsum[e] = sum_w dMc[w][e] N[w][e] over the batch's words in id order
__global__ void __launch_bounds__(256)
decomp1_word_sum_kernel(const float *__restrict__ dN, const float *__restrict__ dMc, const float *__restrict__ Nw,
                        const int *__restrict__ wcount, float *dW, float *__restrict__ dOsum, int V, size_t SS) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= SS) return;
    float sw = 0.0f, so = 0.0f;
    for (int w = 0; w < V; w++)
        if (wcount[w] > 0) {
            sw += dN[(size_t)w * SS + e];
            so = fmaf(dMc[(size_t)w * SS + e], Nw[(size_t)w * SS + e], so);
        }
    if (dW) dW[e] = sw;
    dOsum[e] = so;
}

// One workgroup per output rank r, thread t < S.  Score path: the words' partials in id order.  Osum path (Osum =
// sum_r csum_r S1_output[:,r] S2_output[:,r]^T): dS1_output[t,r] += csum_r sum_j dOsum[t,j] S2_output[j,r], dS2_output[t,r] +=
// csum_r sum_i dOsum[i,t] S1_output[i,r], dcsum[r] = sum_i S1_output[i,r] sum_j dOsum[i,j] S2_output[j,r] (rows in order).
__global__ void __launch_bounds__(128)
decomp1_out_factors_kernel(const float *__restrict__ fpart, const int *__restrict__ wcount, const float *__restrict__ dOsum,
                           const float *__restrict__ S1o, const float *__restrict__ S2o, const float *__restrict__ csum,
                           float *dS1o, float *dS2o, float *dcsum, int V, int S, int RO) {
    __shared__ float rows[OT_MAX_S];
    const int r = blockIdx.x, t = threadIdx.x;
    float u1 = 0.0f, u2 = 0.0f, rs = 0.0f, cs = 0.0f;
    if (t < S) {
        for (int w = 0; w < V; w++)
            if (wcount[w] > 0) {
                const float *src = fpart + ((size_t)w * RO + r) * 2 * S;
                u1 += src[t];
                u2 += src[S + t];
            }
        for (int j = 0; j < S; j++) {
            rs = fmaf(dOsum[(size_t)t * S + j], S2o[(size_t)j * RO + r], rs);
            cs = fmaf(dOsum[(size_t)j * S + t], S1o[(size_t)j * RO + r], cs);
        }
        const float c = csum[r];
        if (dS1o) dS1o[(size_t)t * RO + r] = fmaf(c, rs, u1);
        if (dS2o) dS2o[(size_t)t * RO + r] = fmaf(c, cs, u2);
        rows[t] = rs * S1o[(size_t)t * RO + r];
    }
    __syncthreads();
    if (t == 0) {
        float s = 0.0f;
        for (int i = 0; i < S; i++) s += rows[i];
        dcsum[r] = s;
    }
}

// One workgroup per rank r, thread t < S: dS1[t,r] = sum_j E[r][t,j] S2[j,r], dS2[t,r] = sum_i E[r][i,t] S1[i,r]
__global__ void __launch_bounds__(128)
decomp1_in_factors_kernel(const float *__restrict__ E, const float *__restrict__ S1, const float *__restrict__ S2,
                          float *__restrict__ dS1, float *__restrict__ dS2, int S, int R) {
    const int r = blockIdx.x, t = threadIdx.x;
    if (t >= S) return;
    const float *e = E + (size_t)r * S * S;
    float a = 0.0f, b = 0.0f;
    for (int j = 0; j < S; j++) {
        a = fmaf(e[(size_t)t * S + j], S2[(size_t)j * R + r], a);
        b = fmaf(e[(size_t)j * S + t], S1[(size_t)j * R + r], b);
    }
    dS1[(size_t)t * R + r] = a;
    dS2[(size_t)t * R + r] = b;
}

// HP[b][0][s] = d loss / d h0 from sequence b: GA row 0 (the score of position 0) + sum_j UF[b][1][j] Mc[x_0][s][j] (p_1 = h0
// Mc[x_0]); HP[b][1][s] = d loss / d hT: GB row 0 (the score of the last position) + sum_j DQ[b][1][j] Mc[x_{n-1}][j][s]
// (q_1 = Mc[x_{n-1}] hT; the backward chain has n - 1 steps).  Zero for an empty sequence.  grid (B), thread s < S.
__global__ void __launch_bounds__(128)
decomp1_init_adj_kernel(const OhTrainParams p, float *__restrict__ HP) {
    const int b = blockIdx.x, s = threadIdx.x, S = p.S, L = p.L;
    if (s >= S) return;
    const int n = clamp_len(p.len[b], L);
    const size_t row0 = (size_t)b * (L + 1), SS = (size_t)S * S;
    float d0 = 0.0f, dT = 0.0f;
    if (n > 0) {
        const float *m0 = p.M + (size_t)oh_token(p.x, p.V, (long long)b * L) * SS + (size_t)s * S;
        const float *u = p.UF + (row0 + 1) * S;
        for (int j = 0; j < S; j++) d0 = fmaf(u[j], m0[j], d0);
        d0 += p.GA[row0 * S + s];
        if (n > 1) {
            const float *mt = p.MT + (size_t)oh_token(p.x, p.V, (long long)b * L + n - 1) * SS + (size_t)s * S;
            const float *dq = p.DQ + (row0 + 1) * S;
            for (int j = 0; j < S; j++) dT = fmaf(dq[j], mt[j], dT);
        }
        dT += p.GB[row0 * S + s];
    }
    HP[((size_t)b * 2) * S + s] = d0;
    HP[((size_t)b * 2 + 1) * S + s] = dT;
}

// dh0[s] = sum_b HP[b][0][s], dhT[s] = sum_b HP[b][1][s], sequences in order; one workgroup, thread s < S
__global__ void __launch_bounds__(128)
decomp1_init_sum_kernel(const float *__restrict__ HP, float *dh0, float *dhT, int B, int S) {
    const int s = threadIdx.x;
    if (s >= S) return;
    float a = 0.0f, c = 0.0f;
    for (int b = 0; b < B; b++) { a += HP[((size_t)b * 2) * S + s]; c += HP[((size_t)b * 2 + 1) * S + s]; }
    if (dh0) dh0[s] = a;
    if (dhT) dhT[s] = c;
}

}  // namespace farnn
