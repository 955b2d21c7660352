// The gated recurrences (--farnn 1 | 2) of the decomposed independent=1 training step (FARNN_S_D_W_I; decomp1_train.hip.h has
// everything that does not depend on the gates: N, Osum, Mc, the scores in factor space, the loss, the factor gradients).
// The two chain kernels here are the sum semiring's; decomp1_gated_max_train.hip.h has the max semiring's, and shares
// D1GateParams, the LDS sizes and the gates' gradient kernels below.
//
// Reference: FARNN_S_D_W_I.get_forward_score (model_decompose_independent.py:148-197; the gate parameters :100-131, Sigmoidal
// model_decompose.py:97-102).  With v = Vgen[w], k = sigmoid_exponent, h the previous state and h_init = h0 (forward chain) or
// hT (backward chain), one chain step is
//   z    = sigmoid(k (h Wss1 + v Wrs1 + bs1))                                        farnn 1, 2   (:162, :164)
//   r    = sigmoid(k (h Wss2 + v Wrs2 + bs2))                                        farnn 2      (:165)
//   hbar = (1 - r) * h_init + r * h        (farnn 2; hbar = h under farnn 1)                      (:161, :166)
//   y    = nl(hbar Mc[w])                  (backward chain: hbar Mc[w]^T; the gates read Wss UNtransposed in both)  (:177-188)
//   h'   = (1 - z) * h + z * y                                                                    (:193)
// The input halves GV1 = Vgen Wrs1 + bs1 and GV2 = Vgen Wrs2 + bs2 do not depend on the state: one decomp1_gemm_kernel product
// each per step for the batch's words (its `add` row and `rows` mask), as train.hip.h hoists them for the decomposed i-FST.
//
//   decomp1_gated_chain_kernel   both chains with the stash.  One workgroup per sequence and direction in the mould of
//                                onehot_train_chain_kernel<RS, false>: the next token's Mc block is gathered one step ahead into
//                                one of two register sets; Wss1 / Wss2 are step-invariant and live in LDS ([S][S] each: 2 x 64 KiB
//                                at S = 128).  Per step: the gate products on the raw h, then the block product on hbar, then the
//                                blend.  Stashed per step and direction: z, r (farnn 2), the candidate y, and hbar (farnn 2) at
//                                the row of the state it replaces (so that onehot_dT_kernel takes it as dMc's row factor where the
//                                plain step hands it the state stash).  The state rows behind a sequence's last step are written
//                                as zero: the gate reduction below reads every row of the stash.
//   decomp1_gated_bptt_kernel    the same chains in reverse, with Wss1^T / Wss2^T in LDS.  With dh' the adjoint of a step's output:
//                                  dy = dh' z;  dz = dh' (y - h);  daz = k z (1 - z) dz;  u = dy nl'(y)  -> UF / DQ (dMc's column
//                                  factor), daz -> DAZ;  dhbar = u Mc^T (backward chain: u Mc);  dr = dhbar (h - h_init);
//                                  dar = k r (1 - r) dr -> DAR;  carry dh = dh' (1 - z) + dhbar r + daz Wss1^T + dar Wss2^T.
//                                It carries on into row 0 and writes one partial of d loss / d h_init per sequence and direction:
//                                the score adjoint of row 0 + the carry + sum_t (1 - r_t) dhbar_t.
//   decomp1_gate_word_kernel     dGV1[w] / dGV2[w] = the word's DAZ / DAR rows over both chains, positions in bucket order,
//                                forward before backward; zero for an absent word
//   decomp1_gate_bias_kernel     dbs = sum_w dGV[w], words in id order
//   decomp1_gate_add_kernel      dVgen += dGV1 Wrs1^T (+ dGV2 Wrs2^T), the products from decomp1_gemm_kernel
// dWrs = Vgen^T dGV and dWss = H^T DAZ over every (direction, sequence, step) row are decomp1_gemm_kernel products (k ascending,
// one owner per element): H is the state stash, whose forward and backward halves are neighbours, against DAZ shifted by one row
// (the step that wrote DAZ row t read state row t - 1); DAZ / DAR are cleared before back-propagation, so row 0 and the pad rows
// contribute zeros.  No float atomics: two steps on the same inputs are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

namespace farnn {

struct D1GateParams {
    const float *Wss1, *Wss2;    // [S][S]
    const float *GV1, *GV2;      // [V][S] Vgen Wrs + bs of the batch's words
    float *Z, *Rg, *Y, *HB;      // [2][B][L+1][S] (forward chain, then backward): z_t, r_t, y_t at row t; hbar of step t at row t - 1
    float *DAZ, *DAR;            // [2][B][L+1][S] the gates' pre-activation adjoints of step t at row t, zero elsewhere
    float *HP;                   // [B][2][S] d loss / d h0, d loss / d hT per sequence
    int farnn;
    float k;
};

// static LDS of the two kernels below (an upper bound: the state rows and the shares of three products)
constexpr size_t D1G_STATIC_LDS = (3 * (OT_THREADS / 64) + 4) * OT_MAX_S * sizeof(float);
// dynamic LDS: the gate matrices and the tokens of one sequence
inline size_t decomp1_gated_lds_bytes(size_t S, int farnn, int L) { return (size_t)farnn * S * S * sizeof(float) + (size_t)(L + 1) * sizeof(int); }

// grid (B, 2), OT_THREADS; dynamic LDS decomp1_gated_lds_bytes.  RS: as onehot_train_chain_kernel.
template <int RS>
__global__ void __launch_bounds__(OT_THREADS)
decomp1_gated_chain_kernel(const OhTrainParams p, const D1GateParams g) {
    __shared__ __align__(16) float hv[OT_MAX_S], hb[OT_MAX_S];
    __shared__ __align__(16) float part[3][OT_THREADS / 64][OT_MAX_S];
    extern __shared__ __align__(16) float dyn[];                       // Wss1 [S][S], Wss2 [S][S] (farnn 2), toks [L + 1]
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L, farnn = g.farnn;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    const float *G = dir == 0 ? p.M : p.MT;
    const size_t SS = (size_t)S * S, nS = (size_t)p.B * (L + 1) * S;
    float *W1 = dyn, *W2 = dyn + SS;
    int *toks = (int *)(dyn + (size_t)farnn * SS);
    for (int t = tid; t < nsteps; t += OT_THREADS)
        toks[t + 1] = oh_token(p.x, p.V, (long long)b * L + (dir == 0 ? t : len - 1 - t));
    for (int e = tid; e < (int)SS; e += OT_THREADS) {
        W1[e] = g.Wss1[e];
        if (farnn == 2) W2[e] = g.Wss2[e];
    }
    for (int s = tid; s < OT_MAX_S; s += OT_THREADS) { hv[s] = 0.0f; hb[s] = 0.0f; }   // rows past S stay zero
    __syncthreads();
    const bool jok = j < S, ep = ks == 0 && jok;
    const int jc = jok ? j : S - 1;
    // (the gather and the product of onehot_train_chain_kernel: every slot loaded from a valid address, rows past S clamped)
    auto gather = [&](float (&m)[RS], int tok) {
        const float *src = G + (size_t)__builtin_amdgcn_readfirstlane(tok) * SS;
        int off = i0 * S + jc;
        const int last = (S - 1) * S + jc;
#pragma unroll
        for (int r = 0; r < RS; r++) {
            asm volatile("" : "+v"(off));
            m[r] = src[min(off, last)];
            off += S;
        }
    };
    auto matvec = [&](const float *v, const float (&m)[RS], float (*out)[OT_MAX_S]) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int r = 0; r < RS; r += 2) {
            if (r < rs) a0 = fmaf(v[i0 + r], m[r], a0);
            if (r + 1 < rs) a1 = fmaf(v[i0 + r + 1], m[r + 1], a1);
        }
        out[ks][j] = a0 + a1;
    };
    // the gates' products h Wss1 (and h Wss2) from LDS: this share of rows, column jc (rows past S meet a zero of hv)
    auto gates = [&]() {
        float a1 = 0.0f, a2 = 0.0f;
        const int last = (S - 1) * S + jc;
        int off = i0 * S + jc;
        if (farnn == 2) {
            for (int r = 0; r < rs; r++, off += S) {
                const float h = hv[i0 + r];
                const int o = min(off, last);
                a1 = fmaf(h, W1[o], a1);
                a2 = fmaf(h, W2[o], a2);
            }
            part[1][ks][j] = a2;
        } else {
            for (int r = 0; r < rs; r++, off += S) a1 = fmaf(hv[i0 + r], W1[min(off, last)], a1);
        }
        part[0][ks][j] = a1;
    };
    auto shares = [&](float (*src)[OT_MAX_S]) {
        float s = 0.0f;
        for (int k = 0; k < nks; k++) s += src[k][j];
        return s;
    };
    const size_t row0 = (size_t)b * (L + 1), d0 = (size_t)dir * nS;
    float *stash = dir == 0 ? p.A : p.Bk;
    const float hinit = dir == 0 ? p.h0[jc] : p.hT[jc];
    float h = hinit;
    if (ep) {
        stash[row0 * S + j] = hinit;
        hv[j] = hinit;
    }
    float m0[RS], m1[RS];
    if (nsteps > 0) gather(m0, toks[1]);
    wg_barrier_lds();
    auto step = [&](int t, const float (&cur)[RS], float (&nxt)[RS]) {
        const size_t gvo = (size_t)toks[t] * S + jc, row = d0 + (row0 + t) * S + jc;
        const float gv1 = g.GV1[gvo], gv2 = farnn == 2 ? g.GV2[gvo] : 0.0f;
        if (t < nsteps) gather(nxt, toks[t + 1]);
        gates();
        wg_barrier_lds();
        float z = 0.0f;
        if (ep) {
            z = 1.0f / (1.0f + expf(-g.k * (shares(part[0]) + gv1)));
            float hbar = h;
            if (farnn == 2) {
                const float r = 1.0f / (1.0f + expf(-g.k * (shares(part[1]) + gv2)));
                hbar = (1.0f - r) * hinit + r * h;
                g.Rg[row] = r;
                g.HB[row - S] = hbar;
            }
            g.Z[row] = z;
            hb[j] = hbar;
        }
        wg_barrier_lds();
        matvec(hb, cur, part[2]);
        wg_barrier_lds();
        if (ep) {
            const float y = apply_nl(shares(part[2]), p.nl);
            h = (1.0f - z) * h + z * y;
            g.Y[row] = y;
            stash[(row0 + t) * S + j] = h;
            hv[j] = h;
        }
        wg_barrier_lds();
    };
    for (int t = 1; t <= nsteps; t += 2) {
        step(t, m0, m1);
        if (t + 1 <= nsteps) step(t + 1, m1, m0);
    }
    // the state rows no step wrote: zeros for the product over every row of the stash (dWss)
    for (int e = tid; e < (L - nsteps) * S; e += OT_THREADS) stash[(row0 + nsteps + 1) * S + e] = 0.0f;
}

// grid (B, 2), OT_THREADS; dynamic LDS decomp1_gated_lds_bytes.  DAZ / DAR are zero before.
template <int RS>
__global__ void __launch_bounds__(OT_THREADS)
decomp1_gated_bptt_kernel(const OhTrainParams p, const D1GateParams g) {
    __shared__ __align__(16) float uv[OT_MAX_S], azv[OT_MAX_S], arv[OT_MAX_S];
    __shared__ __align__(16) float part[3][OT_THREADS / 64][OT_MAX_S];
    extern __shared__ __align__(16) float dyn[];                       // Wss1^T [S][S], Wss2^T [S][S] (farnn 2), toks [L + 1]
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L, farnn = g.farnn;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    // dhbar = u Mc^T in the forward chain (gathered from MT), u Mc in the backward chain
    const float *G = dir == 0 ? p.MT : p.M;
    const size_t SS = (size_t)S * S, nS = (size_t)p.B * (L + 1) * S;
    float *W1 = dyn, *W2 = dyn + SS;
    int *toks = (int *)(dyn + (size_t)farnn * SS);
    for (int t = tid; t < nsteps; t += OT_THREADS)
        toks[t + 1] = oh_token(p.x, p.V, (long long)b * L + (dir == 0 ? t : len - 1 - t));
    for (int e = tid; e < (int)SS; e += OT_THREADS) {                  // (once per launch: the strided LDS writes do not matter)
        const int a = e / S, c = e - a * S;
        W1[c * S + a] = g.Wss1[e];
        if (farnn == 2) W2[c * S + a] = g.Wss2[e];
    }
    for (int s = tid; s < OT_MAX_S; s += OT_THREADS) { uv[s] = 0.0f; azv[s] = 0.0f; arv[s] = 0.0f; }
    __syncthreads();
    const bool jok = j < S, ep = ks == 0 && jok;
    const int jc = jok ? j : S - 1;
    auto gather = [&](float (&m)[RS], int tok) {
        const float *src = G + (size_t)__builtin_amdgcn_readfirstlane(tok) * SS;
        int off = i0 * S + jc;
        const int last = (S - 1) * S + jc;
#pragma unroll
        for (int r = 0; r < RS; r++) {
            asm volatile("" : "+v"(off));
            m[r] = src[min(off, last)];
            off += S;
        }
    };
    auto matvec = [&](const float *v, const float (&m)[RS], float (*out)[OT_MAX_S]) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int r = 0; r < RS; r += 2) {
            if (r < rs) a0 = fmaf(v[i0 + r], m[r], a0);
            if (r + 1 < rs) a1 = fmaf(v[i0 + r + 1], m[r + 1], a1);
        }
        out[ks][j] = a0 + a1;
    };
    auto lds_matvec = [&](const float *v, const float *Wt, float (*out)[OT_MAX_S]) {
        float a = 0.0f;
        const int last = (S - 1) * S + jc;
        int off = i0 * S + jc;
        for (int r = 0; r < rs; r++, off += S) a = fmaf(v[i0 + r], Wt[min(off, last)], a);
        out[ks][j] = a;
    };
    auto shares = [&](float (*src)[OT_MAX_S]) {
        float s = 0.0f;
        for (int k = 0; k < nks; k++) s += src[k][j];
        return s;
    };
    const size_t row0 = (size_t)b * (L + 1), d0 = (size_t)dir * nS;
    const float *gadj = dir == 0 ? p.GA : p.GB, *st = dir == 0 ? p.A : p.Bk;
    float *outr = dir == 0 ? p.UF : p.DQ;
    const float hinit = dir == 0 ? p.h0[jc] : p.hT[jc];
    float carry = 0.0f, dinit = 0.0f;
    // what a step reads of its own rows, fetched one step ahead by every thread (clamped column), as onehot_train_chain_kernel's
    // back-propagation does: the adjoint of the step's output, the state before it, z, y and r
    struct Rows { float g, h, z, y, r; };
    auto fetch = [&](Rows &w, int t) {
        const size_t row = (row0 + t) * S + jc;
        w.g = gadj[row]; w.h = st[row - S]; w.z = g.Z[d0 + row]; w.y = g.Y[d0 + row];
        w.r = farnn == 2 ? g.Rg[d0 + row] : 1.0f;
    };
    float m0[RS], m1[RS];
    Rows w0 = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f}, w1 = w0;
    if (nsteps > 0) {
        gather(m0, toks[nsteps]);
        fetch(w0, nsteps);
    }
    auto step = [&](int t, const float (&cur)[RS], float (&nxt)[RS], const Rows &c, Rows &n) {
        if (t > 1) { gather(nxt, toks[t - 1]); fetch(n, t - 1); }
        const size_t row = d0 + (row0 + t) * S + jc;
        const float gt = c.g + carry;
        const float daz = g.k * c.z * (1.0f - c.z) * (gt * (c.y - c.h));
        const float u = (gt * c.z) * nl_grad_from_output(c.y, p.nl);
        if (ep) {
            outr[(row0 + t) * S + j] = u;
            g.DAZ[row] = daz;
            uv[j] = u;
            azv[j] = daz;
        }
        wg_barrier_lds();
        matvec(uv, cur, part[0]);
        lds_matvec(azv, W1, part[1]);
        wg_barrier_lds();
        float dhbar = 0.0f, cg = 0.0f;
        if (ep) {
            dhbar = shares(part[0]);
            cg = shares(part[1]);
        }
        if (farnn == 2) {
            if (ep) {
                const float dar = g.k * c.r * (1.0f - c.r) * (dhbar * (c.h - hinit));
                g.DAR[row] = dar;
                arv[j] = dar;
                dinit += (1.0f - c.r) * dhbar;
            }
            wg_barrier_lds();
            lds_matvec(arv, W2, part[2]);
            wg_barrier_lds();
            if (ep) cg += shares(part[2]);
        }
        carry = gt * (1.0f - c.z) + dhbar * c.r + cg;
    };
    for (int t = nsteps; t >= 1; t -= 2) {
        step(t, m0, m1, w0, w1);
        if (t - 1 >= 1) step(t - 1, m1, m0, w1, w0);
    }
    if (ep) g.HP[((size_t)b * 2 + dir) * S + j] = len > 0 ? gadj[row0 * S + j] + carry + dinit : 0.0f;
}

// dGV[gate][w][s] = sum over the word's positions (b, i) in bucket order of D[0][b][i+1][s] (forward chain, step i + 1) and, for
// i >= 1, D[1][b][len-i][s] (backward chain, step len - i); D = DAZ for gate 0, DAR for gate 1.  grid (V, gates), thread s.
__global__ void __launch_bounds__(128)
decomp1_gate_word_kernel(const float *__restrict__ DAZ, const float *__restrict__ DAR, const int64_t *__restrict__ len,
                         const int *__restrict__ list, const int *__restrict__ wstart, const int *__restrict__ wcount,
                         float *__restrict__ dGV1, float *__restrict__ dGV2, int L, int S, size_t nS) {
    const int w = blockIdx.x, s = threadIdx.x;
    if (s >= S) return;
    const float *D = blockIdx.y == 0 ? DAZ : DAR;
    float *out = blockIdx.y == 0 ? dGV1 : dGV2;
    const int n = wcount[w], first = wstart[w];
    float a = 0.0f;
    for (int q = 0; q < n; q++) {
        const int pos = list[first + q];
        const int b = pos / L, i = pos - b * L, ln = clamp_len(len[b], L);
        const size_t row0 = (size_t)b * (L + 1);
        a += D[(row0 + i + 1) * S + s];
        if (i >= 1) a += D[nS + (row0 + ln - i) * S + s];
    }
    out[(size_t)w * S + s] = a;
}

// dbs[gate][s] = sum_w dGV[gate][w][s], words in id order (an absent word's row is zero).  grid (gates), thread s.
__global__ void __launch_bounds__(128)
decomp1_gate_bias_kernel(const float *__restrict__ dGV1, const float *__restrict__ dGV2, float *dbs1, float *dbs2, int V, int S) {
    const int s = threadIdx.x;
    if (s >= S) return;
    const float *src = blockIdx.x == 0 ? dGV1 : dGV2;
    float a = 0.0f;
    for (int w = 0; w < V; w++) a += src[(size_t)w * S + s];
    (blockIdx.x == 0 ? dbs1 : dbs2)[s] = a;
}

// dVgen[e] += T1[e] (+ T2[e]): the gates' share dGV1 Wrs1^T (+ dGV2 Wrs2^T) on top of the blocks' share; one element per thread
__global__ void __launch_bounds__(256)
decomp1_gate_add_kernel(float *dVgen, const float *__restrict__ T1, const float *__restrict__ T2, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = dVgen[e] + T1[e];
    if (T2) v += T2[e];
    dVgen[e] = v;
}

}  // namespace farnn
