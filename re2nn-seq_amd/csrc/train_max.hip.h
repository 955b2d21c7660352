// Training step of the decomposed i-FST in the max semiring (--train_mode max): the recurrence and its back-propagation.
// Everything else of the step -- the gates' input halves, scores, CE1 / CRF loss, decode, the gate and Vgen reductions --
// is the sum step's (train.hip.h), unchanged.
//
// Reference: FARNN_S_D_W_I_S.get_forward_score with train_mode = 'max' (model_decompose_single.py:156-166) and
// utils._maxmul (utils.py:192-195).  With Tr_w = S1 diag(v_w) S2^T + W (an S x S block per word):
//   forward chain   n[s] = max_j hbar[j] Tr[j,s],   then * Osum, nl, gate mix                       (:159-164,:181-198)
//   backward chain  n[s] = max_j bb[j] Tr[s,j],     bb = hbar * Osum, then nl, gate mix            (:156-157,:165-166)
// torch.max(dim=1) returns ONE index j* per (token, s): the first maximal one under IEEE comparison (-0 == +0), and
// its backward sends the whole adjoint u[s] there:  d in[j*] += u[s] Tr[j*,s],  dTr[j*,s] += u[s] in[j*].
// The per-word sums dM_w of dTr (the backward chain's entries transposed) give
//   dW = sum_w dM_w,  dS1 = sum_w dM_w (S2 . v_w),  dS2 = sum_w dM_w^T (S1 . v_w),  dVgen[w,r] += sum_{j,s} dM_w[j,s] S1[j,r] S2[s,r].
//
// Kernels, in launch order (the bucketing of the positions by word is the onehot step's, onehot_train.hip.h):
//   tmax_slots_kernel     the batch's distinct words in vocabulary order: slot of every word, word of every slot, their count
//   tmax_premix_kernel    M[slot] = Tr_w and MT[slot] = Tr_w^T for every distinct word
//   tmax_forward_kernel   both chains with the state stash, the chain inputs and the argmax j* of every (step, state)
//   tmax_backward_kernel  back-propagation through time: u routed through the stored j*, the gate adjoints as in the sum step
//   tmax_dM_kernel        dM_w of every distinct word from its positions in bucket order: no float atomics, bit-reproducible
//   tmax_wgrad_kernel     dS1 (with dVgen and dW) and dS2 from dM
// A thread owns one state s in the chain kernels; S <= TM_MAX_S (dM_w is accumulated in LDS).
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

namespace farnn {

constexpr int TM_THREADS = 256;   // chain, dM and weight-gradient kernels
constexpr int TM_MAX_S = 192;     // one thread per state; dM_w [S][S] in LDS (144 KiB at 192)
constexpr int TM_WCH = 64;        // word chunks of tmax_wgrad_kernel (the grid's z extent)

struct TrainMaxParams {
    const float *M, *MT;      // [nwmax][S][S] Tr of every distinct word (slot order) and its transpose
    const int *wslot;         // [V] slot of a word that occurs in the batch
    const int *wlist;         // [nwmax] word of every slot
    const int *nwords;        // [1] distinct words of the batch
    int *IDXf, *IDXb;         // [B][L+1][S] j* of every step (row t = step t)
    float *INf, *INb;         // [B][L+1][S] chain input of every step (hbar forward, hbar * Osum backward)
    float *GMf, *GMb;         // [B][L+1][S] u[s] in[j*]: the step's dTr entry of column s (forward) / row s (backward)
};

// wslot[w] = rank of w among the words with positions (vocabulary order), wlist[slot] = w, nwords = their count.
// One workgroup of 1024 threads (oh_block_scan).
__global__ void __launch_bounds__(1024)
tmax_slots_kernel(const int *__restrict__ wcount, int V, int *wslot, int *wlist, int *nwords) {
    __shared__ int red[1024];
    for (int w = threadIdx.x; w < V; w += blockDim.x) wslot[w] = wcount[w] > 0 ? 1 : 0;
    __syncthreads();
    const int total = oh_block_scan(wslot, V, red);
    for (int w = threadIdx.x; w < V; w += blockDim.x)
        if (wcount[w] > 0) wlist[wslot[w]] = w;
    if (threadIdx.x == 0) *nwords = total;
}

// M[slot][j][s] = sum_r S2[s,r] (v[r] S1[j,r]) + W[j,s] (the reference's association, :160-162) and MT[slot] = M[slot]^T.
// grid (nwmax, tiles): one 32 x 32 tile per workgroup of 256 threads, the rank in chunks of 32 through LDS.
__global__ void __launch_bounds__(256)
tmax_premix_kernel(const float *__restrict__ Vgen, const float *__restrict__ S1, const float *__restrict__ S2,
                   const float *__restrict__ W, const int *__restrict__ wlist, const int *__restrict__ nwords,
                   float *M, float *MT, int S, int R) {
    __shared__ float a[32][33], bt[32][33];
    const int slot = blockIdx.x;
    if (slot >= *nwords) return;
    const int nt = (S + 31) >> 5, j0 = (blockIdx.y / nt) * 32, s0 = (blockIdx.y % nt) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *v = Vgen + (size_t)wlist[slot] * R;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r0 = 0; r0 < R; r0 += 32) {
        const int r = r0 + tx;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = ty + 8 * k;
            a[q][tx] = (j0 + q < S && r < R) ? v[r] * S1[(size_t)(j0 + q) * R + r] : 0.0f;
            bt[q][tx] = (s0 + q < S && r < R) ? S2[(size_t)(s0 + q) * R + r] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < 32; rr++) {
            const float b = bt[tx][rr];
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = fmaf(a[ty + 8 * k][rr], b, acc[k]);
        }
        __syncthreads();
    }
    // the tile goes out through LDS a second time for the transpose (reads and writes along rows)
    const size_t base = (size_t)slot * S * S;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = j0 + ty + 8 * k, s = s0 + tx;
        const bool ok = j < S && s < S;
        const float val = ok ? acc[k] + W[(size_t)j * S + s] : 0.0f;
        if (ok) M[base + (size_t)j * S + s] = val;
        a[ty + 8 * k][tx] = val;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = s0 + ty + 8 * k, j = j0 + tx;
        if (j < S && s < S) MT[base + (size_t)s * S + j] = a[tx][ty + 8 * k];
    }
}

// ---- forward pass of both chains with the stash ----------------------------------------------------------------
// grid (B, 2): blockIdx.y = 0 forward, 1 backward chain.  Thread s: the gate pre-activations of state s (Wss read
// through L2 along rows), then n[s] = max_j in[j] G[j][s] with G = M (forward) or MT (backward) of the step's word.
// Writes A / Bk, PRE and the gate stash (ZG, RG, CD) as train_forward_kernel does, plus IN and IDX.
// With a KD / PR teacher (p.full_chain, train_teacher.hip.h) both chains of every sequence, the empty ones too, run L steps:
// the forward chain over x[b, t-1], the backward chain over its len reversed tokens and then the raw pad tokens x[b, len:], and
// every row 1..L of the stashes is written.  The back-propagation then starts at row L; the teacher's loss kernel has left
// the adjoint of a pad position i in row i + 1 of both GA and GB.
// LDS: in[2][TM_MAX_S] (by step parity), hv[TM_MAX_S] raw state, toks[L]
__global__ void __launch_bounds__(TM_THREADS)
tmax_forward_kernel(const TrainParams p, const TrainMaxParams m) {
    __shared__ float inv[2][TM_MAX_S];
    __shared__ float hv[TM_MAX_S];
    extern __shared__ int toks[];                              // [L]: the token of step t at t - 1
    const int b = blockIdx.x, dir = blockIdx.y, s = threadIdx.x, S = p.S, L = p.L;
    // len: the steps of the chain -- the valid length, or L with a teacher (full_chain), whose chains go on through the pad
    // tokens; vlen: the valid length, which only decides the order of the tokens (train_forward_kernel, train.hip.h)
    const int vlen = clamp_len(p.len[b], L), len = p.full_chain ? L : vlen;
    for (int i = s; i < len; i += blockDim.x)
        toks[i] = oh_token(p.x, p.V, (long long)b * L + ((dir == 0 || i >= vlen) ? i : vlen - 1 - i));
    const bool own = s < S;
    const size_t row0 = (size_t)b * (L + 1), SS = (size_t)S * S;
    float *stash = dir == 0 ? p.A : p.Bk;
    int *IDX = dir == 0 ? m.IDXf : m.IDXb;
    float *IN = dir == 0 ? m.INf : m.INb;
    float *ZG = dir == 0 ? p.ZGf : p.ZGb, *RG = dir == 0 ? p.RGf : p.RGb, *CD = dir == 0 ? p.CDf : p.CDb;
    const float *G = dir == 0 ? m.M : m.MT;
    const int farnn = p.farnn;
    const float hin = own ? (dir == 0 ? p.h0[s] : p.hT[s]) : 0.0f, os = own ? p.Osum[s] : 0.0f;
    float hk = hin;
    if (own) { stash[row0 * S + s] = hin; hv[s] = hin; }
    __syncthreads();
    for (int t = 1; t <= len; t++) {
        const int tok = toks[t - 1];
        const size_t row = (row0 + t) * S + s;
        float z = 1.0f, r = 1.0f, hbar = hk;
        if (farnn && own) {                                    // (:146-151); GV = Vgen Wrs hoisted as in the sum step
            float a0 = 0.0f, a1 = 0.0f, c0 = 0.0f, c1 = 0.0f;
            int j = 0;
            for (; j + 2 <= S; j += 2) {
                a0 = fmaf(hv[j], p.Wss1[(size_t)j * S + s], a0);
                a1 = fmaf(hv[j + 1], p.Wss1[(size_t)(j + 1) * S + s], a1);
                if (farnn == 2) {
                    c0 = fmaf(hv[j], p.Wss2[(size_t)j * S + s], c0);
                    c1 = fmaf(hv[j + 1], p.Wss2[(size_t)(j + 1) * S + s], c1);
                }
            }
            if (j < S) {
                a0 = fmaf(hv[j], p.Wss1[(size_t)j * S + s], a0);
                if (farnn == 2) c0 = fmaf(hv[j], p.Wss2[(size_t)j * S + s], c0);
            }
            const float az = (a0 + a1) + p.GV1[(size_t)tok * S + s] + p.bs1[s];
            z = 1.0f / (1.0f + expf(-p.sig_k * az));
            if (farnn == 2) {
                const float ar = (c0 + c1) + p.GV2[(size_t)tok * S + s] + p.bs2[s];
                r = 1.0f / (1.0f + expf(-p.sig_k * ar));
                hbar = (1.0f - r) * hin + r * hk;
            }
        }
        const float in = dir == 0 ? hbar : hbar * os;
        if (own) { inv[t & 1][s] = in; IN[row] = in; }
        wg_barrier_lds();
        float h = 0.0f;
        if (own) {
            // max_j in[j] G[j][s], the first maximal j (strict >, as torch.max); 16 loads in flight per round
            const float *g = G + (size_t)m.wslot[tok] * SS + s;
            const float *iv = inv[t & 1];
            float best = iv[0] * g[0];
            int bi = 0;
            int j = 1;
            for (; j + 16 <= S; j += 16) {
                float gv[16];
#pragma unroll
                for (int u = 0; u < 16; u++) gv[u] = g[(size_t)(j + u) * S];
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const float v = iv[j + u] * gv[u];
                    if (v > best) { best = v; bi = j + u; }
                }
            }
            for (; j < S; j++) {
                const float v = iv[j] * g[(size_t)j * S];
                if (v > best) { best = v; bi = j; }
            }
            IDX[row] = bi;
            if (dir == 0) { p.PRE[row] = best; h = apply_nl(best * os, p.nl); }       // (:181)
            else          { h = apply_nl(best, p.nl); }
            if (farnn) {                                                             // (:193-196)
                CD[row] = h; ZG[row] = z; RG[row] = r;
                h = (1.0f - z) * hk + z * h;
            }
            hk = h;
            stash[row] = h;
        }
        wg_barrier_lds();                                      // every gate read of hv for step t is done
        if (own) hv[s] = h;
        wg_barrier_lds();
    }
}

// ---- back-propagation through time ----------------------------------------------------------------------------
// grid (B, 2).  Thread s: the adjoint of state s, u[s] = d n[s]; the dTr entry u[s] in[j*(s)] goes to GM; then the
// chain input's adjoint d in[j] = sum over the states s with j*(s) = j of u[s] G[j][s] (thread j, s ascending: no
// atomics); the gate adjoints and the carry into step t - 1 as in train_backward_kernel.
// DET (the decomposed FST's step, decomp0_train_max.hip.h): no float atomics, as train_backward_kernel's DET form -- the gates'
// input adjoints stay in their rows DAZ / DAR, the sequence's dh0 / dhT go to HP, and dOsum (a mask of ones there) is dropped.
// LDS: uu, dz, dr, jj [TM_MAX_S], toks[L]
template <bool DET = false>
__global__ void __launch_bounds__(TM_THREADS)
tmax_backward_kernel(const TrainParams p, const TrainMaxParams m) {
    __shared__ float uu[TM_MAX_S], dz[TM_MAX_S], dr[TM_MAX_S];
    __shared__ int jj[TM_MAX_S];
    extern __shared__ int toks[];
    const int b = blockIdx.x, dir = blockIdx.y, s = threadIdx.x, S = p.S, L = p.L;
    // len: the steps of the chain -- the valid length, or L with a teacher (full_chain), whose chains go on through the pad
    // tokens; vlen: the valid length, which only decides the order of the tokens (train_forward_kernel, train.hip.h)
    const int vlen = clamp_len(p.len[b], L), len = p.full_chain ? L : vlen;
    for (int i = s; i < len; i += blockDim.x)
        toks[i] = oh_token(p.x, p.V, (long long)b * L + ((dir == 0 || i >= vlen) ? i : vlen - 1 - i));
    const bool own = s < S;
    const size_t row0 = (size_t)b * (L + 1), SS = (size_t)S * S;
    const float *stash = dir == 0 ? p.A : p.Bk, *Gadj = dir == 0 ? p.GA : p.GB;
    const int *IDX = dir == 0 ? m.IDXf : m.IDXb;
    const float *IN = dir == 0 ? m.INf : m.INb;
    float *GM = dir == 0 ? m.GMf : m.GMb;
    const float *ZG = dir == 0 ? p.ZGf : p.ZGb, *RG = dir == 0 ? p.RGf : p.RGb, *CD = dir == 0 ? p.CDf : p.CDb;
    float *DAZ = dir == 0 ? p.DAZf : p.DAZb, *DAR = dir == 0 ? p.DARf : p.DARb;
    const float *G = dir == 0 ? m.M : m.MT;
    const int farnn = p.farnn;
    const float hin = own ? (dir == 0 ? p.h0[s] : p.hT[s]) : 0.0f, os = own ? p.Osum[s] : 0.0f;
    float gacc = 0.0f, dhin = 0.0f, dOacc = 0.0f;
    __syncthreads();
    for (int t = len; t >= 1; t--) {
        const int tok = toks[t - 1];
        const size_t rb = (row0 + t) * S, row = rb + s;
        float dhk = 0.0f, z = 1.0f, r = 1.0f, hprev = 0.0f, hp = 0.0f;
        if (own) {
            const float gt = gacc + Gadj[row];
            hprev = stash[row - S];
            hp = hprev;
            float yy;
            if (farnn) {                                       // h_t = (1-z) h_{t-1} + z cand
                z = ZG[row];
                const float cand = CD[row];
                dhk = gt * (1.0f - z);
                yy = (gt * z) * nl_grad_from_output(cand, p.nl);
                const float daz = gt * (cand - hprev) * p.sig_k * z * (1.0f - z);
                DAZ[row] = daz;
                dz[s] = daz;
                if constexpr (!DET) atomicAdd(p.dGV1 + (size_t)tok * S + s, daz);
                if (farnn == 2) { r = RG[row]; hp = (1.0f - r) * hin + r * hprev; }     // hbar
            } else {
                yy = gt * nl_grad_from_output(stash[row], p.nl);
            }
            float u;
            if (dir == 0) { u = yy * os; if constexpr (!DET) dOacc = fmaf(yy, p.PRE[row], dOacc); }       // mask on the output
            else          { u = yy; }
            const int j = IDX[row];
            jj[s] = j; uu[s] = u;
            GM[row] = u * IN[rb + j];
        }
        wg_barrier_lds();
        if (own) {
            const float *g = G + (size_t)m.wslot[tok] * SS + (size_t)s * S;      // row s of G
            float din = 0.0f;
            for (int k = 0; k < S; k++)
                if (jj[k] == s) din = fmaf(uu[k], g[k], din);
            float dhb;
            if (dir == 0) dhb = din;
            else { if constexpr (!DET) dOacc = fmaf(din, hp, dOacc); dhb = din * os; }                   // mask on the input
            if (!farnn) gacc = dhb;
            else if (farnn == 2) {                                                    // hbar = (1-r) h_init + r h_{t-1}
                const float dar = dhb * (hprev - hin) * p.sig_k * r * (1.0f - r);
                dhin = fmaf(dhb, 1.0f - r, dhin);
                dhk = fmaf(dhb, r, dhk);
                DAR[row] = dar;
                dr[s] = dar;
                if constexpr (!DET) atomicAdd(p.dGV2 + (size_t)tok * S + s, dar);
            } else {
                dhk += dhb;
            }
        }
        if (farnn) {                                           // the gates read the raw h_{t-1}: + daz Wss1^T + dar Wss2^T
            wg_barrier_lds();
            if (own) {
                float a0 = 0.0f, a1 = 0.0f;
                for (int k = 0; k < S; k++) {
                    a0 = fmaf(dz[k], p.Wss1T[(size_t)k * S + s], a0);
                    if (farnn == 2) a1 = fmaf(dr[k], p.Wss2T[(size_t)k * S + s], a1);
                }
                gacc = dhk + a0 + a1;
            }
        }
        wg_barrier_lds();                                      // uu, jj, dz, dr are rewritten by the next step
    }
    if (own) {
        const float g0 = gacc + Gadj[row0 * S + s] + dhin;
        if constexpr (DET) p.HP[((size_t)b * 2 + dir) * S + s] = g0;
        else {
            if (g0 != 0.0f) atomicAdd((dir == 0 ? p.dh0 : p.dhT) + s, g0);
            if (dOacc != 0.0f) atomicAdd(p.dOsum + s, dOacc);
        }
    }
}

// ---- dM_w: one workgroup per distinct word, [S][S] in LDS ------------------------------------------------------
// The word's positions in bucket order (flat position order); first every forward entry (thread s owns column s: entry
// (j*, s) of step i + 1), then every backward entry (thread s owns row s: entry (s, j*) of step len - i; of step i + 1 at a
// pad position i >= len, which only the teacher's bucketing of every position lists).  Each element is added in a fixed
// order by one thread: two steps on the same inputs give the same bits.
__global__ void __launch_bounds__(TM_THREADS)
tmax_dM_kernel(const TrainParams p, const TrainMaxParams m, const int *__restrict__ list, const int *__restrict__ wstart,
               const int *__restrict__ wcount, float *dM) {
    extern __shared__ float tile[];
    const int slot = blockIdx.x;
    if (slot >= *m.nwords) return;
    const int w = m.wlist[slot], S = p.S, L = p.L, s = threadIdx.x, nt = blockDim.x;
    for (int e = s; e < S * S; e += nt) tile[e] = 0.0f;
    __syncthreads();
    const int n = wcount[w], st = wstart[w];
    if (s < S) {
        for (int q = 0; q < n; q++) {
            const int pos = list[st + q], bb = pos / L, i = pos - bb * L;
            const size_t row = ((size_t)bb * (L + 1) + i + 1) * S + s;
            tile[m.IDXf[row] * S + s] += m.GMf[row];
        }
    }
    __syncthreads();
    if (s < S) {
        for (int q = 0; q < n; q++) {
            const int pos = list[st + q], bb = pos / L, i = pos - bb * L;
            const int len = clamp_len(p.len[bb], L);
            const size_t row = ((size_t)bb * (L + 1) + (i < len ? len - i : i + 1)) * S + s;      // (a pad: full_chain only)
            tile[s * S + m.IDXb[row]] += m.GMb[row];
        }
    }
    __syncthreads();
    float *out = dM + (size_t)slot * S * S;
    for (int e = s; e < S * S; e += nt) out[e] = tile[e];
}

// ---- weight gradients from dM ------------------------------------------------------------------------------------
// grid (ceil(R / 64), ceil(S / 32), TM_WCH): a block of 32 rows a and 64 ranks r over one chunk of the distinct words.
// Lane r = tid & 63; group g = tid >> 6 owns the rows a0 + 8g .. a0 + 8g + 7.
//   TRANS 0: X = dM_w S2 (rows a = j): dS1 += v_w . X, dVgen[w] += sum_j S1[j] . X[j]; the r-block 0 also adds dM_w to dW
//   TRANS 1: Y = dM_w^T S1 (rows a = s): dS2 += v_w . Y
// A chunk's sums go out with atomics (dS1, dS2, dW and dVgen are also fed by other products of the step).
// LDS: F [S][64] (S2 or S1, ranks r0..), T [S][32] (dM_w, reduction index major), DW [S][32], red [4][64]
template <bool TRANS>
__global__ void __launch_bounds__(256)
tmax_wgrad_kernel(const TrainParams p, const TrainMaxParams m, const float *__restrict__ dM, float *out, float *dW) {
    extern __shared__ __align__(16) float sm[];
    const int S = p.S, R = p.R, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
    const int r0 = blockIdx.x * 64, a0 = blockIdx.y * 32;
    const int nw = *m.nwords, c = blockIdx.z;
    const int w0 = (int)((long long)nw * c / gridDim.z), w1 = (int)((long long)nw * (c + 1) / gridDim.z);
    if (w0 >= w1) return;
    const size_t SS = (size_t)S * S;
    float *F = sm, *T = F + S * 64, *DW = T + S * 32, *red = DW + S * 32;
    const bool dw = !TRANS && blockIdx.x == 0;
    const float *Fsrc = TRANS ? p.S1 : p.S2;
    for (int e = tid; e < S * 64; e += 256) {
        const int k = e >> 6, rr = r0 + (e & 63);
        F[e] = rr < R ? Fsrc[(size_t)k * R + rr] : 0.0f;
    }
    if (dw) for (int e = tid; e < S * 32; e += 256) DW[e] = 0.0f;
    const int r = r0 + lane;
    const bool rok = r < R;
    float s1r[8], acc[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int a = a0 + g * 8 + q;
        s1r[q] = (!TRANS && rok && a < S) ? p.S1[(size_t)a * R + r] : 0.0f;
        acc[q] = 0.0f;
    }
    for (int slot = w0; slot < w1; slot++) {
        __syncthreads();                                       // F staged; T and red of the previous word consumed
        const int word = m.wlist[slot];
        const float *D = dM + (size_t)slot * SS;
        for (int e = tid; e < S * 32; e += 256) {
            const int k = e >> 5, a = a0 + (e & 31);
            T[e] = a < S ? (TRANS ? D[(size_t)k * S + a] : D[(size_t)a * S + k]) : 0.0f;
        }
        __syncthreads();
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; q++) x[q] = 0.0f;
        for (int k = 0; k < S; k++) {
            const float f = F[k * 64 + lane];
            const v4f t0 = *(const v4f *)(T + k * 32 + g * 8), t1 = *(const v4f *)(T + k * 32 + g * 8 + 4);
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = fmaf(t0[q], f, x[q]); x[4 + q] = fmaf(t1[q], f, x[4 + q]); }
        }
        const float vr = rok ? p.Vgen[(size_t)word * R + r] : 0.0f;
#pragma unroll
        for (int q = 0; q < 8; q++) acc[q] = fmaf(vr, x[q], acc[q]);
        if (!TRANS) {
            float dv = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; q++) dv = fmaf(s1r[q], x[q], dv);
            red[g * 64 + lane] = dv;
            __syncthreads();
            if (g == 0 && rok) {
                const float sum = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
                if (sum != 0.0f) atomicAdd(p.dVgen + (size_t)word * R + r, sum);
            }
        }
        if (dw)
            for (int e = tid; e < S * 32; e += 256) DW[e] += T[e];          // element e has one owner
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int a = a0 + g * 8 + q;
        if (a < S && rok && acc[q] != 0.0f) atomicAdd(out + (size_t)a * R + r, acc[q]);
    }
    if (dw)
        for (int e = tid; e < S * 32; e += 256) {
            const int k = e >> 5, a = a0 + (e & 31);
            if (a < S && DW[e] != 0.0f) atomicAdd(dW + (size_t)a * S + k, DW[e]);
        }
}

inline size_t tmax_wgrad_lds_bytes(size_t S) { return (S * 128 + 256) * sizeof(float); }

}  // namespace farnn
