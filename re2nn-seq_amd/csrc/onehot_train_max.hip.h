// Training step of the onehot i-FST in the max semiring (--method onehot --independent 2 --train_mode max): both chains with
// an arg-max stash, their back-propagation through time and the per-word dT.  Everything else of the step -- the premix of
// M = T + W and M^T, the bucketing of the positions by word, the scores / CE1 / decode / adjoints (train_loss_kernel<., 0>),
// the loss sum, the reduction of a word's partial tiles -- is the sum step's (onehot_train.hip.h), unchanged.
//
// Reference: FARNN_S_O_I_S.forward_local with semiring_func = _maxmul (model_onehot.py:57, used at :377 and :394) and
// utils._maxmul (utils.py:192-195): torch.max(dim=1), ONE index per (token, state), the first maximal one under IEEE
// comparison (-0 == +0); its backward sends the whole adjoint there.  With M_w = T[w] + W and o = output_mat.sum(0):
//   forward chain   y_t[s] = max_j f_{t-1}[j] M_{x_t}[j,s],  jf_t[s] the first maximal j,  f_t = nl(y_t o),  f_0 = h0   (:376-387)
//   backward chain  c = b_{t-1} o,  q_t[s] = max_j c[j] M_{x'_t}[s,j],  jb_t[s] likewise,  b_t = nl(q_t),  b_0 = hT     (:390-401)
//   BPTT forward    u_t[s] = (GA_t[s] + carry[s]) nl'(f_t[s]) o[s],  dM_{x_t}[jf_t[s], s] += u_t[s] f_{t-1}[jf_t[s]],
//                   carry_{t-1}[j] = sum over the s with jf_t[s] = j of u_t[s] M_{x_t}[j,s]
//   BPTT backward   v_t[s] = (GB_t[s] + carry[s]) nl'(b_t[s]),       dM_{x'_t}[s, jb_t[s]] += v_t[s] c[jb_t[s]],
//                   carry_{t-1}[j] = o[j] sum over the s with jb_t[s] = j of v_t[s] M_{x'_t}[s,j]
//   dT[w] = the sum of dM_w over the valid positions of word w
//
// onehot_max_chain_kernel<RS>   the sum chain kernel's shape: one workgroup per (sequence, direction), a thread owns a column
//                               and a share of the rows, the next token's share gathered one step ahead into the other of two
//                               register sets.  A share reduces to (value, first index, matrix entry) with a strict > while
//                               the rows ascend; the shares combine in ascending row order with a strict >.  Rows past S and
//                               register slots past the share take no part in the comparison (a padded 0 . x = 0 would win
//                               whenever every real candidate is negative).  Stash per (step, state): the state, the index
//                               (8 bits: S <= 128) and the winning matrix entry -- BPTT reads neither M nor M^T.
// onehot_max_bptt_kernel        per step the adjoint row (times the winning entry) and the index row go to LDS; thread j adds
//                               the entries whose index is j, its share of the rows ascending, the shares in order: broadcast
//                               LDS reads, a fixed order, no float atomics.  Writes the step's dM entry per column (forward
//                               chain) or row (backward chain).
// onehot_max_dT_kernel          one workgroup per run of OT_G positions of a word (the sum step's runs): an S x S tile in LDS
//                               (64 KiB at S = 128); first every forward entry (thread s owns column s), then every backward
//                               entry (thread s owns row s), positions in bucket order: bit-reproducible.  A word with several
//                               runs writes partial tiles, added in run order by onehot_dT_reduce_kernel.
#pragma once
#include <stdint.h>
#include "common.hip.h"
#include "train.hip.h"
#include "onehot_train.hip.h"

namespace farnn {

struct OhMaxParams {
    uint8_t *IDXf, *IDXb;     // [B][L+1][S] the first maximal j of every (step, state)
    float *WINf, *WINb;       // [B][L+1][S] the matrix entry that won: M_{x_t}[j*, s] (forward), M_{x'_t}[s, j*] (backward)
    float *GMf, *GMb;         // [B][L+1][S] u_t[s] in[j*]: the step's dM entry of column s (forward) / of row s (backward)
};

// Both chains with the stash; grid (B, 2), the geometry of onehot_train_chain_kernel<RS, false>.
template <int RS>
__global__ void __launch_bounds__(OT_THREADS)
onehot_max_chain_kernel(const OhTrainParams p, const OhMaxParams m) {
    __shared__ __align__(16) float vin[2][OT_MAX_S];
    __shared__ float pval[OT_THREADS / 64][OT_MAX_S], pent[OT_THREADS / 64][OT_MAX_S];
    __shared__ int pidx[OT_THREADS / 64][OT_MAX_S];
    __shared__ float os[OT_MAX_S];
    extern __shared__ int toks[];                           // [L + 1]: the token of step t (t = 1..)
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int nr = min(rs, S - i0);                         // rows of this share that exist (<= 0: none)
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    const float *G = dir == 0 ? p.M : p.MT;                 // max_j in[j] G[j][s]: M forward, M^T backward
    const size_t SS = (size_t)S * S;
    for (int t = tid; t < nsteps; t += blockDim.x)
        toks[t + 1] = oh_token(p.x, p.V, (long long)b * L + (dir == 0 ? t : len - 1 - t));
    for (int s = tid; s < OT_MAX_S; s += blockDim.x) {
        os[s] = s < S ? p.o[s] : 0.0f;
        vin[0][s] = 0.0f; vin[1][s] = 0.0f;
    }
    __syncthreads();
    const bool jok = j < S;
    // every slot is loaded unconditionally from a valid address, as in the sum kernel: rows past S are clamped to row S-1,
    // columns past S to column S-1.  What they hold is excluded from the comparison below, not zeroed.
    const int jc = jok ? j : S - 1;
    auto gather = [&](float (&mm)[RS], int tok) {
        const float *src = G + (size_t)__builtin_amdgcn_readfirstlane(tok) * SS;
        int off = i0 * S + jc;
        const int last = (S - 1) * S + jc;
#pragma unroll
        for (int r = 0; r < RS; r++) {
            asm volatile("" : "+v"(off));
            mm[r] = src[min(off, last)];
            off += S;
        }
    };
    // (pval, pidx, pent)[ks][j] = the maximum over this share's rows i of v[i] G[i][j], its first row, the entry there.
    // Slot 0 starts the scan (an empty share's result is never read); a slot past nr can never win.  No fmaxf: the
    // strict > keeps the first of equal candidates, -0 and +0 included.
    auto maxvec = [&](const float *v, const float (&mm)[RS]) {
        float best = v[i0] * mm[0], be = mm[0];
        int bi = i0;
#pragma unroll
        for (int r = 1; r < RS; r++) {
            const float c = v[i0 + r] * mm[r];
            const bool take = r < nr && c > best;
            best = take ? c : best; be = take ? mm[r] : be; bi = take ? i0 + r : bi;
        }
        pval[ks][j] = best; pidx[ks][j] = bi; pent[ks][j] = be;
    };
    const size_t row0 = (size_t)b * (L + 1);
    float *stash = dir == 0 ? p.A : p.Bk, *WIN = dir == 0 ? m.WINf : m.WINb;
    uint8_t *IDX = dir == 0 ? m.IDXf : m.IDXb;
    float m0[RS], m1[RS];
    if (ks == 0 && jok) {
        const float init = dir == 0 ? p.h0[j] : p.hT[j];
        stash[row0 * S + j] = init;
        vin[0][j] = dir == 0 ? init : init * os[j];
    }
    if (nsteps > 0) gather(m0, toks[1]);
    wg_barrier_lds();
    auto step = [&](int t, const float (&cur)[RS], float (&nxt)[RS]) {
        if (t < nsteps) gather(nxt, toks[t + 1]);
        maxvec(vin[(t - 1) & 1], cur);
        wg_barrier_lds();
        if (ks == 0 && jok) {
            float y = pval[0][j];
            int k = 0;
            for (int q = 1; q < nks && q * rs < S; q++) {        // the shares that have rows, in ascending row order
                const float v = pval[q][j];
                if (v > y) { y = v; k = q; }
            }
            const float h = dir == 0 ? apply_nl(y * os[j], p.nl) : apply_nl(y, p.nl);
            const size_t row = (row0 + t) * S + j;
            stash[row] = h;
            IDX[row] = (uint8_t)pidx[k][j];
            WIN[row] = pent[k][j];
            vin[t & 1][j] = dir == 0 ? h : h * os[j];
        }
        wg_barrier_lds();
    };
    for (int t = 1; t <= nsteps; t += 2) {
        step(t, m0, m1);
        if (t + 1 <= nsteps) step(t + 1, m1, m0);
    }
}

// Back-propagation through time of both chains; grid (B, 2), the shares of the chain kernel.  Threads (0, j) own state j: the
// adjoint, the step's dM entry, the stash rows of the next step fetched one step ahead.
// CARRY0 (the steps that train the chains' initial vectors): step 1 carries on into row 0 as every step does into the row
// before it -- to the winning index only -- and HP[b][dir][j] = the adjoint of row 0 (GA / GB row 0: the score of the first /
// last position) + that carry: d loss / d h0 (dir 0) and d loss / d hT (dir 1) from sequence b; zero for an empty sequence.
template <bool CARRY0>
__device__ __forceinline__ void onehot_max_bptt_body(const OhTrainParams &p, const OhMaxParams &m, float *__restrict__ HP) {
    __shared__ float uw[OT_MAX_S], os[OT_MAX_S];
    __shared__ int jj[OT_MAX_S];
    __shared__ float part[OT_THREADS / 64][OT_MAX_S];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int nr = min(rs, S - i0);
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    for (int s = tid; s < OT_MAX_S; s += blockDim.x) os[s] = s < S ? p.o[s] : 0.0f;
    __syncthreads();
    const bool ep = ks == 0 && j < S;
    const float *gadj = dir == 0 ? p.GA : p.GB, *st = dir == 0 ? p.A : p.Bk, *WIN = dir == 0 ? m.WINf : m.WINb;
    const uint8_t *IDX = dir == 0 ? m.IDXf : m.IDXb;
    float *GM = dir == 0 ? m.GMf : m.GMb;
    const size_t row0 = (size_t)b * (L + 1);
    float carry = 0.0f, g = 0.0f, sv = 0.0f, w = 0.0f;
    int ix = 0;
    if (ep && nsteps > 0) {
        const size_t row = (row0 + nsteps) * S + j;
        g = gadj[row]; sv = st[row]; w = WIN[row]; ix = IDX[row];
    }
    for (int t = nsteps; t >= 1; t--) {
        float gn = 0.0f, sn = 0.0f, wn = 0.0f;
        int ixn = 0;
        if (ep) {
            const size_t row = (row0 + t) * S + j;
            float cin = st[row - S - j + ix];                    // the chain input at j*: f_{t-1}[j*], or b_{t-1}[j*] o[j*]
            if (t > 1) { gn = gadj[row - S]; sn = st[row - S]; wn = WIN[row - S]; ixn = IDX[row - S]; }
            float u = (g + carry) * nl_grad_from_output(sv, p.nl);
            if (dir == 0) u *= os[j];
            else cin *= os[ix];
            uw[j] = u * w; jj[j] = ix;
            GM[row] = u * cin;
        }
        if (!CARRY0 && t == 1) break;
        wg_barrier_lds();
        // the carry into step t - 1: thread (ks, j) adds its share of the states whose index is j, ascending
        float a = 0.0f;
        for (int r = 0; r < nr; r++) a += jj[i0 + r] == j ? uw[i0 + r] : 0.0f;
        part[ks][j] = a;
        wg_barrier_lds();
        if (ep) {
            float c = part[0][j];
            for (int q = 1; q < nks && q * rs < S; q++) c += part[q][j];
            carry = dir == 0 ? c : c * os[j];
            g = gn; sv = sn; w = wn; ix = ixn;
        }
    }
    if (CARRY0 && ep) HP[((size_t)b * 2 + dir) * S + j] = len > 0 ? gadj[row0 * S + j] + carry : 0.0f;
}
__global__ void __launch_bounds__(OT_THREADS)
onehot_max_bptt_kernel(const OhTrainParams p, const OhMaxParams m) { onehot_max_bptt_body<false>(p, m, nullptr); }
// the same with the row-0 carry: HP [B][2][S] (decomp1_init_sum_kernel adds the sequences in order)
__global__ void __launch_bounds__(OT_THREADS)
onehot_max_bptt_carry_kernel(const OhTrainParams p, const OhMaxParams m, float *__restrict__ HP) { onehot_max_bptt_body<true>(p, m, HP); }

// dT: one workgroup per run of up to OT_G positions of one word, the runs of onehot_dT_kernel.  LDS: tile [S][S], then the
// stash rows of the run's positions (forward step i + 1; backward step len - i, which exists for i >= 1: -1 otherwise).
__global__ void __launch_bounds__(256)
onehot_max_dT_kernel(const OhTrainParams p, const OhMaxParams m, const int *__restrict__ list,
                     const int *__restrict__ wstart, const int *__restrict__ wcount, const int *__restrict__ itoff,
                     const int *__restrict__ psoff, float *dT, float *partial) {
    extern __shared__ __align__(16) float tile[];
    const int item = blockIdx.x, V = p.V, S = p.S, L = p.L, s = threadIdx.x;
    if (item >= itoff[V]) return;
    int lo = 0, hi = V - 1;                                   // the word whose runs contain this item
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (itoff[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int w = lo, k = item - itoff[w], runs = itoff[w + 1] - itoff[w];
    const int n0 = k * OT_G, n = min(OT_G, wcount[w] - n0);
    int *rowf = (int *)(tile + S * S), *rowb = rowf + OT_G;
    for (int e = s; e < S * S; e += blockDim.x) tile[e] = 0.0f;
    if (s < n) {
        const int pos = list[wstart[w] + n0 + s];
        const int b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
        rowf[s] = b * (L + 1) + i + 1;
        rowb[s] = i >= 1 ? b * (L + 1) + len - i : -1;
    }
    __syncthreads();
    // eight positions' loads in flight; each tile element has one owner per phase and is added to in bucket order
    auto phase = [&](const int *rows, const uint8_t *IDX, const float *GM, bool fwd) {
        for (int q0 = 0; q0 < n; q0 += 8) {
            int id[8];
            float gv[8];
            bool ok[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                ok[u] = q0 + u < n && rows[q0 + u] >= 0;
                const size_t row = (size_t)(ok[u] ? rows[q0 + u] : rowf[q0]) * S + s;
                id[u] = IDX[row]; gv[u] = GM[row];
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (ok[u]) tile[fwd ? id[u] * S + s : s * S + id[u]] += gv[u];
        }
    };
    if (s < S) phase(rowf, m.IDXf, m.GMf, true);
    __syncthreads();
    if (s < S) phase(rowb, m.IDXb, m.GMb, false);
    __syncthreads();
    float *out = runs > 1 ? partial + (size_t)(psoff[w] + k) * S * S : dT + (size_t)w * S * S;
    for (int e = s; e < S * S; e += blockDim.x) out[e] = tile[e];
}

inline size_t onehot_max_dT_lds_bytes(size_t S) { return S * S * sizeof(float) + 2 * OT_G * sizeof(int); }

}  // namespace farnn
