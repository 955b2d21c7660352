// The gated recurrences (--farnn 1 | 2) of the decomposed independent=1 training step in the max semiring (--train_mode max):
// decomp1_gated_train.hip.h's chains with onehot_train_max.hip.h's block product.
//
// Reference: FARNN_S_D_W_I.get_forward_score (model_decompose_independent.py:148-197) with semiring_func = _maxmul
// (utils.py:192-195).  Only the two block products go through semiring_func; the gate products stay ordinary matrix products:
//   z    = sigmoid(k (h Wss1 + v Wrs1 + bs1))                 farnn 1, 2   (sum-times)
//   r    = sigmoid(k (h Wss2 + v Wrs2 + bs2))                 farnn 2      (sum-times)
//   hbar = (1 - r) h_init + r h                               (farnn 1: hbar = h)
//   q[s] = max_j hbar[j] Mc[w][j,s]   (backward chain: max_j hbar[j] Mc[w][s,j]),  j*[s] the FIRST maximal j under IEEE
//          comparison (-0 == +0): torch.max(dim=1), whose backward sends the whole adjoint there
//   y    = nl(q);   h' = (1 - z) h + z y
//
//   decomp1_gated_max_chain_kernel  decomp1_gated_chain_kernel's geometry, gathers, gate products and stash (the state, z, r,
//                                   y, hbar at the row of the state it replaces; zeros in the state rows behind the last step).
//                                   The block product is onehot_max_chain_kernel's share reduction: (value, first index, entry)
//                                   with a strict > while the rows ascend, the shares combined in ascending row order with a
//                                   strict >; rows past S and register slots past the share take no part in the comparison.
//                                   It stashes the index byte and the winning entry as well (IDXf / IDXb, WINf / WINb).  The
//                                   shares of the gate products and of the max reduction take turns in one LDS array.
//   decomp1_gated_max_bptt_kernel   the same chains in reverse, with Wss1^T / Wss2^T in LDS (no RS: it gathers no block, so one
//                                   kernel serves every S).  With dh' the adjoint of a step's output:
//                                   dy = dh' z;  dz = dh' (y - h);  daz = k z (1 - z) dz -> DAZ;  u = dy nl'(y);
//                                   the step's dMc entry u[s] hbar[j*[s]] -> GMf / GMb (onehot_max_dT_kernel adds them per word);
//                                   dhbar[j] = the sum over the s with j*[s] = j of u[s] WIN[s], in onehot_max_bptt_kernel's
//                                   fixed order: u WIN and the index row go to LDS, thread j adds the entries whose index is j,
//                                   its share ascending, the shares in order;  dr = dhbar (h - h_init);  dar = k r (1 - r) dr
//                                   -> DAR;  carry dh = dh' (1 - z) + dhbar r + daz Wss1^T + dar Wss2^T.  It reads neither M
//                                   nor MT, carries on into row 0 and writes HP [B][2][S]: the score adjoint of row 0 + the
//                                   carry + sum_t (1 - r_t) dhbar_t.
// Everything else of the step is the gated sum step's (the gates stage) and the plain max step's (dM per word).  No float atomics.
#pragma once
#include "decomp1_gated_train.hip.h"
#include "onehot_train_max.hip.h"

namespace farnn {

// grid (B, 2), OT_THREADS; dynamic LDS decomp1_gated_lds_bytes; static LDS within D1G_STATIC_LDS.  RS: as onehot_train_chain_kernel.
template <int RS>
__global__ void __launch_bounds__(OT_THREADS)
decomp1_gated_max_chain_kernel(const OhTrainParams p, const D1GateParams g, const OhMaxParams m) {
    __shared__ __align__(16) float hv[OT_MAX_S], hb[OT_MAX_S];
    // [0], [1]: the shares of the gate products; then [0], [1], [2]: the shares' maximum, its entry and its index (as bits)
    __shared__ __align__(16) float part[3][OT_THREADS / 64][OT_MAX_S];
    extern __shared__ __align__(16) float dyn[];                       // Wss1 [S][S], Wss2 [S][S] (farnn 2), toks [L + 1]
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L, farnn = g.farnn;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int nr = min(rs, S - i0);                                    // rows of this share that exist (<= 0: none)
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    const float *G = dir == 0 ? p.M : p.MT;                            // max_j hbar[j] G[j][s]: Mc forward, Mc^T backward
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
    // every slot is loaded from a valid address (rows past S clamped to row S - 1, columns past S to column S - 1); what the
    // clamped slots hold is excluded from the comparison below, not zeroed
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
    // the share's maximum of v[i] G[i][j] over its rows, the entry there and its first row.  Slot 0 starts the scan (an empty
    // share's result is never read); a slot past nr can never win.  No fmaxf: the strict > keeps the first of equal candidates,
    // -0 and +0 included.
    auto maxvec = [&](const float *v, const float (&mm)[RS]) {
        float best = v[i0] * mm[0], be = mm[0];
        int bi = i0;
#pragma unroll
        for (int r = 1; r < RS; r++) {
            const float c = v[i0 + r] * mm[r];
            const bool take = r < nr && c > best;
            best = take ? c : best; be = take ? mm[r] : be; bi = take ? i0 + r : bi;
        }
        part[0][ks][j] = best; part[1][ks][j] = be; part[2][ks][j] = __int_as_float(bi);
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
    float *stash = dir == 0 ? p.A : p.Bk, *WIN = dir == 0 ? m.WINf : m.WINb;
    uint8_t *IDX = dir == 0 ? m.IDXf : m.IDXb;
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
        maxvec(hb, cur);
        wg_barrier_lds();
        if (ep) {
            float qv = part[0][0][j];
            int k = 0;
            for (int q = 1; q < nks && q * rs < S; q++) {            // the shares that have rows, in ascending row order
                const float v = part[0][q][j];
                if (v > qv) { qv = v; k = q; }
            }
            const float y = apply_nl(qv, p.nl);
            h = (1.0f - z) * h + z * y;
            g.Y[row] = y;
            const size_t srow = (row0 + t) * S + j;
            stash[srow] = h;
            IDX[srow] = (uint8_t)__float_as_int(part[2][k][j]);
            WIN[srow] = part[1][k][j];
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

// grid (B, 2), OT_THREADS; dynamic LDS decomp1_gated_lds_bytes; static LDS within D1G_STATIC_LDS.  DAZ / DAR are zero before.
// No block is gathered, so there are no register slots to size: one kernel for every S (the shares are the chain kernel's).
__global__ void __launch_bounds__(OT_THREADS)
decomp1_gated_max_bptt_kernel(const OhTrainParams p, const D1GateParams g, const OhMaxParams m) {
    __shared__ __align__(16) float uw[OT_MAX_S], azv[OT_MAX_S], arv[OT_MAX_S];
    __shared__ int jj[OT_MAX_S];
    __shared__ __align__(16) float part[3][OT_THREADS / 64][OT_MAX_S];
    extern __shared__ __align__(16) float dyn[];                       // Wss1^T [S][S], Wss2^T [S][S] (farnn 2)
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L, farnn = g.farnn;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int nr = min(rs, S - i0);
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    const size_t SS = (size_t)S * S, nS = (size_t)p.B * (L + 1) * S;
    float *W1 = dyn, *W2 = dyn + SS;
    for (int e = tid; e < (int)SS; e += OT_THREADS) {                  // (once per launch: the strided LDS writes do not matter)
        const int a = e / S, c = e - a * S;
        W1[c * S + a] = g.Wss1[e];
        if (farnn == 2) W2[c * S + a] = g.Wss2[e];
    }
    for (int s = tid; s < OT_MAX_S; s += OT_THREADS) { uw[s] = 0.0f; azv[s] = 0.0f; arv[s] = 0.0f; jj[s] = -1; }
    __syncthreads();
    const bool jok = j < S, ep = ks == 0 && jok;
    const int jc = jok ? j : S - 1;
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
    const float *gadj = dir == 0 ? p.GA : p.GB, *st = dir == 0 ? p.A : p.Bk, *WIN = dir == 0 ? m.WINf : m.WINb;
    const uint8_t *IDX = dir == 0 ? m.IDXf : m.IDXb;
    float *GM = dir == 0 ? m.GMf : m.GMb;
    // the block product's input: hbar of step t at row t - 1 of its stash (farnn 2), the state itself under farnn 1
    const float *hbs = farnn == 2 ? g.HB + d0 : st;
    const float hinit = dir == 0 ? p.h0[jc] : p.hT[jc];
    float carry = 0.0f, dinit = 0.0f;
    // what a step reads of its own rows, fetched one step ahead by the wavefronts that own a state (clamped column): the adjoint
    // of the step's output, the state before it, z, y, r, the winning entry, and hbar at the winning index
    struct Rows { float g, h, z, y, r, w, hb; int ix; };
    auto fetch = [&](Rows &w, int t) {
        if (ks != 0) return;
        const size_t row = (row0 + t) * S + jc;
        w.g = gadj[row]; w.h = st[row - S]; w.z = g.Z[d0 + row]; w.y = g.Y[d0 + row];
        w.r = farnn == 2 ? g.Rg[d0 + row] : 1.0f;
        w.w = WIN[row]; w.ix = IDX[row];
        w.hb = hbs[(row0 + t - 1) * S + min(w.ix, S - 1)];
    };
    Rows w0 = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0}, w1 = w0;
    if (nsteps > 0) fetch(w0, nsteps);
    auto step = [&](int t, const Rows &c, Rows &n) {
        if (t > 1) fetch(n, t - 1);
        const size_t row = d0 + (row0 + t) * S + jc;
        const float gt = c.g + carry;
        const float daz = g.k * c.z * (1.0f - c.z) * (gt * (c.y - c.h));
        const float u = (gt * c.z) * nl_grad_from_output(c.y, p.nl);
        if (ep) {
            GM[(row0 + t) * S + j] = u * c.hb;
            g.DAZ[row] = daz;
            uw[j] = u * c.w; jj[j] = c.ix;
            azv[j] = daz;
        }
        wg_barrier_lds();
        // dhbar: thread (ks, j) adds its share of the states whose index is j, ascending
        float a = 0.0f;
        for (int r = 0; r < nr; r++) a += jj[i0 + r] == j ? uw[i0 + r] : 0.0f;
        part[0][ks][j] = a;
        lds_matvec(azv, W1, part[1]);
        wg_barrier_lds();
        float dhbar = 0.0f, cg = 0.0f;
        if (ep) {
            dhbar = part[0][0][j];
            for (int q = 1; q < nks && q * rs < S; q++) dhbar += part[0][q][j];
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
        step(t, w0, w1);
        if (t - 1 >= 1) step(t - 1, w1, w0);
    }
    if (ep) g.HP[((size_t)b * 2 + dir) * S + j] = len > 0 ? gadj[row0 * S + j] + carry + dinit : 0.0f;
}

}  // namespace farnn
