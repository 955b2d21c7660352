// Training step of the onehot i-FST tagger (FARNN_S_O_I_S, --method onehot --independent 2): the CE1 loss and the
// gradient of language_tensor, by back-propagation through time over the stashed states.
//
// Reference: FARNN_S_O_I_S.forward_local(train=True) (model_onehot.py:131-146, 351-428; sum semiring, CE1 =
// nn.CrossEntropyLoss over the flattened valid positions) followed by loss.backward() (train_onehot.py:156-206).  Only
// language_tensor is trainable there (:330-332).  With M_w = T[w] + W (:370) and o = output_mat.sum(0) (:372):
//   forward chain   p_t = (f_{t-1} M_{x_t}) * o,          f_t = nl(p_t),  f_0 = h0           (:376-387)
//   backward chain  q_t = (b_{t-1} * o) M_{x'_t}^T,       b_t = nl(q_t),  b_0 = hT, x' = reverse(x, len)  (:390-401)
//   score_i = output_mat (f_{i+1} * b_{len-1-i}) [. P]                                      (:339-342,:404-426)
//   dT[w] = sum_{fwd t: x_t = w} f_{t-1}^T (dp_t * o) + sum_{bwd t: x'_t = w} dq_t^T (b_{t-1} * o)
// The scores, the cross-entropy, the decode and the adjoints of alpha / beta are train_loss_kernel<., 0> of train.hip.h
// with output_mat in C_output_mat's place; this header adds the chains and the per-word reduction.
//
// Chains: one workgroup per sequence and direction, 8 wavefronts.  A step is one row-vector x S x S product: a thread
// owns column j and a share of the rows, keeps its share of the NEXT token's matrix in registers (gathered one step
// ahead, the barriers wait for LDS only), and the shares meet in LDS.  Products with M (forward chain, the backward
// chain's back-propagation) gather M, products with M^T gather MT: both premixed for every word once per step
// (onehot_premix_kernel), as T changes at every optimizer step and no layout of the tagging handle can serve.  (Adding W
// while gathering T saves the premix of M, but the W slice took 32 more registers per thread: at S > 96 the chain
// kernels then spilled -- 256 VGPRs, 18 / 50 spilled, 76 / 92 bytes of scratch.)
// dT: the valid positions are bucketed by word with a stable counting sort (integer atomics count; the order inside a
// bucket is the flat position order, fixed), and every word's rows are reduced in (sequence, position, direction) order
// by one workgroup per run of OT_G positions; a word with several runs adds their partial tiles in run order.  No float
// atomics anywhere: two steps on the same inputs are bit-identical.
#pragma once
#include "common.hip.h"
#include "train.hip.h"

namespace farnn {

constexpr int OT_THREADS = 512;   // chain kernels: 8 wavefronts
constexpr int OT_MAX_S = 128;     // columns: 64 or 128 lanes; rows split over 8 or 4 shares
constexpr int OT_G = 32;          // positions per dT workgroup
constexpr int OT_CH = 256;        // positions per bucketing chunk

struct OhTrainParams {
    const float *M, *MT, *o, *h0, *hT;       // M [V][S][S] = T + W, MT [V][S][S] (MT[w] = M[w]^T), o [S]
    const int64_t *x, *len;
    float *A, *Bk;            // [B][L+1][S] f_t after t tokens (A[.][0] = h0), b_t after t reversed tokens (Bk[.][0] = hT)
    float *GA, *GB;           // [B][L+1][S] d loss / d A, d loss / d Bk from the scoring (train_loss_kernel)
    float *UF, *DQ;           // [B][L+1][S] dp_t * o (forward chain), dq_t (backward chain), per step t
    int B, L, V, S, nl;
};

__device__ __forceinline__ int oh_token(const int64_t *x, int V, long long idx) {
    const long long v = x[idx];
    return v < 0 ? 0 : (v >= V ? V - 1 : (int)v);          // out-of-range ids are flagged by the bucketing kernel
}

// The chains.  BPTT = 0: forward pass with the stash (dir 0 forward chain over t = 1..len, dir 1 backward chain over
// t = 1..len-1; b_len feeds no score).  BPTT = 1: the same chains in reverse, writing UF / DQ.
// RS: register slots per thread for its share of rows (rows per share = ceil(S / shares) <= RS).
template <int RS, bool BPTT>
__global__ void __launch_bounds__(OT_THREADS)
onehot_train_chain_kernel(const OhTrainParams p) {
    __shared__ __align__(16) float vin[2][OT_MAX_S];
    __shared__ __align__(16) float part[OT_THREADS / 64][OT_MAX_S];
    __shared__ float os[OT_MAX_S];
    extern __shared__ int toks[];                           // [L + 1]: the token of step t (t = 1..)
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int S = p.S, L = p.L;
    const int ncol = S > 64 ? 128 : 64, lc = S > 64 ? 7 : 6;
    const int nks = OT_THREADS >> lc, j = tid & (ncol - 1), ks = tid >> lc;
    const int rs = (S + nks - 1) / nks, i0 = ks * rs;
    const int len = clamp_len(p.len[b], L);
    const int nsteps = dir == 0 ? len : (len > 0 ? len - 1 : 0);
    // M when the product is f M (forward pass, dir 0) or dq M (back-propagation, dir 1); M^T otherwise
    const float *G = (dir == 0) != BPTT ? p.M : p.MT;
    const size_t SS = (size_t)S * S;
    for (int t = tid; t < nsteps; t += blockDim.x)
        toks[t + 1] = oh_token(p.x, p.V, (long long)b * L + (dir == 0 ? t : len - 1 - t));
    for (int s = tid; s < OT_MAX_S; s += blockDim.x) {
        os[s] = s < S ? p.o[s] : 0.0f;
        vin[0][s] = 0.0f; vin[1][s] = 0.0f;            // rows past S meet zero matrix slots: no stale NaN may reach a sum
    }
    __syncthreads();
    const bool jok = j < S;
    // Every slot is loaded unconditionally from a valid address: rows past S are clamped to row S-1 (their inputs in vin
    // are zero), columns past S to column S-1 (never stored), slots past rs read rows the matvec skips.  (Predicated
    // loads compiled to a branch per slot, and the merges made the wait for the step's matrix drain the prefetch too.)
    const int jc = jok ? j : S - 1;
    auto gather = [&](float (&m)[RS], int tok) {
        const float *src = G + (size_t)__builtin_amdgcn_readfirstlane(tok) * SS;    // scalar base, one VGPR offset
        int off = i0 * S + jc;
        const int last = (S - 1) * S + jc;
#pragma unroll
        for (int r = 0; r < RS; r++) {
            asm volatile("" : "+v"(off));       // (opaque: hoisted out of the step loop, each row's offset took a register)
            m[r] = src[min(off, last)];
            off += S;
        }
    };
    // part[ks][j] = sum over this share of rows i of v[i] M[i][j]
    auto matvec = [&](const float *v, const float (&m)[RS]) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int r = 0; r < RS; r += 2) {
            if (r < rs) a0 = fmaf(v[i0 + r], m[r], a0);
            if (r + 1 < rs) a1 = fmaf(v[i0 + r + 1], m[r + 1], a1);
        }
        part[ks][j] = a0 + a1;
    };
    auto shares = [&]() {
        float s = 0.0f;
        for (int k = 0; k < nks; k++) s += part[k][j];
        return s;
    };
    const size_t row0 = (size_t)b * (L + 1);
    // two register sets in turn (no copy of a set whose loads are still in flight: a copy waits for them)
    float m0[RS], m1[RS];
    if (!BPTT) {
        float *stash = dir == 0 ? p.A : p.Bk;
        if (ks == 0 && jok) {
            const float init = dir == 0 ? p.h0[j] : p.hT[j];
            stash[row0 * S + j] = init;
            vin[0][j] = dir == 0 ? init : init * os[j];
        }
        if (nsteps > 0) gather(m0, toks[1]);
        wg_barrier_lds();
        auto step = [&](int t, const float (&cur)[RS], float (&nxt)[RS]) {
            if (t < nsteps) gather(nxt, toks[t + 1]);
            matvec(vin[(t - 1) & 1], cur);
            wg_barrier_lds();
            if (ks == 0 && jok) {
                const float y = shares();
                const float h = dir == 0 ? apply_nl(y * os[j], p.nl) : apply_nl(y, p.nl);
                stash[(row0 + t) * S + j] = h;
                vin[t & 1][j] = dir == 0 ? h : h * os[j];
            }
            wg_barrier_lds();
        };
        for (int t = 1; t <= nsteps; t += 2) {
            step(t, m0, m1);
            if (t + 1 <= nsteps) step(t + 1, m1, m0);
        }
    } else {
        // dir 0: u_t = (GA_t + carry) nl'(f_t) o -> UF_t, carry = u_t M_{x_t}^T   (gathered from MT)
        // dir 1: dq_t = (GB_t + carry) nl'(b_t)  -> DQ_t, carry = (dq_t M_{x'_t}) o (gathered from M)
        const float *gadj = dir == 0 ? p.GA : p.GB, *st = dir == 0 ? p.A : p.Bk;
        float *outr = dir == 0 ? p.UF : p.DQ;
        float carry = 0.0f, g0 = 0.0f, s0 = 0.0f, g1 = 0.0f, s1 = 0.0f;
        const bool ep = ks == 0 && jok;
        // the adjoint and state rows of a step are fetched one step ahead by every thread (clamped column), into the
        // register pair of that step's parity: loads under the epilogue's branch, or a copy of a pending pair, made the
        // wait at the top of a step drain the matrix prefetch as well
        if (nsteps > 0) {
            gather(m0, toks[nsteps]);
            g0 = gadj[(row0 + nsteps) * S + jc]; s0 = st[(row0 + nsteps) * S + jc];
        }
        // step t: the adjoint row of step t, then (t > 1) the carry into step t - 1 through step t's matrix
        auto step = [&](int t, const float (&cur)[RS], float (&nxt)[RS], const float &gc, const float &sc, float &gx, float &sx) {
            const int buf = t & 1;
            const float g = gc + carry, y = sc;
            gx = gadj[(row0 + t - 1) * S + jc]; sx = st[(row0 + t - 1) * S + jc];     // (row t - 1 = 0 exists: unused)
            float u = g * nl_grad_from_output(y, p.nl);
            if (dir == 0) u *= os[jc];
            if (ep) {
                outr[(row0 + t) * S + j] = u;
                vin[buf][j] = u;
            }
            if (t == 1) return;
            if (t > 2) gather(nxt, toks[t - 1]);
            wg_barrier_lds();
            matvec(vin[buf], cur);
            wg_barrier_lds();
            if (ep) carry = dir == 0 ? shares() : shares() * os[j];
        };
        for (int t = nsteps; t >= 1; t -= 2) {
            step(t, m0, m1, g0, s0, g1, s1);
            if (t - 1 >= 1) step(t - 1, m1, m0, g1, s1, g0, s0);
        }
    }
}

// M[w] = T[w] + W and MT[w] = M[w]^T: one 32 x 32 tile per workgroup of 256 threads (reads and writes along rows)
__global__ void __launch_bounds__(256)
onehot_premix_kernel(const float *__restrict__ T, const float *__restrict__ W, float *__restrict__ M, float *__restrict__ MT,
                     int S) {
    __shared__ float tile[32][33];
    const int nt = (S + 31) >> 5, w = blockIdx.x / (nt * nt), tt = blockIdx.x - w * nt * nt;
    const int r0 = (tt / nt) * 32, c0 = (tt % nt) * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t base = (size_t)w * S * S;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        const float v = (r < S && c < S) ? T[base + r * S + c] + W[r * S + c] : 0.0f;
        if (r < S && c < S) M[base + r * S + c] = v;
        tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (r < S && c < S) MT[base + c * S + r] = tile[tx][ty + 8 * k];
    }
}

// ---- bucketing of the valid positions by word (a stable counting sort) ----------------------------------------
// cnt[w * nch + chunk] = number of valid positions of word w in chunk (OT_CH flat positions b * L + i)
__global__ void __launch_bounds__(OT_CH)
onehot_bucket_count_kernel(const int64_t *__restrict__ x, const int64_t *__restrict__ len, int B, int L, int V, int nch,
                           int *cnt, int *err) {
    const long long pos = (long long)blockIdx.x * OT_CH + threadIdx.x;
    if (pos >= (long long)B * L) return;
    const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
    if (i >= clamp_len(len[b], L)) return;
    const long long v = x[pos];
    if ((v < 0 || v >= V) && err) atomicOr(err, 2);
    atomicAdd(&cnt[(size_t)oh_token(x, V, pos) * nch + blockIdx.x], 1);
}

// in-place exclusive scan of n ints by one workgroup of 1024 threads (each thread a contiguous run); returns the total
__device__ int oh_block_scan(int *a, int n, int *red) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per = (n + nt - 1) / nt, lo = min(n, tid * per), hi = min(n, lo + per);
    int s = 0;
    for (int k = lo; k < hi; k++) s += a[k];
    red[tid] = s;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {                 // Hillis-Steele inclusive scan of the run sums
        const int v = tid >= off ? red[tid - off] : 0;
        __syncthreads();
        red[tid] += v;
        __syncthreads();
    }
    const int total = red[nt - 1];
    int run = red[tid] - s;
    for (int k = lo; k < hi; k++) { const int v = a[k]; a[k] = run; run += v; }
    __syncthreads();
    return total;
}

// cnt -> offsets (word-major, chunk-minor); per word: first slot, count, dT runs (at least one: absent words get a
// zero tile) and the partial-tile slots of words with more than one run
// (the counts are scanned in LDS when they fit -- lds_n = V nch -- else in place in global memory: 97 us at ATIS size)
__global__ void __launch_bounds__(1024)
onehot_bucket_scan_kernel(int *cnt, int V, int nch, int *wstart, int *wcount, int *itoff, int *psoff, int lds_n) {
    __shared__ int red[1024];
    extern __shared__ int cl[];
    const int n = V * nch;
    int *a = cnt;
    if (lds_n >= n) {
        for (int k0 = threadIdx.x; k0 < n; k0 += 8 * blockDim.x) {     // eight loads in flight per thread
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int k = k0 + u * blockDim.x; v[u] = k < n ? cnt[k] : 0; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const int k = k0 + u * blockDim.x; if (k < n) cl[k] = v[u]; }
        }
        __syncthreads();
        a = cl;
    }
    const int total = oh_block_scan(a, n, red);
    if (a != cnt)
        for (int k = threadIdx.x; k < n; k += blockDim.x) cnt[k] = cl[k];
    __syncthreads();
    for (int w = threadIdx.x; w < V; w += blockDim.x) {
        const int st = cnt[(size_t)w * nch], en = w + 1 < V ? cnt[(size_t)(w + 1) * nch] : total;
        const int n = en - st, runs = n > OT_G ? (n + OT_G - 1) / OT_G : 1;
        wstart[w] = st; wcount[w] = n;
        itoff[w] = runs;
        psoff[w] = runs > 1 ? runs : 0;
    }
    __syncthreads();
    const int nit = oh_block_scan(itoff, V, red);
    const int nps = oh_block_scan(psoff, V, red);
    if (threadIdx.x == 0) { itoff[V] = nit; psoff[V] = nps; }
}

// list[offset of (word, chunk) + rank among the chunk's earlier positions of that word] = flat position
__global__ void __launch_bounds__(OT_CH)
onehot_bucket_fill_kernel(const int64_t *__restrict__ x, const int64_t *__restrict__ len, int B, int L, int V, int nch,
                          const int *__restrict__ off, int *list) {
    __shared__ int wd[OT_CH];
    const long long pos = (long long)blockIdx.x * OT_CH + threadIdx.x;
    int w = -1;
    if (pos < (long long)B * L) {
        const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
        if (i < clamp_len(len[b], L)) w = oh_token(x, V, pos);
    }
    wd[threadIdx.x] = w;
    __syncthreads();
    if (w < 0) return;
    int rank = 0;
    for (int q = 0; q < (int)threadIdx.x; q++) rank += wd[q] == w;
    list[off[(size_t)w * nch + blockIdx.x] + rank] = (int)pos;
}

// The same two passes over EVERY one of the B L positions, the pads included: the max-semiring step of the decomposed i-FST
// with a KD / PR teacher runs its chains through the pad tokens x[b, len:] (train_max.hip.h), so a word that occurs only there
// needs its block and its bucket too.  An id outside 0..V-1 is flagged at a pad as at a valid position (the reference's
// V_embed[inp] indexes the pads as well).  A second pair, not a flag: the pair above is launched by every other step and its
// code objects stay what they were.
__global__ void __launch_bounds__(OT_CH)
onehot_bucket_count_all_kernel(const int64_t *__restrict__ x, int B, int L, int V, int nch, int *cnt, int *err) {
    const long long pos = (long long)blockIdx.x * OT_CH + threadIdx.x;
    if (pos >= (long long)B * L) return;
    const long long v = x[pos];
    if ((v < 0 || v >= V) && err) atomicOr(err, 2);
    atomicAdd(&cnt[(size_t)oh_token(x, V, pos) * nch + blockIdx.x], 1);
}
__global__ void __launch_bounds__(OT_CH)
onehot_bucket_fill_all_kernel(const int64_t *__restrict__ x, int B, int L, int V, int nch, const int *__restrict__ off,
                              int *list) {
    __shared__ int wd[OT_CH];
    const long long pos = (long long)blockIdx.x * OT_CH + threadIdx.x;
    const int w = pos < (long long)B * L ? oh_token(x, V, pos) : -1;
    wd[threadIdx.x] = w;
    __syncthreads();
    if (w < 0) return;
    int rank = 0;
    for (int q = 0; q < (int)threadIdx.x; q++) rank += wd[q] == w;
    list[off[(size_t)w * nch + blockIdx.x] + rank] = (int)pos;
}

// ---- dT: one workgroup per run of up to OT_G positions of one word --------------------------------------------
// The run's rows are staged in LDS -- per position: f_{t-1} = A[i] and dp_t o = UF[i+1] (forward, t = i+1), dq_t = DQ[len-i]
// and b_{t-1} o = Bk[len-i-1] o (backward, t = len-i, i >= 1) -- then thread (ty, tx) of 16 x 16 adds the rank-one
// updates of rows ty + 16a, columns tx + 16c (a, c < NT) in position order, forward before backward.
// LDS: 4 [OT_G][S]
template <int NT>
__global__ void __launch_bounds__(256)
onehot_dT_kernel(const OhTrainParams p, const int *__restrict__ list,
                 const int *__restrict__ wstart, const int *__restrict__ wcount, const int *__restrict__ itoff,
                 const int *__restrict__ psoff, float *dT, float *partial) {
    extern __shared__ __align__(16) float sm[];
    const int item = blockIdx.x, V = p.V, S = p.S, L = p.L;
    if (item >= itoff[V]) return;
    int lo = 0, hi = V - 1;                                   // the word whose runs contain this item
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (itoff[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int w = lo, k = item - itoff[w], runs = itoff[w + 1] - itoff[w];
    const int n0 = k * OT_G, n = min(OT_G, wcount[w] - n0);
    float *Lf = sm, *Rf = Lf + OT_G * S, *Lb = Rf + OT_G * S, *Rb = Lb + OT_G * S;
    for (int e = threadIdx.x; e < n * S; e += blockDim.x) {
        const int q = e / S, s = e - q * S;
        const int pos = list[wstart[w] + n0 + q];
        const int b = pos / L, i = pos - b * L, len = clamp_len(p.len[b], L);
        const size_t row0 = (size_t)b * (L + 1);
        Lf[e] = p.A[(row0 + i) * S + s];
        Rf[e] = p.UF[(row0 + i + 1) * S + s];
        const bool bw = i >= 1;
        Lb[e] = bw ? p.DQ[(row0 + len - i) * S + s] : 0.0f;
        Rb[e] = bw ? p.Bk[(row0 + len - i - 1) * S + s] * p.o[s] : 0.0f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int c = 0; c < NT; c++) acc[a][c] = 0.0f;
    for (int q = 0; q < n; q++) {
        float lf[NT], rf[NT], lb[NT], rb[NT];
#pragma unroll
        for (int a = 0; a < NT; a++) {
            const int r = ty + 16 * a, c = tx + 16 * a;
            lf[a] = r < S ? Lf[q * S + r] : 0.0f; lb[a] = r < S ? Lb[q * S + r] : 0.0f;
            rf[a] = c < S ? Rf[q * S + c] : 0.0f; rb[a] = c < S ? Rb[q * S + c] : 0.0f;
        }
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int c = 0; c < NT; c++) acc[a][c] = fmaf(lb[a], rb[c], fmaf(lf[a], rf[c], acc[a][c]));
    }
    float *out = runs > 1 ? partial + (size_t)(psoff[w] + k) * S * S : dT + (size_t)w * S * S;
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int c = 0; c < NT; c++) {
            const int r = ty + 16 * a, cc = tx + 16 * c;
            if (r < S && cc < S) out[r * S + cc] = acc[a][c];
        }
}

// dT[w] = sum of the word's partial tiles in run order (words with more than one run only); grid (V, ceil(S S / 256)),
// one element per thread: the runs' loads of an element are independent and in flight together, the adds keep run order
__global__ void __launch_bounds__(256)
onehot_dT_reduce_kernel(const int *__restrict__ itoff, const int *__restrict__ psoff, const float *__restrict__ partial,
                        float *dT, int S) {
    const int w = blockIdx.x, runs = itoff[w + 1] - itoff[w];
    const size_t SS = (size_t)S * S, e = (size_t)blockIdx.y * 256 + threadIdx.x;
    if (runs <= 1 || e >= SS) return;
    const float *src = partial + (size_t)psoff[w] * SS + e;
    float s = 0.0f;
    int k = 0;
    for (; k + 8 <= runs; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = src[(k + u) * SS];
#pragma unroll
        for (int u = 0; u < 8; u++) s += v[u];
    }
    for (; k < runs; k++) s += src[k * SS];
    dT[w * SS + e] = s;
}

// loss = sum of the loss kernel's per-wavefront partials in index order (one wavefront, a fixed tree)
__global__ void __launch_bounds__(64)
onehot_loss_sum_kernel(const float *__restrict__ part, int n, float *loss) {
    const int lane = threadIdx.x;
    float s = 0.0f;
    int k = lane;
    for (; k + 7 * WAVE < n; k += 8 * WAVE) {                 // eight loads in flight, added in index order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = part[k + u * WAVE];
#pragma unroll
        for (int u = 0; u < 8; u++) s += v[u];
    }
    for (; k < n; k += WAVE) s += part[k];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, WAVE);
    if (lane == 0) loss[0] = s;
}

}  // namespace farnn
