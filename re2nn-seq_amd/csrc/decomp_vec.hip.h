// The per-call TOKEN TABLE of the vector-input i-FST tagger (FARNN_S_SF, model_decompose_single.py:307-579): the recurrence
// kernels fetch one row per token from a table indexed by a word id; here the batch brings its own vectors, v[B][L][R], so the
// table is built from them on every call -- one row per (sequence, position), in the layout decomp_rows_kernel reads:
//
//   TT[b L + t] = [ v[b][t] padded to Rp with zeros | v . Wrs1 + bs1 (SP, farnn >= 1) | v . Wrs2 + bs2 (SP, farnn == 2) ]
//
// and the recurrence then runs on the identity ids b L + t with V = B L.  Rows at t >= lengths[b] are neither read from v nor
// written: no kernel behind this one fetches them (a pad row of v may hold anything, NaN included).
//
// The gate halves are a [B L] x [R] x [ng SP] product.  Every ENTRY is accumulated exactly like gate_table_kernel
// (decomp_rows.hip.h) accumulates it -- fmaf over r = 0 .. R-1 in order from 0, then + bs[j], zero for j >= S -- so that a
// vector that is a row of Vgen gets the bits the id path's create-time table holds for that word: tiles and LDS staging only
// decide WHO computes an entry and where its operands come from, never the order of its sum; no matrix-core instruction, no
// split of the r loop between lanes.
//
// A workgroup of 256 threads owns 128 tokens x 64 gate columns; a thread 8 tokens x 4 columns (32 accumulators).  Per 32
// ranks the tile of v lies in LDS transposed ([rank][token]: a thread's tokens are two 16-byte reads) beside the tile of
// [Wrs1 | Wrs2] ([rank][column]: one 16-byte read); per rank a thread issues three ds_read_b128 for 32 FMAs.  The workgroups
// of column block 0 also write the vector segment as they stage it.  At B L = 16 384, R = 250, S = 160, farnn = 2 that is
// 128 x 5 workgroups, 2.6 GFLOP and 16 MB of v + 37 MB of table: bound by f32 FMA issue, not by HBM and not by LDS (three
// reads = 12 LDS cycles per wavefront and rank, four wavefronts per LDS: 48 cycles against 64 of FMA issue per SIMD).
#pragma once
#include "common.hip.h"
#include "host_util.hip.h"

namespace farnn {

constexpr int TV_THREADS = 256;
constexpr int TV_TOK = 128;           // tokens per workgroup
constexpr int TV_COL = 64;            // gate columns per workgroup
constexpr int TV_KC = 32;             // ranks staged per round
constexpr int TV_LDV = TV_TOK + 4;    // row stride (floats) of the staged v tile: 16-byte aligned rows, the 32 ranks of a store spread over the banks

struct TokenTableParams {
    const float *v;               // [B][L][R] dense
    const int64_t *len;           // [B]
    const float *Wrs1, *bs1;      // [R][SP], [SP]  (farnn >= 1)
    const float *Wrs2, *bs2;      //                (farnn == 2)
    float *TT;                    // [B L][tvl]
    int B, L, R, Rp, S, SP, tvl;
    int ncols;                    // gate columns: 0, SP or 2 SP
};

// GATES = false (farnn = 0): the padded copy alone
template <bool GATES>
__global__ void __launch_bounds__(TV_THREADS)
token_table_kernel(const TokenTableParams p) {
    __shared__ __align__(16) float Vs[GATES ? TV_KC * TV_LDV : 4];
    __shared__ __align__(16) float Ws[GATES ? TV_KC * TV_COL : 4];
    __shared__ int okl[TV_TOK];
    const int tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * TV_TOK, NT = (long long)p.B * p.L;
    const int c0 = blockIdx.y * TV_COL;
    const bool copy = blockIdx.y == 0;
    int mine = 0;
    if (tid < TV_TOK) {
        const long long n = n0 + tid;
        if (n < NT) mine = (int)(n % p.L) < clamp_len(p.len[n / p.L], p.L);
        okl[tid] = mine;
    }
    if (!__syncthreads_or(mine)) return;                      // a tile of pad positions only

    const int tx = tid & 15, ty = tid >> 4;                   // this thread's columns c0 + 4 tx .., tokens 4 ty .. and 64 + 4 ty ..
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[i][q] = 0.0f;

    for (int k0 = 0; k0 < p.Rp; k0 += TV_KC) {
        // ---- stage v[tokens][k0 .. k0 + 32) (transposed), writing the table's vector segment on the way ----
        const int kk = tid & (TV_KC - 1), col = k0 + kk;
#pragma unroll
        for (int i = 0; i < TV_TOK / 32; i++) {
            const int tg = (tid >> 5) + 8 * i;                // a group of four tokens
            v4f val;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int tl = tg * 4 + q;
                const long long n = n0 + tl;
                const bool ok = okl[tl] != 0;
                const float x = (ok && col < p.R) ? p.v[n * p.R + col] : 0.0f;
                if (copy && ok && col < p.Rp) p.TT[n * p.tvl + col] = x;
                val[q] = x;
            }
            if constexpr (GATES) *reinterpret_cast<v4f *>(&Vs[kk * TV_LDV + tg * 4]) = val;
        }
        if constexpr (GATES) {
            // ---- stage [Wrs1 | Wrs2][k0 .. k0 + 32)[c0 .. c0 + 64) ----
#pragma unroll
            for (int i = 0; i < TV_KC * TV_COL / TV_THREADS; i++) {
                const int e = tid + i * TV_THREADS, wk = e >> 6, cc = e & 63, c = c0 + cc;
                float w = 0.0f;
                if (c < p.ncols && k0 + wk < p.R) {
                    const bool second = c >= p.SP;
                    w = (second ? p.Wrs2 : p.Wrs1)[(long long)(k0 + wk) * p.SP + (second ? c - p.SP : c)];
                }
                Ws[wk * TV_COL + cc] = w;
            }
            __syncthreads();
            // (the ranks past R are not run: fmaf(0, 0, acc) is acc for every acc but -0)
            const int kn = p.R - k0 < TV_KC ? p.R - k0 : TV_KC;
#pragma unroll 4
            for (int k = 0; k < kn; k++) {
                const v4f a0 = *reinterpret_cast<const v4f *>(&Vs[k * TV_LDV + ty * 4]);
                const v4f a1 = *reinterpret_cast<const v4f *>(&Vs[k * TV_LDV + 64 + ty * 4]);
                const v4f w = *reinterpret_cast<const v4f *>(&Ws[k * TV_COL + tx * 4]);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        acc[i][q] = fmaf(a0[i], w[q], acc[i][q]);
                        acc[4 + i][q] = fmaf(a1[i], w[q], acc[4 + i][q]);
                    }
            }
            __syncthreads();
        }
    }
    if constexpr (GATES) {
        const int c = c0 + tx * 4;                            // SP is a multiple of 4: the four columns lie in one gate
        if (c >= p.ncols) return;
        const bool second = c >= p.SP;
        const int j = second ? c - p.SP : c;
        const float *bs = second ? p.bs2 : p.bs1;
        float b[4];
#pragma unroll
        for (int q = 0; q < 4; q++) b[q] = j + q < p.S ? bs[j + q] : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int tl = (i < 4 ? 0 : 64) + ty * 4 + (i & 3);
            if (!okl[tl]) continue;
            v4f out;
#pragma unroll
            for (int q = 0; q < 4; q++) out[q] = j + q < p.S ? acc[i][q] + b[q] : 0.0f;
            *reinterpret_cast<v4f *>(&p.TT[(n0 + tl) * p.tvl + p.Rp + c]) = out;
        }
    }
}

// ids[i] = i: with them x[b L + t] = b L + t names the token's own row, whatever the call's L
__global__ void iota_kernel(int64_t *ids, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = i;
}

inline int launch_token_table(const TokenTableParams &p, hipStream_t s) {
    const long long NT = (long long)p.B * p.L;
    const unsigned gx = (unsigned)((NT + TV_TOK - 1) / TV_TOK);
    if (p.ncols > 0) token_table_kernel<true><<<dim3(gx, (p.ncols + TV_COL - 1) / TV_COL), dim3(TV_THREADS), 0, s>>>(p);
    else token_table_kernel<false><<<dim3(gx, 1), dim3(TV_THREADS), 0, s>>>(p);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

}  // namespace farnn
