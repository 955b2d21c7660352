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

// ---- the per-call TOKEN BLOCKS of the vector-input tagger in the max semiring (model_decompose_single.py:435-442) -------------
// h' = max_j hbar[j] Tr[j][s] needs the step's whole transition matrix, Tr[n] = S1 diag(v[n]) S2^T + W, and with vectors that are
// rows of no table that is one S x S block per TOKEN and per call: a [B L S] x [R] x [S] product (51 GFLOP over the 9 516 valid tokens
// of a ragged 256 x 64 batch at S = 104, R = 250) in front of the dense chain kernels, which then read the blocks exactly as they read an id handle's per-word
// blocks -- layout [SR][SP] per block, pads zero, Mf[n][i][j] = Tr[i][j] and Mb[n][j][i] = Tr[i][j] -- on the identity ids.
//
// Every ENTRY is accumulated exactly like materialise_blocks_kernel (layout.hip.h) accumulates it for a word: the product
// v[r] S1[i][r] rounded on its own, fmaf with S2[j][r] over r = 0 .. R-1 in order from 0, then + W[i][j].  A vector that is a row of
// Vgen gets the bits of that word's create-time block.  So, as in token_table_kernel: no matrix-core instruction, no split of the
// r loop between lanes; the tile only decides who computes an entry.
//
// One workgroup per valid token and 128 x 128 tile of its block (one tile up to S = 128); n8 = ceil(min(S, 128) / 8) and
// n8 x n8 threads (169 at S = 104, launched as 192), a thread 8 x 8 accumulators: rows {4 ti .., 4 n8 + 4 ti ..}, columns
// {4 tj .., 4 n8 + 4 tj ..}, so that the lanes of a wavefront read contiguous 16-byte pieces of a staged row.  Per 32 ranks the
// A operand, S1^T's tile scaled by v[n] ([rank][i]: the product is rounded once, by the thread that stages it), lies in LDS beside
// S2^T's tile ([rank][j]); per rank a thread issues four ds_read_b128 for 64 FMAs.  S1^T and S2^T (208 KB at S = 104, R = 250) stay
// in L2: a token re-stages them, 26 flops per byte staged, well under what a compute unit's L2 port delivers -- so one token per
// workgroup, no token loop inside it, and the ragged batch balances itself.  LDS: 2 x 32 x 132 floats = 33 KiB static (four
// workgroups per compute unit); the epilogue's transpose tile aliases it.  The epilogue adds W, stores Mf's rows as 16-byte pieces
// and passes each 4 n8 x 4 n8 quadrant through LDS transposed, so that Mb's rows leave as contiguous runs as well; the tile of
// (0, 0) also zeroes the pad rows S .. SR-1 of both images.
// By design bound by f32 FMA issue: 64 FMAs against 4 LDS reads (16 LDS cycles per wavefront and rank, three wavefronts per
// workgroup) and, per token, 2 SR SP 4 bytes of stores (92 KB at S = 104) against 5.4 MFLOP at R = 250.  Measured (256 x 64 ragged,
// S = 104, profiles/sf_max_tag_timing.json): R = 250 1 026 us, 50 TFLOP/s, 38 % of the packed-FMA rate -- the single staging buffer
// and its two barriers per round, not the FMA pipe, set the pace; R = 50 315 us, bound by the 871 MB of stores.
constexpr int TB_TILE = 128;          // rows and columns of a block per workgroup
constexpr int TB_KC = 32;             // ranks staged per round
constexpr int TB_LD = TB_TILE + 4;    // row stride (floats) of the staged tiles: 16-byte aligned rows
constexpr int TB_LDT = 68;            // row stride of the epilogue's transpose tile (a quadrant is at most 64 x 64)
constexpr int TB_MAX_THREADS = 256;

struct TokenBlocksParams {
    const float *v;               // [B][L][R] dense
    const int64_t *len;           // [B]
    const float *S1T, *S2T;       // [R][SP]
    const float *W;               // [S][SP]
    float *Mf, *Mb;               // [B L][SR][SP]
    int B, L, R, S, SP, SR;
    int n8, ntile;                // threads per side; 128-wide tiles per side
};

__global__ void __launch_bounds__(TB_MAX_THREADS)
token_blocks_kernel(const TokenBlocksParams p) {
    __shared__ __align__(16) float smem[2 * TB_KC * TB_LD];
    float *As = smem, *Bs = smem + TB_KC * TB_LD;
    const long long n = blockIdx.x;
    if ((int)(n % p.L) >= clamp_len(p.len[n / p.L], p.L)) return;             // a pad position: neither read nor written
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int i0 = ((int)blockIdx.y / p.ntile) * TB_TILE, j0 = ((int)blockIdx.y % p.ntile) * TB_TILE;
    const int n8 = p.n8, H = 4 * n8;
    const bool active = tid < n8 * n8;
    const int ti = active ? tid / n8 : 0, tj = active ? tid - ti * n8 : 0;
    const int S = p.S, SP = p.SP, R = p.R;
    const float *vn = p.v + n * R;

    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; a++)
#pragma unroll
        for (int q = 0; q < 8; q++) acc[a][q] = 0.0f;

    for (int k0 = 0; k0 < R; k0 += TB_KC) {
        // ---- stage A = v[n][k] S1T[k][i0 ..) and B = S2T[k][j0 ..): 32 ranks x 32 pieces of four, zero past SP and past R ----
        for (int e = tid; e < TB_KC * (TB_TILE / 4); e += nthr) {
            const int k = e >> 5, c = (e & 31) * 4, r = k0 + k;
            v4f a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
            if (r < R) {
                if (i0 + c < SP) {
                    const v4f s1 = *reinterpret_cast<const v4f *>(&p.S1T[(long long)r * SP + i0 + c]);
                    const float x = vn[r];
#pragma unroll
                    for (int q = 0; q < 4; q++) a[q] = x * s1[q];
                }
                if (j0 + c < SP) b = *reinterpret_cast<const v4f *>(&p.S2T[(long long)r * SP + j0 + c]);
            }
            *reinterpret_cast<v4f *>(&As[k * TB_LD + c]) = a;
            *reinterpret_cast<v4f *>(&Bs[k * TB_LD + c]) = b;
        }
        __syncthreads();
        if (active) {
            // (the ranks past R are not run: fmaf(0, 0, acc) is acc for every acc but -0)
            const int kn = R - k0 < TB_KC ? R - k0 : TB_KC;
#pragma unroll 2
            for (int k = 0; k < kn; k++) {
                const v4f a0 = *reinterpret_cast<const v4f *>(&As[k * TB_LD + ti * 4]);
                const v4f a1 = *reinterpret_cast<const v4f *>(&As[k * TB_LD + H + ti * 4]);
                const v4f b0 = *reinterpret_cast<const v4f *>(&Bs[k * TB_LD + tj * 4]);
                const v4f b1 = *reinterpret_cast<const v4f *>(&Bs[k * TB_LD + H + tj * 4]);
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        acc[a][q] = fmaf(a0[a], b0[q], acc[a][q]);
                        acc[a][4 + q] = fmaf(a0[a], b1[q], acc[a][4 + q]);
                        acc[4 + a][q] = fmaf(a1[a], b0[q], acc[4 + a][q]);
                        acc[4 + a][4 + q] = fmaf(a1[a], b1[q], acc[4 + a][4 + q]);
                    }
            }
        }
        __syncthreads();
    }

    const long long base = n * (long long)p.SR * SP;
    // ---- + W; zero outside S x S; Mf's rows ----
    if (active) {
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const int i = i0 + (a < 4 ? 0 : H) + ti * 4 + (a & 3);
#pragma unroll
            for (int hq = 0; hq < 2; hq++) {
                const int j = j0 + hq * H + tj * 4;
                v4f out = {0.0f, 0.0f, 0.0f, 0.0f};
                if (i < S && j < SP) {
                    const v4f w = *reinterpret_cast<const v4f *>(&p.W[(long long)i * SP + j]);
#pragma unroll
                    for (int q = 0; q < 4; q++) out[q] = j + q < S ? acc[a][hq * 4 + q] + w[q] : 0.0f;
                    *reinterpret_cast<v4f *>(&p.Mf[base + (long long)i * SP + j]) = out;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) acc[a][hq * 4 + q] = out[q];
            }
        }
    }
    // ---- Mb = the transpose, a quadrant at a time through LDS (the loop above ended on a barrier: the staging tiles are free) ----
    float *T = smem;
#pragma unroll
    for (int ha = 0; ha < 2; ha++)
#pragma unroll
        for (int hq = 0; hq < 2; hq++) {
            if (active) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const v4f t = {acc[ha * 4][hq * 4 + q], acc[ha * 4 + 1][hq * 4 + q], acc[ha * 4 + 2][hq * 4 + q], acc[ha * 4 + 3][hq * 4 + q]};
                    *reinterpret_cast<v4f *>(&T[(tj * 4 + q) * TB_LDT + ti * 4]) = t;
                }
            }
            __syncthreads();
            for (int e = tid; e < H * n8; e += nthr) {
                const int jl = e / n8, c = (e - jl * n8) * 4;
                const int j = j0 + hq * H + jl, i = i0 + ha * H + c;
                if (j < S && i < SP)
                    *reinterpret_cast<v4f *>(&p.Mb[base + (long long)j * SP + i]) = *reinterpret_cast<const v4f *>(&T[jl * TB_LDT + c]);
            }
            __syncthreads();
        }
    // ---- the pad rows S .. SR-1 of both images ----
    if (blockIdx.y == 0) {
        const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
        const long long r0 = base + (long long)S * SP;           // (S SP is a multiple of four)
        for (int e = tid; e < (p.SR - S) * SP / 4; e += nthr) {
            *reinterpret_cast<v4f *>(&p.Mf[r0 + 4LL * e]) = z;
            *reinterpret_cast<v4f *>(&p.Mb[r0 + 4LL * e]) = z;
        }
    }
}

inline int launch_token_blocks(TokenBlocksParams p, hipStream_t s) {
    const long long NT = (long long)p.B * p.L;
    const int side = p.S < TB_TILE ? p.S : TB_TILE;
    p.n8 = (side + 7) / 8;
    p.ntile = (p.S + TB_TILE - 1) / TB_TILE;
    const int threads = (p.n8 * p.n8 + 63) / 64 * 64;
    token_blocks_kernel<<<dim3((unsigned)NT, p.ntile * p.ntile), dim3(threads), 0, s>>>(p);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
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
