// Kernels of the float64 CP-ALS on coordinate lists (farnn_cp_*; include/farnn.h).  Host code: farnn_cp.hip.
//
// One ALS stage for mode n is: H = the Hadamard product of the other factors' Gram matrices (two at order 3, three at order 4),
// M = the MTTKRP on the nonzeros, A_n = M H^-1 by Cholesky.  Every sum below is taken in an order fixed by the DATA (chunks of a row, panels of a factor, a fixed tree), never by the
// launch geometry, and there is no float atomic anywhere: a repeated call gives the same bits.
//   cp_mttkrp_chunk_kernel   <ORDER> one thread per (chunk of <= CP_CHUNK nonzeros of one row, rank column): the chunk's sum, in list
//                            order; a term is val * Fa[ia] * Fb[ib] (* Fc[ic] at order 4), the other modes ascending
//   cp_mttkrp_row_kernel     one thread per (row, rank column): the row's chunk sums in chunk order (an empty row: zero) -- the one
//                            owner of the output element.  A long row (state 0 owns most edges) is spread over its chunks' threads
//   cp_gram_kernel           one wavefront per (16 x 16 tile of the upper triangle, panel of CP_PANEL factor rows): v_mfma_f64_16x16x4_f64
//                            down the panel, one accumulator, rows in order
//   cp_hadamard_kernel       <NG> H[i][j] = (sum of the a-panels) * (sum of the b-panels) (* (sum of the c-panels) at order 4), panels in
//                            order, read from the upper triangle only: H is symmetric bit for bit
//   cp_cholesky_kernel       one workgroup, left-looking in 16-column panels: the panel and the 16 finished rows it needs live in LDS,
//                            the factor L (and its transpose, for the solves' contiguous reads) in global memory
//   cp_trisolve_kernel       one workgroup per CP_TILE right-hand-side rows (in LDS): L y = m, then L^T x = y, column by column
//   cp_error_kernel          the two sums of the reconstruction error, a fixed tree in one workgroup
#pragma once
#include <hip/hip_runtime.h>

#include "common.hip.h"

namespace farnn {

constexpr int CP_CHUNK = 64;        // nonzeros per MTTKRP chunk
constexpr int CP_PANEL = 1024;      // factor rows per Gram panel (a multiple of 4)
constexpr int CP_TILE = 16;         // right-hand-side rows per triangular-solve workgroup
constexpr int CP_NB = 16;           // Cholesky panel width
constexpr int CP_MAX_RANK = 352;    // the reference's largest rank is 350; the LDS of the Cholesky panel kernel is 2 * 16 * R doubles
constexpr int CP_THREADS = 256;

typedef double cp_f64x4 __attribute__((ext_vector_type(4)));

struct CpSlot {                     // what the host reads once per sweep
    double err;
    long long flag;                 // != 0: a Cholesky pivot was not a positive finite number
};

// ---- MTTKRP -----------------------------------------------------------------------------------------------------------------
// chunk_beg / chunk_end: the nonzero range of a chunk (one row's, at most CP_CHUNK long); ia / ib / ic: the other modes' indices in
// ascending mode order (ic and Fc are not read at ORDER 3, whose sum is the one it always was)
template <int ORDER>
__global__ void __launch_bounds__(CP_THREADS) cp_mttkrp_chunk_kernel(const int *__restrict__ chunk_beg, const int *__restrict__ chunk_end,
                                                                     int nchunks, const int *__restrict__ ia, const int *__restrict__ ib,
                                                                     const int *__restrict__ ic, const double *__restrict__ val,
                                                                     const double *__restrict__ Fa, const double *__restrict__ Fb,
                                                                     const double *__restrict__ Fc, int R, double *__restrict__ part) {
    static_assert(ORDER == 3 || ORDER == 4, "CP-ALS of order 3 or 4");
    const int ch = blockIdx.x * 4 + threadIdx.y, r = blockIdx.y * 64 + threadIdx.x;
    if (ch >= nchunks || r >= R) return;
    const int beg = chunk_beg[ch], end = chunk_end[ch];
    double acc = 0.0;
    if constexpr (ORDER == 3) {
        for (int e = beg; e < end; e++)
            acc += val[e] * Fa[(size_t)ia[e] * R + r] * Fb[(size_t)ib[e] * R + r];
    } else {
        for (int e = beg; e < end; e++)
            acc += val[e] * Fa[(size_t)ia[e] * R + r] * Fb[(size_t)ib[e] * R + r] * Fc[(size_t)ic[e] * R + r];
    }
    part[(size_t)ch * R + r] = acc;
}

__global__ void __launch_bounds__(CP_THREADS) cp_mttkrp_row_kernel(const int *__restrict__ chunkptr, int nrows, int R,
                                                                   const double *__restrict__ part, double *__restrict__ out) {
    const int row = blockIdx.x * 4 + threadIdx.y, r = blockIdx.y * 64 + threadIdx.x;
    if (row >= nrows || r >= R) return;
    double acc = 0.0;
    for (int ch = chunkptr[row]; ch < chunkptr[row + 1]; ch++) acc += part[(size_t)ch * R + r];
    out[(size_t)row * R + r] = acc;
}

// ---- Gram matrices on the f64 matrix cores -----------------------------------------------------------------------------------
// F [rows][R] row-major.  P [panels][R][R]: tile (ib, jb), jb >= ib, of panel p.  v_mfma_f64_16x16x4_f64: lane l feeds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; its result register g holds D[row = (l >> 4) + 4 g][col = l & 15]
// (NOT the f32 form's row = 4 (l >> 4) + g).
__global__ void __launch_bounds__(WAVE) cp_gram_kernel(const double *__restrict__ F, int rows, int R, double *__restrict__ P) {
    const int ib = blockIdx.x, jb = blockIdx.y, p = blockIdx.z;
    if (jb < ib) return;
    const int lane = threadIdx.x, kk = lane >> 4, cc = lane & 15;
    const int ci = ib * 16 + cc, cj = jb * 16 + cc;
    const int r0 = p * CP_PANEL, r1 = min(rows, r0 + CP_PANEL);
    cp_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = r0; k0 < r1; k0 += 4) {
        const int row = k0 + kk;
        const bool ok = row < r1;
        const double a = (ok && ci < R) ? F[(size_t)row * R + ci] : 0.0;
        const double b = (ok && cj < R) ? F[(size_t)row * R + cj] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double *tile = P + (size_t)p * R * R;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int i = ib * 16 + kk + 4 * g, j = jb * 16 + cc;
        if (i < R && j < R) tile[(size_t)i * R + j] = acc[g];
    }
}

__device__ __forceinline__ double cp_gram_at(const double *__restrict__ P, int panels, int R, int i, int j) {
    const int lo = min(i, j), hi = max(i, j);
    double s = 0.0;
    for (int p = 0; p < panels; p++) s += P[((size_t)p * R + lo) * R + hi];
    return s;
}

template <int NG>
__global__ void __launch_bounds__(CP_THREADS) cp_hadamard_kernel(const double *__restrict__ Pa, int panels_a, const double *__restrict__ Pb,
                                                                 int panels_b, const double *__restrict__ Pc, int panels_c, int R,
                                                                 double *__restrict__ H) {
    static_assert(NG == 2 || NG == 3, "two Grams at order 3, three at order 4");
    const int idx = blockIdx.x * CP_THREADS + threadIdx.x;
    if (idx >= R * R) return;
    const int i = idx / R, j = idx - i * R;
    if constexpr (NG == 2)
        H[idx] = cp_gram_at(Pa, panels_a, R, i, j) * cp_gram_at(Pb, panels_b, R, i, j);
    else
        H[idx] = cp_gram_at(Pa, panels_a, R, i, j) * cp_gram_at(Pb, panels_b, R, i, j) * cp_gram_at(Pc, panels_c, R, i, j);
}

// ---- Cholesky: H = L L^T, lower; H's lower triangle is read -------------------------------------------------------------------
// LDS: pan [R][CP_NB] (the panel's rows j0 .. R-1), blk [CP_NB][R] (rows j0 .. j0+15 of the finished part of L)
__global__ void __launch_bounds__(CP_THREADS) cp_cholesky_kernel(const double *__restrict__ H, int R, double *__restrict__ L,
                                                                 double *__restrict__ Lt, CpSlot *slot) {
    extern __shared__ double cp_lds[];
    double *pan = cp_lds, *blk = cp_lds + (size_t)R * CP_NB;
    const int tid = threadIdx.x;
    for (int j0 = 0; j0 < R; j0 += CP_NB) {
        const int nb = min(CP_NB, R - j0), m = R - j0;
        for (int idx = tid; idx < nb * j0; idx += CP_THREADS) {
            const int c = idx / j0, k = idx - c * j0;
            blk[c * R + k] = L[(size_t)(j0 + c) * R + k];
        }
        __syncthreads();
        for (int idx = tid; idx < m * CP_NB; idx += CP_THREADS) {
            const int i = idx >> 4, c = idx & 15;
            double acc = 0.0;
            if (c < nb && c <= i) {
                acc = H[(size_t)(j0 + i) * R + j0 + c];
                const double *li = L + (size_t)(j0 + i) * R, *lc = blk + c * R;
                for (int k = 0; k < j0; k++) acc -= li[k] * lc[k];
            }
            pan[idx] = acc;
        }
        __syncthreads();
        for (int jj = 0; jj < nb; jj++) {
            double d = pan[jj * CP_NB + jj];
            if (!(d > 0.0 && isfinite(d))) {             // not positive definite to working precision: flag it, keep the barriers uniform
                if (tid == 0) slot->flag = 1;
                d = 1.0;
            }
            const double s = sqrt(d);
            __syncthreads();
            for (int i = jj + tid; i < m; i += CP_THREADS) pan[i * CP_NB + jj] = (i == jj) ? s : pan[i * CP_NB + jj] / s;
            __syncthreads();
            for (int idx = tid; idx < m * CP_NB; idx += CP_THREADS) {
                const int i = idx >> 4, c = idx & 15;
                if (c > jj && c < nb && i >= c) pan[idx] -= pan[i * CP_NB + jj] * pan[c * CP_NB + jj];
            }
            __syncthreads();
        }
        for (int idx = tid; idx < m * CP_NB; idx += CP_THREADS) {
            const int i = idx >> 4, c = idx & 15;
            if (c < nb && i >= c) {
                const double v = pan[idx];
                L[(size_t)(j0 + i) * R + j0 + c] = v;
                Lt[(size_t)(j0 + c) * R + j0 + i] = v;
            }
        }
        __syncthreads();
    }
}

// ---- X (L L^T) = M for CP_TILE rows of M per workgroup -----------------------------------------------------------------------
// LDS: m [CP_TILE][R].  The 16 threads of a right-hand-side row share it; column j is final when step j starts.
__global__ void __launch_bounds__(CP_THREADS) cp_trisolve_kernel(const double *__restrict__ L, const double *__restrict__ Lt, int R,
                                                                 const double *__restrict__ M, int rows, double *__restrict__ out) {
    extern __shared__ double cp_lds[];
    const int t = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int row = blockIdx.x * CP_TILE + t;
    const bool valid = row < rows;
    double *m = cp_lds + (size_t)t * R;
    for (int k = c; k < R; k += 16) m[k] = valid ? M[(size_t)row * R + k] : 0.0;
    __syncthreads();
    for (int j = 0; j < R; j++) {                        // L y = m: after y_j, take column j of L (row j of Lt) off the rest
        const double *lj = Lt + (size_t)j * R;
        const double yj = m[j] / lj[j];
        __syncthreads();
        for (int i = j + 1 + c; i < R; i += 16) m[i] -= lj[i] * yj;
        if (c == 0) m[j] = yj;
        __syncthreads();
    }
    for (int j = R - 1; j >= 0; j--) {                   // L^T x = y: column j of L^T is row j of L
        const double *lj = L + (size_t)j * R;
        const double xj = m[j] / lj[j];
        __syncthreads();
        for (int i = c; i < j; i += 16) m[i] -= lj[i] * xj;
        if (c == 0) m[j] = xj;
        __syncthreads();
    }
    if (valid)
        for (int k = c; k < R; k += 16) out[(size_t)row * R + k] = m[k];
}

// ---- the error terms: sum(H o G_last) and sum(M o A_last), then sqrt(|normx2 + that - 2 this|) / sqrt(normx2) -----------------
__global__ void __launch_bounds__(CP_THREADS) cp_error_kernel(const double *__restrict__ H, const double *__restrict__ P, int panels, int R,
                                                              const double *__restrict__ M, const double *__restrict__ A, int rows,
                                                              double normx2, CpSlot *slot) {
    __shared__ double s1[CP_THREADS], s2[CP_THREADS];
    const int tid = threadIdx.x;
    double a1 = 0.0, a2 = 0.0;
    for (int idx = tid; idx < R * R; idx += CP_THREADS) {
        const int i = idx / R, j = idx - i * R;
        a1 += H[idx] * cp_gram_at(P, panels, R, i, j);
    }
    const size_t n = (size_t)rows * R;
    for (size_t idx = tid; idx < n; idx += CP_THREADS) a2 += M[idx] * A[idx];
    s1[tid] = a1; s2[tid] = a2;
    __syncthreads();
    for (int w = CP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s1[tid] += s1[tid + w]; s2[tid] += s2[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) slot->err = sqrt(fabs(normx2 + s1[0] - 2.0 * s2[0])) / sqrt(normx2);
}

}  // namespace farnn
