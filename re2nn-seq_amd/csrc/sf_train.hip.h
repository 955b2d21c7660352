// Training step of the vector-input i-FST tagger (FARNN_S_SF): what the decomposed i-FST's step (train.hip.h)
// does per WORD, done per TOKEN.  The input is one rule-space vector per token, v [B][L][R], and the step returns d loss / d v
// beside the loss, the tags and the weight gradients.
//
// Reference: FARNN_S_SF.forward(train=True) (model_decompose_single.py:483-580) followed by loss.backward().  Its recurrence is
// FARNN_S_D_W_I_S's with input[:, i, :] in place of Vgen[x[:, i]], so both chains, the loss and the back-propagation through time
// are train.hip.h's kernels, unchanged, run on the position ids b L + t with v as their "word table" (they read a row only at a
// step t <= len of its sequence: a pad row of v reaches no output).  This header adds what was per word:
//   sf_iota_kernel   the position ids, once per growth of the context's id buffer (awaited there: no step depends on another's stream)
//   sf_gate_kernel   the gates' input halves v_t Wrs1, v_t Wrs2 of every valid position (zero rows at the pads, whose v is not
//                    read) and the masked copy of v that dWrs is reduced from
//   sf_dv_kernel     dv[b][t] = (DVf[forward step t + 1] + DVb[backward step len - t]) + (DAZf + DAZb) Wrs1^T + (DARf + DARb) Wrs2^T,
//                    one owner per element and k ascending: no float atomic, the same bits every call; zeros at the pads.  The
//                    summed gate adjoints are kept per position for dWrs = v^T (.)
//   sf_seq_sum_kernel  dh0, dhT and dOsum from the sequences' shares, in order
// The loss is summed from per-wavefront (CE1) or per-sequence (CRF) partials in index order, and every output of
// atb_reduce_kernel has at most two addends, so every output of the step has the same bits from call to call.
// Both products are 16-position tiles on the f32 matrix cores (decomp0_train.hip.h's d0_mma: the A tile in LDS with a
// conflict-free row stride, B straight from global memory in operand order).
#pragma once
#include "common.hip.h"
#include "train.hip.h"
#include "decomp0_train.hip.h"

namespace farnn {

constexpr int SF_TP = D0_TP;             // positions per tile
constexpr int SF_THREADS = D0_THREADS;   // four wavefronts, each takes every fourth block of 16 output columns

__global__ void __launch_bounds__(256)
sf_iota_kernel(int64_t *__restrict__ ids, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) ids[e] = (int64_t)e;
}

struct SfGateParams {
    const float *v;                      // [B L][R]
    const int64_t *len;
    const float *Wrs1, *Wrs2;            // [R][S]
    float *GV1, *GV2;                    // [B L][S]
    float *VM;                           // [B L][R] v at the valid positions, zero at the pads
    int B, L, S, R, farnn;
};
inline size_t sf_gate_lds_bytes(size_t R) { return ((size_t)SF_TP * d0_pad((int)R) + SF_TP) * sizeof(float); }

// LDS: vt [16][d0_pad(R)], ok [16]
__global__ void __launch_bounds__(SF_THREADS)
sf_gate_kernel(const SfGateParams p) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.S, R = p.R, L = p.L, RP = d0_pad(R);
    float *vt = smem;
    int *m_ok = (int *)(vt + SF_TP * RP);
    const long long N0 = (long long)p.B * L;
    for (long long pos0 = (long long)blockIdx.x * SF_TP; pos0 < N0; pos0 += (long long)gridDim.x * SF_TP) {
        __syncthreads();                                        // the last round's readers are done
        if (tid < SF_TP) {
            const long long pos = pos0 + tid;
            int ok = 0;
            if (pos < N0) {
                const int b = (int)(pos / L), i = (int)(pos - (long long)b * L);
                ok = i < clamp_len(p.len[b], L);
            }
            m_ok[tid] = ok;
        }
        __syncthreads();
        for (int e = tid; e < SF_TP * RP; e += SF_THREADS) {
            const int m = e / RP, r = e - m * RP;
            float x = 0.0f;
            if (r < R && pos0 + m < N0) {
                if (m_ok[m]) x = p.v[(size_t)(pos0 + m) * R + r];               // a pad row is never read
                p.VM[(size_t)(pos0 + m) * R + r] = x;
            }
            vt[e] = x;
        }
        __syncthreads();
        d0_mma(vt, RP, p.Wrs1, S, 1, R, nullptr, 0, nullptr, 0, 0, 0, S, wave, lane, [&](int m, int n, float a) {
            if (pos0 + m < N0) p.GV1[(size_t)(pos0 + m) * S + n] = m_ok[m] ? a : 0.0f;
        });
        if (p.farnn == 2)
            d0_mma(vt, RP, p.Wrs2, S, 1, R, nullptr, 0, nullptr, 0, 0, 0, S, wave, lane, [&](int m, int n, float a) {
                if (pos0 + m < N0) p.GV2[(size_t)(pos0 + m) * S + n] = m_ok[m] ? a : 0.0f;
            });
    }
}

struct SfDvParams {
    const int64_t *len;
    const float *DVf, *DVb;              // [B (L+1)][R]
    const float *DAZf, *DAZb, *DARf, *DARb;   // [B (L+1)][S]
    const float *Wrs1T, *Wrs2T;          // [S][R]
    float *dv;                           // [B L][R]
    float *dG1, *dG2;                    // [B L][S] DAZf + DAZb, DARf + DARb of the position's two steps; zero at the pads
    int B, L, S, R, farnn;
};
inline size_t sf_dv_lds_bytes(size_t S, int farnn) {
    return ((farnn ? 2 * (size_t)SF_TP * d0_pad((int)S) : 0) + 3 * SF_TP) * sizeof(float);
}

// LDS: [g1 g2 [16][d0_pad(S)]] ok rf rb [16]
__global__ void __launch_bounds__(SF_THREADS)
sf_dv_kernel(const SfDvParams p) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.S, R = p.R, L = p.L, SP = d0_pad(S), farnn = p.farnn;
    float *g1 = smem, *g2 = g1 + SF_TP * SP;
    int *m_ok = (int *)(smem + (farnn ? 2 * SF_TP * SP : 0)), *m_rf = m_ok + SF_TP, *m_rb = m_rf + SF_TP;
    const long long N0 = (long long)p.B * L;
    for (long long pos0 = (long long)blockIdx.x * SF_TP; pos0 < N0; pos0 += (long long)gridDim.x * SF_TP) {
        __syncthreads();
        if (tid < SF_TP) {
            const long long pos = pos0 + tid;
            int ok = 0, rf = 0, rb = 0;
            if (pos < N0) {
                const int b = (int)(pos / L), i = (int)(pos - (long long)b * L), len = clamp_len(p.len[b], L);
                if (i < len) { ok = 1; rf = b * (L + 1) + i + 1; rb = b * (L + 1) + len - i; }   // the backward chain reads token i at its step len - i
            }
            m_ok[tid] = ok; m_rf[tid] = rf; m_rb[tid] = rb;
        }
        __syncthreads();
        if (!farnn) {
            for (int e = tid; e < SF_TP * R; e += SF_THREADS) {
                const int m = e / R, r = e - m * R;
                if (pos0 + m < N0)
                    p.dv[(size_t)(pos0 + m) * R + r] = m_ok[m] ? p.DVf[(size_t)m_rf[m] * R + r] + p.DVb[(size_t)m_rb[m] * R + r] : 0.0f;
            }
            continue;
        }
        for (int e = tid; e < SF_TP * SP; e += SF_THREADS) {
            const int m = e / SP, s = e - m * SP;
            const bool ok = m_ok[m] && s < S;
            const float a = ok ? p.DAZf[(size_t)m_rf[m] * S + s] + p.DAZb[(size_t)m_rb[m] * S + s] : 0.0f;
            const float c = (ok && farnn == 2) ? p.DARf[(size_t)m_rf[m] * S + s] + p.DARb[(size_t)m_rb[m] * S + s] : 0.0f;
            g1[e] = a; g2[e] = c;
            if (s < S && pos0 + m < N0) {
                p.dG1[(size_t)(pos0 + m) * S + s] = a;
                if (farnn == 2) p.dG2[(size_t)(pos0 + m) * S + s] = c;
            }
        }
        __syncthreads();
        d0_mma(g1, SP, p.Wrs1T, R, 1, S, g2, SP, p.Wrs2T, R, 1, farnn == 2 ? S : 0, R, wave, lane, [&](int m, int n, float a) {
            if (pos0 + m < N0)
                p.dv[(size_t)(pos0 + m) * R + n] =
                    m_ok[m] ? (p.DVf[(size_t)m_rf[m] * R + n] + p.DVb[(size_t)m_rb[m] * R + n]) + a : 0.0f;
        });
    }
}

// dh0[s], dhT[s] and dOsum[s] from the sequences' shares (train_backward_kernel's SEQ_ROWS form), the sequences in order
__global__ void __launch_bounds__(256)
sf_seq_sum_kernel(const float *__restrict__ HP, const float *__restrict__ OP, float *dh0, float *dhT, float *dOsum, int B, int S) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * S) return;
    const int which = t / S, s = t - which * S;
    float a = 0.0f;
    if (which < 2) {
        for (int b = 0; b < B; b++) a += HP[((size_t)b * 2 + which) * S + s];
        (which == 0 ? dh0 : dhT)[s] = a;
    } else {
        for (int b = 0; b < B; b++) a += OP[((size_t)b * 2) * S + s] + OP[((size_t)b * 2 + 1) * S + s];
        dOsum[s] = a;
    }
}

}  // namespace farnn
