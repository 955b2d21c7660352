// K12 "rows" kernel -- the decomposed recurrence (FARNN_S_D_W_I_S.get_forward_score,
// model_decompose_single.py:138-200; FARNN_S_D_W.get_forward_score, model_decompose.py:243-307) for
// the sum semiring, any gate mode (farnn 0/1/2) and any update non-linearity.
//
// Per step and direction the state-dependent work is three dense products against weights that are
// the SAME for every sequence (fwd shown; bwd swaps S1/S2 and transposes W):
//
//   P1 (farnn==2)  [z_pre ; r_pre] = [Wss1^T ; Wss2^T] . h                    2S rows x S
//                  hb = (1-r) * h_init + r * h
//   P2             rr = v_t * (S1^T . hb)      (+ z_pre = Wss1^T . h, farnn==1)  R (+S) rows x S
//   P3             nx = [S2 | W^T] . [rr ; hb]                                   S rows x (R+S)
//                  h' = farnn ? (1-z) h + z nl(nx) : nl(nx)
//
// The token-dependent halves of the gates, v_t . Wrs + bs, do not depend on the state: they are
// folded into per-word gate rows when the handle is built (weights are frozen on the
// tagging path), like Vgen.  The o scaling (:156-157 input side backward, :180-181 output side
// forward) is folded into the packed rows.
//
// Every product is a set of ROW dot products.  A workgroup of 8 wavefronts owns NSEQ sequences of one
// direction; four adjacent lanes share a row and split its columns in 32-column chunks, every 16-byte
// weight read is used for the NSEQ sequences, the math is packed f32 (v_pk_fma_f32) and the quad's
// partial sums meet on the DPP network (quad_perm), never in LDS; 128 rows per pass make a phase of
// S <= 128 rows one pass.  The packed rows live in LDS as far as the 160 KiB go (a rank-50 model fits
// whole: ~105 KiB); the rest is streamed from L2 every step (a gated rank-250 model: ~390 KiB of rows
// per step).  Element-wise work (gates, non-linearity, stash) runs on the few wavefronts that own
// state entries, between raw LDS barriers.  Bound: LDS-array cycles and VALU issue per step, not HBM:
// the weights are a few hundred KiB for the whole batch ("decomposed path: not HBM-bound").
//
// Measured history (B=256, L=64, S=104, MI355X):
//   * one wavefront per sequence, factors in LDS: 3.5 us/step at R=50 (LDS-latency bound, 2 waves/CU);
//     gated or rank >= 150 models fell back to a generic kernel at ~90 us/step.
//   * 16 waves, 16..64 lanes per row, epilogue inside the row loop: 3.3 us/step -- every wavefront
//     executed the tanh/gate/store epilogue for its 1-4 rows at 6% lane utilisation.
//   * the same with row sums parked in LDS and element-wise phases on 4 waves: 2.2 us/step.
//   * the products on v_mfma_f32_4x4x1_16b_f32 (scripts/probe/): parity-green but 3.0 us/step; the
//     16-block form issues 256 MACs per 32 cycles per SIMD, a quarter of the f32 VALU rate.
//   * this version: 2.2 us/step at NSEQ=2, 1.0 us/step per sequence at NSEQ=1 (0.66 us of it the
//     barrier/element-wise skeleton); whole farnn_tag 145 us at R=50 (was 237), 374 us for the gated
//     rank-250 model (was 5960).
#pragma once
#include <type_traits>
#include "common.hip.h"
#include "decomp_chain.hip.h"
#include "chain.hip.h"      // select_by_length_rank

namespace farnn {

constexpr int DR_THREADS = 512;       // 8 wavefronts: 256 VGPRs each, cheap barriers
constexpr int DR_LPR = 4;             // lanes per row
constexpr int DR_RPP = DR_THREADS / DR_LPR;   // rows per pass (128)
constexpr int DR_CHUNK = 32;          // floats of a row one quad covers per chunk (2 x 16 bytes per lane)
constexpr int DR_MAX_PF = 4;          // prefetch registers per thread for the per-token vectors
constexpr int DR_MIXED_NCH3 = 9;      // chunks of an output row a mixed form keeps in registers (the rest: streamed per step)
constexpr int DR_T3_CHUNKS = 2;       // 64-column chunks of an output row that the all-in-registers form keeps in LDS instead
constexpr int DR_T3LD = DR_T3_CHUNKS * 64 + 32;   // row stride (floats) of that LDS copy: the two rows of a 16-lane access group land in
                                      // different halves of the banks
constexpr int DR_FORM_PF = 2;         // ... of a register-resident form (one sequence; rows_plan_try: its per-token vector <= 1024 floats)

struct DecompRowsParams {
    const float *P1;              // [2S][ld2]   gate rows (farnn==2) or nullptr
    const float *P2[2];           // [n2][ld2]   per direction
    const float *P3[2];           // [S][ld3]    per direction
    int n1, n2, n3, ld2, ld3, nch2, nch3;
    int res1, res2, res3;         // leading rows of each matrix kept in LDS
    const float *TVt;             // [V][tvl]: per word [Vgen row (Rp) | update-gate row (SP, farnn >= 1) | reset-gate row (SP, farnn == 2)]
    const float *h0, *hT;
    const int64_t *x, *len;
    const int *order;             // folded launch order (batch_prep) or nullptr
    int sort;                     // 1: no order array, the workgroup selects its sequences by length rank itself
    float *A, *Bk;
    int B, L, S, SP, R, Rp, farnn, nl, full, V;
    float sig_k;
    int dbg;                      // diagnostic ablation mask (FARNN_DBG); 0 in production
    int lds_floats;               // the launch's dynamic LDS size (a whole KiB), in floats
    int groups;                   // groups of NSEQ sequences per direction: a workgroup walks groups slot, 2 slots - 1 - slot, ... (gridDim.x / 2 slots)
};

typedef float v2f __attribute__((ext_vector_type(2)));

// sum over the 4 lanes of a quad, result in all four (two DPP butterflies, no LDS)
__device__ __forceinline__ float quad_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));   // quad_perm:[1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));   // quad_perm:[2,3,0,1]
    return v;
}

// the epilogue's operands for `row` (rowdots_regs' `pre` callback), or nothing
template <bool PRE, typename Pre>
__device__ __forceinline__ auto opa_fetch(Pre &pre, int row) {
    if constexpr (PRE) return pre(row);
    else return 0;
}

// sum over the LPR (4 or 8) adjacent lanes that share a row, result in all of them
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
    v = quad_sum(v);
    if constexpr (LPR == 8)       // the other quad of the eight: row_half_mirror (lane i <-> 7 - i), both hold their quad's total
        v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));   // (bound_ctrl: every lane has a
                                                                                                         //  source; lets the add fold the DPP move)
    return v;
}

// group_sum of N values at once, every level ONE v_add_f32_dpp per value (left to the compiler, a third of the levels became a
// v_mov_b32_dpp + v_add_f32 pair).  The s_nop in front of a level covers the two wait states between a vector write and a DPP read
// of the same register when fewer than two other instructions separate them.
#define FARNN_DPP_ADD(V, CTRL) "v_add_f32_dpp " V ", " V ", " V " " CTRL " row_mask:0xf bank_mask:0xf\n\t"
#define FARNN_DPP_LEVEL1(CTRL) "s_nop 1\n\t" FARNN_DPP_ADD("%0", CTRL)
#define FARNN_DPP_LEVEL2(CTRL) "s_nop 1\n\t" FARNN_DPP_ADD("%0", CTRL) FARNN_DPP_ADD("%1", CTRL)
#define FARNN_DPP_LEVEL3(CTRL) "s_nop 1\n\t" FARNN_DPP_ADD("%0", CTRL) FARNN_DPP_ADD("%1", CTRL) FARNN_DPP_ADD("%2", CTRL)
#define FARNN_DPP_LEVEL4(CTRL) "s_nop 1\n\t" FARNN_DPP_ADD("%0", CTRL) FARNN_DPP_ADD("%1", CTRL) FARNN_DPP_ADD("%2", CTRL) FARNN_DPP_ADD("%3", CTRL)
#define FARNN_DPP_LEVEL5(CTRL) "s_nop 1\n\t" FARNN_DPP_ADD("%0", CTRL) FARNN_DPP_ADD("%1", CTRL) FARNN_DPP_ADD("%2", CTRL) FARNN_DPP_ADD("%3", CTRL) FARNN_DPP_ADD("%4", CTRL)
template <int LPR, int N>
__device__ __forceinline__ void group_sum_n(float (&v)[N]) {
    static_assert(N >= 1 && N <= 5, "up to five passes");
#define FARNN_GS(LV, ...)                                                                                                   \
    do {                                                                                                                    \
        if constexpr (LPR == 8)                                                                                             \
            asm volatile(LV("quad_perm:[1,0,3,2]") LV("quad_perm:[2,3,0,1]") LV("row_half_mirror") "s_nop 0" : __VA_ARGS__); \
        else                                                                                                                \
            asm volatile(LV("quad_perm:[1,0,3,2]") LV("quad_perm:[2,3,0,1]") "s_nop 0" : __VA_ARGS__);                      \
    } while (0)
    if constexpr (N == 1) FARNN_GS(FARNN_DPP_LEVEL1, "+v"(v[0]));
    if constexpr (N == 2) FARNN_GS(FARNN_DPP_LEVEL2, "+v"(v[0]), "+v"(v[1]));
    if constexpr (N == 3) FARNN_GS(FARNN_DPP_LEVEL3, "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
    if constexpr (N == 4) FARNN_GS(FARNN_DPP_LEVEL4, "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    if constexpr (N == 5) FARNN_GS(FARNN_DPP_LEVEL5, "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]));
#undef FARNN_GS
}
#undef FARNN_DPP_LEVEL5
#undef FARNN_DPP_LEVEL4
#undef FARNN_DPP_LEVEL3
#undef FARNN_DPP_LEVEL2
#undef FARNN_DPP_LEVEL1
#undef FARNN_DPP_ADD

// out[row] = <M[row, :], x_s> for s < NSEQ.  Four adjacent lanes share a row; per chunk of 32 columns a
// lane reads two 16-byte pieces of the row and of every x_s and does packed f32 FMAs (v_pk_fma_f32), so
// the instruction stream is mostly math; the quad's partial sums meet on the DPP network.  With 128
// rows per pass a phase of S <= 128 rows is ONE pass.  Rows [0, nres) come from LDS, the rest from
// global memory (L2): two loops over pointers of explicit address spaces -- a loop over one selected
// generic pointer compiles to flat_load + a full vmcnt/lgkmcnt drain per pass.
template <int NSEQ, typename Epi>
__device__ __forceinline__ void rowdots(const float *ml, const float *mg, int nres, int nrows, int ld, int nch,
                                        const float *X, int xs, int tid, Epi &&epi) {
    const int k = tid & (DR_LPR - 1), rloc = tid >> 2;
    lds_cfloat *xl = (lds_cfloat *)X + k * 4;
    auto body = [&](auto src, int row, bool ok) {
        v2f tl[NSEQ], th[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) { tl[s] = v2f{0.f, 0.f}; th[s] = v2f{0.f, 0.f}; }
#pragma unroll 2
        for (int c = 0; c < nch; c++) {
            const v4f a0 = src[c * 8], a1 = src[c * 8 + 4];
#pragma unroll
            for (int s = 0; s < NSEQ; s++) {
                lds_cv4f *xp = (lds_cv4f *)(xl + s * xs + c * DR_CHUNK);
                const v4f x0 = xp[0], x1 = xp[4];
                tl[s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0.x, x0.y}, tl[s]);
                th[s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0.z, x0.w}, th[s]);
                tl[s] = __builtin_elementwise_fma(v2f{a1.x, a1.y}, v2f{x1.x, x1.y}, tl[s]);
                th[s] = __builtin_elementwise_fma(v2f{a1.z, a1.w}, v2f{x1.z, x1.w}, th[s]);
            }
        }
        float acc[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) { const v2f t = tl[s] + th[s]; acc[s] = quad_sum(t.x + t.y); }
        if (k == 0 && ok) epi(row, acc);
    };
    int row0 = 0;
    for (; row0 < nres; row0 += DR_RPP) {
        const int row = row0 + rloc;
        const bool ok = row < nrows;
        body((lds_cv4f *)((lds_cfloat *)ml + (ok ? row : nrows - 1) * ld + k * 4), row, ok);
    }
    for (; row0 < nrows; row0 += DR_RPP) {
        const int row = row0 + rloc;
        const bool ok = row < nrows;
        body((glb_cv4f *)(mg + (long long)(ok ? row : nrows - 1) * ld + k * 4), row, ok);
    }
}

// A FEW rows (the rows behind a mixed form's register passes: 6 or 12 of them), all LDS-resident: a 128-row pass would spend a
// whole pass's reads and FMAs on them.  Here a wavefront takes a row, lane l the columns 4l .. 4l+3 (+ 256): two 16-byte
// reads of the row, eight FMAs, a wave sum; the input vector's pieces are read once for all of a wavefront's rows.
template <int NSEQ, typename Epi>
__device__ __forceinline__ void rowdots_few(const float *ml, int nrows, int ld, int nch, const float *X, int xs, int tid, Epi &&epi) {
    const int lane = tid & 63, wv = tid >> 6;
    const int ncol = nch * DR_CHUNK;                            // nch <= 16: two column blocks of 256
    for (int row = wv; row < nrows; row += DR_THREADS / 64) {
        lds_cfloat *rl = (lds_cfloat *)ml + row * ld;
        float acc[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) acc[s] = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; i++) {                           // (the input vector's pieces are re-read per row: registers are what
            const int c = 4 * lane + 256 * i;                   //  a mixed form has least of)
            if (c < ncol) {
                const v4f a = *(lds_cv4f *)(rl + c);
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    const v4f x = *(lds_cv4f *)((lds_cfloat *)X + s * xs + c);
                    acc[s] += (a.x * x.x + a.y * x.y) + (a.z * x.z + a.w * x.w);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NSEQ; s++) acc[s] = wave_sum_dpp(acc[s]);
        if (lane == 0) epi(row, acc);
    }
}

// The same row dot products with the rows held in REGISTERS for the whole sequence: pass i covers the rows i*128 + tid/4,
// w[i][2c], w[i][2c+1] are this lane's two 16-byte pieces of chunk c.  The chunk of every x_s is read from LDS once and used
// by all NP passes.
// NP and NCH are upper bounds: passes past the last row are not written; chunks past the model's hold zero weights, and their
// x reads run on into the LDS vectors behind x (state / gate / row floats, or past the allocation: zeros) -- finite times
// zero.  (Clamping the chunk index instead turned the reads' immediate offsets into address arithmetic: +7 % per step.)
// NCHG > 0 (one pass only): the row's chunks NCH .. NCH + NCHG - 1 are not register-resident -- g holds this step's copy of them,
// fetched from L2 by the caller a phase ahead (decomp_rows_kernel: a form whose rows do not fit the registers whole).
// LPR = lanes per row (4 or 8): a pass covers 512 / LPR rows, a chunk 8 LPR columns (two 16-byte pieces per lane: columns
// c 8 LPR + 4 k and + 4 LPR behind them).  Eight lanes per row HALVE the reads of x a wavefront issues for the same products
// (every lane of the workgroup reads its piece of x once per chunk, whatever the number of passes that share it), and the step
// of the large gated models is bound by exactly those LDS reads: 64 ds_read_b128 per lane and step at rank 250, farnn 2 with four
// lanes per row = 4 096 LDS cycles of the step's ~3 700 (round 3: 209 us per batch).
// NCHL > 0 (eight lanes per row): the chunks NCH .. NCH + NCHL - 1 of every row lie in LDS, [row][DR_T3LD] at tail_lds (the
// form with all three matrices register-resident but for the output rows' last chunk).
// pre (LPR = 8, optional): row -> the epilogue's LDS operands (they depend on the row only); called in FRONT of the products with
// the lane's row clamped into the matrix, its result handed to epi(row, acc, operands) -- the reads run under the products instead
// of opening the epilogue's latency chain behind the reduction.
// HALF = 1: the last chunk holds its first piece only (w[.][2 NCH - 1]): a matrix of 2.5 chunks does not pay registers for three.
// NPL = 1 (the mixed forms): the rows BEHIND the NP register passes (fewer than a pass) lie in LDS, [.][ldl] at rows_lds; they are
// swept as pass NP of the same loop -- their pieces read beside the x pieces every pass shares, their sums reduced and finished
// like any pass's.  (Round 3 gave them to rowdots_few: a wavefront per row, a six-level reduction and an epilogue run per round.)
template <int NSEQ, int NP, int NCH, int NCHG = 0, int LPR = DR_LPR, int NCHL = 0, int HALF = 0, int NPL = 0, typename Epi, typename Pre = int>
__device__ __forceinline__ void rowdots_regs(const v4f (&w)[NP][2 * NCH - HALF], int nrows, int nch, const float *X, int xs, int tid, Epi &&epi,
                                             const v4f *g = nullptr, const float *tail_lds = nullptr, Pre pre = 0,
                                             const float *rows_lds = nullptr, int ldl = 0) {
    constexpr bool PRE = std::is_invocable_v<Pre, int>;
    static_assert(NPL == 0 || (NP + 1 <= LPR && NCHG == 0), "rows behind the register passes: one more pass");
    static_assert(!PRE || NP <= LPR, "operands ahead: one lane of the group per pass");
    static_assert(NCHG == 0 || NP == 1, "streamed tail chunks: one pass");
    static_assert(NCHL == 0 || (LPR == 8 && NCHL == DR_T3_CHUNKS && NCHG == 0), "LDS tail: eight lanes per row");
    constexpr int RPP = DR_THREADS / LPR, CH = 8 * LPR;
    const int k = tid & (LPR - 1), rloc = tid / LPR;
    lds_cfloat *xl = (lds_cfloat *)X + k * 4;
    // the row this lane finishes (LPR = 8), opaque to the optimiser: as a loop invariant every address the epilogue derives from it
    // is hoisted out of the time loop into a register of its own -- the register forms have none to spare.  Made opaque HERE, in
    // front of the products, so that the epilogue's LDS operands (they depend on the row only) can be fetched under them.
    int myrow = k * RPP + rloc;
    asm volatile("" : "+v"(myrow));
    const auto ops = opa_fetch<PRE>(pre, myrow < nrows ? myrow : nrows - 1);
    v2f tl[NP][NSEQ], th[NP][NSEQ];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int s = 0; s < NSEQ; s++) { tl[i][s] = v2f{0.f, 0.f}; th[i][s] = v2f{0.f, 0.f}; }
    v2f tlx[NSEQ], thx[NSEQ];                                 // (NPL) the pass from LDS
#pragma unroll
    for (int s = 0; s < NSEQ; s++) { tlx[s] = v2f{0.f, 0.f}; thx[s] = v2f{0.f, 0.f}; }
    const int ntail = nrows - NP * RPP;                       // rows behind the register passes (NPL; <= RPP by the plan)
    lds_cv4f *xsrc = nullptr;
    if constexpr (NPL > 0) {
        int rl = tid / LPR;
        asm volatile("" : "+v"(rl));                          // (opaque: the address stays out of the time loop's live set)
        xsrc = (lds_cv4f *)((lds_cfloat *)rows_lds + (rl < ntail ? rl : (ntail > 0 ? ntail - 1 : 0)) * ldl + k * 4);
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            lds_cv4f *xp = (lds_cv4f *)(xl + s * xs + c * CH);   // compile-time offsets: the reads stay `ds_read ... offset:`
            const bool second = !(HALF && c == NCH - 1);
            const v4f x0 = xp[0], x1 = second ? xp[LPR] : v4f{0.f, 0.f, 0.f, 0.f};
            if constexpr (NPL > 0) {
                // (a piece past the row's last 32-column block lies in its pad / the next row: its products are dropped)
                const bool ok0 = (2 * c) * LPR / 8 < nch, ok1 = second && (2 * c + 1) * LPR / 8 < nch;
                const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
                const v4f b0 = xsrc[ok0 ? c * 2 * LPR : 0], b1 = xsrc[ok1 ? c * 2 * LPR + LPR : 0];
                const v4f a0 = ok0 ? b0 : zero, a1 = ok1 ? b1 : zero;
                tlx[s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0.x, x0.y}, tlx[s]);
                thx[s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0.z, x0.w}, thx[s]);
                tlx[s] = __builtin_elementwise_fma(v2f{a1.x, a1.y}, v2f{x1.x, x1.y}, tlx[s]);
                thx[s] = __builtin_elementwise_fma(v2f{a1.z, a1.w}, v2f{x1.z, x1.w}, thx[s]);
            }
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const v4f a0 = w[i][2 * c];
                tl[i][s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0.x, x0.y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0.z, x0.w}, th[i][s]);
                if (second) {
                    const v4f a1 = w[i][2 * c + (second ? 1 : 0)];
                    tl[i][s] = __builtin_elementwise_fma(v2f{a1.x, a1.y}, v2f{x1.x, x1.y}, tl[i][s]);
                    th[i][s] = __builtin_elementwise_fma(v2f{a1.z, a1.w}, v2f{x1.z, x1.w}, th[i][s]);
                }
            }
        }
    if constexpr (NCHG > 0) {
#pragma unroll
        for (int c = 0; c < NCHG; c++)
#pragma unroll
            for (int s = 0; s < NSEQ; s++) {
                lds_cv4f *xp = (lds_cv4f *)(xl + s * xs + (NCH + c) * CH);
                const v4f x0 = xp[0], x1 = xp[LPR];
                const v4f a0 = g[2 * c], a1 = g[2 * c + 1];
                tl[0][s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0.x, x0.y}, tl[0][s]);
                th[0][s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0.z, x0.w}, th[0][s]);
                tl[0][s] = __builtin_elementwise_fma(v2f{a1.x, a1.y}, v2f{x1.x, x1.y}, tl[0][s]);
                th[0][s] = __builtin_elementwise_fma(v2f{a1.z, a1.w}, v2f{x1.z, x1.w}, th[0][s]);
            }
    }
    // every lane of the group holds every pass's sum: lane k turns pass k's into its row's result -- ONE run of the epilogue
    // (a sigmoid or tanh between LDS reads and writes: a latency chain) for all passes, not one per pass
#pragma unroll
    for (int c = 0; c < NCHL; c++) {
        v4f a0[NP], a1[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int row = i * RPP + rloc;
            lds_cv4f *src = (lds_cv4f *)((lds_cfloat *)tail_lds + (row < nrows ? row : nrows - 1) * DR_T3LD + c * CH + k * 4);
            a0[i] = src[0]; a1[i] = src[LPR];
        }
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            lds_cv4f *xp = (lds_cv4f *)(xl + s * xs + (NCH + c) * CH);
            const v4f x0 = xp[0], x1 = xp[LPR];
#pragma unroll
            for (int i = 0; i < NP; i++) {
                tl[i][s] = __builtin_elementwise_fma(v2f{a0[i].x, a0[i].y}, v2f{x0.x, x0.y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a0[i].z, a0[i].w}, v2f{x0.z, x0.w}, th[i][s]);
                tl[i][s] = __builtin_elementwise_fma(v2f{a1[i].x, a1[i].y}, v2f{x1.x, x1.y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a1[i].z, a1[i].w}, v2f{x1.z, x1.w}, th[i][s]);
            }
            if constexpr (NPL > 0) {                          // the rows behind the register passes: these chunks from their own full rows
                const bool ok0 = (2 * (NCH + c)) * LPR / 8 < nch, ok1 = (2 * (NCH + c) + 1) * LPR / 8 < nch;
                const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
                const v4f b0 = xsrc[ok0 ? (NCH + c) * 2 * LPR : 0], b1 = xsrc[ok1 ? (NCH + c) * 2 * LPR + LPR : 0];
                const v4f e0 = ok0 ? b0 : zero, e1 = ok1 ? b1 : zero;
                tlx[s] = __builtin_elementwise_fma(v2f{e0.x, e0.y}, v2f{x0.x, x0.y}, tlx[s]);
                thx[s] = __builtin_elementwise_fma(v2f{e0.z, e0.w}, v2f{x0.z, x0.w}, thx[s]);
                tlx[s] = __builtin_elementwise_fma(v2f{e1.x, e1.y}, v2f{x1.x, x1.y}, tlx[s]);
                thx[s] = __builtin_elementwise_fma(v2f{e1.z, e1.w}, v2f{x1.z, x1.w}, thx[s]);
            }
        }
    }
    if constexpr (LPR == 8 || PRE) {
        static_assert(NP <= LPR, "one lane of the group per pass");
        float acc[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            float v[NP + NPL];
#pragma unroll
            for (int i = 0; i < NP; i++) { const v2f t = tl[i][s] + th[i][s]; v[i] = t.x + t.y; }
            if constexpr (NPL > 0) { const v2f t = tlx[s] + thx[s]; v[NP] = t.x + t.y; }
            group_sum_n<LPR, NP + NPL>(v);
            acc[s] = v[0];
#pragma unroll
            for (int i = 1; i < NP + NPL; i++) acc[s] = k == i ? v[i] : acc[s];
        }
        if (k < NP + NPL && myrow < nrows) {
            if constexpr (PRE) epi(myrow, acc, ops);
            else epi(myrow, acc);
        }
    } else {                              // (four lanes per row: round 3's form, one run of the epilogue per pass)
#pragma unroll
        for (int i = 0; i < NP; i++) {
            float acc[NSEQ];
#pragma unroll
            for (int s = 0; s < NSEQ; s++) { const v2f t = tl[i][s] + th[i][s]; acc[s] = group_sum<LPR>(t.x + t.y); }
            const int row = i * RPP + rloc;
            if (k == 0 && row < nrows) epi(row, acc);
        }
        if constexpr (NPL > 0) {
            float acc[NSEQ];
#pragma unroll
            for (int s = 0; s < NSEQ; s++) { const v2f t = tlx[s] + thx[s]; acc[s] = group_sum<LPR>(t.x + t.y); }
            const int row = NP * RPP + rloc;
            if (k == 0 && row < nrows) epi(row, acc);
        }
    }
}

// this lane's pieces of the rows of a packed matrix (rows past the last one: a copy of the last, never used; pieces past the
// model's last 32-column block: zeros -- nch counts 32-column blocks whatever LPR is)
template <int NP, int NCH, int LPR = DR_LPR, int HALF = 0>
__device__ __forceinline__ void load_rows_regs(v4f (&w)[NP][2 * NCH - HALF], const float *M, int nrows, int ld, int nch, int tid) {
    constexpr int RPP = DR_THREADS / LPR;
    const int k = tid & (LPR - 1), rloc = tid / LPR;
    const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int row = i * RPP + rloc;
        glb_cv4f *src = (glb_cv4f *)(M + (long long)(row < nrows ? row : nrows - 1) * ld + k * 4);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            w[i][2 * c] = (2 * c) * LPR / 8 < nch ? src[c * 2 * LPR] : zero;               // (the piece's 32-column block)
            if (!(HALF && c == NCH - 1)) w[i][2 * c + 1] = (2 * c + 1) * LPR / 8 < nch ? src[c * 2 * LPR + LPR] : zero;
        }
    }
}

// LDS-resident rows, EIGHT lanes per row, NPASS passes of 64 rows in ONE sweep over the columns: x is read once per chunk for all
// passes (rowdots re-reads it per pass).  Passes past the last row re-read the last row (their sums are dropped).  nch counts
// 32-column blocks; an odd count's last half chunk is skipped (behind it lie the row's pad and the next row).
template <int NSEQ, int NPASS, typename Epi, typename Pre = int>
__device__ __forceinline__ void rowdots_lds8(const float *ml, int nrows, int ld, int nch, const float *X, int xs, int tid, Epi &&epi, Pre pre = 0) {
    constexpr int LPR = 8, RPP = DR_THREADS / LPR, CH = 8 * LPR;
    constexpr bool PRE = std::is_invocable_v<Pre, int>;
    const int k = tid & (LPR - 1);
    int rloc = tid / LPR;
    asm volatile("" : "+v"(rloc));        // (opaque, like the row below: the NPASS row addresses stay out of the time loop's live set)
    int myrow = k * RPP + rloc;
    asm volatile("" : "+v"(myrow));       // (opaque: rowdots_regs)
    const auto ops = opa_fetch<PRE>(pre, myrow < nrows ? myrow : nrows - 1);
    lds_cfloat *xl = (lds_cfloat *)X + k * 4;
    lds_cv4f *src[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; i++) {
        const int row = i * RPP + rloc;
        src[i] = (lds_cv4f *)((lds_cfloat *)ml + (row < nrows ? row : nrows - 1) * ld + k * 4);
    }
    v2f tl[NPASS][NSEQ], th[NPASS][NSEQ];
#pragma unroll
    for (int i = 0; i < NPASS; i++)
#pragma unroll
        for (int s = 0; s < NSEQ; s++) { tl[i][s] = v2f{0.f, 0.f}; th[i][s] = v2f{0.f, 0.f}; }
    const int nfull = nch >> 1;                                // whole 64-column chunks
#pragma unroll 2
    for (int c = 0; c < nfull; c++) {
        v4f x0[NSEQ], x1[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            lds_cv4f *xp = (lds_cv4f *)(xl + s * xs + c * CH);
            x0[s] = xp[0]; x1[s] = xp[LPR];
        }
#pragma unroll
        for (int i = 0; i < NPASS; i++) {
            const v4f a0 = src[i][c * 2 * LPR], a1 = src[i][c * 2 * LPR + LPR];
#pragma unroll
            for (int s = 0; s < NSEQ; s++) {
                tl[i][s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0[s].x, x0[s].y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0[s].z, x0[s].w}, th[i][s]);
                tl[i][s] = __builtin_elementwise_fma(v2f{a1.x, a1.y}, v2f{x1[s].x, x1[s].y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a1.z, a1.w}, v2f{x1[s].z, x1[s].w}, th[i][s]);
            }
        }
    }
    if (nch & 1) {                                             // the odd 32-column block: first pieces only
        const int c = nfull;
#pragma unroll
        for (int i = 0; i < NPASS; i++) {
            const v4f a0 = src[i][c * 2 * LPR];
#pragma unroll
            for (int s = 0; s < NSEQ; s++) {
                const v4f x0 = *(lds_cv4f *)(xl + s * xs + c * CH);
                tl[i][s] = __builtin_elementwise_fma(v2f{a0.x, a0.y}, v2f{x0.x, x0.y}, tl[i][s]);
                th[i][s] = __builtin_elementwise_fma(v2f{a0.z, a0.w}, v2f{x0.z, x0.w}, th[i][s]);
            }
        }
    }
    static_assert(NPASS <= LPR, "one lane of the group per pass");
    float acc[NSEQ];
#pragma unroll
    for (int s = 0; s < NSEQ; s++) acc[s] = 0.0f;
#pragma unroll
    for (int i = 0; i < NPASS; i++)
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            const v2f t = tl[i][s] + th[i][s];
            const float v = group_sum<LPR>(t.x + t.y);
            acc[s] = k == i ? v : acc[s];
        }
    if (k < NPASS && myrow < nrows) {
        if constexpr (PRE) epi(myrow, acc, ops);
        else epi(myrow, acc);
    }
}

// Gates and update non-linearity on the hardware exponential; |error| ~1e-7 against the 1e-4 parity bar.  FAST (the eight-lane
// forms, round 4): the quotient by v_rcp_f32 and one Newton step -- two dependent FMAs, within rounding of the division -- instead
// of the IEEE division the `/` compiles to (v_div_scale, v_rcp, four FMAs, v_div_fmas, v_div_fixup: a dozen dependent instructions
// on every phase's epilogue chain; rank 250, farnn 2: 157.5 -> 152.0 us per batch).  The other forms keep the division: the gated
// 134-state models are sensitive enough that ANY change of the last bit moves one bench-size case across its 1e-4 bar against
// float64, and their fixtures were captured with it.
__device__ __forceinline__ float dr_rcp(float d) {       // d finite and >= 1
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r, 1.0f), r, r);
}
template <bool FAST = false>
__device__ __forceinline__ float gate_sigmoid(float x, float k) {
    if constexpr (FAST) return dr_rcp(1.0f + __expf(fminf(-(x * k), 80.0f)));     // (the clamp keeps the Newton step off infinity)
    else return 1.0f / (1.0f + __expf(-(x * k)));
}
template <bool FAST = false>
__device__ __forceinline__ float dr_tanh(float x) {
    const float e = __expf(-2.0f * fabsf(x));          // in (0, 1]: no overflow for any x
    const float big = FAST ? copysignf((1.0f - e) * dr_rcp(1.0f + e), x) : copysignf((1.0f - e) / (1.0f + e), x);
    return fabsf(x) < TANH_SERIES_BELOW ? tanh_series(x) : big;    // (common.hip.h: 1 - e cancels for small |x|)
}
template <bool FAST = false>
__device__ __forceinline__ float dr_nl(float x, NlMode m) {                // branch-free (common.hip.h: the mode as two scalars)
    const float y = nl_floor(x, m);
    return nl_pick(dr_tanh<FAST>(y), y, m);
}

// NP1R / NP2R / NP3R > 0: the matrix lives in REGISTERS (that many 128-row passes of NCH2R / NCH3R chunks) instead of LDS /
// L2: with the gates, or at rank 250, the packed rows exceed the 160 KiB of LDS and r02a streamed the rest from L2 on every
// step (the shipped example configuration's shape, S = 104, rank 250, farnn = 2: 286 KB per workgroup per step, 5.1 us per
// step).  Eight wavefronts have 512 KB of registers between them: P1 (gates) and P3 in registers + P2 in LDS hold that
// model whole, and a step touches neither L2 nor HBM for weights.
// LPR = 8 (forms 7, 8): eight lanes per row for the register-resident matrices and for P2's LDS-resident rows (rowdots_regs) --
// NPxR then count passes of 64 rows and NCHxR chunks of 64 columns.
template <int NSEQ, int NP1R = 0, int NP2R = 0, int NCH2R = 0, int NP3R = 0, int NCH3R = 0, bool MIXED = false, int LPR = DR_LPR>
__global__ void __launch_bounds__(DR_THREADS)
decomp_rows_kernel(const DecompRowsParams p) {
    static_assert(LPR == 4 || LPR == 8, "lanes per row");
    constexpr int RPPR = DR_THREADS / LPR;                    // rows per pass of a register-resident matrix
    // register-resident matrices: lane k finishes pass k in ONE run of the epilogue, its LDS operands fetched ahead of the products,
    // quotients by reciprocal (not the mixed forms -- their rows behind the register passes go through rowdots_few's epilogue --
    // and not form 3: twelve chunks of output row beside two passes of gate rows leave it no register, 56 spilled)
    constexpr int NPLX = (MIXED && LPR == 8) ? 1 : 0;         // the rows behind the register passes as one more pass of the sweep
    constexpr bool OPA = (!MIXED && (LPR == 8 || NCH3R <= 8)) || NPLX;
    constexpr bool FASTQ = !MIXED;                            // (the 134-state fixtures sit at the 1e-4 bar: the mixed form keeps the division)
    extern __shared__ __align__(16) float smem[];
    const long long t_kernel = FARNN_PROBE_ON((p.dbg & 16) != 0) ? (long long)__builtin_amdgcn_s_memtime() : 0;
    const int tid = threadIdx.x;
    const int dir = blockIdx.x & 1;
    const int S = p.S, SP = p.SP, R = p.R, Rp = p.Rp, ld2 = p.ld2, ld3 = p.ld3;
    const int c2p = p.nch2 * DR_CHUNK, c3p = p.nch3 * DR_CHUNK;      // floats of the input vectors
    // (a form with gate rows in registers is chosen for farnn = 2 only -- rows_plan_try: A_ > 0 needs n1 > 0 -- and the compiler should
    //  know: with the farnn != 2 prefetch block compiled in beside P1, it took the prefetch registers' re-use in P1 for a possible pending
    //  load and opened every step with s_waitcnt vmcnt(0) -- a wait for the previous step's stash stores to be acknowledged)
    const int farnn = NP1R > 0 ? 2 : p.farnn;
    const int Lr = (p.L + 3) & ~3;
    const int tvl = Rp + (farnn >= 1 ? SP : 0) + (farnn == 2 ? SP : 0);

    // ---- LDS carve (every block a multiple of 16 bytes) ----------------------------------------
    int *tok = reinterpret_cast<int *>(smem);                 // [NSEQ][Lr]
    float *Hinit = smem + NSEQ * Lr;                          // [SP]
    float *H = Hinit + SP;                                    // [NSEQ][c2p]   state h (input of P1)
    float *HB = H + NSEQ * c2p;                               // [2][NSEQ][c2p]  hb: input of P2 (ping-pong)
    float *X3 = HB + 2 * NSEQ * c2p;                          // [2][NSEQ][c3p]  rr | hb: input of P3
    float *Z = X3 + 2 * NSEQ * c3p;                           // [NSEQ][SP]    update gate
    float *TV = Z + NSEQ * SP;                                // [2][NSEQ][tvl]  per-token vectors
    float *L1 = TV + 2 * NSEQ * tvl;                          // resident rows
    float *L2 = L1 + (long long)p.res1 * ld2;
    float *L3 = L2 + (long long)p.res2 * ld2;

    // ---- this lane's slices of the register-resident matrices: issued FIRST (round 4) -- they depend on the direction only, and
    // the ~0.5 MB a workgroup pulls in (64 B per clock per compute unit: ~8 k cycles) used to start behind the length-rank selection,
    // the token loads and the LDS zeroing (set-up 17.7 k cycles, twice per compute unit at B = 256)
    // (the mixed eight-lane form: 128 < S <= 160 columns are 2.5 chunks of 64 -- the sixth piece would be 16 registers of zeros)
    constexpr int HALF2 = (MIXED && LPR == 8 && NCH2R > 0) ? 1 : 0;
    v4f w1[NP1R > 0 ? NP1R : 1][2 * (NCH2R > 0 ? NCH2R : 1) - HALF2], w2[NP2R > 0 ? NP2R : 1][2 * (NCH2R > 0 ? NCH2R : 1) - HALF2];
    // (a mixed form with more than DR_MIXED_NCH3 chunks of output row: two passes of gate rows + 13 chunks are 184 registers of
    // weights, and the compiler kept ~50 of them in scratch memory -- a reload per step from the same L2.  The chunks behind
    // the first DR_MIXED_NCH3 are fetched from L2 explicitly instead, a phase ahead of their use: no scratch, same bits)
    // (eight lanes per row with P2 in registers too: 64 + 64 registers of gate and P2 rows leave 64 for the output rows -- four chunks
    // of a rank-250 model's six; the others lie in LDS, which this form hardly uses otherwise.  Five in registers: 8 spilled)
    constexpr int NCH3L = (LPR == 8 && NP2R > 0 && NP3R > 0) ? DR_T3_CHUNKS : 0;
    constexpr int NCH3G = (MIXED && NP3R == 1 && NCH3R > DR_MIXED_NCH3) ? NCH3R - DR_MIXED_NCH3 : 0, NCH3K = NCH3R - NCH3G - NCH3L;
    v4f w3[NP3R > 0 ? NP3R : 1][2 * (NCH3K > 0 ? NCH3K : 1)];
    // (not the mixed eight-lane form: issued early, its code object keeps a 20-byte stack object nothing reads or writes, and with it
    // the private segment -- the compiler's bookkeeping, but "no scratch" is a property the library asserts)
    constexpr bool EARLYW = !(MIXED && LPR == 8);
#define FARNN_DR_LOAD_WEIGHTS()                                                                                              \
    do {                                                                                                                     \
        if constexpr (NP1R > 0) load_rows_regs<NP1R, NCH2R, LPR, HALF2>(w1, p.P1, p.n1, ld2, p.nch2, tid);                   \
        if constexpr (NP2R > 0) load_rows_regs<NP2R, NCH2R, LPR, HALF2>(w2, p.P2[dir], p.n2, ld2, p.nch2, tid);              \
        if constexpr (NP3R > 0)                                                                                              \
            load_rows_regs<NP3R, NCH3K, LPR>(w3, p.P3[dir], p.n3, ld3, p.nch3 < NCH3K * (LPR / 4) ? p.nch3 : NCH3K * (LPR / 4), tid); \
    } while (0)
    // Round 6: the set-up's barriers order LDS traffic only (a __syncthreads() drains the vector-memory counter of ALL wavefronts:
    // round 5's "selection 10 k cycles" was the wait for everybody's weights), the selection hands the length back (no dependent load
    // of len[b]), and the LDS fills below are DMAs in front of the weights: set-up 17.3 k -> 16.3 k cycles at rank 250
    // (profiles/r06_base_probe_decomp_rows_* / r06_probe_decomp_rows_*).  What remains is the weights themselves: at the start of a
    // launch every compute unit pulls the same ~0.5 MB out of L2 at once -- 128 MB through ~7 KB per clock: ~12 k cycles whatever the
    // order.  (Measured and dropped: wavefront 0 -- selection, tokens -- issuing its share of the weights BEHIND that chain, 19.4 k: its
    // loads only join the end of the same queue.)
    const int wv0 = __builtin_amdgcn_readfirstlane(tid >> 6);
    // The LDS-resident rows (and, all-in-registers form, the output rows' last chunks) go to LDS by LDS-DMA, FIRST: no register
    // round trip -- as `st4(dst, ld4(src))` loops behind the weights every store waited for a load that returned behind ~50 weight
    // loads (a wavefront's loads return in order), one round trip per iteration: 3.7 k cycles for 53 KB at rank 250, 10 k for the
    // 134-state mixed form's rows.  Lanes past a region's end are masked off (a DMA writes at M0 + lane * 16 for its active lanes).
    constexpr int R1 = NP1R * RPPR, R2 = NP2R * RPPR, R3 = NP3R * RPPR;       // rows held in registers: the resident rows start there
    {
        const int lane = tid & 63;
        const float *src[3] = {p.P1 + (long long)R1 * ld2, p.P2[dir] + (long long)R2 * ld2, p.P3[dir] + (long long)R3 * ld3};
        float *dst[3] = {L1, L2, L3};
        const long long cnt[3] = {(long long)p.res1 * ld2, (long long)p.res2 * ld2, (long long)p.res3 * ld3};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const long long bytes = cnt[q] * 4;
            const unsigned d0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)dst[q]);
            for (long long k = wv0; k * 1024 < bytes; k += DR_THREADS / 64) {
                const long long off = k * 1024 + lane * 16;
                if (off < bytes) lds_dma16((unsigned)off, reinterpret_cast<const char *>(src[q]), d0 + (unsigned)(k * 1024));
            }
        }
        if constexpr (LPR == 8 && NP2R > 0 && NP3R > 0) {      // the output rows' last chunks (NCH3L below): [n3][DR_T3LD]; a row's 32 pieces
            float *t3 = L3 + cnt[2];                           // ride on lanes 0..31 of one DMA (the row stride is not the data's width)
            const int c0 = (NCH3R - DR_T3_CHUNKS) * 64, q = lane * 4;
            const bool in = lane < DR_T3_CHUNKS * 16 && c0 + q < p.nch3 * DR_CHUNK;
            for (int row = wv0; row < p.n3; row += DR_THREADS / 64) {
                const unsigned d0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(t3 + row * DR_T3LD));
                if (in) lds_dma16((unsigned)(((long long)row * ld3 + c0 + q) * 4), reinterpret_cast<const char *>(p.P3[dir]), d0);
            }
        }
    }
    if constexpr (EARLYW) FARNN_DR_LOAD_WEIGHTS();
    glb_cv4f *g3src = nullptr;                                // this lane's piece of its output row, for the streamed chunks
    if constexpr (NCH3G > 0) {
        const int row = tid >> 2;
        g3src = (glb_cv4f *)(p.P3[dir] + (long long)(row < p.n3 ? row : p.n3 - 1) * ld3 + (tid & (DR_LPR - 1)) * 4);
    }
    // ---- the workgroup's sequences, one ROUND after the other (round 6) --------------------------------------------------------
    // The launcher starts no more workgroups than the device runs at once (a register form: one per compute unit) and each walks the
    // length-ranked groups of its direction in snake order -- slot q of Q takes groups q, 2Q - 1 - q, 2Q + q, ...: the longest with the
    // shortest, like the hardware's in-order dispatch of 2 x groups workgroups did -- keeping its weights in registers and its
    // resident rows in LDS: a second group used to start with the whole set-up again (~0.5 MB per compute unit, ~14 k cycles).
    const int slots = gridDim.x >> 1, slot = blockIdx.x >> 1;
    for (int rnd = 0;; rnd++) {
    const int grp = (rnd & 1) ? (rnd + 1) * slots - 1 - slot : rnd * slots + slot;
    if (grp >= p.groups) break;
    // (the round's own copy of the thread index, opaque: what the set-up derives from it -- zeroing, staging and stash addresses -- is
    //  loop-invariant, the compiler hoisted it out of the rounds and kept it alive across the time loop: 38 registers spilled)
    int tid_r = tid;
    asm volatile("" : "+v"(tid_r));
    const int tid = tid_r;
    const long long t_start = rnd == 0 ? t_kernel : (FARNN_PROBE_ON((p.dbg & 16) != 0) ? (long long)__builtin_amdgcn_s_memtime() : 0);
    int bseq[NSEQ], nst[NSEQ], slen[NSEQ];
    int nmax = 0;
#pragma unroll
    for (int s = 0; s < NSEQ; s++) {
        const int r = grp * NSEQ + s;                         // rank by length (descending)
        const bool have = r < p.B;
        int b = 0, l = -1;
        if (have) {
            const int half = p.B / 2;
            b = p.order ? p.order[r < half ? r : half + (p.B - 1 - r)] : r;     // undo the fold
        }
        // (the selection hands the sequence's length back with it -- its class: no dependent load of len[b] behind it)
        if (p.sort && have) b = select_by_length_rank<true>(p.len, p.B, p.L, r, reinterpret_cast<int *>(smem), tid, DR_THREADS, &l);
        b = __builtin_amdgcn_readfirstlane(b);                // workgroup-uniform: keep it in SGPRs
        bseq[s] = b;
        if (have && l < 0) l = __builtin_amdgcn_readfirstlane(clamp_len(p.len[b], p.L));     // (a given launch order: FARNN_PREP / FARNN_NOSORT)
        slen[s] = have ? l : 0;
        nst[s] = have ? (p.full ? p.L : slen[s]) : -1;        // -1: no sequence in this slot
        nmax = nst[s] > nmax ? nst[s] : nmax;
    }
    // the tokens: wavefront 0 alone (the selection's wavefront)
    int *tok0 = reinterpret_cast<int *>(smem);
    if (wv0 == 0) {
#pragma unroll
        for (int s = 0; s < NSEQ; s++)
            for (int k = tid; k < nst[s]; k += 64) {
                const int idx = (dir == 0) ? k : (k < slen[s] ? slen[s] - 1 - k : k);
                tok0[s * ((p.L + 3) & ~3) + k] = clamp_tok(p.x[(long long)bseq[s] * p.L + idx], p.V);
            }
    }
    const float *hinit = dir == 0 ? p.h0 : p.hT;
    float *stash_base = dir == 0 ? p.A : p.Bk;
    // (a sum of selects against zero, not a chain of selects between the entries: the compiler turns the chain into ONE load
    // through a selected address, and the array stays in scratch memory for it -- r03: 32 B at NSEQ = 4)
    auto pick = [&](const int (&arr)[NSEQ], int s) { int v = 0;
#pragma unroll
        for (int q = 0; q < NSEQ; q++) v |= (s == q || NSEQ == 1) ? arr[q] : 0;
        return v; };

    long long st_0 = 0, st_1 = 0, st_2 = 0, st_3 = 0, st_4 = 0;      // (set-up stamps of the profiling build; scalars: an array stayed behind as a dead stack object)
    if (FARNN_PROBE_ON((p.dbg & 16) != 0) && blockIdx.x == 0 && tid == 0) st_0 = (long long)__builtin_amdgcn_s_memtime();
    // ---- set-up ------------------------------------------------------------------------------------
    // everything a vector read can touch is initialised: the register forms read whole (upper-bound) chunk counts and run on
    // into the arrays behind the vector -- with zero weights, but LDS keeps what earlier workgroups left there (-inf pads of the
    // Viterbi kernel: -inf x 0 = NaN).  Vectors and per-token buffers are zeroed here, the tail behind the resident rows below.
    for (int i = tid; i < (int)(L1 - Hinit); i += DR_THREADS) Hinit[i] = 0.0f;
    // (A register form may hold only a matrix's first NPxR passes -- mixed forms: S in 129..160 needs three passes of gate rows or
    // two of output rows; the registers hold the first passes, the few rows behind them are LDS-resident like any other
    // matrix's, or streamed: R1 / R2 / R3 above.)
    if (FARNN_PROBE_ON((p.dbg & 16) != 0) && blockIdx.x == 0 && tid == 0) st_1 = (long long)__builtin_amdgcn_s_memtime();
    if (rnd == 0) {   // what the DMAs at the top do not write: columns past the model, the rows' pads, the LDS behind the rows
        float *tail = L3 + (long long)p.res3 * ld3;
        if constexpr (LPR == 8 && NP2R > 0 && NP3R > 0) {
            constexpr int QPR = DR_T3_CHUNKS * 16;              // 16-byte pieces per row
            const int c0 = (NCH3R - DR_T3_CHUNKS) * 64;
            if (c0 + DR_T3_CHUNKS * 64 > p.nch3 * DR_CHUNK)     // (a rank below the form's chunk count: zero past the model)
                for (int i = tid; i < p.n3 * QPR; i += DR_THREADS) {
                    const int row = i / QPR, q = (i % QPR) * 4;
                    if (c0 + q >= p.nch3 * DR_CHUNK) st4(tail + row * DR_T3LD + q, make_float4(0.f, 0.f, 0.f, 0.f));
                }
            for (int i = tid; i < p.n3 * 32; i += DR_THREADS) tail[(i >> 5) * DR_T3LD + DR_T3_CHUNKS * 64 + (i & 31)] = 0.0f;
            tail += p.n3 * DR_T3LD;
        }
        for (int i = tid; tail + i < smem + p.lds_floats; i += DR_THREADS) tail[i] = 0.0f;
    }
    const float *T3 = L3 + (long long)p.res3 * ld3;
    if constexpr (!EARLYW) { if (rnd == 0) FARNN_DR_LOAD_WEIGHTS(); }
#undef FARNN_DR_LOAD_WEIGHTS
    if (FARNN_PROBE_ON((p.dbg & 16) != 0) && blockIdx.x == 0 && tid == 0) { st_2 = st_3 = (long long)__builtin_amdgcn_s_memtime(); }
    // (LDS traffic only: the zeroing against the state rows, wavefront 0's tokens against the first per-token vectors' addresses.
    //  The weights stay in flight; the first vectors' loads join them, and the barrier behind those drains everything once.)
    wg_barrier_lds();
    for (int j = tid; j < S; j += DR_THREADS) {
        const float hv = hinit[j];
        Hinit[j] = hv;
#pragma unroll
        for (int s = 0; s < NSEQ; s++) {
            if (nst[s] < 0) continue;
            H[s * c2p + j] = hv;
            HB[s * c2p + j] = hv;                              // buffer 0 = step 0's "cur"
            X3[s * c3p + Rp + j] = hv;
            stash_base[(long long)bseq[s] * (p.L + 1) * SP + j] = hv;
        }
    }
    // pad columns of every row the chains will write (the workspace is strided with the call's L and not re-zeroed)
    if (SP > S) {
#pragma unroll
        for (int s = 0; s < NSEQ; s++)
            for (int q = tid; q < (nst[s] + 1) * (SP - S); q += DR_THREADS)
                stash_base[((long long)bseq[s] * (p.L + 1) + q / (SP - S)) * SP + S + q % (SP - S)] = 0.0f;
    }

    // per-token vectors: one row of the combined table per (sequence, step).  A prefetch slot's load is ONE global load off a base that
    // sits in scalar registers, with the token id read from LDS a step earlier (pf_tk): round 5's form selected one of three table
    // pointers per lane, which the compiler turned into a load of the pointer from the kernel arguments, a full vmcnt wait and then the
    // value load, behind an LDS read of the token -- three dependent latencies between P1 and its barrier, every step
    auto tok_at = [&](int s, int t) -> int {
        const int n = pick(nst, s);
        // (an empty or absent sequence has no token in LDS -- the words there are whatever the last kernel left: word 0's row, and
        //  nothing of it is ever stored.  Found by tests/soak_rows_rounds.py: a wild row index out of stale LDS, a memory fault.
        //  The read itself is unconditional -- word 0 of the sequence's slot -- so that the guard is a select, not a branch per step)
        const int i = t < n ? t : n - 1;
        const int v = tok[s * Lr + (i > 0 ? i : 0)];
        return n > 0 ? v : 0;
    };
    const int ntv = NSEQ * tvl;
    // prefetch slots per thread.  A register form whose chunk counts bound the state vector by 128 columns and [rr | h] by 384 has a
    // per-token vector of at most 384 + 128 = 512 floats: ONE slot (rows_form_pf mirrors this for the plan).  The second slot of the
    // shipped shape -- tvl = 512 exactly -- was all-inactive, and cost every wavefront a mask, a taken branch and a select per step
    constexpr int NPF = !(NP1R > 0 || NP2R > 0 || NP3R > 0) ? DR_MAX_PF
                        : (NP3R > 0 && NCH2R * (LPR == 8 ? 64 : 32) <= 128 && NCH3R * (LPR == 8 ? 64 : 32) <= 384) ? 1 : DR_FORM_PF;
    int pf_s[NPF], pf_e[NPF];                                 // loop-invariant split of the prefetch slots
#pragma unroll
    for (int i = 0; i < NPF; i++) {
        const int e = tid + i * DR_THREADS;
        pf_s[i] = e < ntv ? e / tvl : 0;
        pf_e[i] = e < ntv ? e % tvl : -1;
    }
    constexpr int NTK = NSEQ == 1 ? 1 : NPF;                  // one sequence: every slot reads the same (wavefront-uniform) token
    int pf_tk[NTK];
    auto next_tokens = [&](int t) {
#pragma unroll
        for (int i = 0; i < NTK; i++) pf_tk[i] = tok_at(NSEQ == 1 ? 0 : pf_s[i], t);
    };
    auto tv_load = [&](int i) -> float {
        int tk = pf_tk[NSEQ == 1 ? 0 : i];
        if (NSEQ == 1) tk = __builtin_amdgcn_readfirstlane(tk);
        return p.TVt[(long long)tk * tvl + pf_e[i]];
    };
    next_tokens(0);
#pragma unroll
    for (int i = 0; i < NPF; i++)
        if (pf_e[i] >= 0) TV[tid + i * DR_THREADS] = tv_load(i);
    next_tokens(1);
    if (FARNN_PROBE_ON((p.dbg & 16) != 0) && blockIdx.x == 0 && tid == 0) st_4 = (long long)__builtin_amdgcn_s_memtime();
    __syncthreads();

    const float sig_k = p.sig_k;
    const NlMode nl_mode = nl_mode_of(p.nl);
    // (the ablation bits of FARNN_DBG -- 1: no products, 2: no non-linearity, 4: no stash stores, 8: no prefetch -- exist in the profiling
    //  build only: as run-time tests of a kernel argument they were scalar compares and branches in every step of the production kernel)
    auto dbg_on = [&](int bit) { return FARNN_PROBE_ON((p.dbg & bit) != 0); };
    const bool probe = FARNN_PROBE_ON((p.dbg & 16) != 0) && blockIdx.x == 0;     // diagnostic: cycle counts of the phases of a step
    long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (probe && tid == 0) printf("rows wg 0 round %d: set-up %lld cycles: selection %lld, tokens + vectors %lld, rows into LDS + zeroing %lld, register loads issued %lld, their wait + barrier + state rows %lld, the rest %lld\n", rnd, (long long)__builtin_amdgcn_s_memtime() - t_start, st_0 - t_start, st_1 - st_0, st_2 - st_1, st_3 - st_2, st_4 - st_3, (long long)__builtin_amdgcn_s_memtime() - st_4);
    // element-wise phases: element e -> (sequence e % NSEQ, state entry e / NSEQ)
    // P1's epilogue operands of this lane's row (eight lanes per row, gate rows in registers: rowdots_regs hands lane k of a group
    // pass k's row, k * 64 + its group, clamped into the matrix)
    const float *p1_hi = Hinit, *p1_hh = H;
    int p1_g = 0;
    if constexpr (LPR == 8 && NP1R > 0) {
        int row = (tid & 7) * (DR_THREADS / 8) + tid / 8;
        row = row < p.n1 ? row : p.n1 - 1;
        const bool isr = row >= S;
        const int j = isr ? row - S : row;
        p1_hi = Hinit + j; p1_hh = H + j; p1_g = Rp + (isr ? SP : 0) + j;
    }
    float *p3_z = Z, *p3_h = H;
    if constexpr (LPR == 8 && NP3R > 0) {
        int row = (tid & 7) * (DR_THREADS / 8) + tid / 8;
        row = row < p.n3 ? row : p.n3 - 1;
        p3_z = Z + row; p3_h = H + row;
    }
    // the ping-pong buffers of a step (this step's / the next step's per-token vectors, hb, [rr | hb]) as loop-carried pointers, swapped
    // in FRONT of the step's last barrier: computed from t & 1 they were a dozen scalar instructions behind it, at the head of P1
    const float *TVc = TV;
    float *TVn = TV + ntv;
    float *HBc = HB, *HBn = HB + NSEQ * c2p;
    float *X3c = X3, *X3n = X3 + NSEQ * c3p;
    for (int t = 0; t < nmax; t++) {
        const bool pr = probe && t == 8;
        if (pr) pt[0] = (long long)__builtin_amdgcn_s_memtime();
        int act[NSEQ];
#pragma unroll
        for (int s = 0; s < NSEQ; s++) act[s] = NSEQ == 1 || t < nst[s];       // (one sequence: the loop runs to its length)
        // next step's per-token vectors: parked in registers until after P2.  Their loads (a token id from LDS, an address, a
        // global load each) are issued behind P1's products when there is a P1 phase -- at the step's top they sat between the
        // barrier and the step's first LDS reads (the placement that paid 5 % in decomp_regs8_kernel)
        float pf[NPF];
#define FARNN_DR_ISSUE_PREFETCH()                                                                                  \
        _Pragma("unroll")                                                                                          \
        for (int i = 0; i < NPF; i++)                                                                              \
            pf[i] = (pf_e[i] >= 0 && t + 1 < nmax && !dbg_on(8)) ? tv_load(i) : 0.0f;
        // (the token of the vectors prefetched in this step: read at the step's top, used behind P1 -- read beside the prefetch for the
        //  NEXT step's, its LDS latency sat between P1's last store and the barrier)
        if (farnn == 2) next_tokens(t + 1);
        if (farnn != 2) { FARNN_DR_ISSUE_PREFETCH() next_tokens(t + 2); }
        // The element-wise work rides in the row epilogues: the lane that finishes a row sum turns it into
        // a gate, an rr entry or the new state right away, so a step is 2 barriers (3 with farnn==2).
        // hb and [rr | hb] ping-pong because P3's epilogue writes the next step's hb while other
        // wavefronts still read this step's.
        if (farnn == 2) {
            // ---- P1: z, r from h; hb = (1-r) h_init + r h  (:143-151) -----------------------------------
            // (one sigmoid for both kinds of row, every LDS operand read up front: the lanes of a wavefront hold update-gate and
            // reset-gate rows side by side, and two branches ran as two latency chains one after the other)
            auto epi1 = [&](int row, const float (&acc)[NSEQ]) {
                const bool isr = row >= S;
                const int j = isr ? row - S : row;
                const float hi = Hinit[j];
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (!act[s]) continue;
                    const float gpre = TVc[s * tvl + Rp + (isr ? SP : 0) + j], hh = H[s * c2p + j];
                    const float g = gate_sigmoid(acc[s] + gpre, sig_k);
                    if (!isr) {
                        Z[s * SP + j] = g;
                    } else {
                        const float hb = (1.0f - g) * hi + g * hh;
                        HBc[s * c2p + j] = hb;
                        X3c[s * c3p + Rp + j] = hb;
                    }
                }
            };
            struct Ops1 { float gpre[NSEQ], hh[NSEQ], hi; };
            // (eight lanes per row: the lane's row is fixed for the launch, and its three operand addresses with it -- p1_hi / p1_hh /
            //  p1_g above the time loop; derived from the opaque row they were eleven vector instructions at the head of every P1)
            auto pre1 = [&](int row) {
                Ops1 o;
                if constexpr (LPR == 8 && NP1R > 0) {
                    o.hi = *p1_hi;
#pragma unroll
                    for (int s = 0; s < NSEQ; s++) { o.gpre[s] = TVc[s * tvl + p1_g]; o.hh[s] = p1_hh[s * c2p]; }
                } else {
                    const bool isr = row >= S;
                    const int j = isr ? row - S : row;
                    o.hi = Hinit[j];
#pragma unroll
                    for (int s = 0; s < NSEQ; s++) { o.gpre[s] = TVc[s * tvl + Rp + (isr ? SP : 0) + j]; o.hh[s] = H[s * c2p + j]; }
                }
                return o;
            };
            auto epi1o = [&](int row, const float (&acc)[NSEQ], const Ops1 &o) {
                const bool isr = row >= S;
                const int j = isr ? row - S : row;
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (!act[s]) continue;
                    const float g = gate_sigmoid<FASTQ>(acc[s] + o.gpre[s], sig_k);
                    if (!isr) {
                        Z[s * SP + j] = g;
                    } else {
                        const float hb = (1.0f - g) * o.hi + g * o.hh[s];
                        HBc[s * c2p + j] = hb;
                        X3c[s * c3p + Rp + j] = hb;
                    }
                }
            };
            if (!dbg_on(1)) {
                if constexpr (NP1R > 0 && OPA) {
                    rowdots_regs<NSEQ, NP1R, NCH2R, 0, LPR, 0, HALF2, NPLX>(w1, p.n1, p.nch2, H, c2p, tid, epi1o, nullptr, nullptr, pre1, L1, ld2);
                } else if constexpr (NP1R > 0) {
                    // (mixed forms: the rows behind the register passes -- the plan keeps them LDS-resident -- ride as one more pass of
                    //  the eight-lane sweep; the four-lane forms' chunk counts leave no register for that: rowdots_few)
                    rowdots_regs<NSEQ, NP1R, NCH2R, 0, LPR, 0, HALF2, NPLX>(w1, p.n1, p.nch2, H, c2p, tid, epi1, nullptr, nullptr, 0, L1, ld2);
                    if (MIXED && !NPLX && p.n1 > R1) {
                        auto shifted = [&](int row, const float (&acc)[NSEQ]) { epi1(row + R1, acc); };
                        rowdots_few<NSEQ>(L1, p.n1 - R1, ld2, p.nch2, H, c2p, tid, shifted);
                    }
                } else rowdots<NSEQ>(L1, p.P1, p.res1, p.n1, ld2, p.nch2, H, c2p, tid, epi1);
            }
            if (pr) pt[1] = (long long)__builtin_amdgcn_s_memtime();
            FARNN_DR_ISSUE_PREFETCH()
            wg_barrier_lds();
            if (pr) pt[2] = (long long)__builtin_amdgcn_s_memtime();
        }
#undef FARNN_DR_ISSUE_PREFETCH
        {   // ---- P2: rr = v * (Sa^T . hb)  (:169-170 / :174-175); farnn==1: z from the same h ------------
            auto epi2 = [&](int row, const float (&acc)[NSEQ]) {
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (farnn != 1 || row < R) X3c[s * c3p + row] = acc[s] * TVc[s * tvl + row];      // (rows R.. exist with farnn = 1 only)
                    else Z[s * SP + (row - R)] = gate_sigmoid(acc[s] + TVc[s * tvl + Rp + (row - R)], sig_k);
                }
            };
            struct Ops2 { float tv[NSEQ]; };
            auto pre2 = [&](int row) {
                Ops2 o;
#pragma unroll
                for (int s = 0; s < NSEQ; s++) o.tv[s] = TVc[s * tvl + ((farnn != 1 || row < R) ? row : Rp + (row - R))];
                return o;
            };
            auto epi2o = [&](int row, const float (&acc)[NSEQ], const Ops2 &o) {
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (farnn != 1 || row < R) X3c[s * c3p + row] = acc[s] * o.tv[s];                  // (compile-time for the gated forms)
                    else Z[s * SP + (row - R)] = gate_sigmoid<FASTQ>(acc[s] + o.tv[s], sig_k);
                }
            };
            if (!dbg_on(1)) {
                if constexpr (OPA && NP2R > 0) {
                    rowdots_regs<NSEQ, NP2R, NCH2R, 0, LPR, 0, HALF2, NPLX>(w2, p.n2, p.nch2, HBc, c2p, tid, epi2o, nullptr, nullptr, pre2, L2, ld2);
                } else if constexpr (LPR == 8) {                // (rows_plan_try: all of P2 LDS-resident, at most 256 rows)
                    if (p.n2 <= 2 * RPPR) rowdots_lds8<NSEQ, 2>(L2, p.n2, ld2, p.nch2, HBc, c2p, tid, epi2o, pre2);
                    else if (p.n2 <= 3 * RPPR) rowdots_lds8<NSEQ, 3>(L2, p.n2, ld2, p.nch2, HBc, c2p, tid, epi2o, pre2);
                    else rowdots_lds8<NSEQ, 4>(L2, p.n2, ld2, p.nch2, HBc, c2p, tid, epi2o, pre2);
                } else if constexpr (NP2R > 0) {
                    rowdots_regs<NSEQ, NP2R, NCH2R>(w2, p.n2, p.nch2, HBc, c2p, tid, epi2);
                    if (MIXED && p.n2 > R2) {                   // (mixed form: the rows behind the register passes)
                        auto shifted = [&](int row, const float (&acc)[NSEQ]) { epi2(row + R2, acc); };
                        rowdots_few<NSEQ>(L2, p.n2 - R2, ld2, p.nch2, HBc, c2p, tid, shifted);   // (the plan keeps them LDS-resident)
                    }
                } else rowdots<NSEQ>(L2, p.P2[dir], p.res2, p.n2, ld2, p.nch2, HBc, c2p, tid, epi2);
            }
        }
        if (pr) pt[3] = (long long)__builtin_amdgcn_s_memtime();
        // (issued behind P2's products: in front of them the 8 NCH3G registers were live beside P2's working set)
        v4f g3[NCH3G > 0 ? 2 * NCH3G : 1];
        if constexpr (NCH3G > 0) {
            const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NCH3G; c++) {
                const bool in = NCH3K + c < p.nch3;
                g3[2 * c] = in ? g3src[(NCH3K + c) * 8] : zero;
                g3[2 * c + 1] = in ? g3src[(NCH3K + c) * 8 + 4] : zero;
            }
        }
        {   // park the prefetched per-token vectors BEFORE this step's stash stores are issued: vmcnt retires
            // in order, so waiting for these loads later would also wait for every younger store
            // (a use on every path: the loads are waited for HERE whatever the slot's condition -- left to the conditional store, the
            //  compiler carried "maybe pending" round the loop and waited vmcnt(0) at the next step's first re-use of the registers)
#pragma unroll
            for (int i = 0; i < NPF; i++) asm volatile("" :: "v"(pf[i]));
#pragma unroll
            for (int i = 0; i < NPF; i++)
                if (pf_e[i] >= 0) TVn[tid + i * DR_THREADS] = pf[i];
        }
        wg_barrier_lds();
        if (pr) pt[4] = (long long)__builtin_amdgcn_s_memtime();
        {   // ---- P3: nx = Sb . rr + W(^T) . hb, non-linearity, gate mix, stash  (:171-196) -----------------
            auto epi3 = [&](int row, const float (&acc)[NSEQ]) {
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (!act[s]) continue;
                    const float nx = dbg_on(2) ? acc[s] : dr_nl(acc[s], nl_mode);
                    float hn = nx;
                    if (farnn == 2) {
                        const float z = Z[s * SP + row];
                        hn = (1.0f - z) * H[s * c2p + row] + z * nx;
                        H[s * c2p + row] = hn;
                    } else {
                        if (farnn == 1) {
                            const float z = Z[s * SP + row];
                            hn = (1.0f - z) * HBc[s * c2p + row] + z * nx;
                        }
                        HBn[s * c2p + row] = hn;
                        X3n[s * c3p + Rp + row] = hn;
                    }
                    if (!dbg_on(4)) stash_base[((long long)bseq[s] * (p.L + 1) + t + 1) * SP + row] = hn;
                }
            };
            struct Ops3 { float z[NSEQ], h[NSEQ]; };             // (the eight-lane forms: farnn = 2)
            // (p3_z / p3_h: this lane's row of Z and H, fixed above the time loop like P1's operands -- the same two addresses serve the
            //  reads in front of the products and the state's write behind them)
            auto pre3 = [&](int row) {
                Ops3 o;
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if constexpr (LPR == 8 && NP3R > 0) { o.z[s] = p3_z[s * SP]; o.h[s] = p3_h[s * c2p]; }
                    else { o.z[s] = Z[s * SP + row]; o.h[s] = H[s * c2p + row]; }
                }
                return o;
            };
            auto epi3o = [&](int row, const float (&acc)[NSEQ], const Ops3 &o) {
#pragma unroll
                for (int s = 0; s < NSEQ; s++) {
                    if (!act[s]) continue;
                    const float nx = dbg_on(2) ? acc[s] : dr_nl<FASTQ>(acc[s], nl_mode);
                    const float hn = (1.0f - o.z[s]) * o.h[s] + o.z[s] * nx;
                    if constexpr (LPR == 8 && NP3R > 0) p3_h[s * c2p] = hn;
                    else H[s * c2p + row] = hn;
                    if (!dbg_on(4)) stash_base[((long long)bseq[s] * (p.L + 1) + t + 1) * SP + row] = hn;
                }
            };
            if (!dbg_on(1)) {
                if constexpr (NP3R > 0 && OPA) {
                    if constexpr (NPLX) rowdots_regs<NSEQ, NP3R, NCH3K, 0, LPR, NCH3L, 0, 1>(w3, p.n3, p.nch3, X3c, c3p, tid, epi3o, nullptr, T3, pre3, L3, ld3);
                    else rowdots_regs<NSEQ, NP3R, NCH3K, NCH3G, LPR, NCH3L>(w3, p.n3, p.nch3, X3c, c3p, tid, epi3o, g3, T3, pre3);
                } else if constexpr (NP3R > 0) {
                    if constexpr (NPLX)
                        rowdots_regs<NSEQ, NP3R, NCH3K, 0, LPR, 0, 0, 1>(w3, p.n3, p.nch3, X3c, c3p, tid, epi3, nullptr, nullptr, 0, L3, ld3);
                    else {
                        rowdots_regs<NSEQ, NP3R, NCH3K, NCH3G, LPR, NCH3L>(w3, p.n3, p.nch3, X3c, c3p, tid, epi3, g3, T3);
                        if (MIXED && p.n3 > R3) {               // (the four-lane mixed forms)
                            auto shifted = [&](int row, const float (&acc)[NSEQ]) { epi3(row + R3, acc); };
                            rowdots_few<NSEQ>(L3, p.n3 - R3, ld3, p.nch3, X3c, c3p, tid, shifted);
                        }
                    }
                } else rowdots<NSEQ>(L3, p.P3[dir], p.res3, p.n3, ld3, p.nch3, X3c, c3p, tid, epi3);
            }
        }
        if (pr) pt[5] = (long long)__builtin_amdgcn_s_memtime();
        { const float *a = TVc; TVc = TVn; TVn = const_cast<float *>(a); float *b = HBc; HBc = HBn; HBn = b; b = X3c; X3c = X3n; X3n = b; }
        wg_barrier_lds();
        if (pr) {
            pt[6] = (long long)__builtin_amdgcn_s_memtime();
            if ((tid & 63) == 0)
                printf("rows wg 0 wave %d step 8: P1 %lld (+barrier %lld), P2 %lld (+park, barrier %lld), P3 %lld (+barrier %lld), step %lld cycles\n",
                       tid >> 6, pt[1] - pt[0], pt[2] - pt[1], pt[3] - pt[2], pt[4] - pt[3], pt[5] - pt[4], pt[6] - pt[5], pt[6] - pt[0]);
        }
    }
    }   // rounds
}

// ---- packing (create time) ------------------------------------------------------------------------
// P2[dir] row r < R: Sa[:, r] (fwd Sa = S1, bwd Sa = S2 with the backward input scaling o folded in);
//          row R + j (farnn==1): Wss1[:, j].     P1 row j: Wss1[:, j]; row S + j: Wss2[:, j].
// P3[dir] row j: [Sb[j, :] | pad to Rp | Wd[:, j]] (fwd Sb = S2, Wd[s] = W[s][j], row scaled by o[j];
//          bwd Sb = S1, Wd[s] = W[j][s] * o[s]).
struct PackSrc {
    const float *S1, *S2, *W;     // [S][Rp], [S][Rp], [S][SP]
    const float *Wss1, *Wss2;     // [S][SP] or nullptr
    const float *o;               // [SP]
    int S, SP, R, Rp, farnn;
};

__global__ void pack_p2_kernel(PackSrc q, float *out, int nrows, int ld, int dir) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nrows * ld) return;
    const int row = (int)(idx / ld), s = (int)(idx % ld);
    float v = 0.0f;
    if (s < q.S) {
        if (row < q.R) v = dir == 0 ? q.S1[(long long)s * q.Rp + row] : q.S2[(long long)s * q.Rp + row] * q.o[s];
        else v = q.Wss1[(long long)s * q.SP + (row - q.R)];
    }
    out[idx] = v;
}

__global__ void pack_p1_kernel(PackSrc q, float *out, int ld) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2LL * q.S * ld) return;
    const int row = (int)(idx / ld), s = (int)(idx % ld);
    float v = 0.0f;
    if (s < q.S) v = row < q.S ? q.Wss1[(long long)s * q.SP + row] : q.Wss2[(long long)s * q.SP + (row - q.S)];
    out[idx] = v;
}

__global__ void pack_p3_kernel(PackSrc q, float *out, int ld, int dir) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)q.S * ld) return;
    const int j = (int)(idx / ld), c = (int)(idx % ld);
    float v = 0.0f;
    if (c < q.R) {
        v = dir == 0 ? q.S2[(long long)j * q.Rp + c] * q.o[j] : q.S1[(long long)j * q.Rp + c];
    } else if (c >= q.Rp && c < q.Rp + q.S) {
        const int s = c - q.Rp;
        v = dir == 0 ? q.W[(long long)s * q.SP + j] * q.o[j] : q.W[(long long)j * q.SP + s] * q.o[s];
    }
    out[idx] = v;
}

// G[v][j] = sum_r Vgen[v][r] Wrs[r][j] + bs[j]   (the token half of a gate, :144-148)
// written at column `col0` of the combined per-word table T[V][ldt]
__global__ void gate_table_kernel(const float *Vgen, const float *Wrs, const float *bs, float *T, int ldt, int col0,
                                  int V, int R, int Rp, int S, int SP) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)V * SP) return;
    const int v = (int)(idx / SP), j = (int)(idx % SP);
    float acc = 0.0f;
    if (j < S) {
        for (int r = 0; r < R; r++) acc = fmaf(Vgen[(long long)v * Rp + r], Wrs[(long long)r * SP + j], acc);
        acc += bs[j];
    }
    T[(long long)v * ldt + col0 + j] = acc;
}

// T[v][0..Rp) = Vgen[v][0..Rp): the first segment of the combined per-word table
__global__ void word_rows_kernel(const float *Vgen, float *T, int ldt, int V, int Rp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)V * Rp) return;
    T[idx / Rp * ldt + idx % Rp] = Vgen[idx];
}

// everything the launcher needs, filled by build_rows_pack() in farnn_hip.hip
struct DecompRowsPack {
    bool ok = false;
    float *P1 = nullptr, *P2[2] = {nullptr, nullptr}, *P3[2] = {nullptr, nullptr};
    const float *TVt = nullptr;     // [V][tvl] per-word rows: Vgen | update-gate table | reset-gate table (farnn = 0: Vgen itself)
    int n1 = 0, n2 = 0, n3 = 0, ld2 = 0, ld3 = 0, nch2 = 0, nch3 = 0;
};

// row length in floats for `cols` columns: whole 32-column chunks, +16 so that the four rows a 16-lane
// LDS access group touches (64 contiguous bytes each) start in different quarters of the 64 banks
inline int rows_ld(int cols) { return (cols + DR_CHUNK - 1) / DR_CHUNK * DR_CHUNK + 16; }

struct RowsPlan { int nseq, res1, res2, res3; size_t lds; int form; };   // form: which matrices live in registers (0: none)

// register-resident forms that are instantiated (one sequence per workgroup): UPPER BOUNDS on the passes of P1 / P2, the
// chunks of their rows and the passes / chunks of P3 (in order of cost; the first that holds the model is taken).
// 1: farnn = 2, S <= 128, Rp + SP <= 224 (rank ~100-120); 2: farnn = 1 with R + S <= 256; 3: farnn = 2, S <= 128,
// Rp + SP <= 384 (rank 150 / 250: the shipped example configurations).
// 4: farnn = 2 at 128 < S <= 160 (the shipped configurations with --additional_states 30 at this automaton size): the gate
// rows alone in registers, P2 / P3 in LDS as far as it goes, the rest streamed.
// 5 / 6 (round 3, MIXED: the registers hold a matrix's first passes, the rows behind them are LDS-resident): farnn = 2 at
// 128 < S <= 160 with the output rows in registers too: two passes of gate rows + the 12 behind them in LDS, one pass of output
// rows + the 6 behind it in LDS, P2 in LDS -- 5: Rp + SP <= 288 (rank 150 + additional states: P2 fits whole, nothing is
// streamed); 6: Rp + SP <= 416 (rank 250 + additional states: P2 as far as the LDS goes, 128 of its 250 rows).  (Three passes
// of gate rows beside a pass of output rows do not fit the 256 VGPRs of a lane: 46 spilled.)
// 7 / 8 (round 4): farnn = 2, S <= 128 like 1 / 3, with EIGHT lanes per row (passes of 64 rows, chunks of 64 columns: half the x
// reads per wavefront) and P2's rows (rank <= 256, all LDS-resident) swept in one go -- 8: Rp + SP <= 256, 7: Rp + SP <= 384.  They
// come first; FARNN_ROWS_LPR4=1 leaves them out.
// 10 (round 4, MIXED with eight lanes per row): farnn = 2 at 128 < S <= 160 with rank <= 192 (`--additional_states 30` at rank 150):
// four passes of gate rows, two of P2 and two of output rows (their first three chunks) in registers; in LDS the rows behind the
// register passes (12 gate rows, up to 64 of P2, 6 output rows) -- swept as one more pass -- and the output rows' last two chunks.
#define FARNN_ROWS_FORMS(X) X(9, 4, 4, 2, 2, 6) X(8, 4, 0, 2, 2, 4) X(7, 4, 0, 2, 2, 6) X(10, 4, 2, 3, 2, 5) X(1, 2, 0, 4, 1, 7) X(2, 0, 2, 4, 0, 0) X(3, 2, 0, 4, 1, 12) X(5, 2, 0, 5, 1, 9) X(6, 2, 0, 5, 1, 13) X(4, 3, 0, 5, 0, 0)
constexpr bool rows_form_mixed(int form) { return form == 5 || form == 6 || form == 10; }
constexpr int rows_form_lpr(int form) { return (form == 7 || form == 8 || form == 9 || form == 10) ? 8 : DR_LPR; }
constexpr bool rows_form_tail3(int form) { return form == 9 || form == 10; }
// prefetch slots of a form's instantiation (the kernel's NPF): forms whose chunk bounds keep the per-token vector within 512 floats
constexpr int rows_form_pf(int lpr, int nch2r, int np3r, int nch3r) {
    return (np3r > 0 && nch2r * (lpr == 8 ? 64 : 32) <= 128 && nch3r * (lpr == 8 ? 64 : 32) <= 384) ? 1 : DR_FORM_PF;
}       // the output rows' last 64-column chunk in LDS

// one attempt at `nseq` sequences per workgroup; forms: may a register-resident form be chosen
inline bool rows_plan_try(const DecompRowsPack &k, const DecompWeights &w, int L, int nseq, bool forms, RowsPlan &pl) {
    const int Lr = (L + 3) & ~3;
    const int tvl = w.Rp + (w.farnn >= 1 ? w.SP : 0) + (w.farnn == 2 ? w.SP : 0);
    if (nseq * tvl > DR_MAX_PF * DR_THREADS) return false;
    const size_t fixed = 4 * ((size_t)nseq * Lr + w.SP + 3ull * nseq * k.nch2 * DR_CHUNK +
                              2ull * nseq * k.nch3 * DR_CHUNK + (size_t)nseq * w.SP + 2ull * nseq * tvl);
    const size_t cap = 159 * 1024;
    if (fixed + 16 * 1024 > cap) return false;               // leave room for at least some resident rows
    size_t left = cap - fixed;
    auto take = [&](int nrows, int ld) {
        if (nrows == 0) return 0;
        long long fit = (long long)(left / ((size_t)ld * 4));
        int res = fit >= nrows ? nrows : (int)(fit / DR_RPP) * DR_RPP;
        left -= (size_t)res * ld * 4;
        return res;
    };
    pl.form = 0;
    if (forms && nseq == 1 && tvl <= DR_FORM_PF * DR_THREADS) {     // (two sequences per workgroup on these forms: measured slower, spills)
        const bool lpr4_only = tun(TUN_ROWS_LPR4) == 1, no_tail3 = tun(TUN_ROWS_LPR4) == 2;     // (2: without the all-in-registers form)
#define FARNN_ROWS_MATCH(F_, A_, B_, C_, D_, E_)                                                                   \
        if (!pl.form && !(rows_form_lpr(F_) == 8 && lpr4_only) && !(rows_form_tail3(F_) && no_tail3)) {                                            \
            /* passes and chunks in the form's own units (LPR = 8: 64 rows, 64 columns) */                         \
            constexpr int rpp = DR_THREADS / rows_form_lpr(F_), cpc = rows_form_lpr(F_) / 4;                       \
            const int np1 = (k.n1 + rpp - 1) / rpp, np2 = (k.n2 + rpp - 1) / rpp, np3 = (k.n3 + rpp - 1) / rpp;    \
            const int nc2 = (k.nch2 + cpc - 1) / cpc, nc3 = (k.nch3 + cpc - 1) / cpc;                              \
            if ((A_ == 0 || (k.n1 > 0 && (np1 <= A_ || rows_form_mixed(F_)) && nc2 <= C_)) &&                      \
                (B_ == 0 || ((np2 <= B_ || (rows_form_mixed(F_) && rows_form_lpr(F_) == 8 && np2 == B_ + 1)) && nc2 <= C_)) && \
                (D_ == 0 || ((np3 <= D_ || rows_form_mixed(F_)) && nc3 <= E_)) && (A_ > 0 || k.n1 == 0) &&         \
                (!rows_form_mixed(F_) || (np1 > A_ && np3 > D_)) &&  /* (mixed forms: only where the whole-matrix forms do not reach) */ \
                (rows_form_lpr(F_) != 8 || (k.n2 <= 4 * rpp && nc2 <= C_ && k.nch3 >= 8)) &&  /* (shorter rows: form 1 is faster) */ \
                (!(rows_form_mixed(F_) && rows_form_lpr(F_) == 8) || k.nch2 <= 2 * C_ - 1) &&  /* (its last chunk of gate row: the first piece only) */ \
                tvl <= rows_form_pf(rows_form_lpr(F_), C_, D_, E_) * DR_THREADS) {  /* (its prefetch slots hold the per-token vector) */ \
                /* the matrices left outside the registers go to the LDS as far as it holds them (whole, for forms 1-3 at   \
                   the sizes they were made for), the remainder is streamed as before; a mixed form's rows behind its     \
                   register passes first: they are few */                                                          \
                pl.form = F_;                                                                                      \
                const size_t left0 = left;                                                                         \
                const int t3 = k.n3 > D_ * rpp ? k.n3 - D_ * rpp : 0, t1 = k.n1 > A_ * rpp ? k.n1 - A_ * rpp : 0;  \
                pl.res3 = take(t3, k.ld3);                                                                         \
                pl.res1 = take(t1, k.ld2);                                                                         \
                if (rows_form_mixed(F_) && (pl.res3 < t3 || pl.res1 < t1 || k.nch2 > 16 || k.nch3 > 16)) {         \
                    pl.form = 0; left = left0;          /* its rows behind the register passes must all be LDS-resident */ \
                } else {                                                                                           \
                    const int t2 = k.n2 > B_ * rpp ? k.n2 - B_ * rpp : 0;                                          \
                    pl.res2 = take(t2, k.ld2);                                                                     \
                    const size_t tail3 = rows_form_tail3(F_) ? (size_t)k.n3 * DR_T3LD * 4 : 0;                     \
                    if (rows_form_lpr(F_) == 8 && (pl.res2 < t2 || left < tail3)) { pl.form = 0; left = left0; }   /* (its P2 sweep: all rows resident) */ \
                    else left -= tail3;                                                                            \
                }                                                                                                  \
            }                                                                                                      \
        }
        FARNN_ROWS_FORMS(FARNN_ROWS_MATCH)
#undef FARNN_ROWS_MATCH
    }
    if (!pl.form) {
        pl.res3 = take(k.n3, k.ld3);
        pl.res2 = take(k.n2, k.ld2);
        pl.res1 = take(k.n1, k.ld2);
    }
    pl.nseq = nseq;
    // Register forms read whole vector chunks, up to a chunk past the model's width: everything up to the end of the ALLOCATION
    // must be initialised.  The kernel zeroes its tail up to lds_floats; round that up to a multiple of both 1 KiB (LDS-DMA
    // pieces) and the LDS allocation granule (1280 B on gfx950: what the hardware hands out beyond the request), capped by
    // the 160 KiB of the CU, so that no allocated-but-unzeroed slack can sit behind it
    pl.lds = (cap - left + 5119) / 5120 * 5120;
    if (pl.lds > 160 * 1024) pl.lds = 160 * 1024;
    return true;
}

inline bool rows_plan(const DecompRowsPack &k, const DecompWeights &w, int B, int L, RowsPlan &pl) {
    const bool forms = !tun(TUN_ROWS_NOREGS);
    if (const int v = tun(TUN_ROWS_NSEQ)) {
        if (v == 1 || v == 2 || v == 4) {
            for (int n = v; n >= 1; n /= 2)
                if (rows_plan_try(k, w, L, n, forms, pl)) return true;
            return false;
        }
    }
    // a register-resident form (one sequence per workgroup, no weight leaves the CU after set-up) beats sharing streamed
    // weights between sequences for any batch that is not huge: 210 vs 354 us at B = 256 for the gated rank-250 shape
    if (forms && B <= 1024 && rows_plan_try(k, w, L, 1, true, pl) && pl.form) return true;
    // measured (B=256, S=104): one sequence per workgroup in two rounds beats two per workgroup in one
    // (145 vs 168 us at R=50, 374 vs 450 us gated R=250): the x reads and FMAs scale with NSEQ, only the
    // weight reads are shared
    int nseq = 1;
    while (nseq < 4 && 2 * ((B + nseq - 1) / nseq) > 512 * nseq) nseq *= 2;
    for (; nseq >= 1; nseq /= 2)
        if (rows_plan_try(k, w, L, nseq, forms, pl)) return true;
    return false;
}

template <int NSEQ, int A_ = 0, int B_ = 0, int C_ = 0, int D_ = 0, int E_ = 0, bool MIXED = false, int LPR = DR_LPR>
inline int launch_rows_n(const DecompRowsParams &p, int wg_limit, size_t lds, hipStream_t s) {
    static int raised = -1;     // per process and instantiation; the attribute is per (device, function) but monotone in lds
    const void *fn = reinterpret_cast<const void *>(decomp_rows_kernel<NSEQ, A_, B_, C_, D_, E_, MIXED, LPR>);
    if ((int)lds > raised) {
        FARNN_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        raised = 160 * 1024;
    }
    // wg_limit > 0 (a register form on a device of wg_limit compute units): no more workgroups than run at once, each walking the
    // groups of its slot (the kernel's rounds); else one workgroup per group and direction
    int slots = p.groups;
    if (wg_limit > 0) {
        static size_t occ_lds = 0; static int occ = 0;
        if (occ == 0 || occ_lds != lds) {
            int n = 0;
            FARNN_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, DR_THREADS, lds));
            occ = n > 0 ? n : 1; occ_lds = lds;
        }
        const int fit = wg_limit * occ / 2;
        if (fit >= 1 && fit < slots) slots = fit;
        if (FARNN_PROBE_ON((p.dbg & 16) != 0)) fprintf(stderr, "rows launch: %d groups per direction, %d workgroups per compute unit, %d slots\n", p.groups, occ, slots);
    }
    decomp_rows_kernel<NSEQ, A_, B_, C_, D_, E_, MIXED, LPR><<<dim3(2 * slots), dim3(DR_THREADS), lds, s>>>(p);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

inline int launch_decomp_rows(const DecompRowsPack &k, const DecompWeights &w, const RowsPlan &pl,
                              const int64_t *x, const int64_t *len, const int *order, int sort,
                              float *A, float *Bk, int B, int L, int full, int cu_limit, hipStream_t s) {
    DecompRowsParams p;
    p.P1 = k.P1; p.P2[0] = k.P2[0]; p.P2[1] = k.P2[1]; p.P3[0] = k.P3[0]; p.P3[1] = k.P3[1];
    p.n1 = k.n1; p.n2 = k.n2; p.n3 = k.n3; p.ld2 = k.ld2; p.ld3 = k.ld3; p.nch2 = k.nch2; p.nch3 = k.nch3;
    p.res1 = pl.res1; p.res2 = pl.res2; p.res3 = pl.res3;
    p.TVt = k.TVt; p.h0 = w.h0; p.hT = w.hT;
    p.x = x; p.len = len; p.order = order; p.sort = sort; p.A = A; p.Bk = Bk;
    p.B = B; p.L = L; p.S = w.S; p.SP = w.SP; p.R = w.R; p.Rp = w.Rp; p.farnn = w.farnn; p.nl = w.nl;
    p.full = full; p.V = w.V; p.sig_k = w.sig_k;
    p.dbg = tun(TUN_DBG);
    p.lds_floats = (int)(pl.lds / 4);
    const int groups = (B + pl.nseq - 1) / pl.nseq;
    p.groups = groups;
#define FARNN_ROWS_LAUNCH(F_, A_, B_, C_, D_, E_) if (pl.form == F_) return launch_rows_n<1, A_, B_, C_, D_, E_, rows_form_mixed(F_), rows_form_lpr(F_)>(p, cu_limit, pl.lds, s);
    FARNN_ROWS_FORMS(FARNN_ROWS_LAUNCH)
#undef FARNN_ROWS_LAUNCH
    if (pl.nseq == 4) return launch_rows_n<4>(p, cu_limit, pl.lds, s);
    if (pl.nseq == 2) return launch_rows_n<2>(p, cu_limit, pl.lds, s);
    return launch_rows_n<1>(p, cu_limit, pl.lds, s);
}

}  // namespace farnn
