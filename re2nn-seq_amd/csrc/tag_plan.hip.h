// The plan of ONE farnn_tag / farnn_tag_vectors call: everything that is decided about it -- which launches serve it and in which form -- as plain
// host state.  plan_tag (farnn_hip.hip) fills it from the model, (B, L), the mode and the outputs asked for, before anything is
// enqueued; the launch_* helpers there read it and decide nothing; the handle keeps the last call's plan, and farnn_kernel_name /
// farnn_kernel_algorithmic_bytes report from it.
#pragma once
#include "decomp_rows.hip.h"
#include "decomp_regs.hip.h"

namespace farnn {

enum PrepForm { PREP_NONE, PREP_SMALL /* batch_prep_small_kernel */, PREP_LARGE /* batch_prep_kernel */ };
enum RecForm {
    REC_COMPACT_TAG,          // compact_tag_kernel<NW, nonlinearity>: both chains, label-map scores and decode in one launch
    REC_COMPACT_CHAIN,        // compact_chain_kernel
    REC_CHAIN_REGS,           // chain_regs_kernel (S <= 72)
    REC_CHAIN_WIDE,           // chain_wide_kernel (72 < S <= 128), one workgroup per compute unit
    REC_CHAIN_WIDE_PAIRED,    // ... two workgroups per compute unit, label-map scores beside the recurrence
    REC_CHAIN_VITERBI,        // chain_viterbi_kernel: recurrence + scores + CRF decode (A/B build only)
    REC_CHAIN_KERNEL,         // chain_kernel<NCH, maxsr, FQ>
    REC_DECOMP_REGS,          // decomp_regs_kernel / decomp_regs8_kernel
    REC_DECOMP_ROWS,          // decomp_rows_kernel
    REC_DECOMP_CHAIN,         // decomp_chain_kernel
};
enum ScoreForm {
    SCORE_NONE,               // scores and decode ran in the recurrence launch
    SCORE_VITERBI_FUSED,      // viterbi_hist_kernel<IB4, true>: stash -> scores -> Viterbi -> tags
    SCORE_LABEL_MAP,          // label_map_score_kernel
    SCORE_TILE,               // score_tile_kernel<KCH> (+ the Viterbi launch under a CRF)
    SCORE_FST4,               // fst4_score_kernel
    SCORE_IND1,               // ind1_score_kernel
    SCORE_DECOMP1,            // decomp1_br_mfma_kernel + decomp1_label_kernel, or decomp1_score_kernel (+ Viterbi)
    SCORE_DECOMP0,            // decomp0_score_kernel (+ Viterbi)
};
enum ViterbiForm { VITERBI_NONE, VITERBI_HIST /* partition history in LDS */, VITERBI_BP /* stored back-pointers */ };

struct TagPlan {
    bool planned = false;                   // false: no call planned since the handle was created (or farnn_set_compact changed its form)
    int B = 0, L = 0, full = 0;             // L: every stride of the workspace arrays in this call
    // ---- batch prep: flat-output offsets and the length-sorted launch order
    bool want_order = false, want_offs = false;
    bool prep_in_kernel = false;            // no prep launch: the workgroups rank and sum the lengths themselves
    bool sort_in_kernel = false;            // ... and select their sequence by length rank
    bool order_valid = false;               // the recurrence reads the launch order the prep launch wrote
    int prep = PREP_NONE, prep_G = 1;       // PREP_SMALL: lanes per sequence
    // ---- the token table of a vector-input call (farnn_tag_vectors): token_table_kernel in front of the recurrence, which then
    // runs on the identity ids with V = B L
    bool table = false;
    int table_cols = 0;                     // its gate columns: 0 (farnn = 0: the padded copy alone), SP or 2 SP
    // ---- the token blocks of a max-semiring vector-input call: token_blocks_kernel in front of the dense chain kernels, which then
    // read the workspace's blocks on the identity ids with V = B L
    bool blocks = false;
    // ---- recurrence
    int rec = REC_CHAIN_KERNEL;
    bool fused = false;                     // scores + decode beside the recurrence: the call's ONE launch
    // the register-fed forms (chain_regs_params.hip.h)
    bool lm_path = false;                   // ... scored through the label map
    bool dest = false, half = false, row80 = false;     // RegsParams::dest / half / row80
    bool host_epoch = false;                // diagnostic FARNN_HOST_EPOCH=1
    size_t lds = 0;                         // dynamic LDS of the recurrence launch (register-fed forms, chain_kernel, compact_tag_kernel)
    int NCH = 1, FQ = 0, KS = 2, NQP = 1, PPS = 1, block = 0;      // chain_kernel: instantiation, ring shape, threads
    int NW = 1, nlk = 0;                    // compact_tag_kernel: 32-bit words of a bitmap row in use, nonlinearity index
    RegsPlan regs;                          // decomp_regs
    RowsPlan rows; int rows_cu = 0;         // decomp_rows; compute units its register forms walk their groups over (0: one workgroup per group)
    // ---- scores + decode
    int score = SCORE_NONE;
    int kch = 1;                            // score_tile_kernel<KCH>
    int viterbi = VITERBI_NONE, ib4 = 0;    // the Viterbi launch behind (or instead of) the score launch, its IB4
    size_t viterbi_lds = 0;
    bool d1_mfma = false, d1_staged = false;    // SCORE_DECOMP1: the per-word table on the matrix cores; its label kernel with the weights in LDS
};

}  // namespace farnn
