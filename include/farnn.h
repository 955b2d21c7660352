/*
 * farnn.h -- C-ABI of the MI355X-native FA-RNN forward tagging path (libfarnn_hip.so).
 *
 * The reference (jeffchy/RE2NN-SEQ) is pure PyTorch and has no FFI of its own; the seam this
 * library replaces is the nn.Module method contract consumed by the reference's callers
 * (SURVEY.md section 8b).  Each entry point cites the reference interface it stands in for
 * (paths relative to the reference checkout).  The reference-side binding a maintainer would
 * add (a ctypes stub inside the model classes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch / C++ types in any signature;
 *   - every function returns FARNN_OK (0) or a negative errno-style code, never throws;
 *     farnn_last_error() returns a human-readable message for the calling thread;
 *   - weights are given as HOST pointers (float32, C-contiguous) unless desc.weights_on_device
 *     is set; create() copies them into device-resident, re-laid-out storage that the handle
 *     owns until farnn_destroy();
 *   - x / lengths / tags / scores of farnn_tag() are DEVICE pointers (e.g. tensor.data_ptr()
 *     of PyTorch-ROCm tensors used purely as containers); the library never retains them
 *     after the call's work has been enqueued on `stream`;
 *   - one caller thread per handle (the reference is single-threaded Python); one workspace per handle: a call on another
 *     stream than the previous call's is ordered behind that call's work by the library.  The ONE thing the handle keeps of a
 *     call is its stream handle, until the next call: the first time a handle is called on a different stream, the previous
 *     call's stream must still exist (the library records its ordering event there); from then on every call leaves the
 *     handle's own event behind itself and earlier streams are never touched again.  A call that is being captured into a
 *     HIP graph is not ordered against other streams.
 *
 * Environment switches (read ONCE per handle, when farnn_*_create / farnn_train_create builds it; no call on the tagging path
 * touches the environment).  Every one selects between code paths that the test suite holds to the same results.  Those marked
 * [A/B build only] select forms the production library does not carry (its dispatch never picks them: 54 kernels): they exist in
 * the A/B build (csrc/build.py --probes -> libfarnn_hip_probes.so, loaded through FARNN_LIB; farnn_ab_build() says which one is
 * loaded), and farnn_*_create of the production library answers them with FARNN_EINVAL and a message that says so (like every
 * switch they are resolved when the handle is created, never at tag time); switches of earlier rounds that no longer exist
 * (FARNN_CV_WIDE, FARNN_DECOMP_OLD) are refused the same way by both builds:
 *   FARNN_NOFUSE=1          the multi-launch forms (recurrence kernel, then score / Viterbi kernel) instead of one launch per step
 *                           (also: the compact form's two launches instead of compact_tag_kernel)
 *   FARNN_FUSE=1            onehot i-FST, S <= 72, label-map scores: ONE launch per step (scores + decode beside the recurrence) instead of
 *                           the default there, the recurrence kernel + the label-map score launch (faster at every measured shape)
 *   FARNN_NOREGS=1          the LDS-ring recurrence kernel where the register-fed one (S <= 128) would run
 *   FARNN_NODEST=1          [A/B build only] S <= 72, sum semiring: round 3's compute wavefronts (a block split by SOURCE rows,
 *                           partial sums reduced across the wavefronts) instead of the destination-split ones (chain_dest.hip.h)
 *   FARNN_NOHALF=1          onehot i-FST, S <= 72, sum semiring: the recurrence reads the f32 blocks even where every block entry is an
 *                           IEEE f16 exactly (a 0/1 or small-integer automaton: the default there reads a 16-bit image of the blocks,
 *                           the same f32 arithmetic in the same order, bit-identical results); no image is built at create
 *   FARNN_NOLABELMAP=1      scores on the matrix cores even when the output matrix is a label map (one state, one label, weight 1)
 *   FARNN_CV_ONE=1          [A/B build only] a CRF on the onehot i-FST, S <= 108: recurrence + scores + Viterbi in ONE launch
 *                           (chain_viterbi_kernel).  Two launches are faster at every measured shape
 *   FARNN_WIDE_UNPAIRED=1   72 < S <= 108: one workgroup per compute unit for the wide recurrence (default: two, label-map scores)
 *   FARNN_CV_STASH=1        [A/B build only] the one-launch CRF kernel with the state rows through the stash instead of LDS
 *   FARNN_VITERBI_BP=1 / FARNN_VITERBI_UNFUSED=1   the stored-back-pointer Viterbi kernel / scores through HBM in front of it
 *   FARNN_PREP=1, FARNN_NOSORT=1                   the separate batch-prep kernel / the batch's own launch order
 *   FARNN_DECOMP_NOREGS=1, FARNN_ROWS_NOREGS=1     the decomposed recurrence's LDS-fed kernels instead of the register forms
 *   FARNN_ROWS_LPR4=1|2     gated decomposed models (farnn = 2, S <= 160): 1 = four lanes per row instead of eight (round 3's forms),
 *                           2 = eight lanes per row but P2 swept from LDS (without the all-in-registers / mixed eight-lane forms)
 *   FARNN_ROWS_NOROUNDS=1   the decomposed recurrence's register forms with one workgroup per sequence and direction (round 5) instead of
 *                           one per compute unit walking its sequences with the weights kept in registers
 *   FARNN_TRAIN_NOLDS=1|2, FARNN_TRAIN_NSEQ=2|4    training chains with the matrices read through L2 / sequences per workgroup
 * Diagnostic switches (ablations, geometry overrides: FARNN_DBG, FARNN_KS, FARNN_RPG, FARNN_NLD, FARNN_FUSE_SPIN, FARNN_SOLO_MARGIN,
 * ...) exist only in the profiling build of the library (csrc/build.py --probes); the production library ignores them.
 */
#ifndef FARNN_H
#define FARNN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: FARNN_MODE_RE, farnn_tag_host_submit/_wait, farnn_flatten_host, the compact / folded creators, farnn_set_compact
 * (round 2); calls on different streams of one handle are ordered by the library (round 3).  1: round 1. */
#define FARNN_ABI_VERSION 2

/* ---- return codes ------------------------------------------------------------------- */
#define FARNN_OK         0
#define FARNN_EINVAL   (-22)   /* bad argument / unsupported combination               */
#define FARNN_ENOMEM   (-12)   /* device or host allocation failed                     */
#define FARNN_ENODEV   (-19)   /* no usable HIP device                                 */
#define FARNN_EIO       (-5)   /* a HIP runtime call failed (see farnn_last_error)     */
#define FARNN_ERANGE   (-34)   /* size beyond what the kernels support                 */

/* ---- enumerations ------------------------------------------------------------------- */
/* --update_nonlinear (reference main.py:93, model_onehot.py:379-386) */
#define FARNN_NL_NONE      0
#define FARNN_NL_RELU      1
#define FARNN_NL_TANH      2
#define FARNN_NL_RELUTANH  3
#define FARNN_NL_SIGMOID   4   /* only --additional_nonlinear uses it (model_decompose.py:232) */
/* --train_mode (reference main.py:33, utils.py:192-199) */
#define FARNN_SEMIRING_SUM 0
#define FARNN_SEMIRING_MAX 1
/* farnn_tag() modes */
#define FARNN_MODE_LOCAL   0   /* forward_local: valid positions only (model_onehot.py:131-146) */
#define FARNN_MODE_FULL    1   /* forward_score: all L positions incl. pads, scores unclamped (:351-428) */
#define FARNN_MODE_RE      2   /* forward_RE (:148-160): FULL, and the `oo` column (C-1) of `scores` comes back capped at the
                                  threshold (:153-154); onehot models only */

typedef struct farnn_model farnn_model;   /* opaque handle */

/* ---- onehot i-FST: FARNN_S_O_I_S (reference model_onehot.py:310-428), --independent 2 ---- */
typedef struct farnn_onehot_ifst_desc {
    int32_t V, S, C;            /* vocabulary (incl. pad row), states, label columns (len(s2i)+1) */
    const float *T;             /* [V,S,S] language_tensor   (:326-328)                     */
    const float *W;             /* [S,S]   wildcard_mat      (:329-331)                     */
    const float *O;             /* [C,S]   output_mat        (:332-333)                     */
    const float *h0;            /* [S]     start_vector      (:322-323)                     */
    const float *hT;            /* [S]     final_vector      (:324-325)                     */
    const float *P;             /* [C,C] expanded priority matrix (priority.py:6-18) or NULL */
    int32_t nl;                 /* FARNN_NL_*                                                */
    int32_t semiring;           /* FARNN_SEMIRING_*                                          */
    float   threshold;          /* --threshold: clamp of the `oo` column (:166-167)          */
    int32_t o_idx;              /* s2i['o']: what the `oo` column decodes to (:169)          */
    int32_t use_crf;            /* 0: threshold+argmax; 1: Viterbi over C+2 tags */
    const float *crf_trans;     /* [(C+2),(C+2)] CRF.transitions (crf.py:39-46) or NULL=defaults */
    int32_t weights_on_device;  /* 1: T/W/O/h0/hT/P/crf_trans are device pointers            */
} farnn_onehot_ifst_desc;

int farnn_onehot_ifst_create(const farnn_onehot_ifst_desc *desc, int device, farnn_model **out);

/* ---- onehot models built on the device from the automaton's edge list -----------------
 * The reference's loaders (wfa/fsa_to_tensor.py:398-615) write dense float64 tensors on the host
 * ([V,S,S]: 21 GB at BASELINE configs[4]; [V,C,S,S]: 2.5 GB at ATIS size).  These entries take the edges
 * the loader would have written and scatter them straight into HBM.  Per edge e, with w = word[e],
 * f = from[e], t = to[e], l = label[e] (label column of the edge; destination-state label in the i-FST):
 *     i-FST   (:546-615)  w >= 0: T[w,f,t] = v     w == -1: W[f,t] = v        l >= 0: O[l,t] = 1
 *     FST 4-D (:398-474)  w >= 0: T4[w,l,f,t] = v  w == -1: W4[l,f,t] = v
 *     indep=1 (:477-543)  w >= 0: T[w,f,t] = v     w == -1: W[f,t] = v        l >= 0: Oten[l,f,t] = 1
 * w < -1 marks an entry that only carries its label (a class edge, '&' / '%', none of whose words is in
 * the vocabulary).  Assignment, not accumulation, like the reference (duplicates are idempotent); class
 * edges are expanded to one entry per word by the caller.  The edge arrays are host pointers (they are
 * small).  The dense tensor fields of `base` are ignored; `base.weights_on_device` covers h0/hT/P/crf_trans. */
typedef struct farnn_edge_list {
    int64_t n_edges;
    const int32_t *word;           /* [n_edges] word id, -1 wildcard edge, < -1 label only         */
    const int32_t *from, *to;      /* [n_edges] state indices                                      */
    const int32_t *label;          /* [n_edges] label column, or -1 (NULL: no labels)              */
    const float *val;              /* [n_edges] edge weight, or NULL (= 1)                         */
} farnn_edge_list;

int farnn_onehot_ifst_create_from_edges(const farnn_onehot_ifst_desc *base, const farnn_edge_list *edges,
                                        int device, farnn_model **out);

/* ---- compact form of the onehot i-FST ----------------------------------------------------------
 * With --rand_constant 0 (all main.py allows for --method onehot, :175-176) every entry of T and W is 0 or 1 and a
 * word's S x S block holds a handful of edges; the loader still writes dense float64 tensors
 * (wfa/fsa_to_tensor.py:546-615).  The compact form keeps a block as S rows of S bits (forward: sources of every
 * destination; backward: destinations of every source) and the recurrence walks only the non-zero entries of the
 * current state: 2*S*ceil(S/64)*8 bytes per token instead of 2*S*S*4, same results (bit-identical for `none` / `relu`,
 * within rounding order for tanh).  Sum semiring, S <= 512, L <= 1024.  Contract numbers stay fp32-dense; bench.py
 * reports this path separately (`compact`).
 *   farnn_onehot_ifst_create / _create_from_edges build the bitmaps beside the dense blocks whenever the weights are
 *   0/1 (farnn_has_compact); farnn_set_compact(m, 1) makes farnn_tag use them, (m, 0) goes back to the dense blocks.
 *   farnn_onehot_ifst_create_compact builds ONLY the bitmaps, straight from the edge list (no dense tensor on the host
 *   or in HBM: BASELINE's largest config is 0.66 GB instead of 2 x 21 GB); edge weights must be 1 (or val == NULL). */
int farnn_has_compact(const farnn_model *m);
int farnn_set_compact(farnn_model *m, int32_t enable);
int farnn_onehot_ifst_create_compact(const farnn_onehot_ifst_desc *base, const farnn_edge_list *edges, int device,
                                     farnn_model **out);

/* ---- onehot FST 4-D: FARNN_S_O (reference model_onehot.py:8-129), --independent 0 ---- */
typedef struct farnn_onehot_fst4_desc {
    int32_t V, S, C;
    const float *T4;            /* [V,C,S,S] language_tensor (:34)  */
    const float *W4;            /* [C,S,S]   wildcard_tensor (:35)  */
    const float *h0, *hT;       /* [S]                              */
    const float *P;             /* [C,C] or NULL                    */
    int32_t semiring;           /* relu is unconditional (:93-94)   */
    float   threshold;
    int32_t o_idx;
    int32_t weights_on_device;
} farnn_onehot_fst4_desc;

int farnn_onehot_fst4_create(const farnn_onehot_fst4_desc *desc, int device, farnn_model **out);

/* ---- onehot independent=1: FARNN_S_O_I (reference model_onehot.py:184-306) ---- */
typedef struct farnn_onehot_ind1_desc {
    int32_t V, S, C;
    const float *T;             /* [V,S,S]                           */
    const float *W;             /* [S,S]                             */
    const float *Oten;          /* [C,S,S] output_tensor (:212-213)  */
    const float *h0, *hT;
    const float *P;
    int32_t semiring;
    int32_t mask_by_output;     /* the `args.independent == 2` branch (:259-262) */
    float   threshold;
    int32_t o_idx;
    int32_t weights_on_device;
} farnn_onehot_ind1_desc;

int farnn_onehot_ind1_create(const farnn_onehot_ind1_desc *desc, int device, farnn_model **out);

/* the same two models from the edge list (see farnn_edge_list above) */
int farnn_onehot_fst4_create_from_edges(const farnn_onehot_fst4_desc *base, const farnn_edge_list *edges,
                                        int device, farnn_model **out);
int farnn_onehot_ind1_create_from_edges(const farnn_onehot_ind1_desc *base, const farnn_edge_list *edges,
                                        int device, farnn_model **out);

/* ---- decomposed i-FST: FARNN_S_D_W_I_S (reference model_decompose_single.py:12-304) ---- */
typedef struct farnn_decomp_ifst_desc {
    int32_t V, S, R, K;         /* S incl. additional_states; K = score columns (C, or C+2 with CRF) */
    const float *Vgen;          /* [V,R] generalized word table: V_embed*beta + nl_add(E@G)*(1-beta),
                                   model_decompose.py:222-241, precomputed once (weights frozen)   */
    const float *S1, *S2;       /* [S,R]  (model_decompose_single.py:70-71)                        */
    const float *W;             /* [S,S]  wildcard_mat (:84-86)                                     */
    const float *Cout;          /* [K,S]  C_output_mat (:81-82)                                     */
    const float *h0, *hT;       /* [S]                                                              */
    const float *P;             /* [K,K] or NULL                                                    */
    int32_t farnn;              /* 0 plain, 1 update gate, 2 update+reset gates (:143-154)          */
    const float *Wss1, *Wrs1, *bs1;   /* [S,S], [R,S], [S]   (farnn >= 1)                           */
    const float *Wss2, *Wrs2, *bs2;   /* [S,S], [R,S], [S]   (farnn == 2)                           */
    float   sigmoid_exponent;   /* gate_activation scale (model_decompose.py:97-102)                */
    int32_t nl;
    int32_t semiring;
    float   threshold;
    int32_t o_idx;
    int32_t use_crf;
    const float *crf_trans;     /* [K,K] when use_crf                                               */
    int32_t weights_on_device;
} farnn_decomp_ifst_desc;

int farnn_decomp_ifst_create(const farnn_decomp_ifst_desc *desc, int device, farnn_model **out);

/* The same model with the word table -- and --normalize_automata -- computed ON THE DEVICE.  The
 * reference recomputes get_generalized_v_embed_vec twice per time step (model_decompose_single.py:140-141):
 *     Vgen[w] = V_embed[w] * beta + nl_add(E[w] @ G) * (1 - beta)                 (model_decompose.py:222-241)
 * and its loader scales V_embed, S1, S2 by the averaged column norms on the host (init_params.py:285-297):
 *     factor = cbrt(avg(V) avg(S1) avg(S2)),  M <- M * factor / avg(M),  avg(M)[c] = ||M[:, c]|| / rows  (utils.py:202-225).
 * Here desc->Vgen is ignored: V_embed / E / G / beta go to the device once, the scaling (all four modes) and the fold
 * run there, and nothing of size V x R comes back to the host.  G = pinv(E) @ V_embed (model_decompose_single.py:73-76)
 * is given for the UN-normalised V_embed; its columns take V_embed's scale (the bridge is linear in them). */
#define FARNN_NORM_NONE     0
#define FARNN_NORM_L1       1      /* --normalize_automata l1: numpy's matrix 1-norm (largest column sum) / size          */
#define FARNN_NORM_L2       2      /* --normalize_automata l2: the spectral norm / size (Gram matrix on the device, its    */
                                   /*   largest eigenvalue by a Jacobi sweep over R x R doubles on the host)               */
#define FARNN_NORM_L1_RANK  3      /* --normalize_automata l1-rank */
#define FARNN_NORM_L2_RANK  4      /* --normalize_automata l2-rank (main.py:55 default) */
typedef struct farnn_vgen_fold {
    const float *V_embed;       /* [V,R]  (pad row included)                                                  */
    const float *E;             /* [V,D]  embedding.weight                                                    */
    const float *G;             /* [D,R]  embed_r_generalized                                                 */
    const float *beta;          /* [R]    beta_vec                                                            */
    int32_t D;
    int32_t add_nl;             /* FARNN_NL_*: --additional_nonlinear                                         */
    int32_t normalize;          /* FARNN_NORM_*: applied to V_embed (and G), desc->S1, desc->S2 before the fold */
    int32_t on_device;          /* 1: V_embed / E / G / beta are device pointers                              */
} farnn_vgen_fold;
int farnn_decomp_ifst_create_folded(const farnn_decomp_ifst_desc *desc, const farnn_vgen_fold *fold, int device,
                                    farnn_model **out);

/* ---- decomposed independent=1: FARNN_S_D_W_I (reference model_decompose_independent.py:11-300) ---- */
typedef struct farnn_decomp_ind1_desc {
    int32_t V, S, R, RO, K;     /* S incl. additional_states; RO = rank of the output factors        */
    const float *Vgen;          /* [V,R]  generalized word table (model_decompose.py:222-241)        */
    const float *S1, *S2;       /* [S,R]                                                              */
    const float *W;             /* [S,S]  wildcard_mat                                                */
    const float *Cout;          /* [K,RO] C_output (:82-83)                                           */
    const float *S1o, *S2o;     /* [S,RO] S1_output / S2_output (:85-89)                              */
    const float *Wo;            /* [S,S]  wildcard_output, added to the output sum unless CE1; NULL   */
    const float *h0, *hT;       /* [S]                                                                */
    const float *P;             /* [K,K] or NULL                                                      */
    int32_t farnn;
    const float *Wss1, *Wrs1, *bs1;
    const float *Wss2, *Wrs2, *bs2;
    float   sigmoid_exponent;
    int32_t nl;
    int32_t semiring;
    float   threshold;
    int32_t o_idx;
    int32_t use_crf;
    const float *crf_trans;     /* [K,K] when use_crf                                                 */
    int32_t weights_on_device;
} farnn_decomp_ind1_desc;

int farnn_decomp_ind1_create(const farnn_decomp_ind1_desc *desc, int device, farnn_model **out);

/* ---- decomposed independent=0: FARNN_S_D_W (reference model_decompose.py:10-459) ------------------ */
typedef struct farnn_decomp_fst_desc {
    int32_t V, S, R, RW, K;     /* S incl. additional_states; RW = rank of the wildcard factors       */
    const float *Vgen;          /* [V,R]  generalized word table (model_decompose.py:222-241)        */
    const float *C;             /* [K,R]  C_embed (:125); the recurrence sees Vgen * sum_c C (:253)   */
    const float *S1, *S2;       /* [S,R]                                                              */
    const float *Cw;            /* [K,RW] C_wildcard (:122-123)                                       */
    const float *S1w, *S2w;     /* [S,RW] S1_wildcard / S2_wildcard (:127-131)                        */
    const float *WW;            /* [S,S]  wildcard_wildcard (:133-135)                                */
    const float *h0, *hT;       /* [S]                                                                */
    const float *P;             /* [K,K] or NULL                                                      */
    int32_t farnn;
    const float *Wss1, *Wrs1, *bs1;
    const float *Wss2, *Wrs2, *bs2;
    float   sigmoid_exponent;
    int32_t nl;
    int32_t semiring;
    float   threshold;
    int32_t o_idx;
    int32_t use_crf;
    const float *crf_trans;     /* [K,K] when use_crf                                                 */
    int32_t weights_on_device;
} farnn_decomp_fst_desc;

int farnn_decomp_fst_create(const farnn_decomp_fst_desc *desc, int device, farnn_model **out);

/* ---- the hot path ------------------------------------------------------------------- */
/*
 * farnn_tag: model.forward_local / forward_RE / forward_score of the reference
 *            (model_onehot.py:131-160, model_decompose_single.py:207-304), minus the loss.
 *
 *   x        int64 [B,L]   token ids, pad id at positions >= lengths[b]        (device)
 *   lengths  int64 [B]     1..L                                                (device)
 *   mode     FARNN_MODE_LOCAL: only positions < lengths[b] are tagged; FARNN_MODE_FULL: all L
 *            positions run through the recurrence exactly like the reference's padded loop.
 *   tags     int32 [B,L] or NULL. LOCAL: positions >= lengths[b] are set to -1.       (device)
 *   flat_tags int64 [sum(lengths)] or NULL: the reference's flattened prediction order
 *            (utils.py:153-164): for b in batch, positions 0..lengths[b]-1.            (device)
 *   scores   float32 [B,L,K] or NULL: per-token label scores BEFORE the threshold clamp
 *            (K = farnn_num_columns()).  LOCAL: rows at pad positions are zero-filled. (device)
 *   stream   hipStream_t (as void*), NULL = the default stream.  Work is enqueued, not awaited.
 */
int farnn_tag(farnn_model *m, const int64_t *x, const int64_t *lengths, int32_t B, int32_t L,
              int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream);

/* Pre-size the handle's device workspace so that farnn_tag() for up to (B,L) allocates nothing
 * (required before capturing farnn_tag() into a hipGraph).  On a vector-input handle (below) this also sizes the token
 * table [B L][Rp + SP per gate] and the identity id array: a later farnn_tag_vectors() within (B,L) allocates nothing. */
int farnn_reserve(farnn_model *m, int32_t B, int32_t L);

/* ---- vector input: FARNN_S_SF (reference model_decompose_single.py:307-579) -------------------------------------------
 * The decomposed i-FST recurrence on a dense input, one rule-space vector per token, in place of word ids and a per-word
 * table: whatever produces contextual token vectors (the reference: EmbedAggregator behind an encoder) reaches the
 * automaton through it.
 *
 * farnn_decomp_sf_create takes farnn_decomp_ifst_desc with V = 0 and Vgen = NULL (anything else: FARNN_EINVAL); nothing
 * per word is ever built.  Sum semiring only: the max semiring needs an S x S block per token and is refused with
 * FARNN_EINVAL.  The CRF, the priority layer P and the gates (farnn 0 / 1 / 2) are the id handle's.
 *
 * farnn_tag_vectors:
 *   v        float32 [B,L,R] dense (device); rows at positions >= lengths[b] are never read (they may hold anything).
 *   lengths, tags, flat_tags, scores, stream: as in farnn_tag.
 *   mode     FARNN_MODE_LOCAL only (forward_score / forward_RE exist on the onehot models): anything else FARNN_EINVAL.
 * Every call first builds a token table -- per valid position [v padded to Rp | v . Wrs1 + bs1 | v . Wrs2 + bs2], the gate
 * halves summed in exactly the order the id handle's create-time table uses -- and then runs the id path's recurrence,
 * score and decode kernels unchanged on the ids b L + t.  A vector that is bit for bit a row of Vgen is therefore tagged
 * bit for bit like that word on an id handle of the same weights.
 * Shapes the packed-rows kernels do not hold fall back to decomp_chain_kernel on an id handle; that kernel is NOT served
 * from the token table: such a shape is refused with FARNN_ERANGE before anything is launched -- at create when
 * Rp + SP per gate > 2048, at the call when no packed-rows form fits the call's L.
 * farnn_tag on a vector-input handle, and farnn_tag_vectors on any other handle, are refused with FARNN_EINVAL (so is
 * farnn_tag_host_submit, which calls farnn_tag).
 * These two entry points were ADDED to ABI version 2: no existing signature or struct changed, so the number stands. */
int farnn_decomp_sf_create(const farnn_decomp_ifst_desc *desc, int device, farnn_model **out);
/* ---- ... in the max semiring (reference model_decompose_single.py:435-442: Tr[b] = S1 diag(v_b) S2^T + W,
 * h' = max_j hbar[j] Tr[j, s]) ------------------------------------------------------------------------------------------
 * farnn_decomp_sf_max_create takes the same descriptor with semiring == FARNN_SEMIRING_MAX, V = 0 and Vgen = NULL (anything
 * else: FARNN_EINVAL; farnn_decomp_sf_create goes on refusing the max semiring).  Tagging only: a training context with vector
 * input and the max semiring is still refused.  farnn_tag_vectors serves the handle, FARNN_MODE_LOCAL only, by one of two routes
 * chosen per call before anything is launched:
 *   dense    farnn == 0 and a model the dense chain kernels hold (what an id handle of the max semiring requires for its per-word
 *            blocks), up to 16 GiB of blocks a call: token_blocks_kernel writes one [SR][SP] block per valid token and its
 *            transpose into the handle's grow-only workspace (farnn_reserve sizes it), each entry summed exactly like the id
 *            handle's create-time block of a word; the chain, score and decode kernels of that id handle follow on the ids b L + t.
 *   generic  farnn 1 / 2, or anything the dense route does not take: token_table_kernel writes the padded copy [B L][Rp] and
 *            decomp_chain_kernel materialises Tr per step from it, as on an id handle.
 * On either route a vector that is bit for bit a row of Vgen is tagged bit for bit like that word on a max-semiring
 * farnn_decomp_ifst_create handle of the same weights.  A shape neither route holds: FARNN_ERANGE, nothing launched.
 * farnn_kernel_name(m, 3) names the kernel in front of the last call's recurrence: token_blocks_kernel or token_table_kernel.
 * ADDED to ABI version 2: no existing signature or struct changed, so the number stands. */
int farnn_decomp_sf_max_create(const farnn_decomp_ifst_desc *desc, int device, farnn_model **out);
int farnn_tag_vectors(farnn_model *m, const float *v, const int64_t *lengths, int32_t B, int32_t L,
                      int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream);

void farnn_destroy(farnn_model *m);

/* ---- the same call with HOST buffers: what the reference's eval loop hands over (val.py:17-31) -----------------------
 * model.forward_local(x, label, lengths, train=False) is called with CPU tensors and its flat predictions are read on
 * the CPU.  farnn_tag_host_submit stages [x | lengths] through a pinned buffer the handle owns, enqueues ONE H2D copy,
 * farnn_tag(FARNN_MODE_LOCAL) and the D2H copy of the flat predictions on a stream of the handle, and returns a ticket at
 * once; farnn_tag_host_wait blocks until that batch is done and copies its predictions out.  Up to FARNN_HOST_SLOTS
 * batches may be in flight (the host prepares batch i+1 while batch i runs); tickets are waited for in submission order.
 * x_host / len_host may be reused as soon as submit returns.  PCIe-inclusive path: bench.py reports it as
 * `host_inclusive`, never as the headline value.
 *   x_host    int64 [B,L]   (host)          len_host  int64 [B]  (host)
 *   ticket    out: names THIS submit (slot | generation << 8) for farnn_tag_host_wait; a ticket that was already waited for, or
 *             whose slot has since been reclaimed for a later submit, is refused with FARNN_EINVAL and consumes nothing;
 *             n_flat out (or NULL): sum(clamp(len, 0, L))
 *   flat_out  int64 [n_flat] (host)         n_out (or NULL): how many were written
 * farnn_flatten_host: utils.flatten (utils.py:153-164) of a host int64 [B,L] array (the flat gold labels the same
 * call returns beside the predictions); returns the element count, -1 on a null argument. */
#define FARNN_HOST_SLOTS 4
int farnn_tag_host_submit(farnn_model *m, const int64_t *x_host, const int64_t *len_host, int32_t B, int32_t L,
                          int32_t *ticket, int64_t *n_flat);
int farnn_tag_host_wait(farnn_model *m, int32_t ticket, int64_t *flat_out, int64_t *n_out);
int64_t farnn_flatten_host(const int64_t *a, const int64_t *len_host, int32_t B, int32_t L, int64_t *out);

/* ---- training step of the decomposed i-FST -----------------------------------
 * Replaces FARNN_S_D_W_I_S.forward_local(train=True) + loss.backward()
 * (model_decompose_single.py:207-304, train_decompose.py:186-190) for farnn = 0/1/2, the sum or the max semiring
 * (farnn_train_set_semiring) and the CE1 loss: cross-entropy (mean over the valid tokens) of the scores, or with use_crf the CRF negative
 * log-likelihood, and the gradient with respect to every tensor the recurrence and the scoring read.  The generalized word table Vgen
 * (model_decompose.py:222-241) is an input; the caller differentiates it from dVgen.
 * All pointers are DEVICE pointers; matrices are row-major and unpadded. */
typedef struct farnn_train_ctx farnn_train_ctx;

typedef struct {
    int32_t V, S, R, K;         /* vocabulary rows of Vgen, states (incl. additional states), rank, score columns */
    int32_t nl;                 /* FARNN_NL_* (update_nonlinear)                                               */
    float   threshold;          /* decode clamp of column K-1 (model_decompose.py:365)                         */
    int32_t o_idx;              /* label written for column K-1 (:367) / K-3 with the CRF (:356)                 */
    int32_t farnn;              /* 0 plain recurrence, 1 update gate, 2 update + reset gate (:143-154,:193-198) */
    float   sigmoid_exponent;   /* k of the gate activation sigmoid(k x) (model_decompose.py:97-103)              */
    int32_t use_crf;            /* 1: loss = CRF.neg_log_likelihood_loss (baselines/crf.py:250-260, a sum over the
                                   batch) on the scores, K = labels + 2 (START, STOP); decode = Viterbi (:351-356) */
} farnn_train_dims;

typedef struct {
    const float *Vgen;          /* [V][R]   */
    const float *S1, *S2;       /* [S][R]   */
    const float *W;             /* [S][S] wildcard_mat   */
    const float *C;             /* [K][S] C_output_mat   */
    const float *h0, *hT;       /* [S]      */
    const float *P;             /* [K][K] priority matrix or NULL (args.use_priority = 0) */
    const float *crf_trans;     /* [K][K] crf.transitions (use_crf = 1), else NULL        */
    const float *Wss1, *Wrs1, *bs1;   /* [S][S], [R][S], [S] update gate (farnn >= 1), else NULL */
    const float *Wss2, *Wrs2, *bs2;   /* reset gate (farnn = 2), else NULL                       */
} farnn_train_weights;

typedef struct {
    float *loss;                /* [1]                                                  */
    float *dVgen;               /* [V][R]  (rows of words that do not occur stay zero)  */
    float *dS1, *dS2;           /* [S][R]  */
    float *dW;                  /* [S][S]  */
    float *dC;                  /* [K][S]  */
    float *dh0, *dhT;           /* [S]     */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions */
    float *dtrans;              /* [K][K] gradient of crf.transitions (use_crf = 1), else NULL     */
    float *dWss1, *dWrs1, *dbs1;      /* gate gradients (farnn >= 1), else NULL */
    float *dWss2, *dWrs2, *dbs2;      /* (farnn = 2), else NULL                 */
} farnn_train_outputs;

int  farnn_train_create(const farnn_train_dims *dims, int device, farnn_train_ctx **out);
void farnn_train_destroy(farnn_train_ctx *ctx);
/* One step on the given stream: zeroes the outputs, runs both chains with the state stash, the loss, the
 * back-propagation through time and the parameter-gradient reductions.  x, lengths, labels: int64
 * [B][L], [B], [B][L] (labels outside 0..K-1 are treated as 0; they only matter at valid positions).
 * Every FARNN_ERANGE (the CRF limit, more than 512 states or rank, the 2^30 element bound, a launch above 160 KiB of LDS) is
 * returned before anything is enqueued: a refused step leaves the output buffers untouched. */
int  farnn_decomp_ifst_train_step(farnn_train_ctx *ctx, const farnn_train_weights *w, const int64_t *x,
                                  const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                  int64_t valid_tokens, const farnn_train_outputs *out, void *stream);
/* The same step with regular expressions as a teacher (--marryup_type kd | pr; model_decompose_single.py:291-300,
 * baselines/KD.py:3-18), sum semiring, farnn = 0/1/2, with or without the CRF and the priority layer:
 *   loss = pi * original + (1 - pi) * KL,   the original loss being the cross-entropy or the CRF sum of the plain step,
 *   KD: KL = KLDivLoss()(log_softmax(scores / c1), softmax(re / c1)) c1^2                                  (KD.py:3-7)
 *   PR: KL = KLDivLoss()(log_softmax(scores), softmax(softmax(scores) * exp(re - 1) * c1)), the teacher NOT detached:
 *       the gradient flows through it as well                                                               (KD.py:10-18)
 * KLDivLoss() is torch's default 'mean': the sum over all B L K elements over B L K, pad positions INCLUDED.  The scores of a
 * pad position i >= len are C (f_{i+1} * b_{i+1}) of both chains continued through the raw tokens x[b][len..] (reverse() flips
 * only the first len tokens, reverse(.., lengths + 1) only the first len + 1 rows of the backward stash; :222,:261), so both
 * chains of every sequence, a sequence of length 0 included, and their back-propagation run L steps, x is read at every
 * position (a word outside 0..V-1 is clamped) and the pad word's row of dVgen is not zero.  The cross-entropy / CRF term, the
 * decode and the tags stay on the valid positions (tags are -1 at the pads).
 * re_scores: float [B][L][K], the RE tagger's scores with the zero columns already appended (one without the CRF, three with
 * it; :213-218) and cut to L.  pi is the weight of the original loss: c2_kdpr for KD, max(c2_kdpr, c3_pr ** t) for PR (:299),
 * computed by the caller -- the library has no t.  The KL partials are added in a fixed order (no float atomic).
 * FARNN_EINVAL: a null re_scores / teacher, a mode other than the two, c1 < 1 (main.py asserts c1_kdpr >= 1), pi outside
 * [0, 1], a context set to FARNN_SEMIRING_MAX (its kernels walk the valid positions only).  Like every FARNN_ERANGE of the
 * plain step, these are returned before anything is enqueued and leave the output buffers untouched.  A plain step before or
 * after it on the same context is not affected: the teacher leaves no state behind. */
#define FARNN_TEACHER_KD 1
#define FARNN_TEACHER_PR 2
typedef struct {
    int32_t mode;               /* FARNN_TEACHER_KD or FARNN_TEACHER_PR                                          */
    float   c1;                 /* KD: the temperature T; PR: the strength of the rule constraint (c1_kdpr)        */
    float   pi;                 /* weight of the original loss; 1 - pi weighs the KL term                          */
} farnn_teacher;
int  farnn_decomp_ifst_teacher_train_step(farnn_train_ctx *ctx, const farnn_train_weights *w, const int64_t *x,
                                          const int64_t *lengths, const int64_t *labels, const float *re_scores,
                                          const farnn_teacher *teacher, int32_t B, int32_t L, int64_t valid_tokens,
                                          const farnn_train_outputs *out, void *stream);
/* The teacher step on a context set to FARNN_SEMIRING_MAX (--train_mode max --marryup_type kd | pr; main.py:163,
 * model_decompose_single.py:159-166 for the recurrences, :291-300 for the loss).  Same arguments, same loss and same refusals as
 * above, with one exchanged: FARNN_EINVAL on a context in the SUM semiring (the entry above is the one for it).  Only the two
 * recurrences are max-times (utils._maxmul: ONE source state per target state, the first maximal one); the scores, the KL term
 * and the original loss are sum-times, as the reference sends nothing else through semiring_func.  Both max-times chains of
 * every sequence run L steps through the raw pad tokens, every one of the B L positions is bucketed by word, and a word that
 * occurs at pad positions only gets a block Tr_w and a non-zero row of dVgen (a zero one with pi = 1).  S <= 192 as
 * farnn_train_set_semiring demands. */
int  farnn_decomp_ifst_teacher_max_train_step(farnn_train_ctx *ctx, const farnn_train_weights *w, const int64_t *x,
                                              const int64_t *lengths, const int64_t *labels, const float *re_scores,
                                              const farnn_teacher *teacher, int32_t B, int32_t L, int64_t valid_tokens,
                                              const farnn_train_outputs *out, void *stream);
/* ---- the same step on a dense input: FARNN_S_SF (reference model_decompose_single.py:483-580 with train=True)
 * One rule-space vector per token, v [B][L][R], in place of word ids and the table Vgen, and d loss / d v beside the weight
 * gradients: what an encoder in front of the automaton is trained through.  Scope: the sum semiring, farnn = 0/1/2, every
 * update_nonlinear, the CE1 loss or (use_crf) the CRF negative log-likelihood, the priority layer P; no KD / PR teacher.  The size
 * limits are the id step's (S, R <= 512, B (L+1) max(S, R) < 2^30, the CRF's LDS limit, 160 KiB of LDS per launch).
 *
 * farnn_decomp_sf_train_create: farnn_train_create for such a context; dims->V must be 0 (anything else: FARNN_EINVAL, as
 * farnn_train_create refuses V = 0).  Nothing per word is allocated; the workspaces follow the per-call B L.  The context is
 * destroyed, profiled and timed by farnn_train_destroy / farnn_train_set_profiling / farnn_train_time.
 *
 * farnn_decomp_sf_train_step:
 *   w        the id step's weights with Vgen = NULL;  out: the id step's outputs with dVgen = NULL
 *   v        float32 [B][L][R] dense (device).  A row at a position t >= lengths[b] reaches no arithmetic that reaches an output:
 *            it may hold anything, NaN and Inf included.
 *   dv       float32 [B][L][R] (device), written whole by the step: d loss / d v at the valid positions, exact zeros at the pads.
 *            No float atomic and a fixed summation order: two calls on the same inputs give the same bits.
 *   The loss, the tags and the weight gradients are the id step's on a table whose rows are these vectors and the ids b L + t.
 * FARNN_EINVAL, before anything is enqueued and with the output buffers untouched: a NULL v or dv, a non-NULL w->Vgen or
 * out->dVgen, a context made by farnn_train_create.  On a vector-input context farnn_decomp_ifst_train_step, both teacher entries
 * (their KL term reads the scores at the pad positions, that is the pad vectors) and
 * farnn_train_set_semiring(FARNN_SEMIRING_MAX) (an S x S block per token) return FARNN_EINVAL.
 * These two entry points were ADDED to ABI version 2: no existing signature or struct changed, so the number stands. */
int  farnn_decomp_sf_train_create(const farnn_train_dims *dims, int device, farnn_train_ctx **out);
int  farnn_decomp_sf_train_step(farnn_train_ctx *ctx, const farnn_train_weights *w, const float *v, const int64_t *lengths,
                                const int64_t *labels, int32_t B, int32_t L, int64_t valid_tokens,
                                const farnn_train_outputs *out, float *dv, void *stream);
/* accumulated HIP-event time of the step's launches since the last call (ms) and the number of steps timed;
 * profiling is enabled with farnn_train_set_profiling(ctx, 1) */
int  farnn_train_set_profiling(farnn_train_ctx *ctx, int32_t enable);
int  farnn_train_time(farnn_train_ctx *ctx, double *total_ms, int64_t *steps);
/* The semiring of the recurrence (the reference's --train_mode, model_decompose_single.py:159-166): FARNN_SEMIRING_SUM
 * (the default) or FARNN_SEMIRING_MAX, where a step is n[s] = max_j in[j] Tr_w[j,s] with Tr_w = S1 diag(Vgen[w]) S2^T + W
 * (torch.max: the first maximal j takes the whole adjoint).  Everything else of the step is the same in both.  Returns
 * FARNN_EINVAL for any other value and FARNN_ERANGE for FARNN_SEMIRING_MAX above 192 states.  The max step's workspace
 * (three S x S blocks per distinct word of the batch) is allocated by its first step. */
int  farnn_train_set_semiring(farnn_train_ctx *ctx, int32_t semiring);

/* ---- training step of the decomposed FST (FARNN_S_D_W, --method decompose --independent 0) ----------
 * Replaces FARNN_S_D_W.forward_local(train=True) + loss.backward() (model_decompose.py:243-456) for farnn = 0/1/2, every
 * update_nonlinear, the priority layer, and the CE1 loss or (use_crf) the CRF negative log-likelihood, in the sum semiring or
 * (farnn_decomp_fst_train_set_semiring) the max semiring.  With csum = C_embed.sum(0) and cwsum =
 * C_wildcard.sum(0) the two chains are the decomposed i-FST's recurrence on the word table Vgen * csum and the matrix
 * S1_wildcard diag(cwsum) S2_wildcard^T + wildcard_wildcard (:253, :327-332), and
 *   score[c] = sum_r Vgen[w,r] C_embed[c,r] (alpha S1)[r] (beta S2)[r] + sum_q C_wildcard[c,q] (alpha S1w)[q] (beta S2w)[q]  (:310-325)
 * with alpha the forward state before the token and beta the backward state behind it.  Vgen (model_decompose.py:222-241) is an
 * input; the caller differentiates it from dVgen.  All pointers are DEVICE pointers; matrices are row-major and unpadded.
 * No sum of the step depends on the order in which workgroups finish: two steps on the same inputs are bit-identical. */
typedef struct farnn_decomp_fst_train_ctx farnn_decomp_fst_train_ctx;

typedef struct {
    int32_t V, S, R, Q, K;      /* vocabulary rows, states, rank of the language factors, rank of the wildcard factors, score columns */
    int32_t nl;                 /* FARNN_NL_* (update_nonlinear)                                               */
    float   threshold;          /* decode clamp of column K-1 (:365) / K-3 with the CRF (:353)                 */
    int32_t o_idx;              /* label written for that column (:356, :367)                                  */
    int32_t farnn;              /* 0 plain recurrence, 1 update gate, 2 update + reset gate (:255-266,:301-306) */
    float   sigmoid_exponent;   /* k of the gate activation sigmoid(k x) (:97-103)                             */
    int32_t use_crf;            /* 1: the CRF loss on the scores, K = labels + 2 (START, STOP); decode = Viterbi */
} farnn_decomp_fst_train_dims;

typedef struct {
    const float *Vgen;          /* [V][R]   */
    const float *Ce;            /* [K][R] C_embed       */
    const float *S1, *S2;       /* [S][R]   */
    const float *Cw;            /* [K][Q] C_wildcard    */
    const float *S1w, *S2w;     /* [S][Q] S1_wildcard, S2_wildcard */
    const float *WW;            /* [S][S] wildcard_wildcard */
    const float *h0, *hT;       /* [S]      */
    const float *P;             /* [K][K] priority matrix or NULL */
    const float *crf_trans;     /* [K][K] crf.transitions (use_crf = 1), else NULL */
    const float *Wss1, *Wrs1, *bs1;   /* [S][S], [R][S], [S] update gate (farnn >= 1), else NULL */
    const float *Wss2, *Wrs2, *bs2;   /* reset gate (farnn = 2), else NULL                       */
} farnn_decomp_fst_train_weights;

typedef struct {
    float *loss;                /* [1]                                                  */
    float *dVgen;               /* [V][R]  (rows of words that do not occur are zero)   */
    float *dCe;                 /* [K][R]  */
    float *dS1, *dS2;           /* [S][R]  */
    float *dCw;                 /* [K][Q]  */
    float *dS1w, *dS2w;         /* [S][Q]  */
    float *dWW;                 /* [S][S]  */
    float *dh0, *dhT;           /* [S]     */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions */
    float *dtrans;              /* [K][K] gradient of crf.transitions (use_crf = 1), else NULL     */
    float *dWss1, *dWrs1, *dbs1;      /* gate gradients (farnn >= 1), else NULL */
    float *dWss2, *dWrs2, *dbs2;      /* (farnn = 2), else NULL                 */
} farnn_decomp_fst_train_outputs;

int  farnn_decomp_fst_train_create(const farnn_decomp_fst_train_dims *dims, int device, farnn_decomp_fst_train_ctx **out);
void farnn_decomp_fst_train_destroy(farnn_decomp_fst_train_ctx *ctx);
/* One step on the given stream; x, lengths, labels as farnn_decomp_ifst_train_step's.  Every FARNN_ERANGE (the CRF limit, more
 * than 512 states or either rank above 512, the 2^30 element bound with Q counted like R, a launch above 160 KiB of LDS -- the
 * score head keeps 16 positions' rows of 2 S + 3 R + 3 Q + 2 K floats there) is returned before anything is enqueued: a
 * refused step leaves the output buffers untouched. */
int  farnn_decomp_fst_train_step(farnn_decomp_fst_train_ctx *ctx, const farnn_decomp_fst_train_weights *w, const int64_t *x,
                                 const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                 int64_t valid_tokens, const farnn_decomp_fst_train_outputs *out, void *stream);
/* as farnn_train_set_profiling / farnn_train_time */
int  farnn_decomp_fst_train_set_profiling(farnn_decomp_fst_train_ctx *ctx, int32_t enable);
int  farnn_decomp_fst_train_time(farnn_decomp_fst_train_ctx *ctx, double *total_ms, int64_t *steps);
/* The semiring of the two recurrences (the reference's --train_mode, model_decompose.py:269-276): FARNN_SEMIRING_SUM (the
 * default) or FARNN_SEMIRING_MAX, where a step is n[s] = max_j hbar[j] Tr_w[j,s] (the backward chain: Tr_w[s,j]) with
 * Tr_w = S1 diag(Vgen[w] * csum) S2^T + W (utils._maxmul, utils.py:192-195: the first maximal j takes the whole adjoint).
 * The score head, the priority layer, the loss and the decode stay sum-times; two max steps on the same inputs are
 * bit-identical too.  Returns FARNN_EINVAL for any other value and FARNN_ERANGE for FARNN_SEMIRING_MAX above 192 states.  The
 * max step's workspace (three S x S blocks per distinct word of the batch) is allocated by its first step. */
int  farnn_decomp_fst_train_set_semiring(farnn_decomp_fst_train_ctx *ctx, int32_t semiring);

/* ---- training step of the onehot i-FST (FARNN_S_O_I_S, --method onehot --independent 2) -----------------
 * Replaces FARNN_S_O_I_S.forward_local(train=True) + loss.backward() (model_onehot.py:131-146,351-428,
 * train_onehot.py:156-206) for the sum or the max semiring (farnn_onehot_train_set_semiring) and the CE1 loss: cross-entropy (mean over the valid tokens) of
 * the scores output_mat (alpha * beta) [. P], and its gradient with respect to language_tensor, the only tensor the
 * reference trains (model_onehot.py:326-337).  M_w = T[w] + W; the state mask is output_mat.sum(0).
 * Limits: S <= 128 (farnn_onehot_train_create returns FARNN_ERANGE above), B L < 2^30 (the step returns FARNN_ERANGE
 * before enqueuing anything).  All pointers are DEVICE pointers; matrices are row-major and unpadded. */
typedef struct farnn_onehot_train_ctx farnn_onehot_train_ctx;

typedef struct {
    int32_t V, S, C;            /* vocabulary rows of T, states, score columns (labels + 1)          */
    int32_t nl;                 /* FARNN_NL_NONE .. FARNN_NL_RELUTANH (update_nonlinear, :379-386)  */
    float   threshold;          /* decode clamp of column C-1 (model_onehot.py:171-176)              */
    int32_t o_idx;              /* label written for column C-1 (:175)                               */
} farnn_onehot_train_dims;

typedef struct {
    const float *T;             /* [V][S][S] language_tensor */
    const float *W;             /* [S][S]    wildcard_mat    */
    const float *O;             /* [C][S]    output_mat      */
    const float *h0, *hT;       /* [S]                       */
    const float *P;             /* [C][C] priority matrix or NULL (args.use_priority = 0) */
} farnn_onehot_train_weights;

typedef struct {
    float *loss;                /* [1]                                                                 */
    float *dT;                  /* [V][S][S] (rows of words absent from the batch are written as zero) */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions     */
} farnn_onehot_train_outputs;

int  farnn_onehot_train_create(const farnn_onehot_train_dims *dims, int device, farnn_onehot_train_ctx **out);
void farnn_onehot_train_destroy(farnn_onehot_train_ctx *ctx);
/* One step on the given stream: writes all outputs (no float atomics: bit-identical across runs).  x, lengths,
 * labels: int64 [B][L], [B], [B][L]; labels outside 0..C-1 or words outside 0..V-1 at valid positions are counted
 * as 0 / clamped, and the next call returns FARNN_EINVAL.  valid_tokens = the sum of the lengths clamped to 0..L. */
int  farnn_onehot_ifst_train_step(farnn_onehot_train_ctx *ctx, const farnn_onehot_train_weights *w, const int64_t *x,
                                  const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                  int64_t valid_tokens, const farnn_onehot_train_outputs *out, void *stream);
/* as farnn_train_set_profiling / farnn_train_time */
int  farnn_onehot_train_set_profiling(farnn_onehot_train_ctx *ctx, int32_t enable);
int  farnn_onehot_train_time(farnn_onehot_train_ctx *ctx, double *total_ms, int64_t *steps);
/* The semiring of both chains (the reference's --train_mode: semiring_func = _maxmul, model_onehot.py:57, used at :377 and
 * :394; utils.py:192-195): FARNN_SEMIRING_SUM (the default) or FARNN_SEMIRING_MAX, where a step is
 * y[s] = max_j f[j] M_w[j,s] (forward chain) and q[s] = max_j (b o)[j] M_w[s,j] (backward chain), torch.max's first maximal j
 * taking the whole adjoint.  Scores, loss, decode and every limit are the same in both; the step stays free of float
 * atomics.  Returns FARNN_EINVAL for any other value.  The max step's extra workspace (an index byte and the winning matrix
 * entry per step and state) is allocated by its first step; a context switched back to FARNN_SEMIRING_SUM computes exactly
 * what one that never left it does.  The Python mirror keeps this semiring opt-in for its first release: FARNN_S_O_I_S
 * trains with --train_mode max only when RE2NN_ONEHOT_MAX_TRAIN=1 is set. */
int  farnn_onehot_train_set_semiring(farnn_onehot_train_ctx *ctx, int32_t semiring);

/* ---- training step of the onehot FST (FARNN_S_O, --method onehot --independent 0) ------------------------
 * Replaces FARNN_S_O.forward_local(train=True) + loss.backward() (model_onehot.py:66-146, train_onehot.py:156-206) for
 * the sum semiring and the CE1 loss.  A[w,c] = T4[w,c] + W4[c] (:87), M[w] = sum_c T4[w,c] + sum_c W4[c] (:82); both chains
 * use relu, whatever update_nonlinear says (:94, :101), and have no output mask; score_i[c] = sum_{s,j} relu(A[x_i,c,s,j]
 * alpha_i[s] beta_{i+1}[j]) [. P] with alpha_i the state BEFORE token i (:115-127); the loss is the cross-entropy, mean over
 * the valid tokens (:60, :142); the tags are local_decode's (:172-176).  language_tensor is always trained (:34),
 * wildcard_tensor with --train_wildcard (:35): its gradient is the sum of language_tensor's over the words, as both enter
 * only through A and M.  wildcard_wildcard_mat is not read under CE1 (:81-82).
 * Limits: S <= 128 (the chains' kernels, as farnn_onehot_train_create), C <= 2400 (the loss kernel of this step keeps two
 * score vectors per wavefront, 8 x 2 x C floats, within 150 KiB of LDS), V C <= 2^47 so that every byte offset into
 * [V][C][S][S] fits 63 bits (farnn_fst4_train_create returns FARNN_ERANGE outside), B (L + 1) < 2^30 (the step returns
 * FARNN_ERANGE before enqueuing anything and leaves the outputs untouched).  All pointers are DEVICE pointers; tensors are
 * row-major and unpadded. */
typedef struct farnn_fst4_train_ctx farnn_fst4_train_ctx;

typedef struct {
    int32_t V, S, C;            /* vocabulary rows of T4, states, score columns (labels + 1)        */
    float   threshold;          /* decode clamp of column C-1 (model_onehot.py:172-176)             */
    int32_t o_idx;              /* label written for column C-1 (:176)                              */
} farnn_fst4_train_dims;

typedef struct {
    const float *T4;            /* [V][C][S][S] language_tensor */
    const float *W4;            /* [C][S][S]    wildcard_tensor */
    const float *h0, *hT;       /* [S]                          */
    const float *P;             /* [C][C] priority matrix or NULL (args.use_priority = 0) */
} farnn_fst4_train_weights;

typedef struct {
    float *loss;                /* [1]                                                                    */
    float *dT4;                 /* [V][C][S][S] (rows of words absent from the batch are written as zero) */
    float *dW4;                 /* [C][S][S] or NULL (train_wildcard = 0)                                 */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions        */
} farnn_fst4_train_outputs;

int  farnn_fst4_train_create(const farnn_fst4_train_dims *dims, int device, farnn_fst4_train_ctx **out);
void farnn_fst4_train_destroy(farnn_fst4_train_ctx *ctx);
/* One step on the given stream: writes all outputs (no float atomics: bit-identical across runs).  x, lengths, labels,
 * valid_tokens and the handling of bad labels / words: as farnn_onehot_ifst_train_step. */
int  farnn_fst4_train_step(farnn_fst4_train_ctx *ctx, const farnn_fst4_train_weights *w, const int64_t *x,
                           const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                           int64_t valid_tokens, const farnn_fst4_train_outputs *out, void *stream);
/* as farnn_train_set_profiling / farnn_train_time */
int  farnn_fst4_train_set_profiling(farnn_fst4_train_ctx *ctx, int32_t enable);
int  farnn_fst4_train_time(farnn_fst4_train_ctx *ctx, double *total_ms, int64_t *steps);
/* The semiring of both chains (semiring_func, model_onehot.py:57, used at :93 and :100), with the arguments and error codes
 * of farnn_onehot_train_set_semiring: FARNN_SEMIRING_SUM (the default) or FARNN_SEMIRING_MAX, where a chain step is
 * max_j alpha[j] M_w[j,s] (forward) and max_j beta[j] M_w[s,j] (backward), torch.max's first maximal j taking the whole
 * adjoint.  Only the two recurrences change: the score of a position, the priority layer, the loss, the decode and every
 * limit are the same in both, and so is everything downstream of dM.  No float atomics.  The max step's extra workspace (an
 * index byte and the winning entry per step and state) is allocated by its first step; a context switched back to
 * FARNN_SEMIRING_SUM computes exactly what one that never left it does.  The Python mirror keeps this semiring opt-in for
 * its first release: the three models below train with --train_mode max only when RE2NN_BUCKETED_MAX_TRAIN=1 is set beside
 * the model's own switch (RE2NN_ONEHOT_FST_TRAIN, RE2NN_ONEHOT_IND1_TRAIN, RE2NN_DECOMP_IND1_TRAIN). */
int  farnn_fst4_train_set_semiring(farnn_fst4_train_ctx *ctx, int32_t semiring);

/* ---- training step of the onehot independent=1 model (FARNN_S_O_I, --method onehot --independent 1) --------
 * Replaces FARNN_S_O_I.forward_local(train=True) + loss.backward() (model_onehot.py:184-306, train_onehot.py:156-206) for
 * the sum semiring and the CE1 loss.  N[w] = T[w] + W (:250); Mc[w] = N[w], or N[w] * output_tensor.sum(0) with
 * mask_by_output (args.independent == 2, :252, :260, :272); both chains run on Mc and use relu, whatever update_nonlinear
 * says (:266, :278); score_i[c] = sum_{s,j} O[c,s,j] alpha_i[s] beta_{i+1}[j] N[x_i][s,j] [. P] with alpha_i the state BEFORE
 * token i, N and not Mc, and no relu (:229-233, :293-304); the loss is the cross-entropy, mean over the valid tokens (:60,
 * :142); the tags are local_decode's (:172-176).  language_tensor is the only tensor trained (:213-223);
 * output_wildcard_mat is not read under CE1 (:251-252).
 * Limits: S <= 128 (the chains' kernels, as farnn_onehot_train_create), C <= 2400 (the loss kernel keeps two score vectors
 * per wavefront, 8 x 2 x C floats, within 150 KiB of LDS; farnn_ind1_train_create returns FARNN_ERANGE outside),
 * B (L + 1) < 2^30 (the step returns FARNN_ERANGE before enqueuing anything and leaves the outputs untouched).  All
 * pointers are DEVICE pointers; tensors are row-major and unpadded. */
typedef struct farnn_ind1_train_ctx farnn_ind1_train_ctx;

typedef struct {
    int32_t V, S, C;            /* vocabulary rows of T, states, score columns (labels + 1)         */
    int32_t mask_by_output;     /* args.independent == 2: the chains run on N * O.sum(0) (:260)     */
    float   threshold;          /* decode clamp of column C-1 (model_onehot.py:172-176)             */
    int32_t o_idx;              /* label written for column C-1 (:176)                              */
} farnn_ind1_train_dims;

typedef struct {
    const float *T;             /* [V][S][S] language_tensor (:213) */
    const float *W;             /* [S][S]    wildcard_mat (:216)    */
    const float *O;             /* [C][S][S] output_tensor (:219)   */
    const float *h0, *hT;       /* [S] (:209-212)                   */
    const float *P;             /* [C][C] priority matrix or NULL (args.use_priority = 0, :301) */
} farnn_ind1_train_weights;

typedef struct {
    float *loss;                /* [1]                                                                 */
    float *dT;                  /* [V][S][S] (rows of words absent from the batch are written as zero) */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions     */
} farnn_ind1_train_outputs;

int  farnn_ind1_train_create(const farnn_ind1_train_dims *dims, int device, farnn_ind1_train_ctx **out);
void farnn_ind1_train_destroy(farnn_ind1_train_ctx *ctx);
/* One step on the given stream: writes all outputs (no float atomics: bit-identical across runs).  x, lengths, labels,
 * valid_tokens and the handling of bad labels / words: as farnn_onehot_ifst_train_step. */
int  farnn_ind1_train_step(farnn_ind1_train_ctx *ctx, const farnn_ind1_train_weights *w, const int64_t *x,
                           const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                           int64_t valid_tokens, const farnn_ind1_train_outputs *out, void *stream);
/* as farnn_train_set_profiling / farnn_train_time */
int  farnn_ind1_train_set_profiling(farnn_ind1_train_ctx *ctx, int32_t enable);
int  farnn_ind1_train_time(farnn_ind1_train_ctx *ctx, double *total_ms, int64_t *steps);
/* As farnn_fst4_train_set_semiring (model_onehot.py:264, :276): the chains run max_j over Mc[w] = N[w] (* output_tensor.sum(0)). */
int  farnn_ind1_train_set_semiring(farnn_ind1_train_ctx *ctx, int32_t semiring);

/* ---- training step of the decomposed independent=1 model (FARNN_S_D_W_I, --method decompose --independent 1) ---
 * Replaces FARNN_S_D_W_I.forward_local(train=True) + loss.backward() (model_decompose_independent.py:219-300,
 * train_decompose.py:161-221) for farnn = 0, the sum semiring and the CE1 loss, no CRF.  With v = Vgen[w]
 * (model_decompose.py:222-241): N[w] = sum_r v_r S1[:,r] S2[:,r]^T + wildcard_mat (:171-173);
 * Osum = sum_r (sum_c C_output[c,r]) S1_output[:,r] S2_output[:,r]^T (:210-214; wildcard_output is not read under CE1);
 * Mc[w] = N[w] * Osum (:174); both chains run on Mc with update_nonlinear (:176-188, :239-252);
 * br_i[r] = sum_{ij} alpha_i[i] beta_{i+1}[j] N[x_i][i,j] S1_output[i,r] S2_output[j,r] with alpha_i the state BEFORE token i and
 * N, not Mc; score_i = br_i C_output^T [. P] (:199-208, :260-278); the loss is the cross-entropy, mean over the valid
 * tokens (:295); the tags are local_decode's (:298).  Every gradient output is written in full; dVgen's rows of words absent
 * from the batch are zero.
 * Limits: S <= 128 (the chains' kernels, as farnn_onehot_train_create), C <= 2400 (the loss kernel keeps two score vectors per
 * wavefront within 150 KiB of LDS), R S S and R_O S S below 2^31 (farnn_decomp_ind1_train_create returns FARNN_ERANGE outside,
 * naming the quantity), B (L + 1) < 2^30 (the step returns FARNN_ERANGE before enqueuing anything and leaves the outputs
 * untouched).  All pointers are DEVICE pointers; tensors are row-major and unpadded. */
typedef struct farnn_decomp_ind1_train_ctx farnn_decomp_ind1_train_ctx;

typedef struct {
    int32_t V, S, R, RO, C;     /* vocabulary rows of Vgen, states, rank of S1/S2 (:40), rank of the output factors and score
                                   columns (C_output is [C][RO], :39)                                  */
    int32_t nl;                 /* args.update_nonlinear: FARNN_NL_NONE / RELU / TANH / RELUTANH (:181-188) */
    float   threshold;          /* decode clamp of column C-1 (model_decompose.py local_decode)     */
    int32_t o_idx;              /* label written for column C-1                                     */
} farnn_decomp_ind1_train_dims;

typedef struct {
    const float *Vgen;          /* [V][R] get_generalized_v_embed_vec of every word (model_decompose.py:222-241) */
    const float *S1, *S2;       /* [S][R] (:70-71)                  */
    const float *W;             /* [S][S] wildcard_mat (:91)        */
    const float *C;             /* [C][RO] C_output (:82)           */
    const float *S1o, *S2o;     /* [S][RO] S1_output, S2_output (:85-89) */
    const float *h0, *hT;       /* [S] (:52-55)                     */
    const float *P;             /* [C][C] priority matrix or NULL (args.use_priority = 0, :277) */
} farnn_decomp_ind1_train_weights;

typedef struct {
    float *loss;                /* [1]                                                                 */
    float *dVgen;               /* [V][R] (rows of words absent from the batch are written as zero)    */
    float *dS1, *dS2;           /* [S][R]                                                              */
    float *dW;                  /* [S][S] or NULL (train_wildcard_wildcard = 0, :93)                   */
    float *dC;                  /* [C][RO] or NULL (train_wildcard = 0, :83)                           */
    float *dS1o, *dS2o;         /* [S][RO] or NULL (train_wildcard = 0, :86-89)                        */
    float *dh0, *dhT;           /* [S] or NULL (train_h0 / train_hT = 0, :53-55)                       */
    int32_t *tags;              /* [B][L] decoded labels of this forward pass, -1 at pad positions     */
} farnn_decomp_ind1_train_outputs;

int  farnn_decomp_ind1_train_create(const farnn_decomp_ind1_train_dims *dims, int device, farnn_decomp_ind1_train_ctx **out);
void farnn_decomp_ind1_train_destroy(farnn_decomp_ind1_train_ctx *ctx);
/* One step on the given stream: writes all outputs (no float atomics: bit-identical across runs).  x, lengths, labels,
 * valid_tokens and the handling of bad labels / words: as farnn_onehot_ifst_train_step. */
int  farnn_decomp_ind1_train_step(farnn_decomp_ind1_train_ctx *ctx, const farnn_decomp_ind1_train_weights *w, const int64_t *x,
                                  const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                  int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *out, void *stream);
/* The same step under --use_crf 1, on the same context (as farnn_decomp_ifst_teacher_train_step sits beside the plain f3 step).
 * The context's C is the score width, labels + 2 (model_decompose_independent.py:45-47, :78-80): tags C-2 / C-1 are START / STOP.
 *   emissions = scores [. P]                                                      (model_decompose_independent.py:277-278)
 *   loss = sum over the sequences of log Z - gold (:293; baselines/crf.py:253-260): a SUM, valid_tokens does not scale it.
 *     log Z: alpha_0[j] = trans[START][j] + f_0[j]; alpha_t[j] = logsumexp_i(alpha_{t-1}[i] + trans[i][j]) + f_t[j] over the
 *     valid positions; log Z = logsumexp_i(alpha_{n-1}[i] + trans[i][STOP])       (crf.py:48-99)
 *     gold = sum_t (f_t[y_t] + trans[y_{t-1}][y_t]) with y_{-1} = START, + trans[y_{n-1}][STOP]: no START energy beyond the
 *     bigram of position 0                                                        (crf.py:202-251)
 *   dtrans [C][C] = expected - gold transition counts, the sequences' slices added in sequence order; the gradients of `out`
 *     follow from d loss / d emissions = marginals - gold one-hot through the priority layer and the plain step's backward.
 *   tags: the Viterbi path of the emissions with column C-3 clamped at threshold, the first index winning a tie, column C-3
 *     written as o_idx (model_decompose.py:339-371; crf.py:102-195), -1 at the pads.
 * The context's semiring applies to the two recurrences as in the plain step (the reference sends nothing else through
 * semiring_func).  A sequence of length 0 contributes nothing to the loss, to dtrans or to any gradient; its tags are -1 (the
 * reference cannot run one: crf.py:232 gathers at length - 1).
 * FARNN_EINVAL: crf_trans or dtrans NULL, C < 4.  FARNN_ERANGE, naming the quantity, before anything is enqueued and with the
 * outputs untouched: the CRF kernel's LDS at this (C, L), C (C + 1) * 4 + 9 L C + ... bytes in its large-tag-set form, beyond
 * 160 KiB (the largest C accepted: 190 at L = 8, 140 at L = 64).  No float atomics: two steps on the same inputs are bit-identical. */
int  farnn_decomp_ind1_crf_train_step(farnn_decomp_ind1_train_ctx *ctx, const farnn_decomp_ind1_train_weights *w,
                                      const float *crf_trans /* [C][C] */, const int64_t *x, const int64_t *lengths,
                                      const int64_t *labels, int32_t B, int32_t L, int64_t valid_tokens,
                                      const farnn_decomp_ind1_train_outputs *out, float *dtrans /* [C][C] */, void *stream);
/* The same step for the gated model (--farnn 1 | 2), on the same context.  One chain step, with v = Vgen[w], k =
 * sigmoid_exponent, h the previous state and h_init = h0 (forward chain) or hT (backward chain)
 * (model_decompose_independent.py:148-197):
 *   z = sigmoid(k (h Wss1 + v Wrs1 + bs1));  farnn 2: r = sigmoid(k (h Wss2 + v Wrs2 + bs2)), hbar = (1 - r) h_init + r h
 *   (farnn 1: hbar = h);  y = nl(hbar Mc[w]) (backward chain: hbar Mc[w]^T; the gates read Wss untransposed in both chains);
 *   h' = (1 - z) h + z y.
 * The scores read the gated states; the score, the priority layer, the loss and the decode are the plain step's.  Beside the
 * gradients of `out` (dVgen with the gates' share; dh0 / dhT with the (1 - r) share of every step of every sequence and what
 * the first step carries back) the step writes the gates' gradients in full.
 * crf_trans / dtrans: both NULL for the CE1 loss, both given for --use_crf 1 (as farnn_decomp_ind1_crf_train_step).
 * FARNN_EINVAL, before anything is enqueued and with the outputs untouched: farnn not 1 or 2, a NULL gate pointer (weight or
 * gradient) that farnn needs, sigmoid_exponent <= 0, only one of crf_trans / dtrans, a context in the max semiring (this entry
 * runs the gated chains of the sum semiring; farnn_decomp_ind1_gated_max_train_step below runs those of the max semiring).
 * FARNN_ERANGE likewise: the LDS of the chain kernels -- the gate matrices, farnn S S
 * floats, and a sequence's L + 1 tokens -- beyond 160 KiB (S = 128, farnn 2: L <= 4600).  No float atomics: two steps on the
 * same inputs are bit-identical. */
typedef struct {
    int32_t farnn;                          /* 1 or 2 (:160-169)                                   */
    const float *Wss1, *Wrs1, *bs1;         /* [S][S], [R][S], [S] (:102-104, :112-119)            */
    const float *Wss2, *Wrs2, *bs2;         /* the same for r, farnn 2 only (NULL otherwise) (:120-126) */
    float sigmoid_exponent;                 /* k > 0 (model_decompose.py:97-102)                   */
} farnn_decomp_ind1_gate_weights;

typedef struct {
    float *dWss1, *dWrs1, *dbs1;            /* [S][S], [R][S], [S]                                 */
    float *dWss2, *dWrs2, *dbs2;            /* farnn 2 only (NULL otherwise)                       */
} farnn_decomp_ind1_gate_outputs;

int  farnn_decomp_ind1_gated_train_step(farnn_decomp_ind1_train_ctx *ctx, const farnn_decomp_ind1_train_weights *w,
                                        const farnn_decomp_ind1_gate_weights *g, const float *crf_trans /* [C][C] or NULL */,
                                        const int64_t *x, const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                        int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *out,
                                        const farnn_decomp_ind1_gate_outputs *gout, float *dtrans /* [C][C] or NULL */,
                                        void *stream);
/* The gated step on a context in the max semiring (--farnn 1 | 2 --train_mode max): the same arguments.  Only the block product
 * goes through the semiring (model_decompose_independent.py:177-188, utils.py:192-195); the gate products stay matrix products:
 *   z, r, hbar as above;  q[s] = max_j hbar[j] Mc[w][j,s] (backward chain: max_j hbar[j] Mc[w][s,j]) with j*[s] the FIRST
 *   maximal j under IEEE comparison (-0 == +0; torch.max(dim=1));  y = nl(q);  h' = (1 - z) h + z y.
 * Back-propagation sends a step's block adjoint u = dh' z nl'(y) to the winning index only: dMc[w] gets u[s] hbar[j*[s]] at
 * (j*[s], s) (backward chain: (s, j*[s])), dhbar[j] = the sum over the s with j*[s] = j of u[s] times the winning entry, the
 * states s ascending.  The gates' adjoints, the carry, dh0 / dhT (with the (1 - r) share and the carry into row 0) and every
 * gradient downstream of dMc are farnn_decomp_ind1_gated_train_step's.  crf_trans / dtrans as there.
 * FARNN_EINVAL, before anything is enqueued and with the outputs untouched: a context in the sum semiring, and that entry's
 * other refusals (farnn not 1 or 2, a NULL gate pointer that farnn needs, sigmoid_exponent <= 0, only one of crf_trans /
 * dtrans).  FARNN_ERANGE likewise: the same LDS bound (the kernels' static LDS is the sum kernels').  No float atomics: two
 * steps on the same inputs are bit-identical, and the plain, CRF, gated and plain max steps on the same context return the
 * same bits before and after one of these. */
int  farnn_decomp_ind1_gated_max_train_step(farnn_decomp_ind1_train_ctx *ctx, const farnn_decomp_ind1_train_weights *w,
                                            const farnn_decomp_ind1_gate_weights *g, const float *crf_trans /* [C][C] or NULL */,
                                            const int64_t *x, const int64_t *lengths, const int64_t *labels, int32_t B, int32_t L,
                                            int64_t valid_tokens, const farnn_decomp_ind1_train_outputs *out,
                                            const farnn_decomp_ind1_gate_outputs *gout, float *dtrans /* [C][C] or NULL */,
                                            void *stream);
/* as farnn_train_set_profiling / farnn_train_time */
int  farnn_decomp_ind1_train_set_profiling(farnn_decomp_ind1_train_ctx *ctx, int32_t enable);
int  farnn_decomp_ind1_train_time(farnn_decomp_ind1_train_ctx *ctx, double *total_ms, int64_t *steps);
/* As farnn_fst4_train_set_semiring (model_decompose_independent.py:177-179): the chains run max_j over Mc[w] = N[w] * Osum with
 * the model's update_nonlinear.  dh0 / dhT receive, beside the score adjoint of the first / last position, what the first chain
 * step carries back -- in the max semiring to the winning index only. */
int  farnn_decomp_ind1_train_set_semiring(farnn_decomp_ind1_train_ctx *ctx, int32_t semiring);

/* ---- multi-tensor optimizer step: torch.optim.Adam / torch.optim.SGD (train_onehot.py:78-81 of this package) ----------
 * One launch updates every tensor of a training step (more than 32 tensors: one launch per 32).  Adam with torch's arithmetic,
 * no weight decay, no amsgrad:
 *     exp_avg    += (grad - exp_avg) (1 - beta1)
 *     exp_avg_sq  = beta2 exp_avg_sq + (1 - beta2) grad^2
 *     param      -= (lr / bc1) exp_avg / (sqrt(exp_avg_sq) / sqrt(bc2) + eps),   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
 * with t the tensor's OWN step count, kept by the handle on the host (bc1, bc2 in double); SGD: param -= lr grad.
 * The handle owns the chunk table of the tensors' sizes and the step counts, nothing else: parameters, gradients and both
 * moments are the caller's device memory (float32, contiguous), handed over per step and never retained.
 * farnn_optim_step must NOT be captured into a HIP graph: the bias corrections are computed on the host per call and travel
 * as kernel arguments, so a replayed capture would repeat the corrections of the step it was captured at. */
typedef struct farnn_optim farnn_optim;
#define FARNN_OPTIM_SGD   0
#define FARNN_OPTIM_ADAM  1

typedef struct {
    int32_t kind;               /* FARNN_OPTIM_SGD or FARNN_OPTIM_ADAM                                        */
    double  lr;                 /* >= 0                                                                        */
    double  beta1, beta2;       /* Adam: in [0, 1) (torch's defaults: 0.9, 0.999); SGD: ignored                */
    double  eps;                /* Adam: >= 0 (torch's default: 1e-8); SGD: ignored                            */
} farnn_optim_desc;

/* numel[n]: the element count of each tensor, in the order every later call lists them.  FARNN_EINVAL: an unknown kind, n <= 0,
 * a numel <= 0, lr / betas / eps outside the ranges above. */
int  farnn_optim_create(const farnn_optim_desc *desc, const int64_t *numel, int32_t n, int device, farnn_optim **out);
void farnn_optim_destroy(farnn_optim *opt);
/* One step on the given stream (hipStream_t as void*, NULL = the default stream; enqueued, not awaited).  params, grads, exp_avg,
 * exp_avg_sq: HOST arrays of n DEVICE pointers; exp_avg and exp_avg_sq may be NULL for SGD.  A tensor whose grads[i] is NULL is
 * skipped: its memory is untouched and its step count does not advance (torch's behaviour for `grad is None`).  FARNN_EINVAL
 * (a NULL params[i], or a NULL moment under Adam, for a tensor that has a gradient) is returned before anything is enqueued
 * or counted. */
int  farnn_optim_step(farnn_optim *opt, float *const *params, const float *const *grads, float *const *exp_avg,
                      float *const *exp_avg_sq, void *stream);
int  farnn_optim_set_lr(farnn_optim *opt, double lr);
/* the step count of tensor i (the steps in which it had a gradient); farnn_optim_set_steps restores it from saved state */
int  farnn_optim_steps(const farnn_optim *opt, int32_t i, int64_t *out);
int  farnn_optim_set_steps(farnn_optim *opt, int32_t i, int64_t steps);

/* ---- device-side scorer of an epoch's loss and tag metrics (metrics/metrics.py:17-28 eval_seq_token, :121-157
 * get_ner_fmeasure of this package; reference src_seq/metrics/metrics.py:7-42, :96-129) ----------------------------------
 * The reference scores ONE flat list per data set: the valid tokens of every sequence of every batch, in order.  A handle counts
 * that list batch by batch, on the device: farnn_score_add takes one batch's padded tags, gold labels, lengths and (optionally)
 * the step's loss scalar in ONE launch and waits for nothing; farnn_score_read is the only call that waits.  Every number is an
 * integer count, or a double sum taken in stream order, so the host's ratios over them equal metrics.py's bit for bit.
 *
 * Per label id the caller's tables give kind (0 other, 1 B-, 2 I-), type (-1 or 0 .. n_types - 1) and canon (the first id with the
 * same spelling).  With `prev` the previous valid token of the whole stream (across sequences, batches and adds; none before the
 * first), link[j] = kind[j] == 2 && kind[prev] != 0 && type[j] == type[prev], for the tags and for the labels separately.  A
 * position where tag and label are both B- of one type opens a candidate; the candidate is a match at the next position where
 * both links are false (which may open the next candidate), dies at the next position where exactly one is false, and is a match
 * if the stream ends first (both spans are then open-ended).  What an add leaves for the next lives in the handle: the last tag
 * and label ids, the open candidate's type, the flat length.
 * The adds (and resets) of one handle must be ordered on ONE stream: an add reads what the previous one left. */
typedef struct farnn_score farnn_score;

typedef struct {
    int64_t n;                  /* valid tokens (the flat length)                                               */
    int64_t same;               /* tag == label                                                                 */
    int64_t canon_same;         /* canon[tag] == canon[label] (get_ner_fmeasure's accuracy)                     */
    int64_t tp, fp, fn;         /* eval_seq_token's: same & tag != o; !same & tag != o; !same & label != o      */
    int64_t pred_spans;         /* B- tags                                                                      */
    int64_t gold_spans;         /* B- labels                                                                    */
    int64_t matches;            /* spans equal in start, end and type; a candidate still open counts            */
    int64_t errors;             /* valid positions whose tag or label lies outside [0, n_labels)                */
    int64_t adds;               /* farnn_score_add calls since create / reset                                   */
    double  loss_sum;           /* one double addition of the float32 loss per add that passed one              */
    int64_t *per_type;          /* HOST, [5][n_types] or NULL: B- tags, B- labels, matches, then the flat index
                                 * of the first B- tag and of the first B- label of the type (-1: none)         */
} farnn_score_counts;

/* kind, type, canon: HOST arrays [n_labels] (copied).  FARNN_EINVAL, before any device is touched: a null table or `out`,
 * n_labels <= 0, n_types < 0, a kind outside 0..2, a type outside [-1, n_types), a canon outside [0, n_labels). */
int  farnn_score_create(farnn_score **out, const int32_t *kind, const int32_t *type, const int32_t *canon, int32_t n_labels,
                        int32_t n_types, int32_t o_idx, int device);
void farnn_score_destroy(farnn_score *h);
/* tags int32 [B][L], labels int64 [B][L], lengths int64 [B], loss float[1] or NULL: DEVICE pointers.  One launch on `stream`
 * (hipStream_t as void*, NULL = the default stream), no host synchronisation and no allocation, except that the per-sequence
 * work buffer grows (after a device synchronise) when B exceeds every earlier B.  Lengths are clamped to [0, L]; positions at
 * or beyond a sequence's length are never read.  A valid position whose tag or label lies outside [0, n_labels) indexes no
 * table: it counts as kind 0 (and as its raw id in same / canon_same / tp / fp / fn) and adds one to `errors`.
 * FARNN_EINVAL: a null handle, tags, labels or lengths; B <= 0 or L <= 0. */
int  farnn_score_add(farnn_score *h, const int32_t *tags, const int64_t *labels, const int64_t *lengths, int32_t B, int32_t L,
                     const float *loss, void *stream);
/* Copies the counts to the host behind everything enqueued on `stream` and waits for it: the only call that waits.  per_type may
 * be NULL.  The handle keeps counting: a later add continues the same stream of tokens. */
int  farnn_score_read(farnn_score *h, farnn_score_counts *counts, void *stream);
/* Back to the state after create (enqueued on `stream`, not awaited). */
int  farnn_score_reset(farnn_score *h, void *stream);

/* ---- CP-ALS of a 3-way tensor given as a coordinate list, float64 ------------------------------
 * Stands in for tensorly.parafac as the reference calls it (wfa/tensor_func.py:7-13: init='random', normalize_factors=False, no
 * weights): the step from an automaton's [V',S,S] tensor to the factors of IIID / IID.automata.*.pkl.  One sweep is, for mode
 * n = 0, 1, 2:  H = Hadamard product of the two other factors' Gram matrices;  M = X_(n) (Khatri-Rao product of the two other
 * factors), on the nonzeros;  A_n = solve(H^T, M^T)^T by Cholesky.  After each sweep, with the last mode's M,
 *     rec_error = sqrt(| ||X||^2 + sum(G0 o G1 o G2) - 2 sum(M o A_2) |) / ||X||,
 * and from the second sweep on the run stops when |rec_errors[-2] - rec_errors[-1]| < tol, or at n_iter_max.  The initial
 * factors are the caller's (numpy.random.RandomState(seed).random_sample((dim_n, rank)), mode order 0, 1, 2, in the mirror).
 * Factors are [dim_n][rank] doubles, C-contiguous.  Every sum is taken in an order fixed by the data (64-nonzero chunks of a
 * row, 1024-row panels of a factor, a fixed tree), there is no float atomic: repeated calls are bit-identical.
 * Limits: 1 <= rank <= min(max_rank, 352) (FARNN_ERANGE above, before any launch); dims below 2^22; nnz below 2^30.
 * One caller thread and one stream at a time per context. */
#define FARNN_ENUMERIC (-33)   /* a Cholesky pivot of a CP-ALS normal matrix was not a positive finite number (EDOM) */
typedef struct farnn_cp_ctx farnn_cp_ctx;

/* dims[3], idx0 / idx1 / idx2 [nnz] (int32), val [nnz] (double): HOST arrays, copied.  Repeated coordinates add.  The context
 * keeps the nonzeros in three orders, one grouped by each mode's index, and ||X||^2; its buffers are sized for
 * min(max_rank, 352).  FARNN_EINVAL: a null pointer, nnz <= 0, max_rank < 1, a dimension outside [1, 2^22), a coordinate outside
 * its dimension, a norm that is zero or not finite. */
int  farnn_cp_create(const int32_t *dims, int64_t nnz, const int32_t *idx0, const int32_t *idx1, const int32_t *idx2,
                     const double *val, int32_t max_rank, int device, farnn_cp_ctx **out);
void farnn_cp_destroy(farnn_cp_ctx *ctx);
/* The three stages on their own; f0 / f1 / f2, out, H, M are DEVICE pointers (the factor of `mode` itself is not read by the
 * first two and may be NULL); enqueued on `stream` (hipStream_t as void*, NULL = the default stream).
 * out [dims[mode]][rank] = the MTTKRP; a row without a nonzero gives zeros. */
int  farnn_cp_mttkrp(farnn_cp_ctx *ctx, int32_t mode, int32_t rank, const double *f0, const double *f1, const double *f2,
                     double *out, void *stream);
/* H [rank][rank] = (A_a^T A_a) o (A_b^T A_b) of the two other modes, on v_mfma_f64_16x16x4_f64; symmetric bit for bit. */
int  farnn_cp_normal_matrix(farnn_cp_ctx *ctx, int32_t mode, int32_t rank, const double *f0, const double *f1, const double *f2,
                            double *H, void *stream);
/* out [rows][rank] = M H^-1 for the symmetric positive definite H (its lower triangle is read): Cholesky, two triangular solves,
 * no explicit inverse.  This entry waits for `stream` and reads the pivot flag: FARNN_ENUMERIC if a pivot was not a positive
 * finite number (`out` is then meaningless; the flag is cleared and the context stays usable). */
int  farnn_cp_solve(farnn_cp_ctx *ctx, int32_t rank, const double *H, const double *M, int32_t rows, double *out, void *stream);
/* A whole run.  f0 / f1 / f2: HOST arrays, the initial factors in and the result out; rec_errors: HOST, [n_iter_max];
 * *n_sweeps: the sweeps done (= the entries of rec_errors written).  The factors cross the bus once each way; in between the
 * host reads one double and the pivot flag per sweep.  FARNN_ENUMERIC as farnn_cp_solve (the factors are then left as given). */
int  farnn_cp_run(farnn_cp_ctx *ctx, int32_t rank, int32_t n_iter_max, double tol, double *f0, double *f1, double *f2,
                  double *rec_errors, int32_t *n_sweeps, void *stream);
/* enable != 0: the following runs time their stages with HIP events (and wait after every stage); also clears the totals.
 * stage_ms[4]: normal matrix, MTTKRP, solve, error terms -- milliseconds summed over `*sweeps` timed sweeps. */
int  farnn_cp_set_profiling(farnn_cp_ctx *ctx, int32_t enable);
int  farnn_cp_time(farnn_cp_ctx *ctx, double *stage_ms, int64_t *sweeps);
/* ||X||^2 and the number of distinct coordinates, as create computed them */
int  farnn_cp_norm2(const farnn_cp_ctx *ctx, double *normx2, int64_t *nnz);

/* ---- the same for a tensor of order 3 or 4 -------------------------------------------------------------
 * Order 4 is tensorly.parafac as the reference's tensor4_to_factors calls it (wfa/tensor_func.py:16-27; the mirror passes
 * tol = 1e-6): the step from an automaton's [V',C,S,S] tensor to the factors of D.automata.*.pkl.  One sweep is, for mode
 * n = 0 .. order-1:  H = Hadamard product of the OTHER factors' Gram matrices (three at order 4);  M = the MTTKRP on the nonzeros,
 * each term val * Fa[ia] * Fb[ib] (* Fc[ic]) with the other factors in ascending mode order;  A_n = M H^-1 as above.  After the
 * sweep, with M of the last mode (order - 1),
 *     rec_error = sqrt(| ||X||^2 + sum(G0 o .. o G_last) - 2 sum(M o A_last) |) / ||X||;
 * the stop rule, the pivot flag, the limits and the fixed summation orders are the 3-way entries'.  The context keeps the
 * nonzeros in `order` orders, one grouped by each mode.  Repeated coordinates are found by comparing coordinate TUPLES and
 * ||X||^2 is the merged values' sum of squares: nothing rests on a flattened index, so no product of dims is refused.
 * An order-3 context made here is the one farnn_cp_create makes, bit for bit, and serves the 3-way entries too.  The 3-way
 * entries (farnn_cp_mttkrp, _normal_matrix, _run) on an order-4 context return FARNN_EINVAL before any launch; farnn_cp_solve,
 * _set_profiling, _time, _norm2 and _destroy serve both orders. */
/* dims[order]; idx[order]: HOST pointers to HOST int32 arrays [nnz].  FARNN_EINVAL as farnn_cp_create, and for an order outside
 * {3, 4}. */
int  farnn_cp_create_n(int32_t order, const int32_t *dims, int64_t nnz, const int32_t *const *idx, const double *val,
                       int32_t max_rank, int device, farnn_cp_ctx **out);
int  farnn_cp_order(const farnn_cp_ctx *ctx, int32_t *order);
/* f[order]: a HOST array of DEVICE pointers (f[mode] is not read and may be NULL).  FARNN_EINVAL before any launch for
 * mode >= the context's order. */
int  farnn_cp_mttkrp_n(farnn_cp_ctx *ctx, int32_t mode, int32_t rank, const double *const *f, double *out, void *stream);
int  farnn_cp_normal_matrix_n(farnn_cp_ctx *ctx, int32_t mode, int32_t rank, const double *const *f, double *H, void *stream);
/* f[order]: HOST pointers to HOST arrays, the initial factors in and the result out; the rest as farnn_cp_run. */
int  farnn_cp_run_n(farnn_cp_ctx *ctx, int32_t rank, int32_t n_iter_max, double tol, double *const *f, double *rec_errors,
                    int32_t *n_sweeps, void *stream);

/* ---- introspection / measurement ----------------------------------------------------- */
int  farnn_abi_version(void);
/* 1: the A/B (profiling) build of the library (csrc/build.py --probes): it also carries the forms the production build left behind --
 * FARNN_CV_ONE / FARNN_CV_STASH, the one-launch CRF step -- and the in-kernel probes (FARNN_DBG); 0: the production build. */
int  farnn_ab_build(void);
int  farnn_device_count(void);
const char *farnn_last_error(void);
int  farnn_num_columns(const farnn_model *m);              /* K of the scores tensor */
/* algorithmic HBM bytes of one farnn_tag() call with `valid_tokens` tagged tokens
 * (SURVEY.md 8d / DESIGN.md: per-token figure x tokens), for the roofline line of bench.py */
double farnn_algorithmic_bytes(const farnn_model *m, int64_t valid_tokens);
/* the share of that figure read/written by kernel `which` (0 = recurrence chain, 1 = score+decode), for the form the plan of the
 * handle's last farnn_tag() call chose (before the first call: the model kind's default recurrence kernel) */
double farnn_kernel_algorithmic_bytes(const farnn_model *m, int32_t which, int64_t valid_tokens);
/* per-kernel timing with HIP events recorded on the launch stream.  enable=N>0 starts collecting
 * on every N-th farnn_tag() call (N=1: every call; event records cost a few microseconds of
 * launch latency each, so a stride keeps the timed region honest); enable=0 stops.
 * farnn_kernel_time() synchronises, then reports the accumulated milliseconds and the number of
 * timed launches of kernel `which` (0 = recurrence chain, 1 = score+decode, 2 = prep, 3 = the token table of
 * farnn_tag_vectors). */
int  farnn_set_profiling(farnn_model *m, int32_t enable);
int  farnn_kernel_time(farnn_model *m, int32_t which, double *total_ms, int64_t *launches);
/* the kernel behind slot `which`, read from the plan of the handle's last farnn_tag() call (before the first call, and after
 * farnn_set_compact(): the model kind's default).  The score slot is named by the model's kind whatever that call launched. */
const char *farnn_kernel_name(const farnn_model *m, int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* FARNN_H */
