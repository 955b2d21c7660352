// Host side of the training steps that run the onehot chains over per-word blocks M[w] (farnn_train.hip): the chain and dT
// launches of the onehot i-FST step, and BucketedStep -- what the onehot FST, the onehot independent=1 and the decomposed
// independent=1 step share: the plan, the head and tail of the workspace, and every stage but the ones that build M and
// score in the step's own weights.
#pragma once
#include <assert.h>
#include "train_host.hip.h"
#include "fst4_train.hip.h"
#include "onehot_train_max.hip.h"

namespace farnn {

// farnn_{fst4,ind1,decomp_ind1}_train_set_semiring: the arguments and error codes of farnn_onehot_train_set_semiring
template <typename Ctx>
inline int bucketed_set_semiring(const char *name, Ctx *c, int32_t semiring) {
    if (!c) return fail(FARNN_EINVAL, "%s_set_semiring: null context%s", name);
    if (semiring != FARNN_SEMIRING_SUM && semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "%s_set_semiring: semiring must be FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX%s", name);
    c->semiring = semiring;
    return FARNN_OK;
}

// Both chains (BPTT = false: with the state stash; true: back-propagation through time), register slots by S
template <bool BPTT>
inline int launch_onehot_chains(const OhTrainParams &q, size_t lds_tok, hipStream_t s) {
    return with_chain_slots(q.S, [&](auto RS) { return launch(onehot_train_chain_kernel<RS(), BPTT>, dim3(q.B, 2), OT_THREADS, lds_tok, s, q); });
}
// d loss / d M[w] (the i-FST step's language_tensor), word by word from the sorted positions; tiles per workgroup by S
inline int launch_onehot_dT(const OhTrainParams &q, const Buckets &bk, float *dT, float *partial, hipStream_t s) {
    const size_t V = q.V, S = q.S, N0 = (size_t)q.B * q.L;
    const unsigned ngrid = (unsigned)(V + (N0 + OT_G - 1) / OT_G);   // bound on the runs: sum_w max(1, ceil(n_w / G))
    auto go = [&](auto NT) {
        return launch(onehot_dT_kernel<NT()>, ngrid, 256, 4 * (size_t)OT_G * S * sizeof(float), s, q, bk.list, bk.wstart, bk.wcount,
                      bk.itoff, bk.psoff, dT, partial);
    };
    if (int rc = S <= 32 ? go(int_c<2>()) : S <= 64 ? go(int_c<4>()) : S <= 96 ? go(int_c<6>()) : go(int_c<8>())) return rc;
    onehot_dT_reduce_kernel<<<dim3((unsigned)V, (unsigned)((S * S + 255) / 256)), 256, 0, s>>>(bk.itoff, bk.psoff, partial, dT, (int)S);
    return FARNN_OK;
}

// One step of a model whose chains run on per-word blocks and whose score kernel (F: its parameters) walks the positions in
// bucket order, a word's columns split into groups: the plan and what the stages hand on.  The step itself adds its own
// arrays between carve_head and carve_tail, the stages that build M / MT and the score launches.
// In the max semiring (the context's semiring; the reference sends only the two recurrences through semiring_func) the chains,
// their back-propagation and dM_words are the onehot i-FST's max kernels (onehot_train_max.hip.h) on the same M / MT, mask of
// ones and nl: the stash rows keep their meaning (A[b][t] = alpha_t, Bk[b][t] = beta_{len-t}), so the score passes, the loss,
// the adjoint reduction and everything downstream of dM are the sum step's, untouched.
template <typename Ctx, typename W, typename O, typename F>
struct BucketedStep {
    bool mx;                      // the max semiring: its own chain, BPTT and dM stages
    int B, L, ngrp, cpg;          // groups per word of the score kernels, columns (labels or output ranks) per group
    size_t S, K, V, N1, N0;
    unsigned lgrid;               // workgroups of the loss kernel
    size_t need, ineed;           // floats of ws, ints of iws: the totals of the step's carve_ws and of carve_bucket_ints
    size_t lds_tok, lds_sc, lds_loss;   // LDS bytes of the chain, score and loss kernels
    size_t lds_mdt;               // and of the max semiring's dM kernel
    Ctx *c; const W *w; const O *o; hipStream_t s;
    OhTrainParams q;
    OhMaxParams mq;
    float *carry0;                // max semiring: [B][2][S] d loss / d h0, d loss / d hT per sequence, written by BPTT (null: not asked for)
    F f;
    float *SC, *DS, *M, *MT, *dM, *ones, *loss_part, *partial, *part;
    Buckets bk;
    const int64_t *labels; float inv_tokens;

    // Stage 2 (after the arguments): host arithmetic only; every size the step refuses is refused here, before anything is
    // enqueued.  columns: what the groups of the score kernels divide; lds_floats: the LDS of the step's score kernel
    int plan_bucketed(const char *name, int B_, int L_, size_t columns, size_t (*lds_floats)(int, int, int)) {
        // positions are 32-bit flat indices b L + i in the bucketing, dM and score kernels
        if ((unsigned long long)B_ * (L_ + 1) >= (1ull << 30)) return fail(FARNN_ERANGE, "%s_step: B (L+1) must stay below 2^30%s", name);
        mx = c->semiring == FARNN_SEMIRING_MAX;
        B = B_; L = L_; S = c->d.S; K = c->d.C; V = c->d.V;
        N1 = (size_t)B * (L + 1); N0 = (size_t)B * L;
        // a word's columns are split over enough workgroups to fill the chip when the batch has few distinct words
        const size_t words = std::min(V, N0), want = std::min<size_t>({(1024 + words - 1) / words, columns, (size_t)F4_MAX_GROUPS});
        cpg = (int)((columns + want - 1) / want); ngrp = (int)((columns + cpg - 1) / cpg);
        lgrid = (unsigned)std::min<size_t>(768, (N0 + 7) / 8);
        f.SP = (int)((S + 3) & ~(size_t)3); f.CPR = f.SP / 4; f.GW = 64 / f.CPR;
        lds_tok = (size_t)(L + 1) * sizeof(int);
        lds_sc = lds_floats(f.SP, f.CPR, f.GW) * sizeof(float);
        lds_loss = fst4_loss_lds_bytes(K); lds_mdt = onehot_max_dT_lds_bytes(S);
        ineed = carve_bucket_ints(nullptr, bk, V, N0);
        int rc;
        if ((rc = lds_fits(lds_tok)) || (rc = lds_fits(lds_sc)) || (mx && (rc = lds_fits(lds_mdt)))) return rc;
        return lds_fits(lds_loss);
    }
    // the head and the tail of the float workspace; the step's own arrays lie between them
    void carve_head(Carver<float> &a) {
        const size_t nS = N1 * S;
        q.A = a.take(nS); q.Bk = a.take(nS); q.GA = a.take(nS); q.GB = a.take(nS); q.UF = a.take(nS); q.DQ = a.take(nS);
    }
    void carve_tail(Carver<float> &a) {
        ones = a.take((S + 3) & ~(size_t)3);
        loss_part = a.take((size_t)lgrid * 8);
        partial = a.take((2 * ((N0 + OT_G - 1) / OT_G) + 1) * S * S);    // dM: partial tiles of the words with several runs
        part = a.take(N0 * (size_t)ngrp * 2 * S);                        // d alpha / d beta per position and group
    }
    // the max semiring, behind everything the sum step lays out (the last call of the step's carve_ws; the buffer is grown by
    // the first max step): the winning entries, and the indices as bytes (S <= 128).  The per-step dM entries take the rows the
    // sum step's BPTT writes (UF, DQ), which the max step does not use.
    void carve_max(Carver<float> &a) {
        if (!mx) return;
        const size_t nS = N1 * S;
        mq.WINf = a.take(nS); mq.WINb = a.take(nS);
        mq.IDXf = (uint8_t *)a.take((nS + 3) / 4); mq.IDXb = (uint8_t *)a.take((nS + 3) / 4);
        mq.GMf = q.UF; mq.GMb = q.DQ;
    }
    // Stage 3's common part, once the step's carve_ws has run: the int workspace, the chains' parameters (the output mask is
    // never the chains' own here: a mask of ones), the loss kernel's
    void carve_bucketed(const int64_t *x, const int64_t *lengths, const int64_t *labels_, int64_t valid_tokens, int nl) {
        [[maybe_unused]] const size_t icarved = carve_bucket_ints(c->iws.p, bk, V, N0);
        assert(icarved == ineed);
        q.M = M; q.MT = MT; q.o = ones; q.h0 = w->h0; q.hT = w->hT; q.x = x; q.len = lengths;
        q.B = B; q.L = L; q.V = (int)V; q.S = (int)S; q.nl = nl;
        labels = labels_; inv_tokens = 1.0f / (float)valid_tokens;
    }
    // Stage 4 (behind the step's memsets): the positions bucketed by word, the chains' mask of ones
    int bucket_and_fill() {
        if (int rc = launch_bucketing(q.x, q.len, B, L, (int)V, bk, c->err.dev, s)) return rc;
        fst4_fill_kernel<<<(unsigned)((S + 255) / 256), 256, 0, s>>>(ones, 1.0f, (int)S);
        return FARNN_OK;
    }
    // Stages 6 and 10: both chains with the stash (max: with the arg-max index and the winning entry as well), then their
    // back-propagation through time (max: to the winning index only; with carry0, on into row 0)
    template <bool BPTT>
    int chains() {
        if (!mx) return launch_onehot_chains<BPTT>(q, lds_tok, s);
        if (!BPTT) return with_chain_slots(S, [&](auto RS) { return launch(onehot_max_chain_kernel<RS()>, dim3(B, 2), OT_THREADS, lds_tok, s, q, mq); });
        if (carry0) return launch(onehot_max_bptt_carry_kernel, dim3(B, 2), OT_THREADS, 0, s, q, mq, carry0);
        return launch(onehot_max_bptt_kernel, dim3(B, 2), OT_THREADS, 0, s, q, mq);
    }
    // Stage 8, on the scores SC: priority layer, cross-entropy, decode, d loss / d scores; the loss as per-wavefront partials
    int loss_on_scores() {
        if (int rc = launch(fst4_loss_kernel, lgrid, 512, lds_loss, s, SC, w->P, q.len, labels, c->err.dev, DS, o->tags, loss_part, B, L,
                            (int)K, c->d.o_idx, c->d.threshold, inv_tokens)) return rc;
        launch_loss_sum(loss_part, lgrid, o->loss, s);
        return FARNN_OK;
    }
    // Stage 9: d loss / d alpha_i and d loss / d beta_{i+1} of every position: the groups' partials (scores1: the step's score
    // kernel in MODE 1) added in group order
    template <typename Scores1>
    int adjoints(Scores1 &&scores1) {
        if (int rc = scores1()) return rc;
        fst4_adj_reduce_kernel<<<(unsigned)N0, 128, 0, s>>>(part, bk.list, bk.wstart, bk.wcount, q.len, q.GA, q.GB, (int)V, L, (int)S, ngrp);
        return FARNN_OK;
    }
    // Stage 11: dM[w] of the chains, the i-FST step's per-word reduction (max: of the per-step entries, in bucket order)
    int dM_words() {
        if (!mx) return launch_onehot_dT(q, bk, dM, partial, s);
        const unsigned ngrid = (unsigned)(V + (N0 + OT_G - 1) / OT_G);
        if (int rc = launch(onehot_max_dT_kernel, ngrid, 256, lds_mdt, s, q, mq, bk.list, bk.wstart, bk.wcount, bk.itoff, bk.psoff,
                            dM, partial)) return rc;
        onehot_dT_reduce_kernel<<<dim3((unsigned)V, (unsigned)((S * S + 255) / 256)), 256, 0, s>>>(bk.itoff, bk.psoff, partial, dM, (int)S);
        return FARNN_OK;
    }
};

}  // namespace farnn
