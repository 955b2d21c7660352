// libfarnn_hip.so -- C-ABI entry points (include/farnn.h) of the MI355X-native FA-RNN tagging path.
// gfx950 only; no CPU fallback lives here (the CPU oracle is test infrastructure under oracle/).
// The handle, its owner and the temporaries: tag_host.hip.h; the creates: tag_create.hip.h (one translation unit with this file).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "common.hip.h"
#include "host_util.hip.h"
#include "chain.hip.h"
#include "score_decode.hip.h"
#include "layout.hip.h"
#include "fst4_score.hip.h"
#include "decomp_chain.hip.h"
#include "decomp1_score.hip.h"
#include "decomp_rows.hip.h"
#include "compact_tag.hip.h"
#include "decomp_regs.hip.h"
#include "compact.hip.h"
#include "chain_regs_params.hip.h"
#include "tag_host.hip.h"
#include "tag_create.hip.h"

namespace farnn {
thread_local char g_err[512] = "";
thread_local const Tunables *g_tun = nullptr;
}

extern "C" int farnn_has_compact(const farnn_model *m) { return (m && m->bmNS > 0 && m->bmF) ? 1 : 0; }

extern "C" int farnn_set_compact(farnn_model *m, int32_t enable) {
    if (!m) return fail(FARNN_EINVAL, "set_compact: null model%s%s");
    if (enable && !farnn_has_compact(m))
        return fail(FARNN_EINVAL, "set_compact: this model has no compact form (i-FST with 0/1 weights, sum semiring, at most 512 states)%s%s");
    if (!enable && !m->Mf) return fail(FARNN_EINVAL, "set_compact: this handle was created compact-only (no dense blocks)%s%s");
    m->compact_on = enable != 0;
    m->plan = TagPlan();                    // (the handle's form changed: no call has been planned under it)
    return FARNN_OK;
}

// ---- workspace -------------------------------------------------------------------------------
// floats of a row of the token table: what decomp_rows_kernel calls tvl
// (a max-semiring handle's rows are the padded copy alone: decomp_chain_kernel computes its gates itself)
static int sf_row_floats(const farnn_model *m) {
    return m->sf_max ? m->Rp : m->Rp + (m->dw.farnn >= 1 ? m->SP : 0) + (m->dw.farnn == 2 ? m->SP : 0);
}

extern "C" int farnn_reserve(farnn_model *m, int32_t B, int32_t L) {
    if (!m || B <= 0 || L <= 0) return fail(FARNN_EINVAL, "reserve: bad arguments%s%s");
    Workspace &w = m->ws;
    if (B <= w.B && L <= w.L) return FARNN_OK;
    TunScope tun_scope(&m->tun);
    FARNN_HIP_TRY(hipSetDevice(m->device));
    const int nB = B > w.B ? B : w.B, nL = L > w.L ? L : w.L;      // it only grows, per dimension
    if (w.A) FARNN_HIP_TRY(hipDeviceSynchronize());
    w.release();
    size_t stash = (size_t)nB * (nL + 1) * m->SP * sizeof(float);
    FARNN_HIP_TRY(hipMalloc((void **)&w.A, stash));
    FARNN_HIP_TRY(hipMalloc((void **)&w.Bk, stash));
    FARNN_HIP_TRY(hipMalloc((void **)&w.offs, (size_t)(nB + 1) * sizeof(int64_t)));
    FARNN_HIP_TRY(hipMalloc((void **)&w.order, (size_t)nB * sizeof(int)));
    w.hs_bytes = round_up_sz((size_t)(3 * nB + 48) * sizeof(unsigned long long), 16);     // progress [2][nB], arrival [nB], the launch counter
    FARNN_HIP_TRY(hipMalloc((void **)&w.hs, w.hs_bytes));
    FARNN_HIP_TRY(hipMemset(w.hs, 0, w.hs_bytes));
    if (m->use_crf)
        FARNN_HIP_TRY(hipMalloc((void **)&w.crf_scores, (size_t)nB * nL * m->Kp * sizeof(float) + 1024));   // +1 KiB: LDS-DMA pieces
    if (m->d1_BSSp)
        FARNN_HIP_TRY(hipMalloc((void **)&w.d1_br, (size_t)nB * nL * ((m->S + 15) / 16) * ((m->RO + 15) / 16 * 16) * sizeof(float)));
    if (m->sf) {      // the token table (rows of the handle's own tvl floats; +1 KiB like dev_alloc) and the identity ids of the largest call
        const size_t nt = (size_t)nB * nL, tt_bytes = nt * sf_row_floats(m) * sizeof(float) + 1024;
        // a max-semiring handle on the dense route: the two block images of the largest call that route takes (plan_tag), and the
        // token table only when a call within the capacity can fall through to the generic route
        const size_t nblk = (m->sf_max && m->sf_dense) ? std::min(nt, (size_t)m->sf_block_tokens) : 0;
        if (nblk) {
            const size_t tb_bytes = nblk * m->geom.SR * m->SP * sizeof(float) + 1024;      // +1 KiB like dev_alloc
            FARNN_HIP_TRY(hipMalloc((void **)&w.tbf, tb_bytes));
            FARNN_HIP_TRY(hipMalloc((void **)&w.tbb, tb_bytes));
            FARNN_HIP_TRY(hipMemset(w.tbf, 0, tb_bytes));  // (blocks of pad positions are never written; no chain kernel's step reads them)
            FARNN_HIP_TRY(hipMemset(w.tbb, 0, tb_bytes));
        }
        if (!nblk || nt > nblk) {
            FARNN_HIP_TRY(hipMalloc((void **)&w.tt, tt_bytes));
            FARNN_HIP_TRY(hipMemset(w.tt, 0, tt_bytes));   // (rows of pad positions are never written; nothing reads them either)
        }
        FARNN_HIP_TRY(hipMalloc((void **)&w.ids, nt * sizeof(int64_t)));
        iota_kernel<<<(unsigned)((nt + 255) / 256), 256>>>(w.ids, (long long)nt);
        FARNN_HIP_TRY(hipGetLastError());
    }
    FARNN_HIP_TRY(hipMemset(w.A, 0, stash));
    FARNN_HIP_TRY(hipMemset(w.Bk, 0, stash));
    FARNN_HIP_TRY(hipDeviceSynchronize());
    w.B = nB; w.L = nL;
    return FARNN_OK;
}

// ---- profiling -------------------------------------------------------------------------------
struct KernelTimer {
    farnn_model *m; int which; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr;
    // ext = true: the events ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL start/stop events): no
    // extra packets on the stream, so a timed step costs the same as an untimed one; the caller passes e0/e1 to the launch
    bool ext;
    KernelTimer(farnn_model *m_, int w, hipStream_t s_, bool ext_ = false) : m(m_), which(w), s(s_), ext(ext_) {
        if (m->prof_this_call) {
            e0 = m->prof.get(); e1 = m->prof.get();
            if (e0 && e1 && !ext) (void)hipEventRecord(e0, s);
        }
    }
    ~KernelTimer() {
        if (e0 && e1) {
            if (!ext) (void)hipEventRecord(e1, s);
            m->prof.ev[which].push_back(e0);
            m->prof.ev[which].push_back(e1);
        }
    }
};

static void prof_fold(farnn_model *m) {
    for (int k = 0; k < KERN_COUNT; k++) {
        auto &v = m->prof.ev[k];
        for (size_t i = 0; i + 1 < v.size(); i += 2) {
            float ms = 0.f;
            if (hipEventSynchronize(v[i + 1]) == hipSuccess &&
                hipEventElapsedTime(&ms, v[i], v[i + 1]) == hipSuccess) {
                m->prof.ms[k] += ms; m->prof.n[k] += 1;
            }
            m->prof.pool.push_back(v[i]); m->prof.pool.push_back(v[i + 1]);
        }
        v.clear();
    }
}

extern "C" int farnn_set_profiling(farnn_model *m, int32_t enable) {
    if (!m) return fail(FARNN_EINVAL, "null model%s%s");
    prof_fold(m);
    if (enable) {
        for (int k = 0; k < KERN_COUNT; k++) { m->prof.ms[k] = 0; m->prof.n[k] = 0; }
        while (m->prof.pool.size() < 256) {       // events exist before the timed region starts
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) break;
            m->prof.pool.push_back(e);
        }
    }
    m->profiling = enable > 0 ? enable : 0;
    m->calls = 0;
    return FARNN_OK;
}

extern "C" int farnn_kernel_time(farnn_model *m, int32_t which, double *total_ms, int64_t *launches) {
    if (!m || which < 0 || which >= KERN_COUNT) return fail(FARNN_EINVAL, "kernel_time: bad arguments%s%s");
    prof_fold(m);
    if (total_ms) *total_ms = m->prof.ms[which];
    if (launches) *launches = m->prof.n[which];
    return FARNN_OK;
}

// ---- the plan of a call (tag_plan.hip.h) --------------------------------------------------------
// Every decision about a farnn_tag call is made here, from host arithmetic alone and before anything is enqueued; the refusals
// the dispatch can raise come from here too.  No FARNN_* switch that selects a form is read anywhere else on the call path.

// the destination-split form of the narrow register-fed kernel (chain_dest.hip.h)
static bool regs_dest(const farnn_model *m) {
    return !m->rgeom.wide && m->semiring != FARNN_SEMIRING_MAX && !tun(TUN_NODEST);
}

// the Viterbi launch behind the scores; fused: it computes the scores itself (no score_tile launch goes before it)
static int plan_viterbi(const farnn_model *m, TagPlan &p, bool fused) {
    if (m->K > 256) return fail(FARNN_ERANGE, "Viterbi: more than 256 tags%s%s");
    const size_t hlds = viterbi_hist_lds_bytes(m->K, m->Kp, m->SP, p.L, fused);
    // (K >= 224 never takes this form: the transposed transition table alone is 196 KiB -- no IB4 = 7, 8 instantiations)
    if (hlds <= 158 * 1024 && viterbi_hist_ib4(m->K) <= 6 && !tun(TUN_VITERBI_BP)) {
        // partition history in LDS, back-pointers recomputed along the path
        p.viterbi = VITERBI_HIST; p.ib4 = viterbi_hist_ib4(m->K); p.viterbi_lds = hlds;
        return FARNN_OK;
    }
    if (fused) return fail(FARNN_EINVAL, "Viterbi: the fused form needs the history in LDS%s%s");
    // long sequences: two partition rows + stored back-pointers
    p.viterbi = VITERBI_BP; p.ib4 = viterbi_ib4(m->K); p.viterbi_lds = viterbi_lds_bytes(m->K, m->Kp, p.L);
    return lds_fits(p.viterbi_lds);
}

// fused: the Viterbi kernel computes the scores itself (no score_tile launch goes before it)
static bool viterbi_can_fuse(const farnn_model *m, int L, bool scores) {
    return m->use_crf && !scores && !m->P && m->ws.A && m->OT && m->K <= 256 &&
           viterbi_hist_lds_bytes(m->K, m->Kp, m->SP, L, true) <= 158 * 1024 && viterbi_hist_ib4(m->K) <= 6 &&
           !tun(TUN_VITERBI_BP) && !tun(TUN_VITERBI_UNFUSED);
}

// the stand-alone scores + decode of the i-FST kinds, behind a recurrence that left the states in the stash
static int plan_score_decode(const farnn_model *m, TagPlan &p, bool flat, bool scores, bool offs) {
    if (viterbi_can_fuse(m, p.L, scores)) {          // stash -> scores -> Viterbi -> tags in one kernel
        p.score = SCORE_VITERBI_FUSED;
        return plan_viterbi(m, p, true);
    }
    if (m->lm.on && !m->P && !scores && !m->use_crf && m->S <= LM_MAXS * 2 && (p.B <= 1024 || !flat || offs)) {
        // K2l: the output matrix is a label map and only tags are asked for -- S multiply-adds and a scan per token, one workgroup
        // per sequence (score_decode.hip.h).  FARNN_NOLABELMAP=1 (no label map is built then) keeps the matrix form.
        p.score = SCORE_LABEL_MAP;
        return FARNN_OK;
    }
    p.score = SCORE_TILE; p.kch = m->Kc / 64;
    return m->use_crf ? plan_viterbi(m, p, false) : FARNN_OK;
}

// The dense-block recurrence.  fuse: the decode is the threshold/argmax one, so the scores and the decode may run beside the
// recurrence (ONE launch) where the geometry allows it; p.fused tells whether it does.
static int plan_chain(const farnn_model *m, TagPlan &p, bool fuse, bool lm_tags, bool offs_ok) {
    const ChainGeom &g = m->geom;
    const int L = p.L;
    // ---- the register-fed kernel (chain_regs.hip.h) where its geometry applies: S <= 72, two workgroups per compute unit, or
    // its wide form (chain_wide.hip.h): 72 < S <= 128, one workgroup per compute unit.
    if (m->rgeom.ok && !tun(TUN_NOREGS)) {
        const RegsGeom &rg = m->rgeom;
        const size_t lds_cap = rg.wide ? 158 * 1024 : 80 * 1024;
        bool score = fuse && m->ws.hs && m->OTm && m->c16 >= 1 && m->c16 <= (rg.wide ? RGW_NG : RG_NG) && m->Kc <= 256 && L <= 31 * RG_TT &&
                     offs_ok && !tun(TUN_NOFUSE);
        // Which form is the faster one was measured, and the faster one is the default.  S <= 72 with a label-map output matrix (tags
        // only): the recurrence-only kernel followed by the label-map score launch (K2l).  Round 5 kept ONE launch (the scores and
        // the decode beside the recurrence: north_star's form) while 2 B <= compute units, on measurements at B = 64 / 256 / 1 024 and
        // L = 64 only; round 6's grid (scripts/gpu_r06_dispatch_grid.py -> profiles/r06_dispatch_grid.txt: B = 16..128 x L = 16..100)
        // has two launches ahead at 32 of its 35 points -- by 5-20 % at the reference's default --seq_max_len 30 and below, within
        // 1 % either way at L = 64 -- so the rule no longer looks at the batch.  FARNN_FUSE=1 keeps the one launch (what a HIP graph
        // replays as one node); tests/test_gpu_dispatch_ab.py holds the default to "not the slower form" at nine (B, L) points.
        if (score && !rg.wide && lm_tags && !tun(TUN_FUSE)) score = false;
        const bool lm_path = score && lm_tags;
        const bool dest = regs_dest(m);
        auto carve = [&](bool sc, bool lm, bool row80) {
            return (size_t)regs_lds(L, m->SP, rg.NP, sc ? m->c16 : 0, sc ? m->Kc : 0, sc, rg.RQ, lm, dest, row80).total * sizeof(float);
        };
        size_t lds = carve(score, lm_path, false);
        // the wide form PAIRED (two workgroups per compute unit, like S <= 72): a ring of two steps and the label-map path's LDS
        const bool paired = rg.wide && lm_path && rg.RQ <= 9 && lds <= 80 * 1024 && !tun(TUN_WIDE_UNPAIRED);
        if (score && lds > lds_cap) {               // the score tiles do not fit (beside a second workgroup): recurrence only
            score = false;
            lds = carve(false, false, false);
        }
        // the 16-bit image where the handle has one (an eligible model, build_half_image): the recurrence-only launch of the
        // destination split reads half the bytes with half the load instructions; FARNN_NOHALF=1 keeps the f32 blocks
        const bool half = dest && !score && m->Mf16 && m->Mb16 && !tun(TUN_NOHALF);
        // ... on a model whose o is absent or all ones it keeps `hist` in rows of RD_XS floats where that fits beside a second
        // workgroup (chain_dest.hip.h: one store per step, chain_regs_one_kernel); where it does not -- the longest sequences this
        // kernel takes -- rows of SP floats and two stores as before
        bool row80 = false;
        if (half && (!m->o || m->o_ones) && FARNN_STEP_ONESTORE && FARNN_CHAIN_HEAD) {
            const size_t lds80 = carve(false, false, true);
            if (lds80 <= lds_cap) { row80 = true; lds = lds80; }
        }
        if (lds <= lds_cap) {
            p.rec = (paired && score) ? REC_CHAIN_WIDE_PAIRED : rg.wide ? REC_CHAIN_WIDE : REC_CHAIN_REGS;
            p.fused = score; p.lm_path = lm_path; p.dest = dest; p.half = half; p.row80 = row80; p.lds = lds;
            p.host_epoch = score && tun(TUN_HOST_EPOCH);       // diagnostic A/B: the epoch as a kernel argument (not graph-capturable)
            return FARNN_OK;
        }
    }
    p.rec = REC_CHAIN_KERNEL;
    // ring shape: a whole step per phase when it fits, KS phases deep
    int ks = 2, nqp = g.NQ;
    if (!g.pick_ring(L, m->chain_ks, ks, nqp))
        return fail(FARNN_ERANGE, "chain kernel: LDS ring does not fit (sequence too long for this S)%s%s");
    p.KS = ks; p.NQP = nqp; p.PPS = (g.NQ + nqp - 1) / nqp;
    p.lds = g.lds_bytes(L, ks, nqp);
    p.block = (g.NW + g.NLD + 1) * 64;                          // compute + loader + writer wavefronts
    if (tun(TUN_CHAIN_HELPER) && p.block < 512) p.block += 64;  // experiment: an idle eighth wavefront
    const int fq_max = p.block <= 384 ? 6 : 3;
    p.FQ = (g.NCH == 1 && p.PPS == 1 && g.NQ <= fq_max && !tun(TUN_NOFAST)) ? g.NQ : 0;
    if (g.NCH > 4) return fail(FARNN_ERANGE, "unsupported state count%s%s");
    p.NCH = g.NCH <= 2 ? g.NCH : 4;
    return FARNN_OK;
}

// the dense-block recurrence followed by scores + decode: ONE launch (the decode is the chain kernel's epilogue) when
// the decode is the threshold/argmax one and the geometry allows it, else the chain kernel + the score / Viterbi kernels
static int plan_chain_and_decode(const farnn_model *m, TagPlan &p, bool flat, bool scores, bool offs, bool lm_tags, bool offs_ok) {
    // CRF decode: recurrence + scores + Viterbi in ONE launch (chain_viterbi.hip) where the register-fed recurrence applies and
    // the decode's LDS fits; else the recurrence kernel followed by the (fused score +) Viterbi kernel.
    // The one launch (north_star: "decode fused into the same kernel") exists for S <= 108 and is parity-tested, but is NOT the
    // default (round 5): a compute unit then holds BOTH chains of a sequence, which run 1 390 cycles per step there against
    // 780-960 when a long chain shares its unit with a short one, and the decode waits behind them.  Measured at K = 130,
    // 256 x 64: S = 71 77.7 us in one launch against 72.9 in two (round 4; round 5's recurrence kernel: 69), S = 104 113.8 against
    // 95.7 (profiles/r04_*, r05_*).  FARNN_CV_ONE=1 selects it.
    // The production library does not carry the form's 48 kernels: it lives in the A/B build (build.py --probes, -DFARNN_AB).
#if defined(FARNN_AB)
    if (tun(TUN_CV_ONE) && m->rgeom.ok && !tun(TUN_NOREGS) && !tun(TUN_NOFUSE) && viterbi_can_fuse(m, p.L, scores) && offs_ok &&
        chain_viterbi_fits(p.L, m->SP, m->rgeom.NP, m->K, m->Kp, m->lm.on != 0, m->rgeom.RQ)) {
        p.rec = REC_CHAIN_VITERBI; p.fused = true; p.dest = regs_dest(m);
        return FARNN_OK;
    }
#endif
    if (int rc = plan_chain(m, p, !m->use_crf, lm_tags, offs_ok)) return rc;
    return p.fused ? FARNN_OK : plan_score_decode(m, p, flat, scores, offs);
}

// the recurrence of the three decomposed kinds: the register kernel or the rows kernel when packed, else the older kernel
// fuse: ask for the one-launch form (scores + argmax decode beside the recurrence); p.fused tells whether the model's kernel
// and geometry allow it
static void plan_decomp_recurrence(const farnn_model *m, TagPlan &p, bool fuse, bool offs_ok) {
    if (m->rows.ok && regs_plan(m->rows, m->dw, p.L, p.regs)) {      // farnn = 0, rank <= 64: four wavefronts per chain, the packed rows in registers
        bool score = fuse && m->ws.hs && m->OTm && m->c16 >= 1 && m->c16 <= DG_NG && m->Kc <= 256 && p.L <= 31 * RG_TT &&
                     offs_ok && !tun(TUN_NOFUSE);
        if (score) {
            p.regs.lds_score = regs_score_lds(p.regs, p.L, m->SP, m->c16, m->Kc);
            if (p.regs.lds_score > 80 * 1024) score = false;
        }
        p.rec = REC_DECOMP_REGS; p.fused = score;
    } else if (m->rows.ok && rows_plan(m->rows, m->dw, p.B, p.L, p.rows)) {
        p.rec = REC_DECOMP_ROWS;
        p.rows_cu = (p.rows.form && !tun(TUN_ROWS_NOROUNDS)) ? m->n_cu : 0;      // (launch_rows_n: the register forms walk their groups in rounds)
    } else
        p.rec = REC_DECOMP_CHAIN;
}

static int plan_tag(const farnn_model *m, int B, int L, int full, bool flat, bool scores, TagPlan &p) {
    p = TagPlan();
    p.planned = true; p.B = B; p.L = L; p.full = full;
    // batch preparation: flat-output offsets and the length-sorted launch order (full mode runs
    // every sequence for L steps, so there is nothing to balance)
    p.want_order = !full && B > 2 && !tun(TUN_NOSORT);
    // the plain i-FST path needs no prep launch up to B = 1024: the chain workgroups select their sequence
    // by length rank themselves and the score workgroups sum the lengths in front of theirs
    p.prep_in_kernel = (m->kind == KIND_IFST || (m->kind == KIND_DECOMP && m->rows.ok)) && B <= 1024 && L <= 1023 && !tun(TUN_PREP);
    p.order_valid = p.want_order && !p.prep_in_kernel;
    p.sort_in_kernel = p.want_order && p.prep_in_kernel;
    // the decomposed independent=1 scoring kernel slices the batch by flat offsets even when no flat output is asked for
    p.want_offs = flat || (m->kind == KIND_DECOMP1 && m->d1_BSSp && !full);
    if ((p.want_offs || p.want_order) && !p.prep_in_kernel) {
        p.prep = B <= 1024 ? PREP_SMALL : PREP_LARGE;
        while (p.prep == PREP_SMALL && p.prep_G < 16 && B * p.prep_G * 2 <= 1024) p.prep_G *= 2;      // lanes per sequence
    }
    const bool offs = flat && !p.prep_in_kernel;            // the score stage is handed the prep launch's flat offsets
    const bool offs_ok = B <= 1024 || !flat || offs;        // (beyond 1 024 sequences no workgroup sums the lengths in front of its own)
    const bool lm_tags = m->lm.on && !m->P && !scores;      // bs_label_map_path of this call: the output matrix is a label map, tags only
    switch (m->kind) {
        case KIND_IFST:
            if (!m->compact_on) return plan_chain_and_decode(m, p, flat, scores, offs, lm_tags, offs_ok);
            if (L > 1024) return fail(FARNN_ERANGE, "compact recurrence: more than 1024 positions%s%s");
            // ONE launch (compact_tag.hip.h: both chains of a sequence in LDS, label-map scores, argmax decode) where it
            // applies; FARNN_NOFUSE=1: round 2's two launches
            if (m->bmTok && lm_tags && !m->use_crf && !tun(TUN_NOFUSE) && compact_tag_fits(m->V, m->S, L) && offs_ok) {
                p.rec = REC_COMPACT_TAG; p.fused = true;
                p.lds = (size_t)compact_tag_lds(L, m->bmNS).total * 4;
                p.nlk = m->nl == FARNN_NL_NONE ? 0 : m->nl == FARNN_NL_RELU ? 1 : 2;
                p.NW = (m->S + 31) / 32;                         // 32-bit words of a bitmap row in use
                return FARNN_OK;
            }
            p.rec = REC_COMPACT_CHAIN;
            return plan_score_decode(m, p, flat, scores, offs);
        case KIND_FST4:
        case KIND_IND1:
            p.score = m->kind == KIND_FST4 ? SCORE_FST4 : SCORE_IND1;
            return plan_chain(m, p, false, lm_tags, offs_ok);
        case KIND_DECOMP:
            if (m->dense_decomp) return plan_chain_and_decode(m, p, flat, scores, offs, lm_tags, offs_ok);
            if (m->sf_max) {
                // dense route: one block per token in front of the chain kernels, planned exactly like a dense_decomp id handle
                // with V = B L; beyond the workspace's cap (tag_create.hip.h), or with gates, the generic kernel on the padded copy
                if (m->sf_dense && (long long)B * L <= m->sf_block_tokens) {
                    p.blocks = true;
                    return plan_chain_and_decode(m, p, flat, scores, offs, lm_tags, offs_ok);
                }
                if (decomp_chain_lds_bytes(m->dw, L) > 160 * 1024)
                    return fail(FARNN_ERANGE, "tag_vectors: decomp_chain_kernel's LDS does not hold this model at this sequence length%s%s");
                p.rec = REC_DECOMP_CHAIN;
                p.table = true; p.table_cols = 0;
                return plan_score_decode(m, p, flat, scores, offs);
            }
            plan_decomp_recurrence(m, p, !m->use_crf, offs_ok);
            if (m->sf) {
                if (p.rec == REC_DECOMP_CHAIN)     // (decomp_chain_kernel is not served from the token table: include/farnn.h)
                    return fail(FARNN_ERANGE, "tag_vectors: no packed-rows form holds this model at this sequence length%s%s");
                p.table = true; p.table_cols = sf_row_floats(m) - m->Rp;
            }
            return p.fused ? FARNN_OK : plan_score_decode(m, p, flat, scores, offs);
        case KIND_DECOMP0:
            // the score kernel's tile and its static tokid[] share the workgroup's 160 KiB: refused here, before anything is launched
            // (at exactly 160 KiB of tile the launcher's hipFuncSetAttribute failed behind the recurrence, with a HIP error)
            if (int rc = lds_fits(decomp0_score_lds_bytes(m->SP, m->Rp, m->RWp, m->Kc) + D0_STATIC_LDS)) return rc;
            plan_decomp_recurrence(m, p, false, offs_ok);
            p.score = SCORE_DECOMP0;
            return m->use_crf ? plan_viterbi(m, p, false) : FARNN_OK;
        case KIND_DECOMP1: {
            p.score = SCORE_DECOMP1;
            const int MT = (m->S + 15) / 16, NT = (m->RO + 15) / 16;
            p.d1_mfma = m->d1_BSSp && m->ws.d1_br && decomp1_mfma_lds_bytes(MT, NT) <= 80 * 1024;
            if (p.d1_mfma && NT > 5) return fail(FARNN_ERANGE, "decomp_ind1: output rank above 80 on the MFMA path%s%s");
            // its label kernel: one 16-wavefront workgroup per CU when the weights fit in LDS beside the per-wavefront rows
            p.d1_staged = p.d1_mfma && decomp1_label_lds_bytes(NT * 16, m->RO, m->K, m->Kc, true, 16) <= 150 * 1024;
            if (m->dense_decomp) {
                if (int rc = plan_chain(m, p, false, lm_tags, offs_ok)) return rc;
            } else {
                p.rec = REC_DECOMP_CHAIN;
                p.order_valid = false;                           // (this kind's decomp_chain launch walks the batch in order)
            }
            return m->use_crf ? plan_viterbi(m, p, false) : FARNN_OK;
        }
        default:
            return fail(FARNN_EINVAL, "tag: unknown model kind%s%s");
    }
}

// What the reporting functions answer while no call has been planned (a new handle, or farnn_set_compact changed its form): the
// recurrence kernel the model's kind defaults to, nothing fused.
static TagPlan unplanned(const farnn_model *m) {
    TagPlan p;
    const bool decomp = !m->dense_decomp && (m->kind == KIND_DECOMP || m->kind == KIND_DECOMP1 || m->kind == KIND_DECOMP0);
    p.rec = m->compact_on ? REC_COMPACT_CHAIN : !decomp ? REC_CHAIN_KERNEL : !m->rows.ok ? REC_DECOMP_CHAIN
            : (m->dw.farnn == 0 && m->dw.R <= DG_ROWS && !tun(TUN_DECOMP_NOREGS)) ? REC_DECOMP_REGS : REC_DECOMP_ROWS;
    return p;
}

extern "C" const char *farnn_kernel_name(const farnn_model *m, int32_t which) {
    if (!m) return "";
    TunScope tun_scope(&m->tun);
    const TagPlan p = m->plan.planned ? m->plan : unplanned(m);
    switch (which) {
        case KERN_CHAIN:
            switch (p.rec) {
                case REC_COMPACT_TAG: return "compact_tag_kernel<fused: both chains + label-map scores + decode>";
                case REC_COMPACT_CHAIN: return "compact_chain_kernel";
                case REC_CHAIN_VITERBI: return "chain_viterbi_kernel<fused: recurrence + scores + CRF decode>";
                case REC_CHAIN_WIDE:
                case REC_CHAIN_WIDE_PAIRED: return p.fused ? "chain_wide_kernel<fused: scores + decode beside the recurrence>" : "chain_wide_kernel";
                case REC_CHAIN_REGS: return p.fused ? "chain_regs_kernel<fused: scores + decode beside the recurrence>"
                                                    : (p.half ? "chain_regs_kernel<f16 blocks>" : "chain_regs_kernel");
                case REC_DECOMP_REGS: return p.fused ? "decomp_regs_kernel<fused: scores + decode beside the recurrence>" : "decomp_regs_kernel";
                case REC_DECOMP_ROWS: {      // (a vector-input handle reports the form too; the id handles' name is what it always was)
                    static const char *const forms[] = {"decomp_rows_kernel<form 0>", "decomp_rows_kernel<form 1>", "decomp_rows_kernel<form 2>",
                        "decomp_rows_kernel<form 3>", "decomp_rows_kernel<form 4>", "decomp_rows_kernel<form 5>", "decomp_rows_kernel<form 6>",
                        "decomp_rows_kernel<form 7>", "decomp_rows_kernel<form 8>", "decomp_rows_kernel<form 9>", "decomp_rows_kernel<form 10>"};
                    return (m->sf && p.rows.form >= 0 && p.rows.form <= 10) ? forms[p.rows.form] : "decomp_rows_kernel";
                }
                case REC_DECOMP_CHAIN: return "decomp_chain_kernel";
                default: return "chain_kernel";
            }
        // the score slot is named by the model's kind, whatever the last call launched; m->last_lm_score (tag_host.hip.h) is the one
        // remembered field beside the plan
        case KERN_SCORE: return m->kind == KIND_FST4 ? "fst4_score_kernel"
                              : (m->kind == KIND_IND1 ? "ind1_score_kernel"
                              : (m->kind == KIND_DECOMP1 ? (m->d1_BSSp ? "decomp1_br_mfma_kernel+decomp1_label_kernel" : "decomp1_score_kernel")
                              : (m->kind == KIND_DECOMP0 ? "decomp0_score_kernel"
                              : (m->use_crf ? "score_tile_kernel+viterbi_kernel" : (m->last_lm_score ? "label_map_score_kernel" : "score_tile_kernel")))));
        case KERN_PREP:  return "batch_prep_kernel";
        case KERN_TABLE: return !m->sf ? "" : p.blocks ? "token_blocks_kernel" : "token_table_kernel";
        default: return "";
    }
}

// ---- the hot path: launch from the plan -----------------------------------------------------------
// The helpers below fill parameter structs from the model and the plan, and launch; none of them decides anything.

// template selection, in the style of with_chain_slots (train_host.hip.h)
template <typename F>
static int with_chain_form(int nch, int fq, F &&go) {          // chain_kernel<NCH, _, FQ>: the fast-path widths exist for NCH = 1 only
    if (nch == 2) return go(int_c<2>(), int_c<0>());
    if (nch == 4) return go(int_c<4>(), int_c<0>());
    return fq == 1 ? go(int_c<1>(), int_c<1>()) : fq == 2 ? go(int_c<1>(), int_c<2>()) : fq == 3 ? go(int_c<1>(), int_c<3>())
         : fq == 4 ? go(int_c<1>(), int_c<4>()) : fq == 5 ? go(int_c<1>(), int_c<5>()) : fq == 6 ? go(int_c<1>(), int_c<6>())
         : go(int_c<1>(), int_c<0>());
}
template <typename F>
static int with_hist_ib4(int ib4, F &&go) {                    // viterbi_hist_kernel<IB4, _>: K / 32 = 0 .. 6
    return ib4 == 0 ? go(int_c<0>()) : ib4 == 1 ? go(int_c<1>()) : ib4 == 2 ? go(int_c<2>()) : ib4 == 3 ? go(int_c<3>())
         : ib4 == 4 ? go(int_c<4>()) : ib4 == 5 ? go(int_c<5>()) : go(int_c<6>());
}
template <typename F>
static int with_score_columns(int kch, F &&go) {               // score_tile_kernel<KCH>: 64-column chunks of the scores, 1 .. 4
    return kch == 1 ? go(int_c<1>()) : kch == 2 ? go(int_c<2>()) : kch == 3 ? go(int_c<3>()) : go(int_c<4>());
}
template <typename F>
static int with_bitmap_words(int nw, F &&go) {                 // compact_tag_kernel<NW, _>: 32-bit words of a bitmap row, 1 .. 4
    return nw <= 1 ? go(int_c<1>()) : nw == 2 ? go(int_c<2>()) : nw == 3 ? go(int_c<3>()) : go(int_c<4>());
}

static ScoreParams make_score_params(farnn_model *m, const TagPlan &pl, const int64_t *len, int32_t *tags, int64_t *flat, float *scores) {
    ScoreParams p;
    memset(&p, 0, sizeof(p));
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.OT = m->OT; p.OTm = m->OTm; p.c16 = m->c16; p.P = m->P; p.trT = m->tr; p.len = len;
    p.offs = (flat && !pl.prep_in_kernel) ? m->ws.offs : nullptr; p.tags = tags; p.flat = flat; p.scores = scores;
    p.crf_scores = m->ws.crf_scores;
    p.B = pl.B; p.L = pl.L; p.S = m->S; p.SP = m->SP; p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.kch = m->Kc / 64;
    p.full = pl.full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    p.dbg = tun(TUN_DBG);
    p.kz = (m->kind == KIND_IFST && m->use_crf && !tun(TUN_NOKZ)) ? m->C : 0;      // the library appended the two zero rows itself
    p.lm = m->lm;
    return p;
}

// The register-fed recurrence (chain_regs_params.hip.h), with the scores + decode beside it when the plan fused them.
// The hand-off words of the one-launch forms (chain_regs.hip.h / decomp_regs.hip.h + beside.hip.h) and their launch counter:
// a launch's epoch is (the counter >> BS_EPOCH_SHIFT) + 1, read from device memory by the kernel; every launch adds exactly
// BS_EPOCH_SPAN to the counter whatever its batch size (beside.hip.h, bs_launch_epoch).  Nothing per launch comes from the host and
// nothing is ever reset: the step replays from a HIP graph as the very same launch, and graphs captured at different batch sizes
// and eager calls may interleave on a handle (stream-ordered).  The words are zeroed once, when the workspace is allocated.
static void handoff_words(farnn_model *m, unsigned long long **prog, unsigned long long **arr, unsigned long long **done) {
    *prog = m->ws.hs; *arr = m->ws.hs + (size_t)2 * m->ws.B; *done = m->ws.hs + (size_t)3 * m->ws.B + 16;      // (the counter on a 128-byte line of its own)
}

static int launch_chain_regs_form(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, const ScoreParams &sp, hipStream_t s) {
    const RegsGeom &rg = m->rgeom;
    const bool mx = m->semiring == FARNN_SEMIRING_MAX;
    RegsParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.Mf = pl.blocks ? m->ws.tbf : m->Mf; rp.Mb = pl.blocks ? m->ws.tbb : m->Mb; rp.blk = (long long)m->geom.SR * m->SP;
    rp.o = m->o; rp.h0 = m->h0; rp.hT = m->hT; rp.x = x; rp.len = len;
    rp.order = pl.order_valid ? m->ws.order : nullptr; rp.sort = pl.sort_in_kernel ? 1 : 0;
    rp.A = m->ws.A; rp.Bk = m->ws.Bk; rp.B = pl.B; rp.L = pl.L; rp.S = m->S; rp.SP = m->SP; rp.CPR = rg.CPR; rp.V = pl.blocks ? pl.B * pl.L : m->V;
    rp.G = rg.G; rp.RPG = rg.RPG; rp.RQ = rg.RQ; rp.D = rg.D; rp.PS = rg.PS; rp.pair = rg.wide ? 0 : 1;
    rp.nl = m->nl; rp.full = pl.full; rp.dbg = tun(TUN_DBG);
    rp.dest = pl.dest ? 1 : 0; rp.half = pl.half ? 1 : 0; rp.row80 = pl.row80 ? 1 : 0;          // chain_dest.hip.h
    rp.Mf16 = m->Mf16; rp.Mb16 = m->Mb16; rp.blk16 = (long long)m->SP * RD_XS * 2;              // (null: no image, build_half_image)
    rp.o_ones = (!m->o || m->o_ones) ? 1 : 0;                                                    // (build_output_matrix)
    if (pl.fused && pl.rec != REC_CHAIN_VITERBI) {
        handoff_words(m, &rp.prog, &rp.arr, &rp.done);
        if (pl.host_epoch) {
            if (++m->epoch_u == 0) { FARNN_HIP_TRY(hipMemsetAsync(m->ws.hs, 0, m->ws.hs_bytes, s)); m->epoch_u = 1; }
            rp.done = nullptr; rp.epoch_host = m->epoch_u + 0x40000000u;
        }
        rp.spin = tun(TUN_FUSE_SPIN);
        rp.solo_margin = tun(TUN_SOLO_MARGIN);
        rp.sp = sp;
    }
    KernelTimer kt(m, KERN_CHAIN, s, /*ext=*/true);
#if defined(FARNN_AB)
    if (pl.rec == REC_CHAIN_VITERBI) return launch_chain_viterbi(rp, sp, mx, s, kt.e0, kt.e1);
#endif
    if (pl.rec == REC_CHAIN_WIDE_PAIRED) {
        rp.D = 2; rp.pair = 1;
        return launch_chain_wide_paired(rp, mx, s, kt.e0, kt.e1);
    }
    return pl.rec == REC_CHAIN_WIDE ? launch_chain_wide(rp, mx, pl.fused, s, kt.e0, kt.e1) : launch_chain_regs(rp, mx, pl.fused, s, kt.e0, kt.e1);
}

static int launch_chain_kernel(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, hipStream_t s) {
    const ChainGeom &g = m->geom;
    ChainParams p;
    p.Mf = pl.blocks ? m->ws.tbf : m->Mf; p.Mb = pl.blocks ? m->ws.tbb : m->Mb; p.blk = (long long)m->geom.SR * m->SP;
    p.o = m->o; p.h0 = m->h0; p.hT = m->hT; p.x = x; p.len = len; p.A = m->ws.A; p.Bk = m->ws.Bk;
    p.order = pl.order_valid ? m->ws.order : nullptr;
    p.sort = pl.sort_in_kernel ? 1 : 0;
    p.B = pl.B; p.L = pl.L; p.S = m->S; p.SP = m->SP; p.CPR = g.CPR; p.V = pl.blocks ? pl.B * pl.L : m->V;
    p.NW = g.NW; p.NLD = g.NLD; p.G = g.G; p.LPR = g.LPR; p.RPG = g.RPG; p.RPGp = g.RPGp; p.NQ = g.NQ;
    p.nl = m->nl; p.full = pl.full; p.dbg = tun(TUN_DBG);
    p.KS = pl.KS; p.NQP = pl.NQP; p.PPS = pl.PPS;
    const dim3 grid(2 * pl.B), block(pl.block);
    const bool mx = m->semiring == FARNN_SEMIRING_MAX;
    KernelTimer kt(m, KERN_CHAIN, s, /*ext=*/true);
    const int rc = with_chain_form(pl.NCH, pl.FQ, [&](auto NCH, auto FQ) {
        return mx ? launch_timed(chain_kernel<NCH(), true, FQ()>, grid, block, pl.lds, s, kt.e0, kt.e1, p)
                  : launch_timed(chain_kernel<NCH(), false, FQ()>, grid, block, pl.lds, s, kt.e0, kt.e1, p);
    });
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// the compact handle's recurrence: compact_tag_kernel (the call's one launch) or compact_chain_kernel
static int launch_compact(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, const ScoreParams &sp, hipStream_t s) {
    CompactParams cp;
    cp.bitsF = m->bmF; cp.bitsB = m->bmB; cp.wF = m->bmWF; cp.wB = m->bmWB; cp.o = m->o; cp.h0 = m->h0; cp.hT = m->hT;
    cp.mF = m->bmMF; cp.mB = m->bmMB; cp.xF = m->bmXF; cp.xB = m->bmXB; cp.tokoff = m->bmTok;
    cp.x = x; cp.len = len; cp.order = pl.order_valid ? m->ws.order : nullptr; cp.A = m->ws.A; cp.Bk = m->ws.Bk;
    cp.B = pl.B; cp.L = pl.L; cp.S = m->S; cp.SP = m->SP; cp.V = m->V; cp.nl = m->nl; cp.full = pl.full; cp.dbg = tun(TUN_DBG);
    KernelTimer kt(m, KERN_CHAIN, s);
    if (pl.rec == REC_COMPACT_CHAIN) return launch_compact_chain(cp, m->bmNS, s);
    const int rc = with_bitmap_words(pl.NW, [&](auto NW) {
        const dim3 grid(pl.B), block(CT_WAVES * 64);
        if (pl.nlk == 0) return launch(compact_tag_kernel<NW(), 0>, grid, block, pl.lds, s, cp, sp);
        if (pl.nlk == 1) return launch(compact_tag_kernel<NW(), 1>, grid, block, pl.lds, s, cp, sp);
        return launch(compact_tag_kernel<NW(), 2>, grid, block, pl.lds, s, cp, sp);
    });
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// the recurrence of the decomposed kinds
static int launch_decomp_recurrence(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, const ScoreParams &sp, hipStream_t s) {
    const int *order = pl.order_valid ? m->ws.order : nullptr;
    const int sort = pl.sort_in_kernel ? 1 : 0;
    // a vector-input call: the same kernels on the call's token table -- its rows in place of the per-word rows, one "word" per position
    DecompWeights dw = m->dw;
    DecompRowsPack rows = m->rows;
    if (pl.table) { dw.V = pl.B * pl.L; dw.Vgen = m->ws.tt; rows.TVt = m->ws.tt; }
    KernelTimer kt(m, KERN_CHAIN, s);
    if (pl.rec == REC_DECOMP_ROWS)
        return launch_decomp_rows(rows, dw, pl.rows, x, len, order, sort, m->ws.A, m->ws.Bk, pl.B, pl.L, pl.full, pl.rows_cu, s);
    if (pl.rec == REC_DECOMP_CHAIN) return launch_decomp_chain(dw, x, len, order, m->ws.A, m->ws.Bk, pl.B, pl.L, pl.full, s);
    BesideParams bs;
    if (pl.fused) {
        memset(&bs, 0, sizeof(bs));
        bs.A = m->ws.A; bs.Bk = m->ws.Bk; bs.B = pl.B; bs.L = pl.L; bs.SP = m->SP; bs.CPR = m->SP / 4;
        handoff_words(m, &bs.prog, &bs.arr, &bs.done);
        bs.spin = tun(TUN_FUSE_SPIN); bs.dbg = tun(TUN_DBG); bs.sp = sp;
    }
    return launch_decomp_regs(rows, dw, pl.regs, x, len, order, sort, m->ws.A, m->ws.Bk, pl.B, pl.L, pl.full, s, pl.fused ? &bs : nullptr);
}

static int launch_recurrence(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, const ScoreParams &sp, hipStream_t s) {
    switch (pl.rec) {
        case REC_COMPACT_TAG:
        case REC_COMPACT_CHAIN: return launch_compact(m, pl, x, len, sp, s);
        case REC_CHAIN_KERNEL: return launch_chain_kernel(m, pl, x, len, s);
        case REC_DECOMP_REGS:
        case REC_DECOMP_ROWS:
        case REC_DECOMP_CHAIN: return launch_decomp_recurrence(m, pl, x, len, sp, s);
        default: return launch_chain_regs_form(m, pl, x, len, sp, s);
    }
}

static int launch_viterbi(farnn_model *m, const TagPlan &pl, const ScoreParams &p, hipStream_t s) {
    int rc;
    const int B = pl.B;
    if (pl.viterbi == VITERBI_HIST) {
        const bool fused = pl.score == SCORE_VITERBI_FUSED;
        const int threads = viterbi_hist_score_threads(m->K, fused);
        rc = with_hist_ib4(pl.ib4, [&](auto N) {
            return fused ? launch(viterbi_hist_kernel<N(), true>, dim3(B), dim3(threads), pl.viterbi_lds, s, p)
                         : launch(viterbi_hist_kernel<N(), false>, dim3(B), dim3(threads), pl.viterbi_lds, s, p);
        });
    } else {
        const int threads = round_up(4 * m->K, 64);
        auto go = [&](auto N) { return launch(viterbi_kernel<N()>, dim3(B), dim3(threads), pl.viterbi_lds, s, p); };
        if (pl.ib4 == 2) rc = go(int_c<2>());            // K <= 32
        else if (pl.ib4 == 4) rc = go(int_c<4>());       // K <= 64
        else if (pl.ib4 == 9) rc = go(int_c<9>());       // K <= 144
        else if (pl.ib4 == 13) rc = go(int_c<13>());     // K <= 208
        else rc = go(int_c<16>());                       // K <= 256
    }
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// the Viterbi launch behind the score kernels of the decomposed independent=0 / independent=1 models (they left the emissions in crf_scores)
static int launch_viterbi_tail(farnn_model *m, const TagPlan &pl, const int64_t *len, int32_t *tags, int64_t *flat, hipStream_t s) {
    ScoreParams v;
    memset(&v, 0, sizeof(v));
    v.trT = m->tr; v.len = len; v.offs = flat ? m->ws.offs : nullptr; v.tags = tags; v.flat = flat;
    v.crf_scores = m->ws.crf_scores; v.B = pl.B; v.L = pl.L; v.K = m->K; v.Kp = m->Kp;
    v.full = pl.full; v.use_crf = 1; v.o_idx = m->o_idx; v.threshold = m->threshold;
    return launch_viterbi(m, pl, v, s);
}

static int launch_decomp1_score(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len,
                                int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    const int B = pl.B, full = pl.full;
    Decomp1ScoreParams p;
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.Vgen = m->dw.Vgen; p.S1 = m->dw.S1; p.S2 = m->dw.S2; p.W = m->dw.W;
    p.S1o = m->d1_S1o; p.S2o = m->d1_S2o; p.CoutT = m->d1_CoutT; p.P = m->P;
    p.x = x; p.len = len; p.offs = flat ? m->ws.offs : nullptr;
    p.tags = tags; p.flat = flat; p.scores = scores; p.crf_scores = m->ws.crf_scores;
    p.B = B; p.L = pl.L; p.S = m->S; p.SP = m->SP; p.R = m->R; p.Rp = m->Rp; p.RO = m->RO; p.ROp = m->ROp;
    p.V = m->V;
    p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.full = full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    int rc;
    KernelTimer kt(m, KERN_SCORE, s);
    if (pl.d1_mfma) {
        Decomp1MfmaParams qm;
        qm.base = p; qm.BSSp = m->d1_BSSp; qm.S1oP = m->d1_S1oP; qm.S2oP = m->d1_S2oP; qm.br = m->ws.d1_br;
        if (!full) qm.base.offs = m->ws.offs;       // farnn_tag computes the flat offsets for this path even without flat output
        qm.MT = (m->S + 15) / 16; qm.NT = (m->RO + 15) / 16; qm.KQ4 = (m->S + 15) / 16;
        const size_t mlds = decomp1_mfma_lds_bytes(qm.MT, qm.NT);
        // persistent: two workgroups per CU, every wavefront owns a contiguous slice of the live tokens
        const int nwg = std::min(2 * m->n_cu, (B * p.L + 3) / 4);
        auto go = [&](auto N) { return launch(decomp1_br_mfma_kernel<N()>, dim3(nwg), dim3(256), mlds, s, qm); };
        switch (qm.NT) {
            case 1: rc = go(int_c<1>()); break;
            case 2: rc = go(int_c<2>()); break;
            case 3: rc = go(int_c<3>()); break;
            case 4: rc = go(int_c<4>()); break;
            default: rc = go(int_c<5>()); break;
        }
        if (rc) return rc;
        FARNN_HIP_TRY(hipGetLastError());
        const int NC = qm.NT * 16;
        const bool staged = pl.d1_staged;
        const int lthreads = staged ? 1024 : 256;
        const size_t llds = decomp1_label_lds_bytes(NC, m->RO, m->K, m->Kc, staged, lthreads / 64);
        const int lgrid = std::min((staged ? 1 : 4) * m->n_cu, (B * p.L + lthreads / 64 - 1) / (lthreads / 64));
        if (staged) {
            if ((rc = raise_lds_limit(decomp1_label_kernel<true>, llds))) return rc;
            decomp1_label_kernel<true><<<dim3(lgrid), dim3(lthreads), llds, s>>>(p, m->ws.d1_br, NC, qm.MT, full ? nullptr : m->ws.offs);
        } else {
            decomp1_label_kernel<false><<<dim3(lgrid), dim3(lthreads), llds, s>>>(p, m->ws.d1_br, NC, qm.MT, full ? nullptr : m->ws.offs);
        }
    } else {
        const size_t lds = decomp1_score_lds_bytes(m->S, m->SP, m->Rp, m->ROp, m->Kc);
        if ((rc = raise_lds_limit(decomp1_score_kernel, lds))) return rc;
        decomp1_score_kernel<<<dim3(p.L, B), dim3(256), lds, s>>>(p);
    }
    FARNN_HIP_TRY(hipGetLastError());
    return pl.viterbi ? launch_viterbi_tail(m, pl, len, tags, flat, s) : FARNN_OK;
}

static int launch_decomp0_score(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len,
                                int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    Decomp0ScoreParams p;
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.Vgen = m->d0_Vgen; p.S1 = m->dw.S1; p.S2 = m->dw.S2; p.CT = m->d0_CT;
    p.S1w = m->d0_S1w; p.S2w = m->d0_S2w; p.CwT = m->d0_CwT; p.P = m->P;
    p.x = x; p.len = len; p.offs = flat ? m->ws.offs : nullptr;
    p.tags = tags; p.flat = flat; p.scores = scores; p.crf_scores = m->ws.crf_scores;
    p.B = pl.B; p.L = pl.L; p.S = m->S; p.SP = m->SP; p.R = m->R; p.Rp = m->Rp; p.RW = m->RW; p.RWp = m->RWp;
    p.V = m->V;
    p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.full = pl.full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    const size_t lds = decomp0_score_lds_bytes(m->SP, m->Rp, m->RWp, m->Kc);
    if (int rc = raise_lds_limit(decomp0_score_kernel, lds)) return rc;
    KernelTimer kt(m, KERN_SCORE, s);
    decomp0_score_kernel<<<dim3((p.L + D0_TOK - 1) / D0_TOK, pl.B), dim3(256), lds, s>>>(p);
    FARNN_HIP_TRY(hipGetLastError());
    return pl.viterbi ? launch_viterbi_tail(m, pl, len, tags, flat, s) : FARNN_OK;
}

// the score / decode launch(es) behind the recurrence; one KERN_SCORE timer around whatever runs here
static int launch_score(farnn_model *m, const TagPlan &pl, const int64_t *x, const int64_t *len, const ScoreParams &p,
                        int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    switch (pl.score) {
        case SCORE_NONE: return FARNN_OK;
        case SCORE_DECOMP1: return launch_decomp1_score(m, pl, x, len, tags, flat, scores, s);
        case SCORE_DECOMP0: return launch_decomp0_score(m, pl, x, len, tags, flat, scores, s);
        default: break;
    }
    KernelTimer kt(m, KERN_SCORE, s);
    switch (pl.score) {
        case SCORE_VITERBI_FUSED: return launch_viterbi(m, pl, p, s);
        case SCORE_LABEL_MAP:
            label_map_score_kernel<LMS_WAVES><<<pl.B, LMS_WAVES * 64, 0, s>>>(p);
            FARNN_HIP_TRY(hipGetLastError());
            return FARNN_OK;
        case SCORE_FST4:
        case SCORE_IND1:
            return launch_fst4_score(pl.score == SCORE_FST4 ? m->A4 : m->Ms, m->ws.A, m->ws.Bk, m->P, x, len, flat ? m->ws.offs : nullptr,
                                     tags, flat, scores, pl.B, pl.L, m->S, m->SP, m->C, m->Kc, pl.full,
                                     m->o_idx, m->threshold, pl.score == SCORE_FST4 ? nullptr : m->Oten, m->V, s);
        default: break;
    }
    const size_t lds = score_lds_bytes(m->S, m->Kc);
    const dim3 grid((p.L + SCORE_TT - 1) / SCORE_TT, pl.B), block(SCORE_WAVES * 64);
    const int rc = with_score_columns(pl.kch, [&](auto KCH) { return launch(score_tile_kernel<KCH()>, grid, block, lds, s, p); });
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return pl.viterbi ? launch_viterbi(m, pl, p, s) : FARNN_OK;
}

// forward_RE's view of the scores (model_onehot.py:153-154): the `oo` column (the last one) capped at the threshold
__global__ void clamp_oo_column_kernel(float *scores, long long rows, int K, int col, float threshold) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) {                                  // torch.min: a NaN score stays a NaN (fminf would turn it into the threshold)
        const float x = scores[r * K + col];
        scores[r * K + col] = (x < threshold || x != x) ? x : threshold;
    }
}

// the token table of a vector-input call (decomp_vec.hip.h)
static int launch_table(farnn_model *m, const TagPlan &pl, const float *v, const int64_t *len, hipStream_t s) {
    TokenTableParams p;
    p.v = v; p.len = len; p.Wrs1 = m->dw.Wrs1; p.bs1 = m->dw.bs1; p.Wrs2 = m->dw.Wrs2; p.bs2 = m->dw.bs2; p.TT = m->ws.tt;
    p.B = pl.B; p.L = pl.L; p.R = m->R; p.Rp = m->Rp; p.S = m->S; p.SP = m->SP; p.tvl = sf_row_floats(m); p.ncols = pl.table_cols;
    KernelTimer kt(m, KERN_TABLE, s);
    return launch_token_table(p, s);
}

// the token blocks of a max-semiring vector-input call on the dense route (decomp_vec.hip.h)
static int launch_blocks(farnn_model *m, const TagPlan &pl, const float *v, const int64_t *len, hipStream_t s) {
    TokenBlocksParams p;
    memset(&p, 0, sizeof(p));
    p.v = v; p.len = len; p.S1T = m->dw.S1T; p.S2T = m->dw.S2T; p.W = m->dw.W; p.Mf = m->ws.tbf; p.Mb = m->ws.tbb;
    p.B = pl.B; p.L = pl.L; p.R = m->R; p.S = m->S; p.SP = m->SP; p.SR = m->geom.SR;
    KernelTimer kt(m, KERN_TABLE, s);
    return launch_token_blocks(p, s);
}

// order the streams, reserve, plan, then launch from the plan: prep, (token table,) recurrence, scores + decode
// v != nullptr: farnn_tag_vectors -- x is ignored, the recurrence runs on the workspace's identity ids
static int tag_impl(farnn_model *m, const int64_t *x, const int64_t *lengths, int32_t B, int32_t L,
                    int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream, const float *v = nullptr) {
    TunScope tun_scope(&m->tun);
    FARNN_HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    // One workspace per handle: two calls on different streams (a forward_score on torch's stream while batches submitted
    // through farnn_tag_host_submit are in flight on the handle's own stream, ...) would race on the stash and on the
    // hand-off words.  A stream switch costs one event: recorded NOW on the previous call's stream (i.e. behind all its work),
    // awaited by this call's stream.  Calls that stay on one stream pay nothing.
    // The FIRST switch records the event on the previous call's stream (which must still exist: include/farnn.h); from then on
    // the caller is known to alternate streams and every call leaves the handle's event behind itself on its OWN stream, so the
    // previous stream is never touched again.  A call that is being captured into a graph is not ordered against other streams.
    hipStreamCaptureStatus cap_ = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cap_) != hipSuccess || cap_ != hipStreamCaptureStatusNone;
    if (m->have_last && m->last_stream != s && !capturing) {
        if (!m->ev_order) FARNN_HIP_TRY(hipEventCreateWithFlags(&m->ev_order, hipEventDisableTiming));
        if (!m->multi_stream) FARNN_HIP_TRY(hipEventRecord(m->ev_order, m->last_stream));
        FARNN_HIP_TRY(hipStreamWaitEvent(s, m->ev_order, 0));
        m->multi_stream = true;
    }
    m->last_stream = s; m->have_last = true;
    struct LeaveEvent {            // (multi-stream callers only) the handle's event behind this call's work, on this call's stream
        farnn_model *m; hipStream_t s; bool on;
        ~LeaveEvent() { if (on && m->ev_order) (void)hipEventRecord(m->ev_order, s); }
    } leave_event{m, s, m->multi_stream && !capturing};
    // the workspace arrays are strided with the CALL's L (every kernel writes whatever it later reads, pad columns
    // included), so (B, L) only have to fit the capacity: a loop whose batches vary in size or length allocates once
    if (B > m->ws.B || L > m->ws.L)
        if ((rc = farnn_reserve(m, B, L))) return rc;
    m->prof_this_call = m->profiling > 0 && (m->calls++ % m->profiling) == 0;
    if (m->n_cu <= 0) m->n_cu = device_cus(m->device);
    TagPlan pl;
    if ((rc = plan_tag(m, B, L, mode == FARNN_MODE_FULL, flat_tags != nullptr, scores != nullptr, pl))) return rc;
    m->plan = pl;
    if (pl.score == SCORE_LABEL_MAP || pl.score == SCORE_TILE) m->last_lm_score = pl.score == SCORE_LABEL_MAP;
    if (pl.prep != PREP_NONE) {
        KernelTimer kt(m, KERN_PREP, s);
        int64_t *offs = pl.want_offs ? m->ws.offs : nullptr;
        int *order = pl.want_order ? m->ws.order : nullptr;
        if (pl.prep == PREP_SMALL) batch_prep_small_kernel<<<1, round_up(B * pl.prep_G, 64), 0, s>>>(lengths, offs, order, B, L, pl.prep_G);
        else batch_prep_kernel<<<1, 1024, (size_t)(L + 2) * sizeof(int), s>>>(lengths, offs, order, B, L);
        FARNN_HIP_TRY(hipGetLastError());
    }
    const ScoreParams sp = make_score_params(m, pl, lengths, tags, flat_tags, scores);
    if (pl.table || pl.blocks) {
        if ((rc = pl.blocks ? launch_blocks(m, pl, v, lengths, s) : launch_table(m, pl, v, lengths, s))) return rc;
        x = m->ws.ids;
    }
    if ((rc = launch_recurrence(m, pl, x, lengths, sp, s))) return rc;
    return launch_score(m, pl, x, lengths, sp, tags, flat_tags, scores, s);
}

extern "C" int farnn_tag(farnn_model *m, const int64_t *x, const int64_t *lengths, int32_t B, int32_t L,
                         int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream) {
    if (!m || !x || !lengths) return fail(FARNN_EINVAL, "tag: null model / x / lengths%s%s");
    if (B <= 0 || L <= 0) return fail(FARNN_EINVAL, "tag: B and L must be positive%s%s");
    if (mode != FARNN_MODE_LOCAL && mode != FARNN_MODE_FULL && mode != FARNN_MODE_RE)
        return fail(FARNN_EINVAL, "tag: bad mode%s%s");
    if (m->sf) return fail(FARNN_EINVAL, "tag: this handle takes vectors, not word ids (farnn_decomp_sf_create / farnn_decomp_sf_max_create): call farnn_tag_vectors%s%s");
    if (mode != FARNN_MODE_RE) return tag_impl(m, x, lengths, B, L, mode, tags, flat_tags, scores, stream);
    if (m->kind != KIND_IFST && m->kind != KIND_FST4 && m->kind != KIND_IND1)
        return fail(FARNN_EINVAL, "tag: FARNN_MODE_RE exists on the onehot models only (model_onehot.py:148)%s%s");
    int rc = tag_impl(m, x, lengths, B, L, FARNN_MODE_FULL, tags, flat_tags, scores, stream);
    if (rc || !scores) return rc;
    const long long rows = (long long)B * L;
    clamp_oo_column_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        scores, rows, m->K, m->C - 1, m->threshold);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

extern "C" int farnn_tag_vectors(farnn_model *m, const float *v, const int64_t *lengths, int32_t B, int32_t L,
                                 int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream) {
    if (!m || !v || !lengths) return fail(FARNN_EINVAL, "tag_vectors: null model / v / lengths%s%s");
    if (B <= 0 || L <= 0) return fail(FARNN_EINVAL, "tag_vectors: B and L must be positive%s%s");
    if (!m->sf) return fail(FARNN_EINVAL, "tag_vectors: this handle takes word ids (only farnn_decomp_sf_create makes a vector-input handle): call farnn_tag%s%s");
    if (mode != FARNN_MODE_LOCAL)
        return fail(FARNN_EINVAL, "tag_vectors: FARNN_MODE_LOCAL only (forward_score / forward_RE exist on the onehot models only)%s%s");
    if ((long long)B * L > 0x7fffffffLL) return fail(FARNN_ERANGE, "tag_vectors: more than 2^31 - 1 positions%s%s");
    return tag_impl(m, nullptr, lengths, B, L, mode, tags, flat_tags, scores, stream, v);
}

static void host_slot_free(farnn_model::HostSlot &h) {
    if (h.x_pin) (void)hipHostFree(h.x_pin);
    if (h.flat_pin) (void)hipHostFree(h.flat_pin);
    if (h.x_dev) (void)hipFree(h.x_dev);
    h.x_pin = h.flat_pin = h.x_dev = h.flat_dev = h.x_map = nullptr;
    h.capN = h.capB = 0;
}

// One stream, in order, no copy engine: a staging kernel pulls [x | lengths] out of mapped pinned memory, the tagging launch
// stores its flat predictions straight into mapped pinned memory, one event.  (Measured alternatives, us per 256 x 64
// batch: torch tensors + pinned copies from Python 94; three event-chained streams with SDMA copies 96-120, host bound by
// the extra runtime calls; one stream with SDMA copies 88, of which 38 are copies and engine hand-overs.)
extern "C" int farnn_tag_host_submit(farnn_model *m, const int64_t *x_host, const int64_t *len_host, int32_t B, int32_t L,
                                     int32_t *ticket, int64_t *n_flat) {
    if (!m || !x_host || !len_host || !ticket) return fail(FARNN_EINVAL, "tag_host_submit: null argument%s%s");
    if (B <= 0 || L <= 0) return fail(FARNN_EINVAL, "tag_host_submit: B and L must be positive%s%s");
    FARNN_HIP_TRY(hipSetDevice(m->device));
    if (!m->hs_run) FARNN_HIP_TRY(hipStreamCreateWithFlags(&m->hs_run, hipStreamNonBlocking));
    const int slot = m->hnext;
    farnn_model::HostSlot &h = m->hslot[slot];
    // a ticket nobody waited for (the caller dropped it): the slot is free again once its batch has completed
    if (h.busy && h.ev_out && hipEventQuery(h.ev_out) == hipSuccess) h.busy = false;
    if (h.busy) return fail(FARNN_EINVAL, "tag_host_submit: FARNN_HOST_SLOTS batches already in flight (wait for the oldest ticket first)%s%s");
    const size_t N = (size_t)B * L;
    if (N > h.capN || (size_t)B > h.capB) {
        FARNN_HIP_TRY(hipStreamSynchronize(m->hs_run));
        host_slot_free(h);
        FARNN_HIP_TRY(hipHostMalloc((void **)&h.x_pin, (N + B) * 8 + 16, hipHostMallocMapped));      // [x | lengths]
        FARNN_HIP_TRY(hipHostMalloc((void **)&h.flat_pin, N * 8, hipHostMallocMapped));
        FARNN_HIP_TRY(hipMalloc((void **)&h.x_dev, (N + B) * 8 + 16));
        FARNN_HIP_TRY(hipHostGetDevicePointer((void **)&h.x_map, h.x_pin, 0));
        FARNN_HIP_TRY(hipHostGetDevicePointer((void **)&h.flat_dev, h.flat_pin, 0));                 // device view of flat_pin
        h.capN = N; h.capB = (size_t)B;
    }
    if (!h.ev_out) FARNN_HIP_TRY(hipEventCreateWithFlags(&h.ev_out, hipEventDisableTiming));
    // workspace growth frees device memory: never while older batches still run on it
    if (B > m->ws.B || L > m->ws.L) {
        FARNN_HIP_TRY(hipStreamSynchronize(m->hs_run));
        int rc = farnn_reserve(m, B, L);
        if (rc) return rc;
    }
    memcpy(h.x_pin, x_host, N * 8);
    memcpy(h.x_pin + N, len_host, (size_t)B * 8);
    long long total = 0;
    for (int b = 0; b < B; b++) { const long long v = len_host[b]; total += v < 0 ? 0 : (v > L ? L : v); }
    h.total = total;
    {
        const long long n = (long long)(N + B);
        stage_in_kernel<<<(unsigned)((n / 2 + 256) / 256), 256, 0, m->hs_run>>>(h.x_map, h.x_dev, n);
        FARNN_HIP_TRY(hipGetLastError());
    }
    int rc = farnn_tag(m, h.x_dev, h.x_dev + N, B, L, FARNN_MODE_LOCAL, nullptr, h.flat_dev, nullptr, m->hs_run);
    if (rc) return rc;
    FARNN_HIP_TRY(hipEventRecord(h.ev_out, m->hs_run));
    h.busy = true;
    h.gen = (h.gen + 1) & 0x7fffffu;
    m->hnext = (slot + 1) % FARNN_HOST_SLOTS;
    *ticket = (int32_t)((unsigned)slot | (h.gen << 8));
    if (n_flat) *n_flat = total;
    return FARNN_OK;
}

extern "C" int farnn_tag_host_wait(farnn_model *m, int32_t ticket, int64_t *flat_out, int64_t *n_out) {
    if (!m || ticket < 0 || (ticket & 0xff) >= FARNN_HOST_SLOTS) return fail(FARNN_EINVAL, "tag_host_wait: bad ticket%s%s");
    farnn_model::HostSlot &h = m->hslot[ticket & 0xff];
    // (a ticket names ONE submit: slot | generation << 8.  A ticket whose batch was already waited for, or whose slot was
    //  reclaimed and handed to a later submit, is refused -- it never consumes the newer batch.)
    if (!h.busy || h.gen != ((unsigned)ticket >> 8))
        return fail(FARNN_EINVAL, "tag_host_wait: no batch in flight under this ticket (stale or already waited for)%s%s");
    FARNN_HIP_TRY(hipSetDevice(m->device));
    FARNN_HIP_TRY(hipEventSynchronize(h.ev_out));
    if (flat_out && h.total > 0) memcpy(flat_out, h.flat_pin, (size_t)h.total * 8);
    if (n_out) *n_out = h.total;
    h.busy = false;
    return FARNN_OK;
}

// utils.flatten (reference utils.py:153-164) for a host int64 [B][L] array: the valid prefix of every row, batch-major.
// Host-side helper of the same boundary (the flat gold labels forward_local returns beside the predictions).
extern "C" int64_t farnn_flatten_host(const int64_t *a, const int64_t *len_host, int32_t B, int32_t L, int64_t *out) {
    int64_t n = 0;
    if (!a || !len_host || !out) return -1;
    for (int b = 0; b < B; b++) {
        long long v = len_host[b];
        v = v < 0 ? 0 : (v > L ? L : v);
        memcpy(out + n, a + (size_t)b * L, (size_t)v * 8);
        n += v;
    }
    return n;
}

extern "C" void farnn_destroy(farnn_model *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    for (auto &h : m->hslot) {
        host_slot_free(h);
        if (h.ev_out) (void)hipEventDestroy(h.ev_out);
    }
    if (m->hs_run) (void)hipStreamDestroy(m->hs_run);
    prof_fold(m);
    for (hipEvent_t e : m->prof.pool) (void)hipEventDestroy(e);
    for (void *p : m->owned) (void)hipFree(p);
    m->ws.release();
    if (m->ev_order) (void)hipEventDestroy(m->ev_order);
    delete m;
}

// ---- introspection ---------------------------------------------------------------------------
extern "C" int farnn_abi_version(void) { return FARNN_ABI_VERSION; }
extern "C" int farnn_ab_build(void) {
#if defined(FARNN_AB)
    return 1;
#else
    return 0;
#endif
}

extern "C" int farnn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *farnn_last_error(void) { return g_err; }

extern "C" int farnn_num_columns(const farnn_model *m) { return m ? m->K : 0; }

extern "C" double farnn_algorithmic_bytes(const farnn_model *m, int64_t valid_tokens) {
    if (!m) return 0.0;
    const double S = m->S, C = m->C, R = m->R, K = m->K;
    double per_tok = 0.0, once = 0.0;
    switch (m->kind) {
        case KIND_IFST: per_tok = 2.0 * S * S * 4 + 12; break;
        case KIND_IND1: per_tok = 3.0 * S * S * 4 + 12; once = C * S * S * 4; break;
        case KIND_FST4: per_tok = (C + 2.0) * S * S * 4 + 12; break;
        case KIND_DECOMP0:
        case KIND_DECOMP1:
        case KIND_DECOMP:
            per_tok = R * 4 + 12;
            once = (2.0 * S * R + S * S + K * S) * 4;
            break;
    }
    return per_tok * (double)valid_tokens + once;
}

extern "C" double farnn_kernel_algorithmic_bytes(const farnn_model *m, int32_t which, int64_t valid_tokens) {
    if (!m) return 0.0;
    TunScope tun_scope(&m->tun);
    const TagPlan p = m->plan.planned ? m->plan : unplanned(m);
    const double S = m->S, C = m->C, R = m->R, K = m->K, n = (double)valid_tokens;
    if (which == KERN_CHAIN) {
        switch (p.rec) {
            case REC_COMPACT_TAG:
            case REC_COMPACT_CHAIN: return (2.0 * S * m->bmNS * 8 + 8) * n;      // one bit-packed block per direction + the token id
            case REC_DECOMP_REGS:
            case REC_DECOMP_ROWS:
            case REC_DECOMP_CHAIN: return (R * 4 + 8) * n + (2.0 * S * R + S * S) * 4;
            default: break;
        }
        // one block per direction + the token id (+ the tag when the decode is this kernel's epilogue); the 16-bit image: what the
        // launched form requests
        if (p.half) return (2.0 * S * S * 2 + 8) * n;
        return (2.0 * S * S * 4 + 8 + (p.fused ? 4 : 0)) * n + (p.fused ? K * S * 4 : 0);
    }
    if (which == KERN_SCORE) {
        switch (m->kind) {
            case KIND_FST4: return (C * S * S * 4 + 4) * n;             // the 4-D scoring stream
            case KIND_IND1: return (S * S * 4 + 4) * n + C * S * S * 4;
            default: return 4 * n + K * S * 4;                          // tags out (+ the output matrix once)
        }
    }
    return 0.0;
}


#if defined(FARNN_PROBES)
// profiling build only (not part of include/farnn.h): the per-workgroup stamps of the last compact_tag_kernel launch under FARNN_DBG=2048
extern "C" int farnn_debug_ct_stamps(long long *out, int n_workgroups) {
    if (!out || n_workgroups < 0 || n_workgroups > farnn::CT_STAMP_MAX) return FARNN_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return FARNN_EIO;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(farnn::g_ct_stamps), sizeof(long long) * 16 * (size_t)n_workgroups) == hipSuccess ? FARNN_OK : FARNN_EIO;
}
// ... the state stash of the handle's last call, as it lies in the workspace: `n` floats each of A (forward) and Bk (backward),
// [B][L + 1][SP] of that call (tests/test_gpu_chain_head.py reads the pad columns S .. SP - 1 back)
extern "C" int farnn_debug_stash(farnn_model *m, float *A_out, float *Bk_out, long long n) {
    if (!m || !A_out || !Bk_out || n < 0 || !m->ws.A || !m->ws.Bk) return FARNN_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return FARNN_EIO;
    if (hipMemcpy(A_out, m->ws.A, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return FARNN_EIO;
    return hipMemcpy(Bk_out, m->ws.Bk, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? FARNN_OK : FARNN_EIO;
}
#endif
