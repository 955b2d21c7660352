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
    return FARNN_OK;
}

// ---- workspace -------------------------------------------------------------------------------
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

extern "C" const char *farnn_kernel_name(const farnn_model *m, int32_t which) {
    if (!m) return "";
    TunScope tun_scope(&m->tun);
    switch (which) {
        case KERN_CHAIN:
            if (m->compact_on) return m->last_fused ? "compact_tag_kernel<fused: both chains + label-map scores + decode>" : "compact_chain_kernel";
            if (m->last_regs && m->last_fused && m->use_crf) return "chain_viterbi_kernel<fused: recurrence + scores + CRF decode>";
            if (m->last_regs && m->rgeom.wide) return m->last_fused ? "chain_wide_kernel<fused: scores + decode beside the recurrence>" : "chain_wide_kernel";
            if (m->last_regs) return m->last_fused ? "chain_regs_kernel<fused: scores + decode beside the recurrence>"
                                                   : (m->last_half ? "chain_regs_kernel<f16 blocks>" : "chain_regs_kernel");
            if (m->dense_decomp) return "chain_kernel";
            if (m->kind == KIND_DECOMP && m->last_fused && m->last_wave) return "decomp_regs_kernel<fused: scores + decode beside the recurrence>";
            if (m->kind == KIND_DECOMP || m->kind == KIND_DECOMP1 || m->kind == KIND_DECOMP0)
                return m->rows.ok ? ((m->last_wave || (m->calls == 0 && m->dw.farnn == 0 && m->dw.R <= DG_ROWS && !tun(TUN_DECOMP_NOREGS))) ? "decomp_regs_kernel" : "decomp_rows_kernel") : "decomp_chain_kernel";
            return "chain_kernel";
        case KERN_SCORE: return m->kind == KIND_FST4 ? "fst4_score_kernel"
                              : (m->kind == KIND_IND1 ? "ind1_score_kernel"
                              : (m->kind == KIND_DECOMP1 ? (m->d1_BSSp ? "decomp1_br_mfma_kernel+decomp1_label_kernel" : "decomp1_score_kernel")
                              : (m->kind == KIND_DECOMP0 ? "decomp0_score_kernel"
                              : (m->use_crf ? "score_tile_kernel+viterbi_kernel" : (m->last_lm_score ? "label_map_score_kernel" : "score_tile_kernel")))));
        case KERN_PREP:  return "batch_prep_kernel";
        default: return "";
    }
}

// ---- the hot path ----------------------------------------------------------------------------

// the register-fed recurrence's view of a call (chain_regs_params.hip.h); the hand-off words are filled in by the callers that use them
static RegsParams make_regs_params(farnn_model *m, const int64_t *x, const int64_t *len, int B, int full) {
    const RegsGeom &rg = m->rgeom;
    RegsParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.Mf = m->Mf; rp.Mb = m->Mb; rp.blk = (long long)m->geom.SR * m->SP;
    rp.o = m->o; rp.h0 = m->h0; rp.hT = m->hT; rp.x = x; rp.len = len;
    rp.order = m->order_valid ? m->ws.order : nullptr; rp.sort = m->sort_in_kernel ? 1 : 0;
    rp.A = m->ws.A; rp.Bk = m->ws.Bk; rp.B = B; rp.L = m->curL; rp.S = m->S; rp.SP = m->SP; rp.CPR = rg.CPR; rp.V = m->V;
    rp.G = rg.G; rp.RPG = rg.RPG; rp.RQ = rg.RQ; rp.D = rg.D; rp.PS = rg.PS; rp.pair = rg.wide ? 0 : 1;
    rp.nl = m->nl; rp.full = full; rp.dbg = tun(TUN_DBG);
    rp.dest = (!rg.wide && m->semiring != FARNN_SEMIRING_MAX && !tun(TUN_NODEST)) ? 1 : 0;     // chain_dest.hip.h
    rp.Mf16 = m->Mf16; rp.Mb16 = m->Mb16; rp.blk16 = (long long)m->SP * RD_XS * 2;              // (null: no image, build_half_image)
    rp.o_ones = (!m->o || m->o_ones) ? 1 : 0;                                                    // (build_output_matrix)
    return rp;
}

// The hand-off words of the one-launch forms (chain_regs.hip.h / decomp_regs.hip.h + beside.hip.h) and their launch counter.
// A launch's epoch is (the counter >> BS_EPOCH_SHIFT) + 1, read from device memory by the kernel; every launch adds exactly
// BS_EPOCH_SPAN to the counter whatever its batch size (beside.hip.h, bs_launch_epoch).  Nothing per launch comes from the host and
// nothing is ever reset: the step replays from a HIP graph as the very same launch, and graphs captured at different batch sizes
// and eager calls may interleave on a handle (stream-ordered).  The words are zeroed once, when the workspace is allocated.
static int handoff_words(farnn_model *m, unsigned long long **prog, unsigned long long **arr, unsigned long long **done) {
    *prog = m->ws.hs; *arr = m->ws.hs + (size_t)2 * m->ws.B; *done = m->ws.hs + (size_t)3 * m->ws.B + 16;      // (the counter on a 128-byte line of its own)
    return FARNN_OK;
}

// fuse_sp != nullptr: ask for the fused launch (scores + argmax decode as the chain kernel's epilogue); *fused tells
// whether the geometry allowed it (else the caller launches the score kernel itself)
static int launch_chain(farnn_model *m, const int64_t *x, const int64_t *len, int B, int L, int full,
                        hipStream_t s, const ScoreParams *fuse_sp = nullptr, bool *fused = nullptr) {
    const ChainGeom &g = m->geom;
    if (fused) *fused = false;
    m->last_regs = false;
    m->last_half = false;
    // ---- the register-fed kernel (chain_regs.hip.h) where its geometry applies: S <= 72, two workgroups per compute unit, or
    // its wide form (chain_wide.hip.h): 72 < S <= 128, one workgroup per compute unit.
    // With fuse_sp (threshold/argmax decode, K <= 256) the scores and the decode run beside the recurrence: ONE launch.
    if (m->rgeom.ok && !tun(TUN_NOREGS)) {
        const RegsGeom &rg = m->rgeom;
        const size_t lds_cap = rg.wide ? 158 * 1024 : 80 * 1024;
        bool score = fuse_sp && m->ws.hs && m->OTm && m->c16 >= 1 && m->c16 <= (rg.wide ? RGW_NG : RG_NG) && m->Kc <= 256 && m->curL <= 31 * RG_TT &&
                     (B <= 1024 || !fuse_sp->flat || fuse_sp->offs) && !tun(TUN_NOFUSE);
        // Which form is the faster one was measured, and the faster one is the default.  S <= 72 with a label-map output matrix (tags
        // only): the recurrence-only kernel followed by the label-map score launch (K2l).  Round 5 kept ONE launch (the scores and
        // the decode beside the recurrence: north_star's form) while 2 B <= compute units, on measurements at B = 64 / 256 / 1 024 and
        // L = 64 only; round 6's grid (scripts/gpu_r06_dispatch_grid.py -> profiles/r06_dispatch_grid.txt: B = 16..128 x L = 16..100)
        // has two launches ahead at 32 of its 35 points -- by 5-20 % at the reference's default --seq_max_len 30 and below, within
        // 1 % either way at L = 64 -- so the rule no longer looks at the batch.  FARNN_FUSE=1 keeps the one launch (what a HIP graph
        // replays as one node); tests/test_gpu_dispatch_ab.py holds the default to "not the slower form" at nine (B, L) points.
        if (score && !rg.wide && bs_label_map_path(*fuse_sp) && !tun(TUN_FUSE)) score = false;
        const bool lm_path = score && bs_label_map_path(*fuse_sp);
        const bool dest = !rg.wide && m->semiring != FARNN_SEMIRING_MAX && !tun(TUN_NODEST);
        size_t lds = (size_t)regs_lds(m->curL, m->SP, rg.NP, score ? m->c16 : 0, score ? m->Kc : 0, score, rg.RQ, lm_path, dest).total * sizeof(float);
        // the wide form PAIRED (two workgroups per compute unit, like S <= 72): a ring of two steps and the label-map path's LDS
        const bool paired = rg.wide && lm_path && rg.RQ <= 9 && lds <= 80 * 1024 && !tun(TUN_WIDE_UNPAIRED);
        if (score && lds > lds_cap) {               // the score tiles do not fit (beside a second workgroup): recurrence only
            score = false;
            lds = (size_t)regs_lds(m->curL, m->SP, rg.NP, 0, 0, false, rg.RQ, false, dest).total * sizeof(float);
        }
        // the destination split's recurrence-only launch on the 16-bit image of a model whose o is absent or all ones keeps `hist` in rows of RD_XS floats
        // where that fits beside a second workgroup (chain_dest.hip.h: one store per step, chain_regs_one_kernel); where it does not --
        // the longest sequences this kernel takes -- rows of SP floats and two stores as before
        bool row80 = false;
        if (dest && !score && (!m->o || m->o_ones) && m->Mf16 && m->Mb16 && !tun(TUN_NOHALF) && FARNN_STEP_ONESTORE && FARNN_CHAIN_HEAD) {
            const size_t lds80 = (size_t)regs_lds(m->curL, m->SP, rg.NP, 0, 0, false, rg.RQ, false, dest, true).total * sizeof(float);
            if (lds80 <= lds_cap) { row80 = true; lds = lds80; }
        }
        if (lds <= lds_cap) {
            RegsParams rp = make_regs_params(m, x, len, B, full);
            if (score) {
                int hrc = handoff_words(m, &rp.prog, &rp.arr, &rp.done);
                if (hrc) return hrc;
                if (tun(TUN_HOST_EPOCH)) {       // diagnostic A/B: the epoch as a kernel argument (not graph-capturable)
                    if (++m->epoch_u == 0) { FARNN_HIP_TRY(hipMemsetAsync(m->ws.hs, 0, m->ws.hs_bytes, s)); m->epoch_u = 1; }
                    rp.done = nullptr; rp.epoch_host = m->epoch_u + 0x40000000u;
                }
                rp.spin = tun(TUN_FUSE_SPIN);
                rp.solo_margin = tun(TUN_SOLO_MARGIN);
                rp.sp = *fuse_sp;
                if (fused) *fused = true;
            }
            // the 16-bit image where the handle has one (an eligible model, build_half_image): the recurrence-only launch of the
            // destination split reads half the bytes with half the load instructions; FARNN_NOHALF=1 keeps the f32 blocks
            rp.half = (rp.dest && !score && m->Mf16 && m->Mb16 && !tun(TUN_NOHALF)) ? 1 : 0;
            rp.row80 = row80 ? 1 : 0;
            KernelTimer kt(m, KERN_CHAIN, s, /*ext=*/true);
            if (paired && score) { rp.D = 2; rp.pair = 1; }
            const int rc = (paired && score) ? launch_chain_wide_paired(rp, m->semiring == FARNN_SEMIRING_MAX, s, kt.e0, kt.e1)
                           : rg.wide ? launch_chain_wide(rp, m->semiring == FARNN_SEMIRING_MAX, score, s, kt.e0, kt.e1)
                                     : launch_chain_regs(rp, m->semiring == FARNN_SEMIRING_MAX, score, s, kt.e0, kt.e1);
            if (rc) return rc;
            m->last_regs = true;
            m->last_half = rp.half != 0;
            return FARNN_OK;
        }
    }
    (void)fuse_sp;
    ChainParams p;
    p.Mf = m->Mf; p.Mb = m->Mb; p.blk = (long long)m->geom.SR * m->SP;
    p.o = m->o; p.h0 = m->h0; p.hT = m->hT; p.x = x; p.len = len; p.A = m->ws.A; p.Bk = m->ws.Bk;
    p.order = m->order_valid ? m->ws.order : nullptr;
    p.sort = m->sort_in_kernel ? 1 : 0;
    p.B = B; p.L = m->curL; p.S = m->S; p.SP = m->SP; p.CPR = g.CPR; p.V = m->V;
    p.NW = g.NW; p.NLD = g.NLD; p.G = g.G; p.LPR = g.LPR; p.RPG = g.RPG; p.RPGp = g.RPGp; p.NQ = g.NQ;
    p.nl = m->nl; p.full = full; p.dbg = tun(TUN_DBG);
    // ring shape: a whole step per phase when it fits, KS phases deep
    int ks = 2, nqp = g.NQ;
    if (!g.pick_ring(m->curL, m->chain_ks, ks, nqp))
        return fail(FARNN_ERANGE, "chain kernel: LDS ring does not fit (sequence too long for this S)%s%s");
    p.KS = ks; p.NQP = nqp; p.PPS = (g.NQ + nqp - 1) / nqp;
    const size_t lds = g.lds_bytes(m->curL, ks, nqp);
    dim3 grid(2 * B), block((g.NW + g.NLD + 1) * 64);         // compute + loader + writer wavefronts
    const bool mx = m->semiring == FARNN_SEMIRING_MAX;
    int rc = FARNN_OK;
    if (tun(TUN_CHAIN_HELPER) && block.x < 512) block = dim3(block.x + 64);     // experiment: an idle eighth wavefront
    KernelTimer kt(m, KERN_CHAIN, s, /*ext=*/true);
    const int fq_max = block.x <= 384 ? 6 : 3;
    const int fq = (g.NCH == 1 && p.PPS == 1 && g.NQ <= fq_max && !tun(TUN_NOFAST)) ? g.NQ : 0;
    auto go = [&](auto NCH, auto FQ) {
        return mx ? launch_timed(chain_kernel<NCH(), true, FQ()>, grid, block, lds, s, kt.e0, kt.e1, p)
                  : launch_timed(chain_kernel<NCH(), false, FQ()>, grid, block, lds, s, kt.e0, kt.e1, p);
    };
    if (g.NCH == 1) {
        if (fq == 1) rc = go(int_c<1>(), int_c<1>());
        else if (fq == 2) rc = go(int_c<1>(), int_c<2>());
        else if (fq == 3) rc = go(int_c<1>(), int_c<3>());
        else if (fq == 4) rc = go(int_c<1>(), int_c<4>());
        else if (fq == 5) rc = go(int_c<1>(), int_c<5>());
        else if (fq == 6) rc = go(int_c<1>(), int_c<6>());
        else rc = go(int_c<1>(), int_c<0>());
    } else if (g.NCH == 2) rc = go(int_c<2>(), int_c<0>());
    else if (g.NCH <= 4) rc = go(int_c<4>(), int_c<0>());
    else return fail(FARNN_ERANGE, "unsupported state count%s%s");
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// the recurrence of the three decomposed kinds: rows kernel when packed, else the older kernels
// fuse_sp != nullptr: ask for the one-launch form (scores + argmax decode beside the recurrence); *fused tells whether the
// model's kernel and geometry allowed it (else the caller launches the score kernel itself)
static int launch_decomp_recurrence(farnn_model *m, const int64_t *x, const int64_t *lengths, int B, int full,
                                    hipStream_t s, const ScoreParams *fuse_sp = nullptr, bool *fused = nullptr) {
    if (fused) *fused = false;
    const int *order = m->order_valid ? m->ws.order : nullptr;
    if (m->n_cu <= 0) m->n_cu = device_cus(m->device);
    RegsPlan rp;
    m->last_wave = m->rows.ok && regs_plan(m->rows, m->dw, m->curL, rp);
    if (m->last_wave) {      // farnn = 0, rank <= 64: four wavefronts per chain, the packed rows in registers
        BesideParams bs;
        const BesideParams *use = nullptr;
        bool score = fuse_sp && m->ws.hs && m->OTm && m->c16 >= 1 && m->c16 <= DG_NG && m->Kc <= 256 && m->curL <= 31 * RG_TT &&
                     (B <= 1024 || !fuse_sp->flat || fuse_sp->offs) && !tun(TUN_NOFUSE);
        if (score) {
            rp.lds_score = regs_score_lds(rp, m->curL, m->SP, m->c16, m->Kc);
            if (rp.lds_score > 80 * 1024) score = false;
        }
        if (score) {
            memset(&bs, 0, sizeof(bs));
            bs.A = m->ws.A; bs.Bk = m->ws.Bk; bs.B = B; bs.L = m->curL; bs.SP = m->SP; bs.CPR = m->SP / 4;
            int hrc = handoff_words(m, &bs.prog, &bs.arr, &bs.done);
            if (hrc) return hrc;
            bs.spin = tun(TUN_FUSE_SPIN); bs.dbg = tun(TUN_DBG); bs.sp = *fuse_sp;
            use = &bs;
            if (fused) *fused = true;
        }
        return launch_decomp_regs(m->rows, m->dw, rp, x, lengths, order, m->sort_in_kernel ? 1 : 0, m->ws.A, m->ws.Bk, B, m->curL,
                                  full, s, use);
    }
    RowsPlan pl;
    if (m->rows.ok && rows_plan(m->rows, m->dw, B, m->curL, pl))
        return launch_decomp_rows(m->rows, m->dw, pl, x, lengths, order, m->sort_in_kernel ? 1 : 0, m->ws.A, m->ws.Bk, B,
                                  m->curL, full, m->n_cu, s);
    return launch_decomp_chain(m->dw, x, lengths, order, m->ws.A, m->ws.Bk, B, m->curL, full, s);
}

// fused: the Viterbi kernel computes the scores itself (no score_tile launch went before it)
static bool viterbi_can_fuse(const farnn_model *m, const ScoreParams &p) {
    return m->use_crf && !p.scores && !p.P && p.A && p.OT && m->K <= 256 &&
           viterbi_hist_lds_bytes(m->K, m->Kp, p.SP, p.L, true) <= 158 * 1024 && viterbi_hist_ib4(m->K) <= 6 &&
           !tun(TUN_VITERBI_BP) && !tun(TUN_VITERBI_UNFUSED);
}

static int launch_viterbi(farnn_model *m, const ScoreParams &p, int B, hipStream_t s, bool fused = false) {
    int rc;
    if (m->K > 256) return fail(FARNN_ERANGE, "Viterbi: more than 256 tags%s%s");
    const size_t hlds = viterbi_hist_lds_bytes(m->K, m->Kp, p.SP, p.L, fused);
    // (K >= 224 never takes this form: the transposed transition table alone is 196 KiB -- no IB4 = 7, 8 instantiations)
    if (hlds <= 158 * 1024 && viterbi_hist_ib4(m->K) <= 6 && !tun(TUN_VITERBI_BP)) {
        // partition history in LDS, back-pointers recomputed along the path
        const int threads = viterbi_hist_score_threads(m->K, fused);
        auto go = [&](auto N) {
            return fused ? launch(viterbi_hist_kernel<N(), true>, dim3(B), dim3(threads), hlds, s, p)
                         : launch(viterbi_hist_kernel<N(), false>, dim3(B), dim3(threads), hlds, s, p);
        };
        rc = FARNN_OK;
        switch (viterbi_hist_ib4(m->K)) {
            case 0: rc = go(int_c<0>()); break;
            case 1: rc = go(int_c<1>()); break;
            case 2: rc = go(int_c<2>()); break;
            case 3: rc = go(int_c<3>()); break;
            case 4: rc = go(int_c<4>()); break;
            case 5: rc = go(int_c<5>()); break;
            case 6: rc = go(int_c<6>()); break;
        }
        if (rc) return rc;
        FARNN_HIP_TRY(hipGetLastError());
        return FARNN_OK;
    }
    if (fused) return fail(FARNN_EINVAL, "Viterbi: the fused form needs the history in LDS%s%s");
    // long sequences: two partition rows + stored back-pointers
    const size_t vlds = viterbi_lds_bytes(m->K, m->Kp, p.L);
    const int threads = round_up(4 * m->K, 64);
    auto go = [&](auto N) { return launch(viterbi_kernel<N()>, dim3(B), dim3(threads), vlds, s, p); };
    const int ib4 = viterbi_ib4(m->K);
    if (ib4 == 2) rc = go(int_c<2>());            // K <= 32
    else if (ib4 == 4) rc = go(int_c<4>());       // K <= 64
    else if (ib4 == 9) rc = go(int_c<9>());       // K <= 144
    else if (ib4 == 13) rc = go(int_c<13>());     // K <= 208
    else rc = go(int_c<16>());                    // K <= 256
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

static int launch_decomp1_score(farnn_model *m, const int64_t *x, const int64_t *len, int B, int full,
                                int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    Decomp1ScoreParams p;
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.Vgen = m->dw.Vgen; p.S1 = m->dw.S1; p.S2 = m->dw.S2; p.W = m->dw.W;
    p.S1o = m->d1_S1o; p.S2o = m->d1_S2o; p.CoutT = m->d1_CoutT; p.P = m->P;
    p.x = x; p.len = len; p.offs = flat ? m->ws.offs : nullptr;
    p.tags = tags; p.flat = flat; p.scores = scores; p.crf_scores = m->ws.crf_scores;
    p.B = B; p.L = m->curL; p.S = m->S; p.SP = m->SP; p.R = m->R; p.Rp = m->Rp; p.RO = m->RO; p.ROp = m->ROp;
    p.V = m->V;
    p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.full = full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    int rc;
    KernelTimer kt(m, KERN_SCORE, s);
    Decomp1MfmaParams qm;
    qm.base = p; qm.BSSp = m->d1_BSSp; qm.S1oP = m->d1_S1oP; qm.S2oP = m->d1_S2oP; qm.br = m->ws.d1_br;
    if (!full) qm.base.offs = m->ws.offs;       // farnn_tag computes the flat offsets for this path even without flat output
    qm.MT = (m->S + 15) / 16; qm.NT = (m->RO + 15) / 16; qm.KQ4 = (m->S + 15) / 16;
    const size_t mlds = decomp1_mfma_lds_bytes(qm.MT, qm.NT);
    if (m->d1_BSSp && m->ws.d1_br && mlds <= 80 * 1024) {
        // persistent: two workgroups per CU, every wavefront owns a contiguous slice of the live tokens
        if (m->n_cu <= 0) m->n_cu = device_cus(m->device);
        const int nwg = std::min(2 * m->n_cu, (B * p.L + 3) / 4);
        auto go = [&](auto N) { return launch(decomp1_br_mfma_kernel<N()>, dim3(nwg), dim3(256), mlds, s, qm); };
        switch (qm.NT) {
            case 1: rc = go(int_c<1>()); break;
            case 2: rc = go(int_c<2>()); break;
            case 3: rc = go(int_c<3>()); break;
            case 4: rc = go(int_c<4>()); break;
            case 5: rc = go(int_c<5>()); break;
            default: return fail(FARNN_ERANGE, "decomp_ind1: output rank above 80 on the MFMA path%s%s");
        }
        if (rc) return rc;
        FARNN_HIP_TRY(hipGetLastError());
        const int NC = qm.NT * 16;
        // one 16-wavefront workgroup per CU when the weights fit in LDS beside the per-wavefront rows
        const bool staged = decomp1_label_lds_bytes(NC, m->RO, m->K, m->Kc, true, 16) <= 150 * 1024;
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
    if (m->use_crf) {
        ScoreParams v;
        memset(&v, 0, sizeof(v));
        v.trT = m->tr; v.len = len; v.offs = flat ? m->ws.offs : nullptr; v.tags = tags; v.flat = flat;
        v.crf_scores = m->ws.crf_scores; v.B = B; v.L = m->curL; v.K = m->K; v.Kp = m->Kp;
        v.full = full; v.use_crf = 1; v.o_idx = m->o_idx; v.threshold = m->threshold;
        if ((rc = launch_viterbi(m, v, B, s))) return rc;
    }
    return FARNN_OK;
}

static int launch_decomp0_score(farnn_model *m, const int64_t *x, const int64_t *len, int B, int full,
                                int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    Decomp0ScoreParams p;
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.Vgen = m->d0_Vgen; p.S1 = m->dw.S1; p.S2 = m->dw.S2; p.CT = m->d0_CT;
    p.S1w = m->d0_S1w; p.S2w = m->d0_S2w; p.CwT = m->d0_CwT; p.P = m->P;
    p.x = x; p.len = len; p.offs = flat ? m->ws.offs : nullptr;
    p.tags = tags; p.flat = flat; p.scores = scores; p.crf_scores = m->ws.crf_scores;
    p.B = B; p.L = m->curL; p.S = m->S; p.SP = m->SP; p.R = m->R; p.Rp = m->Rp; p.RW = m->RW; p.RWp = m->RWp;
    p.V = m->V;
    p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.full = full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    const size_t lds = decomp0_score_lds_bytes(m->SP, m->Rp, m->RWp, m->Kc);
    int rc;
    if ((rc = raise_lds_limit(decomp0_score_kernel, lds))) return rc;
    KernelTimer kt(m, KERN_SCORE, s);
    decomp0_score_kernel<<<dim3((p.L + D0_TOK - 1) / D0_TOK, B), dim3(256), lds, s>>>(p);
    FARNN_HIP_TRY(hipGetLastError());
    if (m->use_crf) {
        ScoreParams v;
        memset(&v, 0, sizeof(v));
        v.trT = m->tr; v.len = len; v.offs = flat ? m->ws.offs : nullptr; v.tags = tags; v.flat = flat;
        v.crf_scores = m->ws.crf_scores; v.B = B; v.L = m->curL; v.K = m->K; v.Kp = m->Kp;
        v.full = full; v.use_crf = 1; v.o_idx = m->o_idx; v.threshold = m->threshold;
        if ((rc = launch_viterbi(m, v, B, s))) return rc;
    }
    return FARNN_OK;
}

static ScoreParams make_score_params(farnn_model *m, const int64_t *len, int B, int full, int32_t *tags,
                                     int64_t *flat, float *scores) {
    ScoreParams p;
    memset(&p, 0, sizeof(p));
    p.A = m->ws.A; p.Bk = m->ws.Bk; p.OT = m->OT; p.OTm = m->OTm; p.c16 = m->c16; p.P = m->P; p.trT = m->tr; p.len = len;
    p.offs = (flat && !m->prep_in_kernel) ? m->ws.offs : nullptr; p.tags = tags; p.flat = flat; p.scores = scores;
    p.crf_scores = m->ws.crf_scores;
    p.B = B; p.L = m->curL; p.S = m->S; p.SP = m->SP; p.K = m->K; p.Kp = m->Kp; p.Kc = m->Kc;
    p.kch = m->Kc / 64;
    p.full = full; p.use_crf = m->use_crf; p.o_idx = m->o_idx; p.threshold = m->threshold;
    p.dbg = tun(TUN_DBG);
    p.kz = (m->kind == KIND_IFST && m->use_crf && !tun(TUN_NOKZ)) ? m->C : 0;      // the library appended the two zero rows itself
    p.lm = m->lm;
    return p;
}

static int launch_score_decode(farnn_model *m, const int64_t *len, int B, int full, int32_t *tags,
                               int64_t *flat, float *scores, hipStream_t s) {
    ScoreParams p = make_score_params(m, len, B, full, tags, flat, scores);
    if (viterbi_can_fuse(m, p)) {          // stash -> scores -> Viterbi -> tags in one kernel
        KernelTimer kt(m, KERN_SCORE, s);
        return launch_viterbi(m, p, B, s, true);
    }
    int rc;
    if (p.lm.on && !p.P && !scores && !m->use_crf && m->S <= LM_MAXS * 2 && (B <= 1024 || !flat || p.offs)) {
        // K2l: the output matrix is a label map and only tags are asked for -- S multiply-adds and a scan per token, one workgroup
        // per sequence (score_decode.hip.h).  FARNN_NOLABELMAP=1 (no label map is built then) keeps the matrix form.
        KernelTimer kt(m, KERN_SCORE, s);
        label_map_score_kernel<LMS_WAVES><<<B, LMS_WAVES * 64, 0, s>>>(p);
        FARNN_HIP_TRY(hipGetLastError());
        m->last_lm_score = true;
        return FARNN_OK;
    }
    m->last_lm_score = false;
    const size_t lds = score_lds_bytes(m->S, m->Kc);
    const dim3 grid((p.L + SCORE_TT - 1) / SCORE_TT, B), block(SCORE_WAVES * 64);
    KernelTimer kt(m, KERN_SCORE, s);
    auto go = [&](auto KCH) { return launch(score_tile_kernel<KCH()>, grid, block, lds, s, p); };
    switch (p.kch) {
        case 1: rc = go(int_c<1>()); break;
        case 2: rc = go(int_c<2>()); break;
        case 3: rc = go(int_c<3>()); break;
        default: rc = go(int_c<4>()); break;
    }
    if (rc) return rc;
    FARNN_HIP_TRY(hipGetLastError());
    if (m->use_crf && (rc = launch_viterbi(m, p, B, s))) return rc;
    return FARNN_OK;
}

// the dense-block recurrence followed by scores + decode: ONE launch (the decode is the chain kernel's epilogue) when
// the decode is the threshold/argmax one and the geometry allows it, else the chain kernel + the score / Viterbi kernels
static int launch_chain_and_decode(farnn_model *m, const int64_t *x, const int64_t *len, int B, int L, int full,
                                   int32_t *tags, int64_t *flat, float *scores, hipStream_t s) {
    int rc;
    if (!m->use_crf) {
        const ScoreParams sp = make_score_params(m, len, B, full, tags, flat, scores);
        bool fused = false;
        if ((rc = launch_chain(m, x, len, B, L, full, s, &sp, &fused))) return rc;
        m->last_fused = fused;
        if (fused) return FARNN_OK;
    } else {
        // CRF decode: recurrence + scores + Viterbi in ONE launch (chain_viterbi.hip) where the register-fed recurrence applies and
        // the decode's LDS fits; else the recurrence kernel followed by the (fused score +) Viterbi kernel
        m->last_fused = false;
        const ScoreParams sp = make_score_params(m, len, B, full, tags, flat, scores);
        // The one launch (north_star: "decode fused into the same kernel") exists for S <= 108 and is parity-tested, but is NOT the
        // default (round 5): a compute unit then holds BOTH chains of a sequence, which run 1 390 cycles per step there against
        // 780-960 when a long chain shares its unit with a short one, and the decode waits behind them.  Measured at K = 130,
        // 256 x 64: S = 71 77.7 us in one launch against 72.9 in two (round 4; round 5's recurrence kernel: 69), S = 104 113.8 against
        // 95.7 (profiles/r04_*, r05_*).  FARNN_CV_ONE=1 selects it.
        // The production library does not carry the form's 48 kernels: it lives in the A/B build (build.py --probes, -DFARNN_AB).
#if defined(FARNN_AB)
        if (tun(TUN_CV_ONE) && m->rgeom.ok && !tun(TUN_NOREGS) && !tun(TUN_NOFUSE) && viterbi_can_fuse(m, sp) &&
            (B <= 1024 || !flat || sp.offs) && chain_viterbi_fits(m->curL, m->SP, m->rgeom.NP, m->K, m->Kp, m->lm.on != 0, m->rgeom.RQ)) {
            const RegsParams rp = make_regs_params(m, x, len, B, full);
            KernelTimer kt(m, KERN_CHAIN, s, /*ext=*/true);
            if ((rc = launch_chain_viterbi(rp, sp, m->semiring == FARNN_SEMIRING_MAX, s, kt.e0, kt.e1))) return rc;
            m->last_regs = true; m->last_fused = true;
            return FARNN_OK;
        }
#endif
        if ((rc = launch_chain(m, x, len, B, L, full, s))) return rc;
    }
    return launch_score_decode(m, len, B, full, tags, flat, scores, s);
}

// forward_RE's view of the scores (model_onehot.py:153-154): the `oo` column (the last one) capped at the threshold
__global__ void clamp_oo_column_kernel(float *scores, long long rows, int K, int col, float threshold) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) {                                  // torch.min: a NaN score stays a NaN (fminf would turn it into the threshold)
        const float x = scores[r * K + col];
        scores[r * K + col] = (x < threshold || x != x) ? x : threshold;
    }
}

static int tag_impl(farnn_model *m, const int64_t *x, const int64_t *lengths, int32_t B, int32_t L,
                    int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream) {
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
    m->curL = L;
    const int full = mode == FARNN_MODE_FULL;
    m->prof_this_call = m->profiling > 0 && (m->calls++ % m->profiling) == 0;
    // batch preparation: flat-output offsets and the length-sorted launch order (full mode runs
    // every sequence for L steps, so there is nothing to balance)
    const bool want_order = !full && B > 2 && !tun(TUN_NOSORT);
    // the plain i-FST path needs no prep launch up to B = 1024: the chain workgroups select their sequence
    // by length rank themselves and the score workgroups sum the lengths in front of theirs
    m->prep_in_kernel = (m->kind == KIND_IFST || (m->kind == KIND_DECOMP && m->rows.ok)) && B <= 1024 && L <= 1023 &&
                        !tun(TUN_PREP);
    m->order_valid = want_order && !m->prep_in_kernel;
    m->sort_in_kernel = want_order && m->prep_in_kernel;
    // the decomposed independent=1 scoring kernel slices the batch by flat offsets even when no flat output is asked for
    const bool want_offs = flat_tags || (m->kind == KIND_DECOMP1 && m->d1_BSSp && !full);
    if ((want_offs || want_order) && !m->prep_in_kernel) {
        KernelTimer kt(m, KERN_PREP, s);
        if (B <= 1024) {
            int G = 1;
            while (G < 16 && B * G * 2 <= 1024) G *= 2;               // lanes per sequence
            batch_prep_small_kernel<<<1, round_up(B * G, 64), 0, s>>>(
                lengths, want_offs ? m->ws.offs : nullptr, want_order ? m->ws.order : nullptr, B, L, G);
        }
        else
            batch_prep_kernel<<<1, 1024, (size_t)(L + 2) * sizeof(int), s>>>(
                lengths, want_offs ? m->ws.offs : nullptr, want_order ? m->ws.order : nullptr, B, L);
        FARNN_HIP_TRY(hipGetLastError());
    }
    switch (m->kind) {
        case KIND_IFST:
            if (m->compact_on) {
                if (L > 1024) return fail(FARNN_ERANGE, "compact recurrence: more than 1024 positions%s%s");
                CompactParams cp;
                cp.bitsF = m->bmF; cp.bitsB = m->bmB; cp.wF = m->bmWF; cp.wB = m->bmWB; cp.o = m->o; cp.h0 = m->h0; cp.hT = m->hT;
                cp.mF = m->bmMF; cp.mB = m->bmMB; cp.xF = m->bmXF; cp.xB = m->bmXB; cp.tokoff = m->bmTok;
                cp.x = x; cp.len = lengths; cp.order = m->order_valid ? m->ws.order : nullptr; cp.A = m->ws.A; cp.Bk = m->ws.Bk;
                cp.B = B; cp.L = L; cp.S = m->S; cp.SP = m->SP; cp.V = m->V; cp.nl = m->nl; cp.full = full; cp.dbg = tun(TUN_DBG);
                m->last_fused = false;
                {
                    // ONE launch (compact_tag.hip.h: both chains of a sequence in LDS, label-map scores, argmax decode) where it
                    // applies; FARNN_NOFUSE=1: round 2's two launches
                    const ScoreParams sp = make_score_params(m, lengths, B, full, tags, flat_tags, scores);
                    if (m->bmTok && sp.lm.on && !sp.P && !scores && !m->use_crf && !tun(TUN_NOFUSE) &&
                        compact_tag_fits(m->V, m->S, L) && (B <= 1024 || !flat_tags || sp.offs)) {
                        const size_t lds = (size_t)compact_tag_lds(L, m->bmNS).total * 4;
                        const int nlk = m->nl == FARNN_NL_NONE ? 0 : m->nl == FARNN_NL_RELU ? 1 : 2;
                        const int nw = (m->S + 31) / 32;                       // 32-bit words of a bitmap row in use
                        KernelTimer kt(m, KERN_CHAIN, s);
                        auto go = [&](auto NW) {
                            const dim3 grid(B), block(CT_WAVES * 64);
                            if (nlk == 0) return launch(compact_tag_kernel<NW(), 0>, grid, block, lds, s, cp, sp);
                            if (nlk == 1) return launch(compact_tag_kernel<NW(), 1>, grid, block, lds, s, cp, sp);
                            return launch(compact_tag_kernel<NW(), 2>, grid, block, lds, s, cp, sp);
                        };
                        if (nw <= 1) rc = go(int_c<1>()); else if (nw == 2) rc = go(int_c<2>());
                        else if (nw == 3) rc = go(int_c<3>()); else rc = go(int_c<4>());
                        if (rc) return rc;
                        FARNN_HIP_TRY(hipGetLastError());
                        m->last_fused = true;
                        return FARNN_OK;
                    }
                }
                {
                    KernelTimer kt(m, KERN_CHAIN, s);
                    if ((rc = launch_compact_chain(cp, m->bmNS, s))) return rc;
                }
                return launch_score_decode(m, lengths, B, full, tags, flat_tags, scores, s);
            }
            return launch_chain_and_decode(m, x, lengths, B, L, full, tags, flat_tags, scores, s);
        case KIND_FST4:
            if ((rc = launch_chain(m, x, lengths, B, L, full, s))) return rc;
            {
                KernelTimer kt(m, KERN_SCORE, s);
                return launch_fst4_score(m->A4, m->ws.A, m->ws.Bk, m->P, x, lengths, flat_tags ? m->ws.offs : nullptr,
                                         tags, flat_tags, scores, B, m->curL, m->S, m->SP, m->C, m->Kc, full,
                                         m->o_idx, m->threshold, /*Oten*/ nullptr, m->V, s);
            }
        case KIND_IND1:
            if ((rc = launch_chain(m, x, lengths, B, L, full, s))) return rc;
            {
                KernelTimer kt(m, KERN_SCORE, s);
                return launch_fst4_score(m->Ms, m->ws.A, m->ws.Bk, m->P, x, lengths, flat_tags ? m->ws.offs : nullptr,
                                         tags, flat_tags, scores, B, m->curL, m->S, m->SP, m->C, m->Kc, full,
                                         m->o_idx, m->threshold, m->Oten, m->V, s);
            }
        case KIND_DECOMP: {
            if (m->dense_decomp) return launch_chain_and_decode(m, x, lengths, B, L, full, tags, flat_tags, scores, s);
            bool fused = false;
            {
                KernelTimer kt(m, KERN_CHAIN, s);
                if (!m->use_crf) {
                    const ScoreParams sp = make_score_params(m, lengths, B, full, tags, flat_tags, scores);
                    if ((rc = launch_decomp_recurrence(m, x, lengths, B, full, s, &sp, &fused))) return rc;
                } else if ((rc = launch_decomp_recurrence(m, x, lengths, B, full, s))) return rc;
            }
            m->last_fused = fused;
            if (fused) return FARNN_OK;
            return launch_score_decode(m, lengths, B, full, tags, flat_tags, scores, s);
        }
        case KIND_DECOMP0: {
            {
                KernelTimer kt(m, KERN_CHAIN, s);
                if ((rc = launch_decomp_recurrence(m, x, lengths, B, full, s))) return rc;
            }
            return launch_decomp0_score(m, x, lengths, B, full, tags, flat_tags, scores, s);
        }
        case KIND_DECOMP1: {
            if (m->dense_decomp) {
                if ((rc = launch_chain(m, x, lengths, B, L, full, s))) return rc;
            } else {
                KernelTimer kt(m, KERN_CHAIN, s);
                if ((rc = launch_decomp_chain(m->dw, x, lengths, nullptr, m->ws.A, m->ws.Bk, B, m->curL, full, s))) return rc;
            }
            return launch_decomp1_score(m, x, lengths, B, full, tags, flat_tags, scores, s);
        }
        default:
            return fail(FARNN_EINVAL, "tag: unknown model kind%s%s");
    }
}

extern "C" int farnn_tag(farnn_model *m, const int64_t *x, const int64_t *lengths, int32_t B, int32_t L,
                         int32_t mode, int32_t *tags, int64_t *flat_tags, float *scores, void *stream) {
    if (!m || !x || !lengths) return fail(FARNN_EINVAL, "tag: null model / x / lengths%s%s");
    if (B <= 0 || L <= 0) return fail(FARNN_EINVAL, "tag: B and L must be positive%s%s");
    if (mode != FARNN_MODE_LOCAL && mode != FARNN_MODE_FULL && mode != FARNN_MODE_RE)
        return fail(FARNN_EINVAL, "tag: bad mode%s%s");
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
    const double S = m->S, C = m->C, R = m->R, K = m->K, n = (double)valid_tokens;
    if (which == KERN_CHAIN) {
        if (m->compact_on) return (2.0 * S * m->bmNS * 8 + 8) * n;      // one bit-packed block per direction + the token id
        if (!m->dense_decomp && (m->kind == KIND_DECOMP || m->kind == KIND_DECOMP1 || m->kind == KIND_DECOMP0))
            return (R * 4 + 8) * n + (2.0 * S * R + S * S) * 4;
        // one block per direction + the token id (+ the tag when the decode is this kernel's epilogue); the 16-bit image: what the
        // launched form requests
        if (m->last_regs && m->last_half) return (2.0 * S * S * 2 + 8) * n;
        return (2.0 * S * S * 4 + 8 + (m->last_fused ? 4 : 0)) * n + (m->last_fused ? K * S * 4 : 0);
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
