// The creates of the tagging library (farnn_*_create*), each a list of the stages below.  A create holds its handle in a
// ModelOwner and its device temporaries in a DevTmp (tag_host.hip.h): no return leaves either behind.  Included by farnn_hip.hip only.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "tag_host.hip.h"
#include "score_decode.hip.h"
#include "decomp1_score.hip.h"
#include "compact.hip.h"

// ---- stages shared by the creates ----------------------------------------------------------------
// arguments and *out
static int begin_create(bool args_ok, farnn_model **out) {
    if (!args_ok || !out) return fail(FARNN_EINVAL, "null argument%s%s");
    *out = nullptr;
    return FARNN_OK;
}

// the device and a fresh handle of `kind`; the caller opens its TunScope on the handle's switches next
static int begin_model(ModelOwner &own, int kind, int device) {
    int rc = select_device(device);
    if (rc) return rc;
    own.reset(new (std::nothrow) farnn_model());
    if (!own) return fail(FARNN_ENOMEM, "host allocation failed%s%s");
    own->kind = kind; own->device = device;
    return FARNN_OK;
}

static void set_labels(farnn_model *m, int K) {
    m->K = K; m->Kp = round_up(K, 4); m->Kc = round_up(K, 64);
}

// the dense-block recurrence's geometries: the ring kernel's (chain.hip.h) and the register-fed kernel's (chain_regs.hip.h);
// the blocks get enough zero rows for either
static void pick_chain_geometry(farnn_model *m) {
    m->geom = chain_geometry(m->S, tun(TUN_RPG), tun(TUN_NLD));
    m->rgeom = regs_geometry(m->S);
    if (m->rgeom.SP != m->geom.SP) m->rgeom.ok = false;
    if (m->rgeom.ok && m->rgeom.rows > m->geom.SR) m->geom.SR = m->rgeom.rows;
    m->chain_ks = tun(TUN_KS);
}

// the onehot models: the chain geometry gives the padded state count
static int onehot_geometry(farnn_model *m) {
    pick_chain_geometry(m);
    m->SP = m->geom.SP;
    return m->geom.NCH > 4 ? fail(FARNN_ERANGE, "more than 1024 states%s%s") : FARNN_OK;
}

// (Mf / Mb are written by the stages of a create alone -- premix_chain_blocks, launch_premix_fst4, build_dense_blocks -- and the
//  16-bit image of an eligible handle, build_half_image, is derived from them once.  Whatever ever rewrites the blocks of a LIVE
//  handle must drop m->Mf16 / m->Mb16, or re-run build_half_image, before the next tag call: a stale image is a silent wrong answer.)
static int alloc_chain_blocks(farnn_model *m) {
    const size_t nM = (size_t)m->V * m->geom.SR * m->SP;
    if (int rc = dev_alloc(m, (void **)&m->Mf, nM * 4)) return rc;
    return dev_alloc(m, (void **)&m->Mb, nM * 4);
}

// premix T+W once (the reference re-adds it on every call, model_onehot.py:366)
static int premix_chain_blocks(farnn_model *m, const float *T, const float *W, const float *mask) {
    if (int rc = alloc_chain_blocks(m)) return rc;
    return launch_premix(T, W, mask, m->Mf, m->Mb, m->V, m->S, m->SP, m->geom.SR);
}

// The blocks' 16-bit image for the destination split's recurrence-only launch (chain_dest.hip.h, H16): built only for a handle
// that launch serves (S <= 72: the narrow register-fed form; sum semiring) and only if EVERY entry of Mf and Mb is an f16 exactly.
// Nothing rewrites the blocks of a live handle (every writer of Mf / Mb is a stage of a create), so the image never goes stale.
static int build_half_image(farnn_model *m) {
    if (!m->Mf || !m->Mb || !m->rgeom.ok || m->rgeom.wide || m->semiring == FARNN_SEMIRING_MAX || m->SP > RG_MAXSP || tun(TUN_NOHALF))
        return FARNN_OK;
    const long long nM = (long long)m->V * m->geom.SR * m->SP;
    DevTmp tmp;
    int *bad = nullptr, bad_h = 0;
    if (int rc = tmp.zeros(&bad, 1)) return rc;
    const unsigned nb = (unsigned)std::min<long long>((nM + 255) / 256, 4096);
    half_eligible_kernel<<<nb, 256>>>(m->Mf, nM, bad);
    half_eligible_kernel<<<nb, 256>>>(m->Mb, nM, bad);
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipMemcpy(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad_h) return FARNN_OK;
    const size_t bytes = (size_t)m->V * m->SP * RD_XS * sizeof(unsigned short);
    if (int rc = dev_alloc(m, (void **)&m->Mf16, bytes)) return rc;
    if (int rc = dev_alloc(m, (void **)&m->Mb16, bytes)) return rc;
    const dim3 grid((m->SP * RD_XS + 255) / 256, m->V);
    half_image_kernel<<<grid, 256>>>(m->Mf, m->Mf16, m->SP, m->geom.SR);
    half_image_kernel<<<grid, 256>>>(m->Mb, m->Mb16, m->SP, m->geom.SR);
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipDeviceSynchronize());
    return FARNN_OK;
}

// h0 / hT (dw's aliases are read by the decomposed kinds only)
static int upload_start_final(farnn_model *m, const float *h0, const float *hT, int on_device) {
    int rc;
    if ((rc = dev_upload(m, &m->h0, h0, m->S, m->SP, on_device))) return rc;
    if ((rc = dev_upload(m, &m->hT, hT, m->S, m->SP, on_device))) return rc;
    m->dw.h0 = m->h0; m->dw.hT = m->hT;
    return FARNN_OK;
}

static int default_crf_transitions(std::vector<float> &tr, int K) {
    // CRF.__init__ (crf.py:39-46): zeros, [:,START]=-1e4, [STOP,:]=-1e4
    tr.assign((size_t)K * K, 0.0f);
    for (int i = 0; i < K; i++) tr[(size_t)i * K + (K - 2)] = -10000.0f;
    for (int j = 0; j < K; j++) tr[(size_t)(K - 1) * K + j] = -10000.0f;
    return FARNN_OK;
}

static int setup_priority(farnn_model *m, const float *P, int on_device) {
    // P is [K][K] (already expanded, priority.py:6-18); stored [K][Kc]
    if (!P) return FARNN_OK;
    return upload_padded(m, &m->P, P, m->K, m->K, m->K, m->Kc, on_device);
}

static int setup_crf(farnn_model *m, const float *crf_trans, int on_device) {
    if (!m->use_crf) return FARNN_OK;
    std::vector<float> dflt;
    if (!crf_trans) { default_crf_transitions(dflt, m->K); crf_trans = dflt.data(); on_device = 0; }
    // stored transposed (trT[j][i] = tr[i][j]) so the Viterbi inner loop walks contiguous memory
    return upload_transposed(m, &m->tr, crf_trans, m->K, m->K, m->Kp, on_device);
}
// the tail of every create: the priority matrix and the CRF transitions (no-ops where the model has none)
static int upload_decode_tables(farnn_model *m, const float *P, const float *crf_trans, int on_device) {
    if (int rc = setup_priority(m, P, on_device)) return rc;
    return setup_crf(m, crf_trans, on_device);
}

// the matrix-core image of the transposed output matrix (call once m->OT is final)
static int build_ot_image(farnn_model *m) {
    int rc;
    m->c16 = (m->S + 15) / 16;
    const long long n = (long long)(m->Kc / 16) * m->c16 * 256;
    if ((rc = dev_alloc(m, (void **)&m->OTm, (size_t)n * 4))) return rc;
    ot_to_mfma_kernel<<<(unsigned)((n + 255) / 256), 256>>>(m->OT, m->OTm, m->S, m->Kc, m->c16);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

// The output matrix as a label map (label_map.hip.h): every state at most one label, weight exactly 1, at most 128 labelled
// states.  Read back from the final OT[S][Kc] (a few KB), sorted by (label, state) on the host, uploaded as one table.
static int build_label_map(farnn_model *m) {
    m->lm.on = 0;
    if (!m->OT || m->S > 1024 || tun(TUN_NOLABELMAP)) return FARNN_OK;
    std::vector<float> ot((size_t)m->S * m->Kc);
    FARNN_HIP_TRY(hipMemcpy(ot.data(), m->OT, ot.size() * 4, hipMemcpyDeviceToHost));
    std::vector<std::pair<int, int>> pos;                // (label, state)
    for (int s = 0; s < m->S; s++) {
        int lab = -1;
        for (int c = 0; c < m->K; c++) {
            const float v = ot[(size_t)s * m->Kc + c];
            if (v == 0.0f) continue;
            if (v != 1.0f || lab >= 0) return FARNN_OK;  // a weight, or a second label: the matrix form
            lab = c;
        }
        if (lab >= 0) pos.push_back({lab, s});
    }
    const int n = (int)pos.size();
    if (n > LM_MAXS || m->S > 256 || m->K > 510) return FARNN_OK;      // (8 bits of state, 9 of label per packed word)
    std::sort(pos.begin(), pos.end());
    const int clampcol = m->use_crf ? m->K - 3 : m->K - 1;     // model_decompose.py:353 / model_onehot.py:166
    std::vector<unsigned> tab(128, 0u);
    int lb[128];
    for (int j = 0; j < 128; j++) lb[j] = j < n ? pos[j].first : m->K + j;      // pads: distinct, above every label
    for (int j = 0; j < 128; j++) {
        unsigned wd = j < n ? ((unsigned)pos[j].second | ((unsigned)lb[j] << LM_LB_SHIFT)) : (0x1ffu << LM_LB_SHIFT);
        const int base = j & ~63, r = (j & 63) >> 4;
        const int dd[4] = {1, 2, 4, 8};
        for (int d = 0; d < 4; d++)
            if ((j & 15) >= dd[d] && lb[j - dd[d]] == lb[j]) wd |= 1u << (LM_CF_SHIFT + d);
        if ((r == 1 || r == 3) && lb[base + 16 * r - 1] == lb[j]) wd |= 1u << (LM_CF_SHIFT + 4);
        if ((r == 2 || r == 3) && lb[base + 31] == lb[j]) wd |= 1u << (LM_CF_SHIFT + 5);
        if (j >= 64 && lb[j] == lb[63]) wd |= 1u << LM_CC_BIT;
        if (j < n && (j == n - 1 || lb[j + 1] != lb[j])) wd |= 1u << LM_TL_BIT;
        tab[j] = wd;
    }
    std::vector<char> has((size_t)m->K, 0);
    for (int j = 0; j < n; j++) has[pos[j].first] = 1;
    m->lm.e0 = -1;
    for (int c = 0; c < m->K; c++)
        if (!has[c]) { m->lm.e0 = c; break; }
    m->lm.z0 = (m->lm.e0 == clampcol) ? std::min(0.0f, m->threshold) : 0.0f;
    m->lm.nq = n > 64 ? 2 : 1;
    m->lm.clampcol = clampcol; m->lm.threshold = m->threshold;
    m->lm.clamp_empty = (clampcol >= 0 && clampcol < m->K && !has[clampcol]) ? 1 : 0;
    unsigned *dv = nullptr;
    int rc = dev_alloc(m, (void **)&dv, tab.size() * 4);
    if (rc) return rc;
    FARNN_HIP_TRY(hipMemcpy(dv, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    m->lm.tab = dv;
    m->lm.on = 1;
    return FARNN_OK;
}
// The output matrix src [rows][S] of the two i-FST models: o = its column sums (CE1, model_onehot.py:368 /
// model_decompose_single.py:232), OT = its transpose, padded (zero rows for START/STOP), OT's matrix-core image and the
// label map.  build_label_map reads OT back: the synchronize before it stays where it is.
static int build_output_matrix(farnn_model *m, const float *src, int rows, int on_device) {
    DevTmp tmp;
    const float *O = nullptr;
    int rc;
    if ((rc = tmp.view(&O, src, (size_t)rows * m->S, on_device))) return rc;
    if ((rc = dev_alloc(m, (void **)&m->o, (size_t)m->SP * 4))) return rc;
    if ((rc = dev_alloc(m, (void **)&m->OT, round_up_sz((size_t)m->S * m->Kc * 4, 1024)))) return rc;
    FARNN_HIP_TRY(hipMemset(m->o, 0, (size_t)m->SP * 4));
    FARNN_HIP_TRY(hipMemset(m->OT, 0, round_up_sz((size_t)m->S * m->Kc * 4, 1024)));
    colsum_kernel<<<(m->S + 255) / 256, 256>>>(O, m->o, rows, m->S);
    int n = rows * m->S;
    transpose_pad_kernel<<<(n + 255) / 256, 256>>>(O, m->OT, rows, m->S, m->Kc);
    int *bad = nullptr, bad_h = 1;
    if ((rc = tmp.zeros(&bad, 1))) return rc;
    not_all_ones_kernel<<<1, 256>>>(m->o, m->S, bad);
    FARNN_HIP_TRY(hipGetLastError());
    if ((rc = build_ot_image(m))) return rc;
    FARNN_HIP_TRY(hipDeviceSynchronize());
    FARNN_HIP_TRY(hipMemcpy(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost));
    m->o_ones = bad_h == 0;
    if ((rc = build_label_map(m))) return rc;
    m->dw.o = m->o;
    return FARNN_OK;
}

// ---- compact form of a 0/1 automaton (compact.hip.h): bit-packed blocks beside (or instead of) the dense ones ----------
static int alloc_bitmaps(farnn_model *m) {
    m->bmNS = (m->semiring == FARNN_SEMIRING_SUM) ? compact_ns(m->S) : 0;
    if (!m->bmNS) return FARNN_OK;
    const size_t nb = (size_t)m->V * m->S * m->bmNS * sizeof(u64), nw = (size_t)m->S * m->bmNS * sizeof(u64);
    int rc;
    if ((rc = dev_alloc(m, (void **)&m->bmF, nb)) || (rc = dev_alloc(m, (void **)&m->bmB, nb)) ||
        (rc = dev_alloc(m, (void **)&m->bmWF, nw)) || (rc = dev_alloc(m, (void **)&m->bmWB, nw))) return rc;
    FARNN_HIP_TRY(hipMemset(m->bmF, 0, nb)); FARNN_HIP_TRY(hipMemset(m->bmB, 0, nb));
    FARNN_HIP_TRY(hipMemset(m->bmWF, 0, nw)); FARNN_HIP_TRY(hipMemset(m->bmWB, 0, nw));
    return FARNN_OK;
}

static int finish_bitmaps(farnn_model *m, int *bad_dev) {
    int bad = 0;
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipMemcpy(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) m->bmNS = 0;            // a weight other than 0 / 1: the dense blocks are the only form (the bitmaps stay unused)
    if (m->bmNS >= 1 && m->bmNS <= 2 && (unsigned long long)m->V * m->S * m->bmNS * 8ull < (1ull << 32) - 4096) {     // (= compact_tag_fits' bound)
        // compact_tag_kernel's planes (compact_tag.hip.h).  Its lanes without a state read rows past their block: 4 KiB of slack
        const size_t nb = (size_t)m->V * m->S * m->bmNS * sizeof(u64);
        int rc;
        if ((rc = dev_alloc(m, (void **)&m->bmMF, nb + 4096)) || (rc = dev_alloc(m, (void **)&m->bmMB, nb + 4096)) ||
            (rc = dev_alloc(m, (void **)&m->bmXF, nb + 4096)) || (rc = dev_alloc(m, (void **)&m->bmXB, nb + 4096)) ||
            (rc = dev_alloc(m, (void **)&m->bmTok, (size_t)m->V * sizeof(unsigned)))) return rc;
        FARNN_HIP_TRY(hipMemset(m->bmMF + nb / 8, 0, 4096)); FARNN_HIP_TRY(hipMemset(m->bmMB + nb / 8, 0, 4096));
        FARNN_HIP_TRY(hipMemset(m->bmXF + nb / 8, 0, 4096)); FARNN_HIP_TRY(hipMemset(m->bmXB + nb / 8, 0, 4096));
        std::vector<unsigned> off((size_t)m->V);
        for (int v = 0; v < m->V; v++) off[(size_t)v] = (unsigned)((size_t)v * m->S * m->bmNS * 8);
        FARNN_HIP_TRY(hipMemcpy(m->bmTok, off.data(), off.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        const long long n = (long long)m->V * m->S * m->bmNS;
        merge_planes_kernel<<<(unsigned)((n + 255) / 256), 256>>>(m->bmF, m->bmB, m->bmWF, m->bmWB, m->bmMF, m->bmMB, m->bmXF, m->bmXB,
                                                                  m->bmTok, m->V, m->S, m->bmNS);
        FARNN_HIP_TRY(hipGetLastError());
        FARNN_HIP_TRY(hipDeviceSynchronize());
    }
    return FARNN_OK;
}

struct DevEdges { const int32_t *word, *from, *to; const float *val; long long n; };     // device copies of an edge list

// from the edge list e, or (e == nullptr) from the dense T and W
static int build_bitmaps(farnn_model *m, const float *T, const float *W, const DevEdges *e) {
    DevTmp tmp;
    int *bad = nullptr;
    if (int rc = tmp.zeros(&bad, 1)) return rc;
    if (!e)
        dense_to_bits_kernel<<<dim3(m->V + 1, (m->S * m->S + 255) / 256), 256>>>(T, W, m->bmF, m->bmB, m->bmWF, m->bmWB, m->V, m->S,
                                                                              m->bmNS, bad);
    else if (e->n > 0)
        edges_to_bits_kernel<<<(unsigned)((e->n + 255) / 256), 256>>>(e->word, e->from, e->to, e->val, e->n, m->bmF, m->bmB, m->bmWF,
                                                                      m->bmWB, m->V, m->S, m->bmNS, bad);
    return finish_bitmaps(m, bad);
}

// ---- create: onehot i-FST --------------------------------------------------------------------
// compact_edges != nullptr: build ONLY the compact form, from the edge list (no dense blocks; d->T / d->W unused)
static int ifst_create_impl(const farnn_onehot_ifst_desc *d, int device, farnn_model **out, const DevEdges *compact_edges) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0 || ((!d->T || !d->W) && !compact_edges) || !d->O || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "onehot_ifst: sizes must be positive and T/W/O/h0/hT non-null%s%s");
    if (d->nl < 0 || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "onehot_ifst: bad nl%s%s");
    if (d->semiring != FARNN_SEMIRING_SUM && d->semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "onehot_ifst: bad semiring%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_IFST, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    m->V = d->V; m->S = d->S; m->C = d->C;
    m->use_crf = d->use_crf ? 1 : 0;
    set_labels(m, d->C + (m->use_crf ? 2 : 0));
    m->nl = d->nl; m->semiring = d->semiring; m->threshold = d->threshold; m->o_idx = d->o_idx;
    if (m->K > 64 * SCORE_KCH) return fail(FARNN_ERANGE, "more than 256 label columns%s%s");
    if ((rc = onehot_geometry(m))) return rc;
    const int od = d->weights_on_device;

    if (compact_edges) {
        if ((rc = alloc_bitmaps(m))) return rc;
        if (!m->bmNS) return fail(FARNN_ERANGE, "onehot_ifst compact form: needs the sum semiring and at most 512 states%s%s");
        if ((rc = build_bitmaps(m, nullptr, nullptr, compact_edges))) return rc;
        if (!m->bmNS) return fail(FARNN_EINVAL, "onehot_ifst compact form: an edge is out of range or has a weight other than 1%s%s");
        m->compact_on = true;
    } else {
        DevTmp tmp;
        const float *T = nullptr, *W = nullptr;
        if ((rc = tmp.view(&T, d->T, (size_t)m->V * m->S * m->S, od))) return rc;
        if ((rc = tmp.view(&W, d->W, (size_t)m->S * m->S, od))) return rc;
        if ((rc = premix_chain_blocks(m, T, W, nullptr))) return rc;
        if ((rc = build_half_image(m))) return rc;
        if ((rc = alloc_bitmaps(m))) return rc;
        if (m->bmNS && (rc = build_bitmaps(m, T, W, nullptr))) return rc;
    }
    if ((rc = build_output_matrix(m, d->O, m->C, od))) return rc;
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    // the priority matrix of the onehot models is [C][C]; with CRF the two extra tags pass through
    if (d->P && m->use_crf) {
        std::vector<float> Pc((size_t)m->C * m->C), Pk((size_t)m->K * m->K, 0.0f);
        FARNN_HIP_TRY(hipMemcpy(Pc.data(), d->P, Pc.size() * 4,
                                od ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        for (int i = 0; i < m->C; i++)
            for (int j = 0; j < m->C; j++) Pk[(size_t)i * m->K + j] = Pc[(size_t)i * m->C + j];
        Pk[(size_t)(m->K - 2) * m->K + m->K - 2] = 1.0f;
        Pk[(size_t)(m->K - 1) * m->K + m->K - 1] = 1.0f;
        if ((rc = setup_priority(m, Pk.data(), 0))) return rc;
    } else if ((rc = setup_priority(m, d->P, od))) return rc;
    if ((rc = setup_crf(m, d->crf_trans, od))) return rc;
    *out = own.release();
    return FARNN_OK;
}

extern "C" int farnn_onehot_ifst_create(const farnn_onehot_ifst_desc *d, int device, farnn_model **out) {
    return ifst_create_impl(d, device, out, nullptr);
}

// ---- create: onehot FST 4-D -------------------------------------------------------------------
extern "C" int farnn_onehot_fst4_create(const farnn_onehot_fst4_desc *d, int device, farnn_model **out) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0 || !d->T4 || !d->W4 || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "onehot_fst4: sizes must be positive and T4/W4/h0/hT non-null%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_FST4, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    m->V = d->V; m->S = d->S; m->C = d->C;
    set_labels(m, d->C);
    m->nl = FARNN_NL_RELU;                       // relu is unconditional (model_onehot.py:93-94)
    m->semiring = d->semiring; m->threshold = d->threshold; m->o_idx = d->o_idx;
    if (m->K > 1024) return fail(FARNN_ERANGE, "more than 1024 label columns%s%s");
    if ((rc = onehot_geometry(m))) return rc;
    const int od = d->weights_on_device;
    {
        DevTmp tmp;
        const float *T4 = nullptr, *W4 = nullptr;
        if ((rc = tmp.view(&T4, d->T4, (size_t)m->V * m->C * m->S * m->S, od))) return rc;
        if ((rc = tmp.view(&W4, d->W4, (size_t)m->C * m->S * m->S, od))) return rc;
        if ((rc = alloc_chain_blocks(m))) return rc;
        if ((rc = dev_alloc(m, (void **)&m->A4, (size_t)m->V * m->C * m->S * m->SP * 4))) return rc;
        if ((rc = launch_premix_fst4(T4, W4, m->Mf, m->Mb, m->A4, m->V, m->C, m->S, m->SP, m->geom.SR))) return rc;
    }
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    if ((rc = upload_decode_tables(m, d->P, nullptr, od))) return rc;
    *out = own.release();
    return FARNN_OK;
}

// ---- create: onehot independent=1 -------------------------------------------------------------
extern "C" int farnn_onehot_ind1_create(const farnn_onehot_ind1_desc *d, int device, farnn_model **out) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->C <= 0 || !d->T || !d->W || !d->Oten || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "onehot_ind1: sizes must be positive and T/W/Oten/h0/hT non-null%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_IND1, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    m->V = d->V; m->S = d->S; m->C = d->C;
    set_labels(m, d->C);
    m->nl = FARNN_NL_RELU;                       // relu always (model_onehot.py:266, :278)
    m->semiring = d->semiring; m->threshold = d->threshold; m->o_idx = d->o_idx;
    m->mask_by_output = d->mask_by_output;
    if (m->K > 1024) return fail(FARNN_ERANGE, "more than 1024 label columns%s%s");
    if ((rc = onehot_geometry(m))) return rc;
    // K3 keeps (alpha beta^T) .* Tf[x_i] of a token in LDS: refused here, where S and the label columns are known, not at farnn_tag
    if (fst4_score_lds_bytes(m->S, m->SP, m->Kc, true) > FST4_SCORE_LDS_LIMIT)
        return fail(FARNN_ERANGE, "onehot_ind1: independent=1 scoring needs S*S*4 bytes of LDS per token (S too large)%s%s");
    const int od = d->weights_on_device;
    {
        DevTmp tmp;
        const float *T = nullptr, *W = nullptr, *Ot = nullptr;
        if ((rc = tmp.view(&T, d->T, (size_t)m->V * m->S * m->S, od))) return rc;
        if ((rc = tmp.view(&W, d->W, (size_t)m->S * m->S, od))) return rc;
        if ((rc = tmp.view(&Ot, d->Oten, (size_t)m->C * m->S * m->S, od))) return rc;
        if ((rc = dev_alloc(m, (void **)&m->Ms, (size_t)m->V * m->S * m->SP * 4))) return rc;      // scoring blocks (S rows)
        if ((rc = upload_padded(m, &m->Oten, Ot, m->C * m->S, m->S, m->C * m->S, m->SP, 1))) return rc;
        float *osum = nullptr;                   // the transitions masked by the output sum, or not
        if (m->mask_by_output) {
            if ((rc = dev_alloc(m, (void **)&osum, (size_t)m->S * m->S * 4))) return rc;
            colsum_kernel<<<(m->S * m->S + 255) / 256, 256>>>(Ot, osum, m->C, m->S * m->S);
            FARNN_HIP_TRY(hipGetLastError());
        }
        if ((rc = premix_chain_blocks(m, T, W, osum))) return rc;
        if ((rc = launch_premix(T, W, nullptr, m->Ms, nullptr, m->V, m->S, m->SP, m->S))) return rc;
    }
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    if ((rc = upload_decode_tables(m, d->P, nullptr, od))) return rc;
    *out = own.release();
    return FARNN_OK;
}

// ---- create from the automaton's edge list: dense tensors are scattered on the device ------------
template <typename Desc>
static int begin_edge_create(const Desc *b, farnn_model **out, const char *who, bool args_ok = true) {
    if (int rc = begin_create(b && args_ok, out)) return rc;
    if (b->V <= 0 || b->S <= 0 || b->C <= 0) return fail(FARNN_EINVAL, "%s: V, S, C must be positive%s", who, "");
    return FARNN_OK;
}

// the small host parameters of a desc whose big tensors were built on the device: staged, so that the desc is all-device
// (crf_trans == nullptr: a model without a CRF)
static int stage_small_params(DevTmp &tmp, int on_device, int S, int C, int use_crf, const float **h0, const float **hT,
                              const float **P, const float **crf_trans) {
    if (on_device) return FARNN_OK;
    int rc;
    const size_t K = (size_t)C + (use_crf ? 2 : 0);
    if ((rc = tmp.view(h0, *h0, S, 0)) || (rc = tmp.view(hT, *hT, S, 0)) || (rc = tmp.view(P, *P, (size_t)C * C, 0))) return rc;
    return crf_trans ? tmp.view(crf_trans, *crf_trans, K * K, 0) : FARNN_OK;
}

static int scatter_edges(DevTmp &tmp, const farnn_edge_list *e, float *T, float *W, float *O, int V, int S, int C,
                         int mode) {
    if (!e || e->n_edges < 0 || (e->n_edges > 0 && (!e->word || !e->from || !e->to)))
        return fail(FARNN_EINVAL, "from_edges: edge arrays missing%s%s");
    const size_t ne = (size_t)e->n_edges;
    if (!ne) return FARNN_OK;
    int32_t *word = nullptr;
    float *val = nullptr;
    int *bad = nullptr;
    int rc;
    if ((rc = tmp.raw(&word, ne * 4))) return rc;           // word | from | to | label
    int32_t *from = word + ne, *to = from + ne, *label = to + ne;
    if ((rc = tmp.raw(&val, ne))) return rc;
    if ((rc = tmp.zeros(&bad, 1))) return rc;
    FARNN_HIP_TRY(hipMemcpy(word, e->word, ne * 4, hipMemcpyHostToDevice));
    FARNN_HIP_TRY(hipMemcpy(from, e->from, ne * 4, hipMemcpyHostToDevice));
    FARNN_HIP_TRY(hipMemcpy(to, e->to, ne * 4, hipMemcpyHostToDevice));
    if (e->label) FARNN_HIP_TRY(hipMemcpy(label, e->label, ne * 4, hipMemcpyHostToDevice));
    if (e->val) FARNN_HIP_TRY(hipMemcpy(val, e->val, ne * 4, hipMemcpyHostToDevice));
    scatter_edges_kernel<<<(unsigned)((ne + 255) / 256), 256>>>(word, from, to, e->label ? label : nullptr,
                                                                 e->val ? val : nullptr, (long long)ne, T, W, O,
                                                                 V, S, C, mode, bad);
    FARNN_HIP_TRY(hipGetLastError());
    int hbad = 0;
    FARNN_HIP_TRY(hipMemcpy(&hbad, bad, 4, hipMemcpyDeviceToHost));
    if (hbad) return fail(FARNN_EINVAL, "from_edges: an edge has a word, state or label index out of range%s%s");
    return FARNN_OK;
}

extern "C" int farnn_onehot_ifst_create_from_edges(const farnn_onehot_ifst_desc *b, const farnn_edge_list *e,
                                                   int device, farnn_model **out) {
    int rc = begin_edge_create(b, out, "ifst_from_edges");
    if (rc || (rc = select_device(device))) return rc;
    DevTmp tmp;
    float *T = nullptr, *W = nullptr, *O = nullptr;
    if ((rc = tmp.zeros(&T, (size_t)b->V * b->S * b->S)) || (rc = tmp.zeros(&W, (size_t)b->S * b->S)) ||
        (rc = tmp.zeros(&O, (size_t)b->C * b->S))) return rc;
    if ((rc = scatter_edges(tmp, e, T, W, O, b->V, b->S, b->C, 0))) return rc;
    farnn_onehot_ifst_desc full = *b;
    if ((rc = stage_small_params(tmp, b->weights_on_device, b->S, b->C, b->use_crf, &full.h0, &full.hT, &full.P, &full.crf_trans))) return rc;
    full.T = T; full.W = W; full.O = O; full.weights_on_device = 1;
    return farnn_onehot_ifst_create(&full, device, out);
}

extern "C" int farnn_onehot_ifst_create_compact(const farnn_onehot_ifst_desc *b, const farnn_edge_list *e, int device,
                                                farnn_model **out) {
    int rc = begin_edge_create(b, out, "ifst_create_compact", e != nullptr);
    if (rc) return rc;
    if (e->n_edges < 0 || (e->n_edges > 0 && (!e->word || !e->from || !e->to)))
        return fail(FARNN_EINVAL, "ifst_create_compact: edge arrays missing%s%s");
    if ((rc = select_device(device))) return rc;
    DevTmp tmp;
    float *O = nullptr;
    if ((rc = tmp.zeros(&O, (size_t)b->C * b->S))) return rc;
    if ((rc = scatter_edges(tmp, e, nullptr, nullptr, O, b->V, b->S, b->C, 0))) return rc;       // labels -> O only
    // the edge arrays once more on the device, for the bitmap scatter
    const size_t ne = (size_t)e->n_edges;
    int32_t *dw = nullptr;
    float *dv = nullptr;
    if ((rc = tmp.raw(&dw, (ne ? ne : 1) * 3))) return rc;
    if (ne) {
        FARNN_HIP_TRY(hipMemcpy(dw, e->word, ne * 4, hipMemcpyHostToDevice));
        FARNN_HIP_TRY(hipMemcpy(dw + ne, e->from, ne * 4, hipMemcpyHostToDevice));
        FARNN_HIP_TRY(hipMemcpy(dw + 2 * ne, e->to, ne * 4, hipMemcpyHostToDevice));
        if (e->val && (rc = tmp.copy(&dv, e->val, ne, 0))) return rc;
    }
    DevEdges de{dw, dw + ne, dw + 2 * ne, dv, (long long)ne};
    farnn_onehot_ifst_desc full = *b;
    if ((rc = stage_small_params(tmp, b->weights_on_device, b->S, b->C, b->use_crf, &full.h0, &full.hT, &full.P, &full.crf_trans))) return rc;
    full.T = nullptr; full.W = nullptr; full.O = O; full.weights_on_device = 1;
    return ifst_create_impl(&full, device, out, &de);
}

extern "C" int farnn_onehot_fst4_create_from_edges(const farnn_onehot_fst4_desc *b, const farnn_edge_list *e,
                                                   int device, farnn_model **out) {
    int rc = begin_edge_create(b, out, "fst4_from_edges");
    if (rc || (rc = select_device(device))) return rc;
    DevTmp tmp;
    float *T4 = nullptr, *W4 = nullptr;
    if ((rc = tmp.zeros(&T4, (size_t)b->V * b->C * b->S * b->S)) || (rc = tmp.zeros(&W4, (size_t)b->C * b->S * b->S)))
        return rc;
    if ((rc = scatter_edges(tmp, e, T4, W4, nullptr, b->V, b->S, b->C, 1))) return rc;
    farnn_onehot_fst4_desc full = *b;
    if ((rc = stage_small_params(tmp, b->weights_on_device, b->S, b->C, 0, &full.h0, &full.hT, &full.P, nullptr))) return rc;
    full.T4 = T4; full.W4 = W4; full.weights_on_device = 1;
    return farnn_onehot_fst4_create(&full, device, out);
}

extern "C" int farnn_onehot_ind1_create_from_edges(const farnn_onehot_ind1_desc *b, const farnn_edge_list *e,
                                                   int device, farnn_model **out) {
    int rc = begin_edge_create(b, out, "ind1_from_edges");
    if (rc || (rc = select_device(device))) return rc;
    DevTmp tmp;
    float *T = nullptr, *W = nullptr, *Oten = nullptr;
    if ((rc = tmp.zeros(&T, (size_t)b->V * b->S * b->S)) || (rc = tmp.zeros(&W, (size_t)b->S * b->S)) ||
        (rc = tmp.zeros(&Oten, (size_t)b->C * b->S * b->S))) return rc;
    if ((rc = scatter_edges(tmp, e, T, W, Oten, b->V, b->S, b->C, 2))) return rc;
    farnn_onehot_ind1_desc full = *b;
    if ((rc = stage_small_params(tmp, b->weights_on_device, b->S, b->C, 0, &full.h0, &full.hT, &full.P, nullptr))) return rc;
    full.T = T; full.W = W; full.Oten = Oten; full.weights_on_device = 1;
    return farnn_onehot_ind1_create(&full, device, out);
}

// ---- decomposed modes whose step matrix is materialised anyway: dense per-word blocks + the chain kernel ----
static int build_dense_blocks(farnn_model *m) {
    const DecompWeights &w = m->dw;
    if (w.farnn != 0 || !(w.semiring == FARNN_SEMIRING_MAX || w.mask)) return FARNN_OK;
    pick_chain_geometry(m);
    if (m->geom.NCH > 4 || m->geom.SP != m->SP) return FARNN_OK;
    const size_t nM = (size_t)m->V * m->geom.SR * m->SP;
    if (nM * 8 > (size_t)64 << 30) return FARNN_OK;               // keep it under 64 GB; else the generic kernel
    if (int rc = alloc_chain_blocks(m)) return rc;
    FARNN_HIP_TRY(hipMemset(m->Mb, 0, nM * 4));
    dim3 grid((m->geom.SR * m->SP + 255) / 256, m->V);
    materialise_blocks_kernel<<<grid, 256>>>(w.Vgen, w.S1, w.S2, w.W, w.mask, m->Mf, m->Mb, m->S, m->SP, m->geom.SR,
                                             m->R, m->Rp);
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipDeviceSynchronize());
    m->dense_decomp = true;
    return FARNN_OK;
}

// ---- packed rows + gate tables for decomp_rows_kernel (create time) ------------------------------
static int build_rows_pack(farnn_model *m) {
    DecompWeights &w = m->dw;
    DecompRowsPack &k = m->rows;
    k.ok = false;
    if (w.semiring != FARNN_SEMIRING_SUM || w.mask) return FARNN_OK;
    const int tvl = m->Rp + (w.farnn >= 1 ? m->SP : 0) + (w.farnn == 2 ? m->SP : 0);
    if (tvl > DR_MAX_PF * DR_THREADS) return FARNN_OK;
    k.nch2 = (m->S + DR_CHUNK - 1) / DR_CHUNK; k.nch3 = (m->Rp + m->S + DR_CHUNK - 1) / DR_CHUNK;
    k.ld2 = rows_ld(m->S); k.ld3 = rows_ld(m->Rp + m->S);
    k.n1 = w.farnn == 2 ? 2 * m->S : 0;
    k.n2 = m->R + (w.farnn == 1 ? m->S : 0);
    k.n3 = m->S;
    PackSrc q;
    q.S1 = w.S1; q.S2 = w.S2; q.W = w.W; q.Wss1 = w.Wss1; q.Wss2 = w.Wss2; q.o = w.o;
    q.S = m->S; q.SP = m->SP; q.R = m->R; q.Rp = m->Rp; q.farnn = w.farnn;
    int rc;
    auto blocks = [](long long n) { return (unsigned)((n + 255) / 256); };
    for (int dir = 0; dir < 2; dir++) {
        if ((rc = dev_alloc(m, (void **)&k.P2[dir], (size_t)k.n2 * k.ld2 * 4))) return rc;
        if ((rc = dev_alloc(m, (void **)&k.P3[dir], (size_t)k.n3 * k.ld3 * 4))) return rc;
        pack_p2_kernel<<<blocks((long long)k.n2 * k.ld2), 256>>>(q, k.P2[dir], k.n2, k.ld2, dir);
        pack_p3_kernel<<<blocks((long long)k.n3 * k.ld3), 256>>>(q, k.P3[dir], k.ld3, dir);
    }
    if (k.n1) {
        if ((rc = dev_alloc(m, (void **)&k.P1, (size_t)k.n1 * k.ld2 * 4))) return rc;
        pack_p1_kernel<<<blocks((long long)k.n1 * k.ld2), 256>>>(q, k.P1, k.ld2);
    }
    // the per-word rows a step reads, side by side: [Vgen row | update-gate row | reset-gate row] (one base, one load per prefetch slot)
    if (m->V == 0) {
        k.TVt = nullptr;                    // a vector-input handle: the table is built per call (decomp_vec.hip.h)
    } else if (w.farnn == 0) {
        k.TVt = w.Vgen;
    } else {
        float *T = nullptr;
        if ((rc = dev_alloc(m, (void **)&T, (size_t)m->V * tvl * 4))) return rc;
        word_rows_kernel<<<blocks((long long)m->V * m->Rp), 256>>>(w.Vgen, T, tvl, m->V, m->Rp);
        gate_table_kernel<<<blocks((long long)m->V * m->SP), 256>>>(w.Vgen, w.Wrs1, w.bs1, T, tvl, m->Rp, m->V, m->R, m->Rp, m->S, m->SP);
        if (w.farnn == 2)
            gate_table_kernel<<<blocks((long long)m->V * m->SP), 256>>>(w.Vgen, w.Wrs2, w.bs2, T, tvl, m->Rp + m->SP, m->V, m->R, m->Rp, m->S, m->SP);
        k.TVt = T;
    }
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipDeviceSynchronize());
    k.ok = true;
    return FARNN_OK;
}

// ---- shared by the three decomposed creates: factor tables of the recurrence ---------------------
struct GateSrc { int farnn; const float *Wss1, *Wrs1, *bs1, *Wss2, *Wrs2, *bs2; };

static int check_gates(const GateSrc &g, const char *who) {
    if (g.farnn < 0 || g.farnn > 2) return fail(FARNN_EINVAL, "%s: farnn must be 0, 1 or 2%s", who, "");
    if (g.farnn >= 1 && (!g.Wss1 || !g.Wrs1 || !g.bs1))
        return fail(FARNN_EINVAL, "%s: farnn>=1 needs Wss1/Wrs1/bs1%s", who, "");
    if (g.farnn == 2 && (!g.Wss2 || !g.Wrs2 || !g.bs2))
        return fail(FARNN_EINVAL, "%s: farnn==2 needs Wss2/Wrs2/bs2%s", who, "");
    return FARNN_OK;
}

// Vgen [V,R], S1/S2 [S,R], W [S,S] dense row-major; each with its own host|device flag.
static int upload_chain_factors(farnn_model *m, const float *Vgen, int odV, const float *S1, const float *S2,
                                int odS, const float *W, int odW, const GateSrc &g, int odG) {
    DecompWeights &w = m->dw;
    int rc;
    w.S = m->S; w.SP = m->SP; w.R = m->R; w.Rp = m->Rp; w.V = m->V;
    w.farnn = g.farnn; w.nl = m->nl; w.semiring = m->semiring; w.sig_k = m->sig_k;
    float *tmp = nullptr;
    if (m->V > 0) { if ((rc = upload_padded(m, &tmp, Vgen, m->V, m->R, m->V, m->Rp, odV))) return rc; w.Vgen = tmp; }   // (V = 0: a vector-input handle)
    if ((rc = upload_padded(m, &tmp, S1, m->S, m->R, m->S, m->Rp, odS))) return rc; w.S1 = tmp;
    if ((rc = upload_padded(m, &tmp, S2, m->S, m->R, m->S, m->Rp, odS))) return rc; w.S2 = tmp;
    if ((rc = upload_transposed(m, &tmp, S1, m->S, m->R, m->SP, odS))) return rc; w.S1T = tmp;
    if ((rc = upload_transposed(m, &tmp, S2, m->S, m->R, m->SP, odS))) return rc; w.S2T = tmp;
    if ((rc = upload_padded(m, &tmp, W, m->S, m->S, m->S, m->SP, odW))) return rc; w.W = tmp;
    if ((rc = upload_transposed(m, &tmp, W, m->S, m->S, m->SP, odW))) return rc; w.WT = tmp;
    if (g.farnn >= 1) {
        if ((rc = upload_padded(m, &tmp, g.Wss1, m->S, m->S, m->S, m->SP, odG))) return rc; w.Wss1 = tmp;
        if ((rc = upload_padded(m, &tmp, g.Wrs1, m->R, m->S, m->R, m->SP, odG))) return rc; w.Wrs1 = tmp;
        if ((rc = dev_upload(m, &tmp, g.bs1, m->S, m->SP, odG))) return rc; w.bs1 = tmp;
    }
    if (g.farnn == 2) {
        if ((rc = upload_padded(m, &tmp, g.Wss2, m->S, m->S, m->S, m->SP, odG))) return rc; w.Wss2 = tmp;
        if ((rc = upload_padded(m, &tmp, g.Wrs2, m->R, m->S, m->R, m->SP, odG))) return rc; w.Wrs2 = tmp;
        if ((rc = dev_upload(m, &tmp, g.bs2, m->S, m->SP, odG))) return rc; w.bs2 = tmp;
    }
    return FARNN_OK;
}

static int upload_ones_o(farnn_model *m) {
    std::vector<float> ones((size_t)m->SP, 1.0f);
    int rc = dev_upload(m, &m->o, ones.data(), m->SP, m->SP, 0);
    if (rc) return rc;
    m->dw.o = m->o;
    m->o_ones = true;
    return FARNN_OK;
}

// the sizes and switches the three decomposed descs share
static_assert(64 * SCORE_KCH == 256, "the label-column limit of the decomposed creates");
template <typename Desc>
static int decomp_geometry(farnn_model *m, const Desc *d) {
    m->V = d->V; m->S = d->S; m->R = d->R;
    set_labels(m, d->K);
    m->C = d->use_crf ? d->K - 2 : d->K;
    m->SP = round_up(d->S, 4); m->Rp = round_up(d->R, 4);
    m->nl = d->nl; m->semiring = d->semiring; m->threshold = d->threshold; m->o_idx = d->o_idx;
    m->use_crf = d->use_crf ? 1 : 0; m->farnn_gate = d->farnn; m->sig_k = d->sigmoid_exponent;
    return m->K > 256 ? fail(FARNN_ERANGE, "more than 256 label columns%s%s") : FARNN_OK;
}

// ---- create: decomposed i-FST ------------------------------------------------------------------
// The two block images of a max-semiring vector-input call, 2 B L SR SP 4 bytes, live in the handle's grow-only workspace.  The
// cap keeps one handle from taking the device: 1 024 x 128 positions at S = 104 are 131 072 blocks of SR x SP = 110 x 104
// floats, 12.0 GB for both images -- the largest batch the tagging benchmarks run -- and stay on the dense route under
// 16 GiB, a sixteenth of the card's 288 GB; a larger call tags through decomp_chain_kernel, slower but in B L Rp 4 bytes.
constexpr size_t SF_MAX_BLOCK_BYTES = (size_t)16 << 30;

// od_vgen / od_s12: Vgen resp. S1, S2 are device pointers whatever d->weights_on_device says (the folded creator)
// sf: the vector-input handle (farnn_decomp_sf_create): V = 0 and no Vgen, nothing per word is ever built
// sf_max (with sf): its max-semiring form (farnn_decomp_sf_max_create)
static int decomp_ifst_create_impl(const farnn_decomp_ifst_desc *d, int device, farnn_model **out, int od_vgen, int od_s12, bool sf = false, bool sf_max = false) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (sf && (d->V != 0 || d->Vgen)) return fail(FARNN_EINVAL, "decomp_sf: V must be 0 and Vgen NULL (the vectors come with every call)%s%s");
    if ((!sf && (d->V <= 0 || !d->Vgen)) || d->S <= 0 || d->R <= 0 || d->K <= 0 || !d->S1 || !d->S2 || !d->W ||
        !d->Cout || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "decomp_ifst: sizes must be positive and factor pointers non-null%s%s");
    if (sf && !sf_max && d->semiring != FARNN_SEMIRING_SUM)
        return fail(FARNN_EINVAL, "decomp_sf: the max semiring needs an S x S block per token; vector input exists in the sum semiring only%s%s");
    if (sf_max && d->semiring != FARNN_SEMIRING_MAX)
        return fail(FARNN_EINVAL, "decomp_sf_max: the descriptor's semiring must be FARNN_SEMIRING_MAX (the sum semiring: farnn_decomp_sf_create)%s%s");
    const GateSrc gates{d->farnn, d->Wss1, d->Wrs1, d->bs1, d->Wss2, d->Wrs2, d->bs2};
    if ((rc = check_gates(gates, "decomp_ifst"))) return rc;
    if (d->nl < 0 || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "decomp_ifst: bad nl%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_DECOMP, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    if ((rc = decomp_geometry(m, d))) return rc;
    if (m->S > 1024 || m->R > 4096) return fail(FARNN_ERANGE, "decomp_ifst: S<=1024, R<=4096%s%s");
    const int od = d->weights_on_device;
    if ((rc = upload_chain_factors(m, d->Vgen, od | od_vgen, d->S1, d->S2, od | od_s12, d->W, od, gates, od))) return rc;
    if ((rc = build_output_matrix(m, d->Cout, m->K, od))) return rc;
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    if ((rc = upload_decode_tables(m, d->P, d->crf_trans, od))) return rc;
    if ((rc = build_rows_pack(m))) return rc;
    if (sf_max) {
        // the dense route's test is build_dense_blocks' own; nothing is built here: the blocks are the call's (farnn_reserve, plan_tag)
        m->sf = m->sf_max = true;
        pick_chain_geometry(m);
        m->sf_dense = m->dw.farnn == 0 && m->geom.NCH <= 4 && m->geom.SP == m->SP;
        m->sf_block_tokens = (long long)(SF_MAX_BLOCK_BYTES / (2 * (size_t)m->geom.SR * m->SP * sizeof(float)));
    } else if (sf) {
        // decomp_chain_kernel (the fallback behind the packed rows) reads rows at stride Rp and computes its gates itself: it is not
        // served from the token table, its shapes are refused (include/farnn.h)
        if (!m->rows.ok) return fail(FARNN_ERANGE, "decomp_sf: a per-token row of more than %s floats (Rp + SP per gate) is not supported%s", "2048", "");
        m->sf = true;
    } else if ((rc = build_dense_blocks(m))) return rc;
    *out = own.release();
    return FARNN_OK;
}

extern "C" int farnn_decomp_ifst_create(const farnn_decomp_ifst_desc *d, int device, farnn_model **out) {
    return decomp_ifst_create_impl(d, device, out, 0, 0);
}

extern "C" int farnn_decomp_sf_create(const farnn_decomp_ifst_desc *d, int device, farnn_model **out) {
    return decomp_ifst_create_impl(d, device, out, 0, 0, true);
}

extern "C" int farnn_decomp_sf_max_create(const farnn_decomp_ifst_desc *d, int device, farnn_model **out) {
    return decomp_ifst_create_impl(d, device, out, 0, 0, true, true);
}

// largest eigenvalue of a symmetric positive semi-definite n x n matrix (a Gram matrix; doubles; n <= a few hundred: create time).
// Only the top eigenvalue is needed (the spectral norm of a factor matrix): power iteration on A -- with A squared a few times
// first, so that the eigenvalue ratio that governs convergence is raised to the 2^k-th power -- instead of diagonalising the
// matrix (a cyclic Jacobi sweep is n^2/2 rotations of 4n updates; 60 sweeps at n = 250 were seconds of host time per create).
static double gram_largest_eigenvalue(std::vector<double> &A, int n) {
    if (n <= 0) return 0.0;
    auto matmul_sq = [&](std::vector<double> &M) {       // M <- M . M / trace-scale (keeps the numbers in range)
        double tr = 0.0;
        for (int i = 0; i < n; i++) tr += M[(size_t)i * n + i];
        if (!(tr > 0.0)) return 0.0;
        std::vector<double> N((size_t)n * n, 0.0);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < n; k++) {
                const double a = M[(size_t)i * n + k] / tr;
                if (a == 0.0) continue;
                for (int j = 0; j < n; j++) N[(size_t)i * n + j] += a * (M[(size_t)k * n + j] / tr);
            }
        M.swap(N);
        return tr;
    };
    // lambda_max(A) from the Rayleigh quotient of the dominant eigenvector of A^(2^k): same eigenvector
    std::vector<double> B = A;
    for (int k = 0; k < 6; k++)
        if (!(matmul_sq(B) > 0.0)) return 0.0;
    std::vector<double> v((size_t)n), w((size_t)n);
    for (int i = 0; i < n; i++) v[i] = 1.0 + 1e-3 * ((i * 2654435761u) % 1000);   // (not orthogonal to anything in particular)
    double lam = 0.0;
    for (int it = 0; it < 200; it++) {
        const std::vector<double> &M = it < 8 ? B : A;   // a few steps on A^(64) to land on the eigenvector, then refine on A itself
        double nrm = 0.0;
        for (int i = 0; i < n; i++) { double acc = 0.0; for (int j = 0; j < n; j++) acc += M[(size_t)i * n + j] * v[j]; w[i] = acc; nrm += acc * acc; }
        nrm = sqrt(nrm);
        if (!(nrm > 0.0)) return 0.0;
        for (int i = 0; i < n; i++) v[i] = w[i] / nrm;
        if (it >= 8) {
            double num = 0.0;                            // Rayleigh quotient v^T A v (v has unit length)
            for (int i = 0; i < n; i++) { double acc = 0.0; for (int j = 0; j < n; j++) acc += A[(size_t)i * n + j] * v[j]; num += v[i] * acc; }
            if (fabs(num - lam) <= 1e-14 * fabs(num)) { lam = num; break; }
            lam = num;
        }
    }
    return lam;
}

extern "C" int farnn_decomp_ifst_create_folded(const farnn_decomp_ifst_desc *d, const farnn_vgen_fold *f, int device,
                                               farnn_model **out) {
    int rc = begin_create(d && f, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->R <= 0 || f->D <= 0 || !f->V_embed || !f->E || !f->G || !f->beta || !d->S1 || !d->S2)
        return fail(FARNN_EINVAL, "decomp_ifst_create_folded: V_embed / E / G / beta / S1 / S2 and positive sizes needed%s%s");
    if (f->add_nl < FARNN_NL_NONE || f->add_nl > FARNN_NL_SIGMOID) return fail(FARNN_EINVAL, "decomp_ifst_create_folded: bad add_nl%s%s");
    if (f->normalize < FARNN_NORM_NONE || f->normalize > FARNN_NORM_L2_RANK)
        return fail(FARNN_EINVAL, "decomp_ifst_create_folded: bad normalize mode%s%s");
    if ((rc = select_device(device))) return rc;
    const size_t V = d->V, R = d->R, S = d->S, D = f->D;
    DevTmp tmp;
    float *Vd = nullptr, *S1d = nullptr, *S2d = nullptr, *Vgen = nullptr, *avg = nullptr;
    const float *E = nullptr, *G = nullptr, *beta = nullptr;
    if ((rc = tmp.copy(&Vd, f->V_embed, V * R, f->on_device)) || (rc = tmp.copy(&S1d, d->S1, S * R, d->weights_on_device)) ||
        (rc = tmp.copy(&S2d, d->S2, S * R, d->weights_on_device)) || (rc = tmp.view(&E, f->E, V * D, f->on_device)) ||
        (rc = tmp.view(&G, f->G, D * R, f->on_device)) || (rc = tmp.view(&beta, f->beta, R, f->on_device)) ||
        (rc = tmp.raw(&Vgen, V * R)) || (rc = tmp.raw(&avg, 6 * R))) return rc;
    const float *cv = nullptr;
    if (f->normalize == FARNN_NORM_L1 || f->normalize == FARNN_NORM_L2) {
        // whole-matrix modes (utils.py:211-216): numpy's matrix 1-norm (the largest column sum) or 2-norm (the spectral norm) over
        // the element count -- one scalar per matrix.  The column sums / the R x R Gram matrix are formed on the device; R floats /
        // R x R doubles come back, never anything of size V x R.
        const float *mats[3] = {Vd, S1d, S2d};
        const size_t rows[3] = {V, S, S};
        double avgs[3];
        if (f->normalize == FARNN_NORM_L1) {
            for (int q = 0; q < 3; q++) col_avg_norm_kernel<<<(unsigned)R, 256>>>(mats[q], (int)rows[q], (int)R, (int)R, 1, avg + q * R);
            std::vector<float> hv(3 * R);
            FARNN_HIP_TRY(hipMemcpy(hv.data(), avg, 3 * R * 4, hipMemcpyDeviceToHost));
            for (int q = 0; q < 3; q++) {
                float mx = 0.0f;
                for (size_t c = 0; c < R; c++) mx = hv[q * R + c] > mx ? hv[q * R + c] : mx;       // (column sum / rows)
                avgs[q] = (double)mx / (double)R;
            }
        } else {
            double *Gd = nullptr;
            if ((rc = tmp.raw(&Gd, R * R))) return rc;
            std::vector<double> Gh(R * R);
            for (int q = 0; q < 3; q++) {
                gram_kernel<<<dim3((unsigned)R, (unsigned)R), 256>>>(mats[q], (int)rows[q], (int)R, Gd);
                FARNN_HIP_TRY(hipMemcpy(Gh.data(), Gd, R * R * 8, hipMemcpyDeviceToHost));
                avgs[q] = sqrt(gram_largest_eigenvalue(Gh, (int)R)) / ((double)rows[q] * (double)R);
            }
        }
        if (!(avgs[0] > 0.0) || !(avgs[1] > 0.0) || !(avgs[2] > 0.0))
            return fail(FARNN_EINVAL, "decomp_ifst_create_folded: a factor matrix has zero norm%s%s");
        const double fac = cbrt(avgs[0] * avgs[1] * avgs[2]);
        std::vector<float> sc(3 * R);
        for (int q = 0; q < 3; q++)
            for (size_t c = 0; c < R; c++) sc[q * R + c] = (float)(fac / avgs[q]);
        FARNN_HIP_TRY(hipMemcpy(avg + 3 * R, sc.data(), 3 * R * 4, hipMemcpyHostToDevice));
        scale_cols_kernel<<<(unsigned)((S * R + 255) / 256), 256>>>(S1d, (long long)(S * R), (int)R, avg + 4 * R);
        scale_cols_kernel<<<(unsigned)((S * R + 255) / 256), 256>>>(S2d, (long long)(S * R), (int)R, avg + 5 * R);
        cv = avg + 3 * R;
    } else if (f->normalize != FARNN_NORM_NONE) {
        const int ord = f->normalize == FARNN_NORM_L1_RANK ? 1 : 2;
        col_avg_norm_kernel<<<(unsigned)R, 256>>>(Vd, (int)V, (int)R, (int)R, ord, avg);
        col_avg_norm_kernel<<<(unsigned)R, 256>>>(S1d, (int)S, (int)R, (int)R, ord, avg + R);
        col_avg_norm_kernel<<<(unsigned)R, 256>>>(S2d, (int)S, (int)R, (int)R, ord, avg + 2 * R);
        norm_scales_kernel<<<(unsigned)((R + 255) / 256), 256>>>(avg, avg + 3 * R, (int)R);
        scale_cols_kernel<<<(unsigned)((S * R + 255) / 256), 256>>>(S1d, (long long)(S * R), (int)R, avg + 4 * R);
        scale_cols_kernel<<<(unsigned)((S * R + 255) / 256), 256>>>(S2d, (long long)(S * R), (int)R, avg + 5 * R);
        cv = avg + 3 * R;
    }
    fold_vgen_kernel<<<(unsigned)((V * R + 255) / 256), 256>>>(Vd, E, G, beta, cv, Vgen, (int)V, (int)R, (int)D, f->add_nl);
    FARNN_HIP_TRY(hipGetLastError());
    FARNN_HIP_TRY(hipDeviceSynchronize());
    farnn_decomp_ifst_desc full = *d;
    full.Vgen = Vgen; full.S1 = S1d; full.S2 = S2d;
    return decomp_ifst_create_impl(&full, device, out, 1, 1);
}

// ---- create: decomposed independent=1 ----------------------------------------------------------
extern "C" int farnn_decomp_ind1_create(const farnn_decomp_ind1_desc *d, int device, farnn_model **out) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->R <= 0 || d->RO <= 0 || d->K <= 0 || !d->Vgen || !d->S1 || !d->S2 ||
        !d->W || !d->Cout || !d->S1o || !d->S2o || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "decomp_ind1: sizes must be positive and factor pointers non-null%s%s");
    const GateSrc gates{d->farnn, d->Wss1, d->Wrs1, d->bs1, d->Wss2, d->Wrs2, d->bs2};
    if ((rc = check_gates(gates, "decomp_ind1"))) return rc;
    if (d->nl < 0 || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "decomp_ind1: bad nl%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_DECOMP1, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    m->RO = d->RO; m->ROp = round_up(d->RO, 4);
    if ((rc = decomp_geometry(m, d))) return rc;
    if (decomp1_score_lds_bytes(m->S, m->SP, m->Rp, m->ROp, m->Kc) > 160 * 1024)
        return fail(FARNN_ERANGE, "decomp_ind1: S*S*4 bytes of LDS needed per token (S too large)%s%s");
    const int od = d->weights_on_device;
    if ((rc = upload_chain_factors(m, d->Vgen, od, d->S1, d->S2, od, d->W, od, gates, od))) return rc;
    {   // no per-state output scaling in this model: o = 1; the output sum masks the transitions instead
        if ((rc = upload_ones_o(m))) return rc;
        DevTmp tmp;
        const float *Co = nullptr, *S1o = nullptr, *S2o = nullptr, *Wo = nullptr;
        if ((rc = tmp.view(&Co, d->Cout, (size_t)m->K * m->RO, od))) return rc;
        if ((rc = tmp.view(&S1o, d->S1o, (size_t)m->S * m->RO, od))) return rc;
        if ((rc = tmp.view(&S2o, d->S2o, (size_t)m->S * m->RO, od))) return rc;
        if ((rc = tmp.view(&Wo, d->Wo, (size_t)m->S * m->S, od))) return rc;
        float *osum = nullptr;
        if ((rc = dev_alloc(m, (void **)&osum, (size_t)m->S * m->SP * 4))) return rc;
        FARNN_HIP_TRY(hipMemset(osum, 0, (size_t)m->S * m->SP * 4));
        output_sum_kernel<<<(m->S * m->S + 255) / 256, 256>>>(Co, S1o, S2o, Wo, osum, m->K, m->S, m->SP, m->RO);
        FARNN_HIP_TRY(hipGetLastError());
        FARNN_HIP_TRY(hipDeviceSynchronize());
        m->dw.mask = osum;
    }
    if ((rc = upload_padded(m, &m->d1_S1o, d->S1o, m->S, m->RO, m->S, m->ROp, od))) return rc;
    if ((rc = upload_padded(m, &m->d1_S2o, d->S2o, m->S, m->RO, m->S, m->ROp, od))) return rc;
    if ((rc = upload_transposed(m, &m->d1_CoutT, d->Cout, m->K, m->RO, m->Kc, od))) return rc;
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    if ((rc = upload_decode_tables(m, d->P, d->crf_trans, od))) return rc;
    if (m->RO <= 16 * D1M_MAXNT && m->S <= 16 * D1M_MAXKQ4 && (size_t)m->V * m->S * m->SP * 4 <= ((size_t)32 << 30)) {
        // per-word bss table for the MFMA scoring kernel (unmasked: the mask only enters the recurrence),
        // materialised row-major in a scratch buffer, then re-laid-out in MFMA operand order
        const int MT = (m->S + 15) / 16, NT = (m->RO + 15) / 16, KQ4 = MT;
        DevTmp tmp;
        float *bss = nullptr;
        if ((rc = tmp.raw(&bss, (size_t)m->V * m->S * m->SP))) return rc;
        dim3 grid((m->S * m->SP + 255) / 256, m->V);
        materialise_blocks_kernel<<<grid, 256>>>(m->dw.Vgen, m->dw.S1, m->dw.S2, m->dw.W, nullptr, bss, nullptr,
                                                 m->S, m->SP, m->S, m->R, m->Rp);
        const long long total = (long long)m->V * MT * KQ4 * 256;
        if ((rc = dev_alloc(m, (void **)&m->d1_BSSp, (size_t)total * 4)) ||
            (rc = dev_alloc(m, (void **)&m->d1_S1oP, (size_t)MT * NT * 256 * 4)) ||
            (rc = dev_alloc(m, (void **)&m->d1_S2oP, (size_t)KQ4 * NT * 256 * 4))) return rc;
        pack_s2o_operand_kernel<<<(KQ4 * NT * 256 + 255) / 256, 256>>>(m->d1_S2o, m->d1_S2oP, KQ4 * NT * 256,
                                                                      m->S, m->RO, m->ROp, NT);
        pack_bss_operand_kernel<<<(unsigned)((total + 255) / 256), 256>>>(bss, m->d1_BSSp, total, m->S, m->SP, MT, KQ4);
        pack_s1o_operand_kernel<<<(MT * NT * 256 + 255) / 256, 256>>>(m->d1_S1o, m->d1_S1oP, MT * NT * 256,
                                                                     m->S, m->RO, m->ROp, NT);
        FARNN_HIP_TRY(hipGetLastError());
        FARNN_HIP_TRY(hipDeviceSynchronize());
    }
    if ((rc = build_dense_blocks(m))) return rc;
    *out = own.release();
    return FARNN_OK;
}

// ---- create: decomposed independent=0 ----------------------------------------------------------
extern "C" int farnn_decomp_fst_create(const farnn_decomp_fst_desc *d, int device, farnn_model **out) {
    int rc = begin_create(d != nullptr, out);
    if (rc) return rc;
    if (d->V <= 0 || d->S <= 0 || d->R <= 0 || d->RW <= 0 || d->K <= 0 || !d->Vgen || !d->C || !d->S1 ||
        !d->S2 || !d->Cw || !d->S1w || !d->S2w || !d->WW || !d->h0 || !d->hT)
        return fail(FARNN_EINVAL, "decomp_fst: sizes must be positive and factor pointers non-null%s%s");
    const GateSrc gates{d->farnn, d->Wss1, d->Wrs1, d->bs1, d->Wss2, d->Wrs2, d->bs2};
    if ((rc = check_gates(gates, "decomp_fst"))) return rc;
    if (d->nl < 0 || d->nl > FARNN_NL_RELUTANH) return fail(FARNN_EINVAL, "decomp_fst: bad nl%s%s");
    ModelOwner own;
    if ((rc = begin_model(own, KIND_DECOMP0, device))) return rc;
    farnn_model *m = own.get();
    TunScope tun_scope(&m->tun);
    m->RW = d->RW; m->RWp = round_up(d->RW, 4);
    if ((rc = decomp_geometry(m, d))) return rc;
    if (m->S > 1024 || m->R > 4096 || m->RW > 4096)
        return fail(FARNN_ERANGE, "decomp_fst: S<=1024, R<=4096, RW<=4096%s%s");
    const int od = d->weights_on_device;
    {
        // recurrence inputs: table = Vgen * sum_c C (:253), W = sum_q (sum_c Cw) S1w S2w + WW (:319-324)
        DevTmp tmp;
        const float *Cd = nullptr, *Cwd = nullptr, *S1wd = nullptr, *S2wd = nullptr, *WWd = nullptr;
        if ((rc = tmp.view(&Cd, d->C, (size_t)m->K * m->R, od))) return rc;
        if ((rc = tmp.view(&Cwd, d->Cw, (size_t)m->K * m->RW, od))) return rc;
        if ((rc = tmp.view(&S1wd, d->S1w, (size_t)m->S * m->RW, od))) return rc;
        if ((rc = tmp.view(&S2wd, d->S2w, (size_t)m->S * m->RW, od))) return rc;
        if ((rc = tmp.view(&WWd, d->WW, (size_t)m->S * m->S, od))) return rc;
        float *table = nullptr, *wsum = nullptr;
        if ((rc = tmp.copy(&table, d->Vgen, (size_t)m->V * m->R, od))) return rc;
        if ((rc = tmp.raw(&wsum, (size_t)m->S * m->S))) return rc;
        const long long n = (long long)m->V * m->R;
        scale_by_colsum_kernel<<<(unsigned)((n + 255) / 256), 256>>>(table, Cd, m->V, m->R, m->K);
        output_sum_kernel<<<(m->S * m->S + 255) / 256, 256>>>(Cwd, S1wd, S2wd, WWd, wsum, m->K, m->S, m->S, m->RW);
        FARNN_HIP_TRY(hipGetLastError());
        FARNN_HIP_TRY(hipDeviceSynchronize());
        if ((rc = upload_chain_factors(m, table, 1, d->S1, d->S2, od, wsum, 1, gates, od))) return rc;
    }
    if ((rc = upload_ones_o(m))) return rc;
    if ((rc = upload_padded(m, &m->d0_Vgen, d->Vgen, m->V, m->R, m->V, m->Rp, od))) return rc;
    if ((rc = upload_transposed(m, &m->d0_CT, d->C, m->K, m->R, m->Kc, od))) return rc;
    if ((rc = upload_padded(m, &m->d0_S1w, d->S1w, m->S, m->RW, m->S, m->RWp, od))) return rc;
    if ((rc = upload_padded(m, &m->d0_S2w, d->S2w, m->S, m->RW, m->S, m->RWp, od))) return rc;
    if ((rc = upload_transposed(m, &m->d0_CwT, d->Cw, m->K, m->RW, m->Kc, od))) return rc;
    if ((rc = upload_start_final(m, d->h0, d->hT, od))) return rc;
    if ((rc = upload_decode_tables(m, d->P, d->crf_trans, od))) return rc;
    if ((rc = build_rows_pack(m))) return rc;
    *out = own.release();
    return FARNN_OK;
}
