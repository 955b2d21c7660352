// libfarnn_hip.so -- the device-side scorer of an epoch's loss and tag metrics (farnn_score_*; include/farnn.h, DESIGN.md row
// f10).  One launch per batch counts what metrics/metrics.py computes from the flat list of every batch: token counts, B- counts in
// total and per type, each type's first start, and the span matches in their streaming form (include/farnn.h spells the rule).
//
// The launch is ONE workgroup of SC_WAVES wavefronts; a wavefront takes a sequence at a time, 64 positions per pass:
//   phase 0  (wavefront 0)  64 lengths per pass: each sequence's flat offset (a shuffle scan) and the nearest non-empty sequence
//                           before it (a ballot and a count-leading-zeros under the lane mask), into the work buffer
//   phase 1  (every one)    per pass: the table lookups, the links against the left neighbour (lane 0: the last lane of the pass
//                           before, the last token of the nearest non-empty sequence before, or what the previous add left), a
//                           ballot of the EVENT positions (not both links true) and each event's previous event by
//                           count-leading-zeros.  A candidate lives from the event that opens it to the very next event, so
//                           "both links false here and the previous event opened type t" is a match of type t.  Per sequence it
//                           leaves the class of its first event and what its last event opened.
//   phase 2  (wavefront 0)  64 sequences per pass: each sequence's first event against the last event of the nearest sequence
//                           before it that has one (the same ballot), then the carry for the next add and the loss addition.
// Totals are ballot population counts kept per wavefront and added once at its end; per-type counts and first starts are 64-bit
// integer atomics at the B- positions: no order can change any of them.  The work buffer is global memory written and read by
// the one workgroup, across __syncthreads().
#include <hip/hip_runtime.h>
#include <vector>

#include "common.hip.h"
#include "host_util.hip.h"

using namespace farnn;

namespace farnn {

constexpr int SC_WAVES = 16;                 // sequences in flight: one per wavefront of the workgroup
constexpr int SC_THREADS = WAVE * SC_WAVES;
// the handle's device words (64-bit each): counts, then what one add leaves for the next, then [5][n_types] from SC_HEAD
enum { SC_N, SC_SAME, SC_CANON, SC_TP, SC_FP, SC_FN, SC_PSPANS, SC_GSPANS, SC_MATCH, SC_ERR, SC_ADDS, SC_LOSS,
       SC_FLAT, SC_LASTP, SC_LASTG, SC_ALIVE, SC_HEAD };
enum { SC_T_PRED, SC_T_GOLD, SC_T_MATCH, SC_T_FIRSTP, SC_T_FIRSTG, SC_T_ROWS };
constexpr int SC_NO_EVENT = -2;              // ScoreSeq::last of a sequence without an event (-1: its last event opened nothing)

struct ScoreSeq {                            // the work buffer, per sequence
    long long off;                           // valid tokens of the batch before it
    int len, prevne;                         // clamped length; the nearest non-empty sequence before it (-1: none in this batch)
    int first, last;                         // first event: 0 none, 1 one link false, 2 both false; last event: the type it opened
};

struct ScoreArgs {
    const int *kind, *type, *canon;          // [n_labels] each
    int n_labels, n_types;
    long long o_idx;
    unsigned long long *st;
    ScoreSeq *seq;
    const int *tags;
    const long long *labels, *lengths;
    int B, L;
    const float *loss;
};

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int top_lane(unsigned long long m) { return 63 - __clzll((long long)m); }     // m != 0

// kind and type of an id as the LEFT NEIGHBOUR of a position (an id outside the tables is kind 0; it was counted where it stood)
__device__ __forceinline__ void score_prev_lookup(const ScoreArgs &a, long long id, int &k, int &t) {
    const bool in = id >= 0 && id < a.n_labels;
    k = in ? a.kind[id] : 0;
    t = in ? a.type[id] : -1;
}

__global__ void __launch_bounds__(SC_THREADS) score_add_kernel(ScoreArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *const st = a.st;
    // what the previous add left (read by everyone before anything is written: the writes are behind both barriers)
    const long long flat0 = (long long)st[SC_FLAT], carry_p = (long long)st[SC_LASTP], carry_g = (long long)st[SC_LASTG];
    const int alive0 = (int)(long long)st[SC_ALIVE];
    long long total = 0;                     // (wavefront 0) valid tokens of this batch
    int lastne = -1, lastlen = 0;            // (wavefront 0) the last non-empty sequence and its length

    if (wave == 0) {
        for (int c0 = 0; c0 < a.B; c0 += WAVE) {
            const int b = c0 + lane;
            const int len = b < a.B ? clamp_len(a.lengths[b], a.L) : 0;
            long long s = len;               // inclusive scan of the 64 lengths
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const long long o = __shfl_up(s, d, WAVE);
                if (lane >= d) s += o;
            }
            const unsigned long long ne = __ballot(len > 0);
            const unsigned long long below = ne & lanes_below(lane);
            if (b < a.B) {
                ScoreSeq q;
                q.off = total + s - len; q.len = len; q.prevne = below ? c0 + top_lane(below) : lastne;
                q.first = 0; q.last = SC_NO_EVENT;
                a.seq[b] = q;
            }
            total += __shfl(s, WAVE - 1, WAVE);
            if (ne) { const int t = top_lane(ne); lastne = c0 + t; lastlen = __shfl(len, t, WAVE); }
        }
    }
    __syncthreads();

    unsigned c_n = 0, c_same = 0, c_canon = 0, c_tp = 0, c_fp = 0, c_fn = 0, c_ps = 0, c_gs = 0, c_match = 0, c_err = 0;
    for (int b = wave; b < a.B; b += SC_WAVES) {                     // (wave-uniform)
        const ScoreSeq q = a.seq[b];
        if (q.len == 0) continue;
        long long ip = carry_p, ig = carry_g;
        if (q.prevne >= 0) {
            const size_t at = (size_t)q.prevne * a.L + (a.seq[q.prevne].len - 1);
            ip = a.tags[at]; ig = a.labels[at];
        }
        int lkP, ltP, lkG, ltG;              // the left neighbour of lane 0
        score_prev_lookup(a, ip, lkP, ltP);
        score_prev_lookup(a, ig, lkG, ltG);
        int seq_first = 0, seq_last = SC_NO_EVENT;
        const size_t row = (size_t)b * a.L;
        for (int base = 0; base < q.len; base += WAVE) {
            const int j = base + lane;
            const bool valid = j < q.len;
            const long long p = valid ? (long long)a.tags[row + j] : 0, g = valid ? a.labels[row + j] : 0;
            const bool inP = p >= 0 && p < a.n_labels, inG = g >= 0 && g < a.n_labels;
            const int kP = inP ? a.kind[p] : 0, tP = inP ? a.type[p] : -1;
            const int kG = inG ? a.kind[g] : 0, tG = inG ? a.type[g] : -1;
            const long long cP = inP ? (long long)a.canon[p] : p, cG = inG ? (long long)a.canon[g] : g;
            int ukP = __shfl_up(kP, 1, WAVE), utP = __shfl_up(tP, 1, WAVE), ukG = __shfl_up(kG, 1, WAVE), utG = __shfl_up(tG, 1, WAVE);
            if (lane == 0) { ukP = lkP; utP = ltP; ukG = lkG; utG = ltG; }
            const bool linkP = kP == 2 && ukP != 0 && tP == utP, linkG = kG == 2 && ukG != 0 && tG == utG;
            const bool event = valid && !(linkP && linkG), both = valid && !linkP && !linkG;
            const int opens = (valid && kP == 1 && kG == 1 && tP == tG) ? tP : -1;      // (B- has no link: an opener is a `both` event)
            const unsigned long long evm = __ballot(event), bothm = __ballot(both);
            const unsigned long long below = evm & lanes_below(lane);
            int prev_open = __shfl(opens, below ? top_lane(below) : 0, WAVE);
            if (!below) prev_open = seq_last;                        // the event before this pass (SC_NO_EVENT: of an earlier sequence)
            const bool match = both && prev_open >= 0;
            if (match && prev_open < a.n_types) atomicAdd(&st[SC_HEAD + (size_t)SC_T_MATCH * a.n_types + prev_open], 1ull);
            c_match += __popcll(__ballot(match));
            if (evm) {
                if (seq_last == SC_NO_EVENT && seq_first == 0) seq_first = ((bothm >> (__ffsll((long long)evm) - 1)) & 1) ? 2 : 1;
                seq_last = __shfl(opens, top_lane(evm), WAVE);
            }
            const bool same = valid && p == g;
            const bool predB = valid && kP == 1, goldB = valid && kG == 1;
            c_n += __popcll(__ballot(valid));
            c_same += __popcll(__ballot(same));
            c_canon += __popcll(__ballot(valid && cP == cG));
            c_tp += __popcll(__ballot(same && p != a.o_idx));
            c_fp += __popcll(__ballot(valid && !same && p != a.o_idx));
            c_fn += __popcll(__ballot(valid && !same && g != a.o_idx));
            c_ps += __popcll(__ballot(predB));
            c_gs += __popcll(__ballot(goldB));
            c_err += __popcll(__ballot(valid && !(inP && inG)));
            const unsigned long long flat = (unsigned long long)(flat0 + q.off + j);
            if (predB && tP >= 0 && tP < a.n_types) {
                atomicAdd(&st[SC_HEAD + (size_t)SC_T_PRED * a.n_types + tP], 1ull);
                atomicMin(&st[SC_HEAD + (size_t)SC_T_FIRSTP * a.n_types + tP], flat);
            }
            if (goldB && tG >= 0 && tG < a.n_types) {
                atomicAdd(&st[SC_HEAD + (size_t)SC_T_GOLD * a.n_types + tG], 1ull);
                atomicMin(&st[SC_HEAD + (size_t)SC_T_FIRSTG * a.n_types + tG], flat);
            }
            // the left neighbour of the next pass's lane 0 (there is a next pass only if lane 63 is valid)
            lkP = __shfl(kP, WAVE - 1, WAVE); ltP = __shfl(tP, WAVE - 1, WAVE);
            lkG = __shfl(kG, WAVE - 1, WAVE); ltG = __shfl(tG, WAVE - 1, WAVE);
        }
        if (lane == 0) { a.seq[b].first = seq_first; a.seq[b].last = seq_last; }
    }
    if (lane == 0) {
        if (c_n) atomicAdd(&st[SC_N], (unsigned long long)c_n);
        if (c_same) atomicAdd(&st[SC_SAME], (unsigned long long)c_same);
        if (c_canon) atomicAdd(&st[SC_CANON], (unsigned long long)c_canon);
        if (c_tp) atomicAdd(&st[SC_TP], (unsigned long long)c_tp);
        if (c_fp) atomicAdd(&st[SC_FP], (unsigned long long)c_fp);
        if (c_fn) atomicAdd(&st[SC_FN], (unsigned long long)c_fn);
        if (c_ps) atomicAdd(&st[SC_PSPANS], (unsigned long long)c_ps);
        if (c_gs) atomicAdd(&st[SC_GSPANS], (unsigned long long)c_gs);
        if (c_match) atomicAdd(&st[SC_MATCH], (unsigned long long)c_match);
        if (c_err) atomicAdd(&st[SC_ERR], (unsigned long long)c_err);
    }
    __syncthreads();
    if (wave != 0) return;

    int alive = alive0;                      // the type the last event of the stream so far opened (-1: nothing)
    unsigned r_match = 0;
    for (int c0 = 0; c0 < a.B; c0 += WAVE) {
        const int b = c0 + lane;
        const int first = b < a.B ? a.seq[b].first : 0, last = b < a.B ? a.seq[b].last : SC_NO_EVENT;
        const unsigned long long has = __ballot(last != SC_NO_EVENT);
        const unsigned long long below = has & lanes_below(lane);
        int prev_open = __shfl(last, below ? top_lane(below) : 0, WAVE);
        if (!below) prev_open = alive;
        const bool match = first == 2 && prev_open >= 0;
        if (match && prev_open < a.n_types) atomicAdd(&st[SC_HEAD + (size_t)SC_T_MATCH * a.n_types + prev_open], 1ull);
        r_match += __popcll(__ballot(match));
        if (has) alive = __shfl(last, top_lane(has), WAVE);
    }
    if (lane == 0) {
        if (r_match) atomicAdd(&st[SC_MATCH], (unsigned long long)r_match);
        st[SC_ALIVE] = (unsigned long long)(long long)alive;
        st[SC_FLAT] = (unsigned long long)(flat0 + total);
        if (lastne >= 0) {
            const size_t at = (size_t)lastne * a.L + (lastlen - 1);
            st[SC_LASTP] = (unsigned long long)(long long)a.tags[at];
            st[SC_LASTG] = (unsigned long long)a.labels[at];
        }
        st[SC_ADDS] += 1ull;
        if (a.loss) {                        // the one double addition, in stream order (Python's avg_loss += float(loss))
            double *sum = reinterpret_cast<double *>(&st[SC_LOSS]);
            *sum = *sum + (double)*a.loss;
        }
    }
}

__global__ void score_reset_kernel(unsigned long long *st, int n_types) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = SC_HEAD + (size_t)SC_T_ROWS * n_types;
    if (i >= n) return;
    unsigned long long v = 0;                                        // (SC_LOSS: the bits of 0.0)
    if (i == SC_LASTP || i == SC_LASTG || i == SC_ALIVE) v = ~0ull;  // -1: no token yet, nothing open
    if (i >= SC_HEAD + (size_t)SC_T_FIRSTP * n_types) v = ~0ull;     // no start yet (atomicMin)
    st[i] = v;
}

}  // namespace farnn

struct farnn_score {
    int device = 0;
    int n_labels = 0, n_types = 0, o_idx = 0;
    size_t words = 0;                        // SC_HEAD + SC_T_ROWS * n_types
    DevBuf<int> tables;                      // kind, type, canon
    DevBuf<unsigned long long> st;
    DevBuf<ScoreSeq> seq;                    // grows with B
    unsigned long long *host = nullptr;      // pinned: read's copy of st
};

static int score_reset(farnn_score *h, hipStream_t s) {
    score_reset_kernel<<<(unsigned)((h->words + 255) / 256), 256, 0, s>>>(h->st.p, h->n_types);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

extern "C" int farnn_score_create(farnn_score **out, const int32_t *kind, const int32_t *type, const int32_t *canon, int32_t n_labels,
                                  int32_t n_types, int32_t o_idx, int device) {
    if (!out || !kind || !type || !canon) return fail(FARNN_EINVAL, "score_create: null argument%s%s");
    *out = nullptr;
    if (n_labels <= 0) return fail(FARNN_EINVAL, "score_create: n_labels must be positive%s%s");
    if (n_types < 0) return fail(FARNN_EINVAL, "score_create: n_types cannot be negative%s%s");
    for (int i = 0; i < n_labels; i++) {
        if (kind[i] < 0 || kind[i] > 2) return fail(FARNN_EINVAL, "score_create: a kind must be 0 (other), 1 (B-) or 2 (I-)%s%s");
        if (type[i] < -1 || type[i] >= n_types) return fail(FARNN_EINVAL, "score_create: a type must lie in [-1, n_types)%s%s");
        if (canon[i] < 0 || canon[i] >= n_labels) return fail(FARNN_EINVAL, "score_create: a canon id must lie in [0, n_labels)%s%s");
    }
    int rc;
    if ((rc = select_device(device))) return rc;
    farnn_score *h = new farnn_score();
    h->device = device; h->n_labels = n_labels; h->n_types = n_types; h->o_idx = o_idx;
    h->words = SC_HEAD + (size_t)SC_T_ROWS * n_types;
    const char *oom = "score_create: out of device memory%s%s";
    std::vector<int> tab(3 * (size_t)n_labels);
    for (int i = 0; i < n_labels; i++) { tab[i] = kind[i]; tab[n_labels + i] = type[i]; tab[2 * (size_t)n_labels + i] = canon[i]; }
    if ((rc = h->tables.ensure(tab.size(), oom)) || (rc = h->st.ensure(h->words, oom))) { delete h; return rc; }
    if (hipHostMalloc((void **)&h->host, h->words * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        h->host = nullptr;
        delete h;
        return fail(FARNN_ENOMEM, "score_create: out of pinned host memory%s%s");
    }
    if (hipMemcpy(h->tables.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        score_reset(h, nullptr) != FARNN_OK || hipDeviceSynchronize() != hipSuccess) {
        (void)hipHostFree(h->host);
        delete h;
        return fail(FARNN_EIO, "score_create: writing the tables and the counts to the device failed%s%s");
    }
    *out = h;
    return FARNN_OK;
}

extern "C" void farnn_score_destroy(farnn_score *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->host) (void)hipHostFree(h->host);
    delete h;
}

extern "C" int farnn_score_add(farnn_score *h, const int32_t *tags, const int64_t *labels, const int64_t *lengths, int32_t B, int32_t L,
                               const float *loss, void *stream) {
    if (!h || !tags || !labels || !lengths) return fail(FARNN_EINVAL, "score_add: null argument%s%s");
    if (B <= 0 || L <= 0) return fail(FARNN_EINVAL, "score_add: B and L must be positive%s%s");
    FARNN_HIP_TRY(hipSetDevice(h->device));
    int rc;
    if ((rc = h->seq.ensure((size_t)B, "score_add: out of device memory for the per-sequence work buffer%s%s"))) return rc;
    ScoreArgs a;
    a.kind = h->tables.p; a.type = a.kind + h->n_labels; a.canon = a.type + h->n_labels;
    a.n_labels = h->n_labels; a.n_types = h->n_types; a.o_idx = h->o_idx;
    a.st = h->st.p; a.seq = h->seq.p;
    a.tags = tags; a.labels = reinterpret_cast<const long long *>(labels); a.lengths = reinterpret_cast<const long long *>(lengths);
    a.B = B; a.L = L; a.loss = loss;
    score_add_kernel<<<1, SC_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
    FARNN_HIP_TRY(hipGetLastError());
    return FARNN_OK;
}

extern "C" int farnn_score_read(farnn_score *h, farnn_score_counts *c, void *stream) {
    if (!h || !c) return fail(FARNN_EINVAL, "score_read: null argument%s%s");
    FARNN_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FARNN_HIP_TRY(hipMemcpyAsync(h->host, h->st.p, h->words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    FARNN_HIP_TRY(hipStreamSynchronize(s));
    const unsigned long long *w = h->host;
    const long long alive = (long long)w[SC_ALIVE];
    c->n = (int64_t)w[SC_N]; c->same = (int64_t)w[SC_SAME]; c->canon_same = (int64_t)w[SC_CANON];
    c->tp = (int64_t)w[SC_TP]; c->fp = (int64_t)w[SC_FP]; c->fn = (int64_t)w[SC_FN];
    c->pred_spans = (int64_t)w[SC_PSPANS]; c->gold_spans = (int64_t)w[SC_GSPANS];
    c->matches = (int64_t)w[SC_MATCH] + (alive >= 0 ? 1 : 0);       // the stream ends here: an open candidate is a match
    c->errors = (int64_t)w[SC_ERR]; c->adds = (int64_t)w[SC_ADDS];
    memcpy(&c->loss_sum, &w[SC_LOSS], sizeof(double));
    if (c->per_type) {
        const size_t nt = (size_t)h->n_types;
        for (size_t i = 0; i < SC_T_ROWS * nt; i++) c->per_type[i] = (int64_t)w[SC_HEAD + i];     // (no start: ~0 = -1)
        if (alive >= 0 && alive < (long long)nt) c->per_type[SC_T_MATCH * nt + alive] += 1;
    }
    return FARNN_OK;
}

extern "C" int farnn_score_reset(farnn_score *h, void *stream) {
    if (!h) return fail(FARNN_EINVAL, "score_reset: null handle%s%s");
    FARNN_HIP_TRY(hipSetDevice(h->device));
    return score_reset(h, reinterpret_cast<hipStream_t>(stream));
}
