// Pitch correction: the shifted f0 of every segment snapped towards the notes of a key, between the f0 shift and everything that
// reads the shifted track (f0 re-rank, pitched concat re-selection, vocoder).  include/knnsvc_hip.h ("Pitch correction") is the
// specification; upstream has no counterpart.
// Harmony voice ("Harmony voice" there): the same note decision, then the note moved by scale degrees and the lead's own contour
// carried over to the part.  One kernel body serves both: steps 1-4 are written once.
#include "common.h"

namespace {

// The four per-segment tables: host tables handed over by value like the segment table (64 x 28 B).
struct KnTuneTable {
    int mask[KNNSVC_MAX_SEGMENTS];
    double sigma[KNNSVC_MAX_SEGMENTS], alpha[KNNSVC_MAX_SEGMENTS], log_ref[KNNSVC_MAX_SEGMENTS];
};

// The harmony's: the degree move in place of the strength.
struct KnHarmonyTable {
    int mask[KNNSVC_MAX_SEGMENTS], steps[KNNSVC_MAX_SEGMENTS];
    double alpha[KNNSVC_MAX_SEGMENTS], log_ref[KNNSVC_MAX_SEGMENTS];
};

// What phase A leaves per frame for the walk of phase B, and phase B for phase C: one 32-byte row, so that the sequential lane
// reads a frame with two 16-byte loads.  m: the pitch in semitones, NaN for an unpitched frame (that is what ends a run);
// c: the centre; d: |c - near(c)| after A, the correction g (harmony: the interval h) after B; note: near(c) after A, the note n
// (harmony: the part's note t) after B.
struct KnTuneRow { double m, c, d; int note, pad; };
static_assert(sizeof(KnTuneRow) == 32, "workspace layout");

constexpr int TU_H = 5;            // half width of the centre's median window
constexpr int TU_WIN = 2 * TU_H + 1;
constexpr int TU_THREADS = 1024;
constexpr int TU_AHEAD = 8;        // rows the sequential lane loads ahead of its recurrence
constexpr double TU_HYST = 0.25;

__device__ __forceinline__ bool tu_allowed(int mask, int k) { return (mask >> (((k % 12) + 12) % 12)) & 1; }

// near(c) and |near(c) - c|: the nearest allowed integer below or at c against the nearest above it, the lower of two equally
// near.  mask != 0, so each search ends within 12 steps.
__device__ __forceinline__ int tu_near(int mask, double c, double* dist) {
#pragma clang fp contract(off)
    const int f = (int)floor(c);
    int kl = f, ku = f + 1;
    for (int t = 0; t < 12 && !tu_allowed(mask, kl); ++t) --kl;
    for (int t = 0; t < 12 && !tu_allowed(mask, ku); ++t) ++ku;
    const double dl = fabs((double)kl - c), du = fabs((double)ku - c);
    *dist = dl <= du ? dl : du;
    return dl <= du ? kl : ku;
}

// The degree move of "Harmony voice", step 5: the allowed note `note` moved by `steps` degrees of the scale `mask` (integers only;
// floor division and a non-negative remainder for negative J and negative notes).
__device__ __forceinline__ int tu_degree_move(int mask, int note, int steps) {
    const int pc = ((note % 12) + 12) % 12;
    const int d = __builtin_popcount((unsigned)mask), j = __builtin_popcount((unsigned)mask & ((1u << pc) - 1u));
    const int oct = (note - pc) / 12;              // exact
    const int J = j + steps;
    int q = J / d, r = J - q * d;
    if (r < 0) { r += d; --q; }
    int p = 0;
    for (int seen = 0; p < 12; ++p)                // the r-th allowed pitch class
        if ((mask >> p) & 1) { if (seen == r) break; ++seen; }
    return 12 * (oct + q) + p;
}

// One segment in three phases over its frames, with the rows of the workspace between them.  HARM = false: pitch correction
// (sigma, alpha); HARM = true: the harmony voice (steps, alpha).  Phases A and the note decision of B are the same code.
template <bool HARM>
__device__ __forceinline__ void tu_segment(const float* __restrict__ x, long n, int mask, bool on, double sigma, int steps, double alpha,
                                           double log_ref, float* __restrict__ y, int* __restrict__ nt, KnTuneRow* __restrict__ row) {
#pragma clang fp contract(off)
    const double LN2 = 0.693147180559945309417232121458, S = LN2 / 12.0;
    const int tid = threadIdx.x;
    if (!on) {                                     // off: the bits, and nothing else is looked at
        const unsigned* xb = (const unsigned*)x;
        unsigned* yb = (unsigned*)y;
        for (long i = tid; i < n; i += TU_THREADS) { yb[i] = xb[i]; if (nt) nt[i] = -1; }
        return;
    }
    // ---- (A1) pitch in semitones, NaN where the frame is not pitched
    for (long i = tid; i < n; i += TU_THREADS) {
        const float f = x[i];
        double m = __builtin_nan("");
        if (f > 0.f && f < __builtin_inff()) m = (log((double)f) - log_ref) / S + 69.0;
        row[i].m = m;
    }
    __syncthreads();
    // ---- (A2) centre: lower median of the run's frames within H of this one, by rank (no arithmetic); its nearest note
    for (long i = tid; i < n; i += TU_THREADS) {
        const double mi = row[i].m;
        if (!(mi == mi)) continue;
        double v[TU_WIN];
        v[TU_H] = mi;
        int cnt = 1;
        bool in = true;                             // still inside the run, walking away from i
#pragma unroll
        for (int t = 1; t <= TU_H; ++t) {
            const long j = i - t;
            double mj = __builtin_inf();
            if (in && j >= 0) { const double r = row[j].m; if (r == r) mj = r; }
            in = mj != __builtin_inf();             // (a pitched m is finite)
            cnt += in ? 1 : 0;
            v[TU_H - t] = mj;
        }
        in = true;
#pragma unroll
        for (int t = 1; t <= TU_H; ++t) {
            const long j = i + t;
            double mj = __builtin_inf();
            if (in && j < n) { const double r = row[j].m; if (r == r) mj = r; }
            in = mj != __builtin_inf();
            cnt += in ? 1 : 0;
            v[TU_H + t] = mj;
        }
        const int want = (cnt - 1) / 2;             // frames outside the run hold +inf and rank last
        double c = mi;
#pragma unroll
        for (int a = 0; a < TU_WIN; ++a) {
            int rank = 0;
#pragma unroll
            for (int b = 0; b < TU_WIN; ++b) rank += (v[b] < v[a] || (v[b] == v[a] && b < a)) ? 1 : 0;
            if (rank == want) c = v[a];
        }
        double d;
        const int cand = tu_near(mask, c, &d);
        row[i].c = c; row[i].d = d; row[i].note = cand;
    }
    __syncthreads();
    // ---- (B) the thread whose frame starts a run walks it alone: note with hysteresis, one-pole correction (harmony: the degree
    //      move, looked up again only where the note changes, and the one-pole glide of the interval).  Rows are loaded
    //      TU_AHEAD at a time in front of the recurrence (they do not depend on it); a row beyond the run's end is this segment's.
    for (long i0 = tid; i0 < n; i0 += TU_THREADS) {
        const double m0 = row[i0].m;
        if (!(m0 == m0)) continue;
        if (i0 > 0) { const double mp = row[i0 - 1].m; if (mp == mp) continue; }
        int note = 0, part = 0;
        double g = 0.0;
        bool first = true, open = true;
        for (long base = i0; open && base < n; base += TU_AHEAD) {
            KnTuneRow r[TU_AHEAD];
#pragma unroll
            for (int t = 0; t < TU_AHEAD; ++t) r[t] = row[base + t < n ? base + t : n - 1];
#pragma unroll
            for (int t = 0; t < TU_AHEAD; ++t) {
                if (!open) break;
                if (base + t >= n || !(r[t].m == r[t].m)) { open = false; break; }
                const int held = note;
                if (first) note = r[t].note;
                else if (r[t].d + TU_HYST < fabs(r[t].c - (double)note)) note = r[t].note;
                if (HARM && (first || note != held)) part = tu_degree_move(mask, note, steps);
                const double e = HARM ? (double)(part - note) : (double)note - r[t].m;
                g = first ? e : g + alpha * (e - g);
                first = false;
                row[base + t].d = g; row[base + t].note = HARM ? part : note;
            }
        }
    }
    __syncthreads();
    // ---- (C) the corrected frequency (harmony: the part's)
    for (long i = tid; i < n; i += TU_THREADS) {
        const float f = x[i];
        if (f > 0.f && f < __builtin_inff()) {
            y[i] = (float)exp(log((double)f) + (HARM ? row[i].d : sigma * row[i].d) * S);
            if (nt) nt[i] = row[i].note;
        } else {
            ((unsigned*)y)[i] = ((const unsigned*)x)[i];
            if (nt) nt[i] = -1;
        }
    }
}

// Block s = segment s.
__global__ __launch_bounds__(TU_THREADS) void tune_f0_kernel(const float* __restrict__ f0, const KnSegTable seg, const KnTuneTable tt,
                                                             float* __restrict__ out, int* __restrict__ notes,
                                                             KnTuneRow* __restrict__ ws) {
    const int s = blockIdx.x;
    const long o = seg.off[s], n = seg.off[s + 1] - o;
    tu_segment<false>(f0 + o, n, tt.mask[s], tt.mask[s] != 0 && tt.sigma[s] != 0.0, tt.sigma[s], 0, tt.alpha[s], tt.log_ref[s], out + o,
                      notes ? notes + o : nullptr, ws + o);
}

__global__ __launch_bounds__(TU_THREADS) void harmony_f0_kernel(const float* __restrict__ f0, const KnSegTable seg, const KnHarmonyTable ht,
                                                                float* __restrict__ out, int* __restrict__ notes,
                                                                KnTuneRow* __restrict__ ws) {
    const int s = blockIdx.x;
    const long o = seg.off[s], n = seg.off[s + 1] - o;
    tu_segment<true>(f0 + o, n, ht.mask[s], ht.mask[s] != 0 && ht.steps[s] != 0, 1.0, ht.steps[s], ht.alpha[s], ht.log_ref[s], out + o,
                     notes ? notes + o : nullptr, ws + o);
}

constexpr int64_t TU_MAX_N = (int64_t)1 << 40;

}  // namespace

extern "C" size_t knnsvc_tune_f0_workspace_bytes(int64_t n_total, int32_t n_seg) {
    if (n_seg < 1 || n_seg > KNNSVC_MAX_SEGMENTS || n_total < n_seg || n_total > TU_MAX_N) {
        knnsvc_fail(KNNSVC_EINVAL, "tune_f0: bad sizes (%lld rows in %d segments; 1..%d segments of at least one row)",
                    (long long)n_total, (int)n_seg, KNNSVC_MAX_SEGMENTS);
        return 0;
    }
    return (size_t)n_total * sizeof(KnTuneRow);
}

extern "C" int knnsvc_tune_f0_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_mask,
                                  const double* host_sigma, const double* host_alpha, const double* host_log_ref, float* out,
                                  int32_t* notes, void* ws, size_t ws_bytes, void* stream) {
    const char* entry = "tune_f0_seg";
    const double DMAX = 1.79769313486231570815e308;
    KnSegTable seg;
    if (const int rc = kn_seg_table(host_seg, n_seg, entry, &seg)) return rc;
    KN_REQUIRE(host_mask && host_sigma && host_alpha && host_log_ref, "%s: null table", entry);
    KnTuneTable tt;
    for (int s = 0; s < KNNSVC_MAX_SEGMENTS; ++s) { tt.mask[s] = 0; tt.sigma[s] = 0.0; tt.alpha[s] = 1.0; tt.log_ref[s] = 0.0; }
    for (int s = 0; s < n_seg; ++s) {
        const int m = host_mask[s];
        const double sg = host_sigma[s], a = host_alpha[s], lr = host_log_ref[s];
        KN_REQUIRE(m >= 0 && m <= 0xFFF, "%s: segment %d: mask 0x%x outside 0..0xFFF (bit k: pitch class k, C = 0)", entry, s, (unsigned)m);
        KN_REQUIRE(sg >= 0.0 && sg <= 1.0, "%s: segment %d: sigma %g is not a number in [0, 1]", entry, s, sg);
        KN_REQUIRE(a > 0.0 && a <= 1.0, "%s: segment %d: alpha %g is not a number in (0, 1]", entry, s, a);
        KN_REQUIRE(lr >= -DMAX && lr <= DMAX, "%s: segment %d: log_ref %g is not finite", entry, s, lr);
        tt.mask[s] = m; tt.sigma[s] = sg; tt.alpha[s] = a; tt.log_ref[s] = lr;
    }
    KN_REQUIRE(f0 && out && ws, "%s: null pointer", entry);
    KN_REQUIRE(out != f0, "%s: out must not be the input", entry);
    KN_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: workspace must be 8-byte aligned", entry);
    const size_t need = knnsvc_tune_f0_workspace_bytes(seg.off[seg.n], n_seg);
    if (need == 0) return KNNSVC_EINVAL;
    if (ws_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", entry, ws_bytes, need);
    hipLaunchKernelGGL(tune_f0_kernel, dim3((unsigned)seg.n), dim3(TU_THREADS), 0, (hipStream_t)stream, f0, seg, tt, out, (int*)notes,
                       (KnTuneRow*)ws);
    return knnsvc_check_launch(entry);
}

extern "C" int knnsvc_harmony_f0_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_mask,
                                     const int32_t* host_steps, const double* host_alpha, const double* host_log_ref, float* out,
                                     int32_t* notes, void* ws, size_t ws_bytes, void* stream) {
    const char* entry = "harmony_f0_seg";
    const double DMAX = 1.79769313486231570815e308;
    KnSegTable seg;
    if (const int rc = kn_seg_table(host_seg, n_seg, entry, &seg)) return rc;
    KN_REQUIRE(host_mask && host_steps && host_alpha && host_log_ref, "%s: null table", entry);
    KnHarmonyTable ht;
    for (int s = 0; s < KNNSVC_MAX_SEGMENTS; ++s) { ht.mask[s] = 0; ht.steps[s] = 0; ht.alpha[s] = 1.0; ht.log_ref[s] = 0.0; }
    for (int s = 0; s < n_seg; ++s) {
        const int m = host_mask[s], st = host_steps[s];
        const double a = host_alpha[s], lr = host_log_ref[s];
        KN_REQUIRE(m >= 0 && m <= 0xFFF, "%s: segment %d: mask 0x%x outside 0..0xFFF (bit k: pitch class k, C = 0)", entry, s, (unsigned)m);
        KN_REQUIRE(st >= -KNNSVC_HARMONY_MAX_STEPS && st <= KNNSVC_HARMONY_MAX_STEPS, "%s: segment %d: steps %d outside -%d..%d", entry, s,
                   st, KNNSVC_HARMONY_MAX_STEPS, KNNSVC_HARMONY_MAX_STEPS);
        KN_REQUIRE(a > 0.0 && a <= 1.0, "%s: segment %d: alpha %g is not a number in (0, 1]", entry, s, a);
        KN_REQUIRE(lr >= -DMAX && lr <= DMAX, "%s: segment %d: log_ref %g is not finite", entry, s, lr);
        ht.mask[s] = m; ht.steps[s] = st; ht.alpha[s] = a; ht.log_ref[s] = lr;
    }
    KN_REQUIRE(f0 && out && ws, "%s: null pointer", entry);
    KN_REQUIRE(out != f0, "%s: out must not be the input", entry);
    KN_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: workspace must be 8-byte aligned", entry);
    const size_t need = knnsvc_tune_f0_workspace_bytes(seg.off[seg.n], n_seg);
    if (need == 0) return KNNSVC_EINVAL;
    if (ws_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", entry, ws_bytes, need);
    hipLaunchKernelGGL(harmony_f0_kernel, dim3((unsigned)seg.n), dim3(TU_THREADS), 0, (hipStream_t)stream, f0, seg, ht, out, (int*)notes,
                       (KnTuneRow*)ws);
    return knnsvc_check_launch(entry);
}
