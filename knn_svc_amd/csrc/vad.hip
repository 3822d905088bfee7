// Voice-activity trimming of pool recordings: where speech starts and where it ends, as the sox `vad` effect finds it with
// torchaudio's default parameters, for both ends of every file of a stacked batch.  The reference documents vad_trigger_level on
// get_features ("optionally perform VAD trimming on start/end", ddsp_matcher.py:438-491: trim the front, flip, trim the front
// again, every cut a whole number of 320-sample hops) and passes 7 for the target pool (ddsp_prematch_dataset.py:1131), where
// get_complete_spk_pool drops it.  The algorithm is written out in include/knnsvc_hip.h and, in fp64 numpy, in
// tests/vad_oracle.py; that restatement is the specification.  torchaudio and sox are not part of this build or of its tests:
// parity with torchaudio's own implementation is NOT pinned.
//
// Everything between the fp32 samples and the int64 cut points is fp64 in a fixed order (no atomics): two runs give the same
// bits, and a file's result does not depend on what else is in the batch.
//
// A measurement depends only on the samples before its end, so "measure until the trigger fires" equals "measure everything,
// then scan"; the reversed pass measures on a grid anchored at the file's end.  Both directions of all files are therefore
// independent problems up to the scan, and go through the same launches:
//   0. vad_tables_kernel     FFT twiddles, cepstrum twiddles and the two Hann windows, fp64, into the workspace.
//   1. vad_spectrum_kernel   one workgroup per (file, direction, measurement): the windowed frame (read backwards for the reversed
//                            direction) into LDS in bit-reversed order, a radix-2 FFT of dft_len points in LDS, |X_k| of the
//                            s1 - s0 speech-band bins out.
//   2. vad_track_kernel      one workgroup per (file, direction), one lane per bin, sequential over the measurements: the
//                            smoothed spectrum S, the noise floor N and e = sqrt(max(0, S^2 - 1.35 N)), written over |X|.  The
//                            rows of |X| do not depend on the recurrence: four are loaded while the four before them are worked on.
//   3. vad_cepstrum_kernel   one workgroup per (file, direction, measurement): the c1 - c0 needed bins of the dft_len/2-point DFT of
//                            e * cwin directly against the twiddle table, summed in a fixed order to the measure.
//   4. vad_trigger_kernel    one thread per file: running mean, trigger, walk back over 20 measures, hop rounding; then the
//                            reversed direction over the measurements that fit behind the front cut.
// Measurement m of file s lives in row off[s] / period + m of its direction's half: a file of L samples has at most L / period
// measurements, so the rows of consecutive files never meet and total / period + 1 rows hold any batch - no prefix table.
#include "common.h"
#include <math.h>

namespace {

constexpr int VAD_HOP = 320;                  // the encoder's hop: every cut is a multiple of it (ddsp_matcher.py:467-471)
constexpr int VAD_MAX_DFT = 2048;             // the FFT lives in LDS: 2 x 16 KB of fp64 + 2 x 8 KB of twiddles
constexpr int VAD_MIN_RATE = 8000, VAD_MAX_RATE = 20000;     // measure_len = rate / 10 <= VAD_MAX_DFT
constexpr int VAD_MEASURES = 20, VAD_GAP = 5, VAD_BOOT = 6;
constexpr double VAD_NOISE_REDUCTION = 1.35;
constexpr int VAD_T = 256;                    // threads of the spectrum and cepstrum workgroups
constexpr int VAD_TRACK_T = VAD_MAX_DFT / 2;  // lanes of the tracking workgroup (>= bins)
constexpr int VAD_AHEAD = 4;                  // rows of |X| in flight in the tracking kernel
constexpr int64_t VAD_MAX_N = (int64_t)1 << 36;

struct VadPlan {
    int measure_len, dft_len, dft_log2, period, s0, s1, nb, c0, c1;
    double smooth, up, down, trig;
    long rows;                                // measurement rows per direction
};

// ---- host: every constant from the sample rate.  At 16 kHz: measure_len 1600, dft_len 2048, period 800, spectrum bins
// [6, 768), cepstrum bins [4, 53).
bool vad_rate_ok(int32_t sr) { return sr >= VAD_MIN_RATE && sr <= VAD_MAX_RATE; }

VadPlan vad_plan(int32_t sr, int64_t total) {
    VadPlan p;
    p.measure_len = (int)(sr * 0.1 + .5);
    p.dft_len = 16; p.dft_log2 = 4;
    while (p.dft_len < p.measure_len) { p.dft_len <<= 1; ++p.dft_log2; }
    p.period = (int)(sr / 20.0 + .5);
    const int s0 = (int)(50.0 / sr * p.dft_len + .5), s1 = (int)(6000.0 / sr * p.dft_len + .5);
    p.s0 = s0 > 1 ? s0 : 1;
    p.s1 = s1 < p.dft_len / 2 ? s1 : p.dft_len / 2;
    p.nb = p.s1 - p.s0;
    const int c1 = (int)floor(sr * .5 / 150.0);
    p.c0 = (int)ceil(sr * .5 / 2000.0);
    p.c1 = c1 < p.dft_len / 4 ? c1 : p.dft_len / 4;
    p.smooth = exp(-1.0 / 8.0); p.up = exp(-1.0 / 2.0); p.down = exp(-5.0); p.trig = exp(-1.0 / 5.0);
    p.rows = (long)(total / p.period) + 1;
    return p;
}

// workspace, all doubles: tw_re, tw_im, ctw_re, ctw_im [dft_len / 2 each] | win [measure_len] | cwin [nb] | spectra [2][rows][nb]
// | measures [2][rows]
struct VadWs { double *tw_re, *tw_im, *ctw_re, *ctw_im, *win, *cwin, *spec, *meas; };

size_t vad_workspace(const VadPlan& p, VadWs* w, void* base) {
    double* d = (double*)base;
    const size_t half = (size_t)p.dft_len / 2;
    size_t o = 0;
    auto take = [&](size_t n) { double* r = d + o; o += n; return r; };
    double* t[8] = {take(half), take(half), take(half), take(half), take((size_t)p.measure_len), take((size_t)p.nb),
                    take((size_t)2 * p.rows * p.nb), take((size_t)2 * p.rows)};
    if (w) *w = VadWs{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]};
    return o * sizeof(double);
}

// ---- device
__device__ __forceinline__ long vad_measurements(long len, const VadPlan& p) {
    return len >= p.measure_len ? (len - p.measure_len) / p.period + 1 : 0;
}

// launch 0.  Windows are periodic Hann (denominator n, not n - 1), scaled by 2 / sqrt(n).
__global__ __launch_bounds__(VAD_T) void vad_tables_kernel(VadPlan p, VadWs w) {
    const int i = blockIdx.x * VAD_T + threadIdx.x;
    const int half = p.dft_len / 2;
    if (i < half) {
        double s, c;
        sincospi(-2.0 * (double)i / (double)p.dft_len, &s, &c);        // exp(-2 pi i k / dft_len)
        w.tw_re[i] = c; w.tw_im[i] = s;
        sincospi(-2.0 * (double)i / (double)half, &s, &c);             // exp(-2 pi i j / (dft_len / 2))
        w.ctw_re[i] = c; w.ctw_im[i] = s;
    }
    if (i < p.measure_len) w.win[i] = 2.0 / sqrt((double)p.measure_len) * (0.5 - 0.5 * cospi(2.0 * (double)i / (double)p.measure_len));
    if (i < p.nb) w.cwin[i] = 2.0 / sqrt((double)p.nb) * (0.5 - 0.5 * cospi(2.0 * (double)i / (double)p.nb));
}

// launch 1: grid (most measurements of any file, 2 n_seg); blockIdx.y = 2 file + direction
__global__ __launch_bounds__(VAD_T) void vad_spectrum_kernel(const float* __restrict__ wav, KnSegTable seg, VadPlan p, VadWs w) {
    __shared__ double re[VAD_MAX_DFT], im[VAD_MAX_DFT], tr[VAD_MAX_DFT / 2], ti[VAD_MAX_DFT / 2];
    const int s = blockIdx.y >> 1, d = blockIdx.y & 1;
    const long m = blockIdx.x, base = seg.off[s], len = seg.off[s + 1] - base;
    if (m >= vad_measurements(len, p)) return;
    const int n = p.dft_len, half = n / 2;
    const long first = m * p.period;                      // < len - measure_len + 1: every sample read below is inside the file
    for (int i = threadIdx.x; i < n; i += VAD_T) {
        double v = 0.0;
        if (i < p.measure_len) v = w.win[i] * (double)wav[d ? base + len - 1 - (first + i) : base + first + i];
        const int j = (int)(__brev((unsigned)i) >> (32 - p.dft_log2));
        re[j] = v; im[j] = 0.0;
    }
    for (int i = threadIdx.x; i < half; i += VAD_T) { tr[i] = w.tw_re[i]; ti[i] = w.tw_im[i]; }
    __syncthreads();
    for (int st = 0; st < p.dft_log2; ++st) {             // decimation in time: butterflies of span h = 2^st
        const int h = 1 << st, tstep = half >> st;
        for (int j = threadIdx.x; j < half; j += VAD_T) {
            const int pos = j & (h - 1), i0 = ((j >> st) << (st + 1)) + pos, i1 = i0 + h;
            const double wr = tr[pos * tstep], wi = ti[pos * tstep];
            const double xr = re[i1], xi = im[i1];
            const double ur = wr * xr - wi * xi, ui = wr * xi + wi * xr;
            const double ar = re[i0], ai = im[i0];
            re[i0] = ar + ur; im[i0] = ai + ui;
            re[i1] = ar - ur; im[i1] = ai - ui;
        }
        __syncthreads();
    }
    double* out = w.spec + ((long)d * p.rows + base / p.period + m) * p.nb;
    for (int k = threadIdx.x; k < p.nb; k += VAD_T) out[k] = sqrt(re[p.s0 + k] * re[p.s0 + k] + im[p.s0 + k] * im[p.s0 + k]);
}

// launch 2: grid (2 n_seg); |X| rows in, e rows out (in place: a lane reads and writes only its own column)
__global__ __launch_bounds__(VAD_TRACK_T) void vad_track_kernel(KnSegTable seg, VadPlan p, double* spec) {
#pragma clang fp contract(off)
    const int s = blockIdx.x >> 1, d = blockIdx.x & 1, k = threadIdx.x;
    const long base = seg.off[s], M = vad_measurements(seg.off[s + 1] - base, p);
    if (k >= p.nb) return;
    double* col = spec + ((long)d * p.rows + base / p.period) * p.nb + k;
    double S = 0.0, N = 0.0, cur[VAD_AHEAD], nxt[VAD_AHEAD];
#pragma unroll
    for (int u = 0; u < VAD_AHEAD; ++u) cur[u] = u < M ? col[(long)u * p.nb] : 0.0;
    for (long m0 = 0; m0 < M; m0 += VAD_AHEAD) {
#pragma unroll
        for (int u = 0; u < VAD_AHEAD; ++u) nxt[u] = m0 + VAD_AHEAD + u < M ? col[(m0 + VAD_AHEAD + u) * p.nb] : 0.0;
#pragma unroll
        for (int u = 0; u < VAD_AHEAD; ++u) {
            const long m = m0 + u;
            if (m >= M) break;
            double dd;
            if (m < VAD_BOOT) {
                const double b = (double)(m + 1);
                S = (b / (1.0 + b)) * S + (1.0 / (1.0 + b)) * cur[u];
                dd = S * S;
                N = dd;
            } else {
                S = p.smooth * S + (1.0 - p.smooth) * cur[u];
                dd = S * S;
                const double mu = dd > N ? p.up : p.down;
                N = mu * N + (1.0 - mu) * dd;
            }
            col[m * p.nb] = sqrt(fmax(0.0, dd - VAD_NOISE_REDUCTION * N));
        }
#pragma unroll
        for (int u = 0; u < VAD_AHEAD; ++u) cur[u] = nxt[u];
    }
}

// launch 3: grid as launch 1.  Thread t holds part t % parts of bin c0 + t / parts; the parts of a bin, then the bins, are summed
// in ascending order by one thread each.
__global__ __launch_bounds__(VAD_T) void vad_cepstrum_kernel(KnSegTable seg, VadPlan p, VadWs w, double* __restrict__ meas) {
#pragma clang fp contract(off)
    __shared__ double c[VAD_MAX_DFT / 2], tr[VAD_MAX_DFT / 2], ti[VAD_MAX_DFT / 2], pr[VAD_T], pi[VAD_T];
    const int s = blockIdx.y >> 1, d = blockIdx.y & 1, t = threadIdx.x;
    const long m = blockIdx.x, base = seg.off[s];
    if (m >= vad_measurements(seg.off[s + 1] - base, p)) return;
    const int half = p.dft_len / 2, nc = p.c1 - p.c0, parts = VAD_T / nc;
    const long row = (long)d * p.rows + base / p.period + m;
    const double* e = w.spec + row * p.nb;
    for (int i = t; i < p.nb; i += VAD_T) c[i] = e[i] * w.cwin[i];
    for (int i = t; i < half; i += VAD_T) { tr[i] = w.ctw_re[i]; ti[i] = w.ctw_im[i]; }
    __syncthreads();
    const int q = t / parts, part = t % parts;
    double ar = 0.0, ai = 0.0;
    if (q < nc)
        for (int i = part; i < p.nb; i += parts) {
            const int j = ((p.c0 + q) * (p.s0 + i)) & (half - 1);
            ar += c[i] * tr[j];
            ai += c[i] * ti[j];
        }
    pr[t] = ar; pi[t] = ai;
    __syncthreads();
    double pw = 0.0;
    if (t < nc) {
        double sr = 0.0, si = 0.0;
        for (int u = 0; u < parts; ++u) { sr += pr[t * parts + u]; si += pi[t * parts + u]; }
        pw = sr * sr + si * si;
    }
    __syncthreads();
    if (t < nc) pr[t] = pw;
    __syncthreads();
    if (t == 0) {
        double r = 0.0;
        for (int u = 0; u < nc; ++u) r += pr[u];
        meas[row] = r > 0.0 ? fmax(0.0, 21.0 + log(r / (double)nc)) : 0.0;
    }
}

// the first measurement at which the running mean reaches the level, walked back: -> first sample to keep, or -1
__device__ long vad_scan(const double* __restrict__ ms, long M, double level, const VadPlan& p) {
#pragma clang fp contract(off)
    double mean = 0.0;
    for (long m = 0; m < M; ++m) {
        mean = p.trig * mean + (1.0 - p.trig) * ms[m];
        if (!(mean >= level)) continue;
        int jt = VAD_MEASURES, jz = VAD_MEASURES;
        for (int j = 0; j < VAD_MEASURES; ++j) {
            const double v = m - j >= 0 ? ms[m - j] : 0.0;            // before the file: nothing measured
            if (v >= level && j <= jt + VAD_GAP) jz = jt = j;
            else if (v == 0.0 && jt >= jz) jz = j;
        }
        const long back = jz < VAD_MEASURES ? jz : VAD_MEASURES;
        return (m - back > 0 ? m - back : 0) * p.period;
    }
    return -1;
}

// launch 4
__global__ __launch_bounds__(64) void vad_trigger_kernel(KnSegTable seg, VadPlan p, const double* __restrict__ meas, double level,
                                                        long* __restrict__ strip) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= seg.n) return;
    const long base = seg.off[s], len = seg.off[s + 1] - base, r0 = base / p.period;
    long l = -1, r = -1;
    const long fwd = vad_scan(meas + r0, vad_measurements(len, p), level, p);
    if (fwd >= 0) {
        l = (fwd + VAD_HOP - 1) / VAD_HOP * VAD_HOP;
        const long rev = vad_scan(meas + p.rows + r0, vad_measurements(len - l, p), level, p);
        if (rev >= 0) r = (rev + VAD_HOP - 1) / VAD_HOP * VAD_HOP;
        if (rev < 0 || len - l - r < p.measure_len) l = r = -1;
    }
    strip[2 * s] = l;
    strip[2 * s + 1] = r;
}

}  // namespace

extern "C" size_t knnsvc_vad_workspace_bytes(int64_t total_samples, int32_t n_seg, int32_t sample_rate) {
    if (total_samples < 1 || total_samples > VAD_MAX_N) { knnsvc_fail(KNNSVC_EINVAL, "vad: bad length %lld (1 .. 2^36)", (long long)total_samples); return 0; }
    if (n_seg < 1 || n_seg > KNNSVC_MAX_SEGMENTS) { knnsvc_fail(KNNSVC_EINVAL, "vad: n_seg %d outside 1..%d", (int)n_seg, KNNSVC_MAX_SEGMENTS); return 0; }
    if (!vad_rate_ok(sample_rate)) { knnsvc_fail(KNNSVC_EINVAL, "vad: sample rate %d outside %d .. %d", (int)sample_rate, VAD_MIN_RATE, VAD_MAX_RATE); return 0; }
    return vad_workspace(vad_plan(sample_rate, total_samples), nullptr, nullptr);
}

extern "C" int knnsvc_vad_trim_seg(const float* wav, const int64_t* host_seg_offsets, int32_t n_seg, int32_t sample_rate,
                                   double trigger_level, int64_t* out_strip, double* out_measures, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* entry = "vad_trim_seg";
    KN_REQUIRE(vad_rate_ok(sample_rate), "%s: sample rate %d outside %d .. %d", entry, (int)sample_rate, VAD_MIN_RATE, VAD_MAX_RATE);
    KN_REQUIRE(isfinite(trigger_level) && trigger_level > 0.0, "%s: trigger level must be finite and positive", entry);
    KnSegTable seg;
    int rc = kn_seg_table(host_seg_offsets, n_seg, entry, &seg);
    if (rc) return rc;
    const int64_t total = seg.off[n_seg];
    KN_REQUIRE(total <= VAD_MAX_N, "%s: bad length %lld (1 .. 2^36)", entry, (long long)total);
    KN_REQUIRE(wav && out_strip && workspace, "%s: null pointer", entry);
    KN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out_strip & 7) == 0 && ((uintptr_t)out_measures & 7) == 0,
               "%s: workspace, out_strip and out_measures must be 8-byte aligned", entry);
    const VadPlan p = vad_plan(sample_rate, total);
    VadWs w;
    const size_t need = vad_workspace(p, &w, workspace);
    if (workspace_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", entry, workspace_bytes, need);
    double* meas = out_measures ? out_measures : w.meas;
    hipStream_t st = (hipStream_t)stream;
    long most = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long len = seg.off[s + 1] - seg.off[s], M = len >= p.measure_len ? (len - p.measure_len) / p.period + 1 : 0;
        most = M > most ? M : most;
    }
    if (most > 0) {                          // otherwise no file holds a measurement: every file is dropped below
        const int widest = p.measure_len > p.dft_len / 2 ? p.measure_len : p.dft_len / 2;
        hipLaunchKernelGGL(vad_tables_kernel, dim3((unsigned)cdiv64(widest, VAD_T)), dim3(VAD_T), 0, st, p, w);
        if ((rc = knnsvc_check_launch("vad_trim_seg (tables)"))) return rc;
        const dim3 grid((unsigned)most, (unsigned)(2 * n_seg));
        hipLaunchKernelGGL(vad_spectrum_kernel, grid, dim3(VAD_T), 0, st, wav, seg, p, w);
        if ((rc = knnsvc_check_launch("vad_trim_seg (spectrum)"))) return rc;
        hipLaunchKernelGGL(vad_track_kernel, dim3((unsigned)(2 * n_seg)), dim3(VAD_TRACK_T), 0, st, seg, p, w.spec);
        if ((rc = knnsvc_check_launch("vad_trim_seg (track)"))) return rc;
        hipLaunchKernelGGL(vad_cepstrum_kernel, grid, dim3(VAD_T), 0, st, seg, p, w, meas);
        if ((rc = knnsvc_check_launch("vad_trim_seg (cepstrum)"))) return rc;
    }
    hipLaunchKernelGGL(vad_trigger_kernel, dim3((unsigned)cdiv64(n_seg, 64)), dim3(64), 0, st, seg, p, (const double*)meas, trigger_level,
                       (long*)out_strip);
    return knnsvc_check_launch("vad_trim_seg (trigger)");
}
