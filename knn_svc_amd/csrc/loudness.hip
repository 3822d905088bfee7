// Integrated loudness after ITU-R BS.1770-4 (K-weighting, 400 ms blocks every 100 ms, absolute gate at -70 LKFS, relative gate 10 LU
// under the mean of what the absolute gate kept) of a mono fp32 signal, and the gain that moves a signal to a target loudness.
// Constants and biquad forms are those torchaudio.functional.loudness uses; the reference normalises its output with
// gain(prediction, tgt - loudness(prediction)) (ddsp_matcher.py:533, 947, 997-1003).  The definition is written out in
// include/knnsvc_hip.h and, in fp64 numpy, in tests/loudness_oracle.py.
//
// Everything between the fp32 samples and the fp32 result is fp64, in a fixed order (no atomics): two runs give the same bits.
//
// The K-weighting is a 4th-order recursion over the whole signal (the 38 Hz high-pass has its poles at radius 0.985 at 16 kHz:
// a run-in would take thousands of samples).  It is cut into chunks of LD_C samples, one lane per chunk, and the filter state
// crosses the chunk boundaries EXACTLY, by linearity: with the input history x[-1], x[-2] read from the signal, what a chunk
// needs from its past is s = (y1[-1], y1[-2], y2[-1], y2[-2]) (y1: shelf output, y2: high-pass output), and the state at the end of
// a chunk is   s_end = M s_start + e,   e = the end state reached from s_start = 0,  M = A^LD_C,  A the 4x4 transition of the
// cascade with zero input.  Four launches:
//   1. ld_end_state_kernel   every lane filters its chunk from s = 0 and stores e.
//   2. ld_scan_kernel        ONE workgroup turns the e into the start states: every thread owns a run of `per` consecutive
//                            chunks, reduces it to one affine step, the 1024 steps are scanned with (M^per)^(2^j) (Hillis-Steele,
//                            the matrices come from the host), and every thread walks its run again from its true start.
//   3. ld_energy_kernel      every lane filters its chunk again from its start state and sums y2^2, split at the one boundary
//                            between 100 ms steps that a chunk can contain (LD_C <= step).
//   4. ld_gate_kernel        ONE workgroup: step sums from the chunk sums (ascending chunk order), block means from four
//                            consecutive steps, both gates, the result and the three counts.
// Launches 2 and 4 are one workgroup each, so their serial work per thread grows with the length: chunks / 1024 affine steps
// (twice) and steps / 1024 step sums of ~step / 64 chunk sums.  For a 30 s clip that is 8 and 1; an hour of 16 kHz audio makes it
// 880 and 36 - microseconds against the milliseconds the parallel launches then take; a multi-workgroup scan is not worth having
// below that.
#include "common.h"
#include <math.h>

namespace {

constexpr int LD_C = 64;                      // samples per chunk (= per lane)
constexpr int LD_T = 128;                     // lanes per workgroup of launches 1 and 3
constexpr int LD_W = LD_C * LD_T;             // samples per workgroup
constexpr int LD_SCAN_T = 1024;               // threads of the scan workgroup
constexpr int LD_SCAN_LOG = 10;
constexpr int LD_GATE_T = 1024;
constexpr int LD_MIN_RATE = 8000, LD_MAX_RATE = 768000;      // the shelf's 1500 Hz must sit well below Nyquist; LD_C <= step
constexpr int64_t LD_MAX_N = (int64_t)1 << 36;               // block counts stay inside int32 (documented in the header)

struct LdCoef { double sb0, sb1, sb2, sa1, sa2, hb0, hb1, hb2, ha1, ha2; };      // shelf, high-pass (a0 = 1)
struct LdScan { double m[16]; double p[LD_SCAN_LOG][16]; };                      // M = A^LD_C; p[j] = (M^per)^(2^j), row major

// ---- host: coefficients and transition matrices, fp64
LdCoef ld_coefficients(int sr) {
    const double pi = 3.14159265358979323846;
    LdCoef c;
    {   // high-shelf +4 dB at 1500 Hz, Q = 1/sqrt(2)
        const double w0 = 2.0 * pi * 1500.0 / sr, A = pow(10.0, 4.0 / 40.0), al = sin(w0) / (2.0 / sqrt(2.0)), cw = cos(w0);
        const double t = 2.0 * sqrt(A) * al;
        const double b0 = A * ((A + 1) + (A - 1) * cw + t), b1 = -2 * A * ((A - 1) + (A + 1) * cw), b2 = A * ((A + 1) + (A - 1) * cw - t);
        const double a0 = (A + 1) - (A - 1) * cw + t, a1 = 2 * ((A - 1) - (A + 1) * cw), a2 = (A + 1) - (A - 1) * cw - t;
        c.sb0 = b0 / a0; c.sb1 = b1 / a0; c.sb2 = b2 / a0; c.sa1 = a1 / a0; c.sa2 = a2 / a0;
    }
    {   // high-pass at 38 Hz, Q = 0.5
        const double w0 = 2.0 * pi * 38.0 / sr, al = sin(w0) / (2.0 * 0.5), cw = cos(w0);
        const double b0 = (1 + cw) / 2, b1 = -(1 + cw), b2 = (1 + cw) / 2, a0 = 1 + al, a1 = -2 * cw, a2 = 1 - al;
        c.hb0 = b0 / a0; c.hb1 = b1 / a0; c.hb2 = b2 / a0; c.ha1 = a1 / a0; c.ha2 = a2 / a0;
    }
    return c;
}

void ld_matmul(const double* a, const double* b, double* out) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
            r[i * 4 + j] = s;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

void ld_matpow(const double* a, int64_t e, double* out) {
    double acc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, sq[16];
    for (int i = 0; i < 16; ++i) sq[i] = a[i];
    for (; e > 0; e >>= 1) {
        if (e & 1) ld_matmul(acc, sq, acc);
        ld_matmul(sq, sq, sq);
    }
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
}

// one zero-input sample of the cascade on s = (y1[-1], y1[-2], y2[-1], y2[-2]):  y1 = -sa1 s0 - sa2 s1,
// y2 = hb0 y1 + hb1 s0 + hb2 s1 - ha1 s2 - ha2 s3,  s' = (y1, s0, y2, s2)
void ld_scan_matrices(const LdCoef& c, int64_t per, LdScan* out) {
    const double a[16] = {-c.sa1, -c.sa2, 0, 0,
                          1, 0, 0, 0,
                          c.hb1 - c.hb0 * c.sa1, c.hb2 - c.hb0 * c.sa2, -c.ha1, -c.ha2,
                          0, 0, 1, 0};
    ld_matpow(a, LD_C, out->m);
    ld_matpow(out->m, per, out->p[0]);
    for (int j = 1; j < LD_SCAN_LOG; ++j) ld_matmul(out->p[j - 1], out->p[j - 1], out->p[j]);
}

// ---- device
__device__ __forceinline__ void ld_matvec(const double* __restrict__ m, const double (&v)[4], double (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = ((m[i * 4] * v[0] + m[i * 4 + 1] * v[1]) + m[i * 4 + 2] * v[2]) + m[i * 4 + 3] * v[3];
}

// The workgroup's LD_W samples, coalesced, into LDS rows of LD_C + 1 floats (row = lane: a lane then walks its row without bank
// conflicts); samples past n are zero and never used.
__device__ __forceinline__ void ld_stage(const float* __restrict__ x, long n, long base, float* __restrict__ tile) {
    for (int i = threadIdx.x; i < LD_W; i += LD_T) {
        const long g = base + i;
        tile[(i / LD_C) * (LD_C + 1) + (i % LD_C)] = g < n ? x[g] : 0.f;
    }
    __syncthreads();
}

// `len` samples of the cascade, direct form I, from state s and input history (x1, x2) = (x[-1], x[-2]); out(i, y2[i]) sees
// every output sample.
template <class OUT>
__device__ __forceinline__ void ld_filter(const LdCoef& c, const float* __restrict__ row, int len, double x1, double x2, double (&s)[4],
                                          OUT&& out) {
    // (the term on the newest output comes last: one dependent multiply-add per sample and section)
    for (int i = 0; i < len; ++i) {
        const double x0 = (double)row[i];
        const double y1 = (((c.sb0 * x0 + c.sb1 * x1) + c.sb2 * x2) - c.sa2 * s[1]) - c.sa1 * s[0];
        const double y2 = ((((c.hb1 * s[0] + c.hb2 * s[1]) - c.ha2 * s[3]) + c.hb0 * y1)) - c.ha1 * s[2];
        x2 = x1; x1 = x0;
        s[1] = s[0]; s[0] = y1;
        s[3] = s[2]; s[2] = y2;
        out(i, y2);
    }
}

// launch 1: e[k] for every FULL chunk k that has a chunk behind it (k < chunks - 1)
__global__ __launch_bounds__(LD_T) void ld_end_state_kernel(const float* __restrict__ x, long n, long chunks, LdCoef c,
                                                           double* __restrict__ state) {
    __shared__ float tile[LD_T * (LD_C + 1)];
    const long base = (long)blockIdx.x * LD_W;
    ld_stage(x, n, base, tile);
    const long k = (long)blockIdx.x * LD_T + threadIdx.x;
    if (k >= chunks - 1) return;
    const long start = k * LD_C;
    const double x1 = start >= 1 ? (double)x[start - 1] : 0.0, x2 = start >= 2 ? (double)x[start - 2] : 0.0;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    ld_filter(c, tile + threadIdx.x * (LD_C + 1), LD_C, x1, x2, s, [](int, double) {});
#pragma unroll
    for (int i = 0; i < 4; ++i) state[k * 4 + i] = s[i];
}

// launch 2: state[k] = e[k] (k < chunks - 1)  ->  state[k] = start state of chunk k (k < chunks), in place
__global__ __launch_bounds__(LD_SCAN_T) void ld_scan_kernel(double* __restrict__ state, long chunks, long per, LdScan sc) {
#pragma clang fp contract(off)
    __shared__ double sh[LD_SCAN_T][4];
    const int t = threadIdx.x;
    const long lo = (long)t * per < chunks ? (long)t * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    // the run as one affine step from zero (only runs that have a chunk behind them are read by anybody: those are full, and
    // all their e exist)
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, tmp[4];
    if (hi < chunks)
        for (long k = lo; k < hi; ++k) {
            ld_matvec(sc.m, acc, tmp);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = tmp[i] + state[k * 4 + i];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[t][i] = acc[i];
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < LD_SCAN_LOG; ++j) {
        const int d = 1 << j;
        double u[4] = {0.0, 0.0, 0.0, 0.0};
        if (t >= d) {
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = sh[t - d][i];
        }
        __syncthreads();                     // every read of this round is done before any write
        if (t >= d) {
            ld_matvec(sc.p[j], u, tmp);
#pragma unroll
            for (int i = 0; i < 4; ++i) sh[t][i] += tmp[i];
        }
        __syncthreads();
    }
    // sh[t] = state at the end of run t = start of run t + 1
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (t > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = sh[t - 1][i];
    }
    for (long k = lo; k < hi; ++k) {
        double e[4] = {0.0, 0.0, 0.0, 0.0};
        if (k < chunks - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = state[k * 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) state[k * 4 + i] = s[i];
        ld_matvec(sc.m, s, tmp);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = tmp[i] + e[i];
    }
}

// launch 3: part[2k], part[2k + 1] = sums of y2^2 over the samples of chunk k in its first step and in the next one
__global__ __launch_bounds__(LD_T) void ld_energy_kernel(const float* __restrict__ x, long n, long chunks, int step, LdCoef c,
                                                        const double* __restrict__ state, double* __restrict__ part) {
    __shared__ float tile[LD_T * (LD_C + 1)];
    const long base = (long)blockIdx.x * LD_W;
    ld_stage(x, n, base, tile);
    const long k = (long)blockIdx.x * LD_T + threadIdx.x;
    if (k >= chunks) return;
    const long start = k * LD_C;
    const int len = n - start < LD_C ? (int)(n - start) : LD_C;
    const double x1 = start >= 1 ? (double)x[start - 1] : 0.0, x2 = start >= 2 ? (double)x[start - 2] : 0.0;
    double s[4], e0 = 0.0, e1 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = state[k * 4 + i];
    const long edge = (start / step + 1) * (long)step - start;          // samples of this chunk before the next step boundary
    const int cut = edge < LD_C ? (int)edge : LD_C;
    ld_filter(c, tile + threadIdx.x * (LD_C + 1), len, x1, x2, s, [&](int i, double y) { if (i < cut) e0 += y * y; else e1 += y * y; });
    part[2 * k] = e0;
    part[2 * k + 1] = e1;
}

// fixed-order sum over the workgroup (LDS tree); every thread gets the total
__device__ __forceinline__ double ld_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = LD_GATE_T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ double ld_lkfs(double e) { return -0.691 + 10.0 * log10(e); }

// launch 4
__global__ __launch_bounds__(LD_GATE_T) void ld_gate_kernel(const double* __restrict__ part, long steps, int step,
                                                           double* energy, float* __restrict__ lkfs,
                                                           int* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ double sh[LD_GATE_T];
    const long blocks = steps >= 4 ? steps - 3 : 0;
    if (blocks > 0) {
        for (long s = threadIdx.x; s < steps; s += LD_GATE_T) {
            const long k0 = s * step / LD_C, k1 = ((s + 1) * step - 1) / LD_C;           // chunks that overlap step s (the last one holds sample (s + 1) step - 1 < n)
            double sum = 0.0;
            for (long k = k0; k <= k1; ++k) sum += part[2 * k + (k * LD_C / step == s ? 0 : 1)];
            energy[s] = sum;
        }
        __syncthreads();                     // energy[] is read by other threads of this workgroup below
    }
    const double g = 4.0 * (double)step;
    auto block_mean = [&](long j) { return ((energy[j] + energy[j + 1]) + (energy[j + 2] + energy[j + 3])) / g; };
    double n1 = 0.0, s1 = 0.0;
    for (long j = threadIdx.x; j < blocks; j += LD_GATE_T) {
        const double e = block_mean(j);
        if (ld_lkfs(e) > -70.0) { n1 += 1.0; s1 += e; }
    }
    n1 = ld_block_sum(n1, sh);
    s1 = ld_block_sum(s1, sh);
    const double gamma = ld_lkfs(s1 / n1) - 10.0;                  // NaN when nothing was kept: no comparison below is true
    double n2 = 0.0, s2 = 0.0;
    for (long j = threadIdx.x; j < blocks; j += LD_GATE_T) {
        const double e = block_mean(j), l = ld_lkfs(e);
        if (l > -70.0 && l > gamma) { n2 += 1.0; s2 += e; }
    }
    n2 = ld_block_sum(n2, sh);
    s2 = ld_block_sum(s2, sh);
    if (threadIdx.x == 0) {
        *lkfs = n2 > 0.0 ? (float)ld_lkfs(s2 / n2) : -INFINITY;
        if (counts) { counts[0] = (int)blocks; counts[1] = (int)n1; counts[2] = (int)n2; }
    }
}

__global__ __launch_bounds__(256) void ld_gain_kernel(const float* wav, long n, const float* __restrict__ lkfs, float target,
                                                     float* out) {
    __shared__ float gs;
    if (threadIdx.x == 0) {
        const float l = *lkfs;
        gs = isfinite(l) ? (float)pow(10.0, ((double)target - (double)l) / 20.0) : 1.0f;
    }
    __syncthreads();
    const float g = gs;
    const long base = (long)blockIdx.x * 2048 + threadIdx.x;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long i = base + r * 256;
        if (i < n) out[i] = wav[i] * g;
    }
}

bool ld_rate_ok(int32_t sr) { return sr >= LD_MIN_RATE && sr <= LD_MAX_RATE && sr % 10 == 0; }

// workspace: [chunks][4] states | [chunks][2] chunk sums | [steps] step sums, all doubles (+ one, so that a valid size is never 0)
size_t ld_workspace(int64_t n, int32_t sr) {
    const int64_t chunks = cdiv64(n, LD_C), steps = n / (sr / 10);
    return (size_t)(6 * chunks + steps + 1) * 8;
}

}  // namespace

extern "C" void knnsvc_loudness_layout(int32_t* chunk, int32_t* group) {
    if (chunk) *chunk = LD_C;
    if (group) *group = LD_W;
}

extern "C" size_t knnsvc_loudness_workspace_bytes(int64_t n, int32_t sample_rate) {
    if (n < 0 || n > LD_MAX_N) { knnsvc_fail(KNNSVC_EINVAL, "loudness: bad length %lld (0 .. 2^36)", (long long)n); return 0; }
    if (!ld_rate_ok(sample_rate)) {
        knnsvc_fail(KNNSVC_EINVAL, "loudness: sample rate %d is not a multiple of 10 in %d .. %d", (int)sample_rate, LD_MIN_RATE, LD_MAX_RATE);
        return 0;
    }
    return ld_workspace(n, sample_rate);
}

extern "C" int knnsvc_loudness(const float* wav, int64_t n, int32_t sample_rate, float* lkfs, int32_t* counts, void* ws,
                               size_t ws_bytes, void* stream) {
    KN_REQUIRE(n >= 0 && n <= LD_MAX_N, "loudness: bad length %lld (0 .. 2^36)", (long long)n);
    KN_REQUIRE(ld_rate_ok(sample_rate), "loudness: sample rate %d is not a multiple of 10 in %d .. %d", (int)sample_rate, LD_MIN_RATE,
               LD_MAX_RATE);
    KN_REQUIRE(lkfs && ws && (wav || n == 0), "loudness: null pointer");
    KN_REQUIRE(((uintptr_t)ws & 7) == 0, "loudness: workspace must be 8-byte aligned");
    const size_t need = ld_workspace(n, sample_rate);
    if (ws_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "loudness: workspace of %zu bytes, %zu needed", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int step = sample_rate / 10;
    const long chunks = (long)cdiv64(n, LD_C), steps = (long)(n / step);
    double* state = (double*)ws;
    double* part = state + 4 * chunks;
    double* energy = part + 2 * chunks;
    if (steps >= 4) {                        // otherwise no block: -inf and zero counts, nothing to filter
        const LdCoef c = ld_coefficients(sample_rate);
        const long per = (long)cdiv64(chunks, LD_SCAN_T);
        LdScan sc;
        ld_scan_matrices(c, per, &sc);
        const dim3 grid((unsigned)cdiv64(chunks, LD_T));
        hipLaunchKernelGGL(ld_end_state_kernel, grid, dim3(LD_T), 0, st, wav, (long)n, chunks, c, state);
        int rc = knnsvc_check_launch("loudness (end states)");
        if (rc) return rc;
        hipLaunchKernelGGL(ld_scan_kernel, dim3(1), dim3(LD_SCAN_T), 0, st, state, chunks, per, sc);
        if ((rc = knnsvc_check_launch("loudness (scan)"))) return rc;
        hipLaunchKernelGGL(ld_energy_kernel, grid, dim3(LD_T), 0, st, wav, (long)n, chunks, step, c, (const double*)state, part);
        if ((rc = knnsvc_check_launch("loudness (energy)"))) return rc;
    }
    hipLaunchKernelGGL(ld_gate_kernel, dim3(1), dim3(LD_GATE_T), 0, st, (const double*)part, steps, step, energy, lkfs, counts);
    return knnsvc_check_launch("loudness (gate)");
}

extern "C" int knnsvc_loudness_gain(float* wav, int64_t n, const float* lkfs, float target_db, float* out, void* stream) {
    KN_REQUIRE(n >= 0 && n <= LD_MAX_N, "loudness_gain: bad length %lld (0 .. 2^36)", (long long)n);
    KN_REQUIRE(lkfs && ((wav && out) || n == 0), "loudness_gain: null pointer");
    KN_REQUIRE(isfinite(target_db), "loudness_gain: target is not finite");
    if (n == 0) return KNNSVC_OK;
    hipLaunchKernelGGL(ld_gain_kernel, dim3((unsigned)cdiv64(n, 2048)), dim3(256), 0, (hipStream_t)stream, (const float*)wav, (long)n,
                       lkfs, target_db, out);
    return knnsvc_check_launch("loudness_gain");
}
