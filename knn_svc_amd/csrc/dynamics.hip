// Output dynamics behind the generator: the SOURCE's volume envelope put back on the converted waveform (envelope mix), and a
// look-ahead sample-peak ceiling.  Both are extensions (the reference has neither); the definitions are written out in
// include/knnsvc_hip.h and, in fp64 numpy, in tests/dynamics_oracle.py.
//
// Everything between the fp32 samples and the fp32 result is fp64, in a fixed order; the only atomics are integer ones whose
// result does not depend on the order (a count and a minimum): two runs give the same bits.
//
// Envelope mix, three launches:
//   1. ev_energy_kernel   one wave per hop-sized block and both signals: lane l sums samples l, l + 64, ... in fp64, the lanes
//                         are folded by the xor butterfly (fixed order); the source is zero past its end.
//   2. ev_total_kernel    ONE workgroup: the two totals (strided partial sums, LDS tree), in the manner of ld_gate_kernel.
//   3. ev_apply_kernel    four samples per thread (hop is a multiple of 64: the four share their two neighbouring frame
//                         centres); the thread derives G[t0], G[t1] from the block energies around them and scales; 16-byte loads
//                         and stores when both pointers allow it, else the same arithmetic with 4-byte ones.
//
// Peak ceiling, one launch (plus a one-wave launch that resets the statistics when they are asked for): a workgroup takes a tile
// of PK_TILE samples plus 2L on each side into LDS as the required gain r, builds the sliding minimum over 2L + 1 by doubling
// (windows of 1, 2, 4, ... W <= 2L + 1 samples; two overlapping W-windows cover 2L + 1), and runs the 2L + 1-tap sum per sample.
// A tile whose r are all 1, halo included, copies its samples.
// out == y: a tile's halo lies in its neighbours' samples, so in a parallel launch a neighbour could overwrite it before it is
// read, and no order of passes avoids that without scratch memory (a sample and every sample within 2L of it would have to be
// written in the same pass).  The aliased call therefore runs ONE workgroup that walks the tiles in order and carries the last
// 2L required gains of a tile over to the next in LDS: same arithmetic, same bits, serial (see DESIGN.md for what that costs).
#include "common.h"
#include <math.h>

namespace {

constexpr int64_t DY_MAX_N = (int64_t)1 << 36;      // as the loudness entries: grids and block counts stay inside int32
constexpr int EV_T = 256;                           // launch 1: four waves = four blocks per workgroup; launch 3: 1024 samples
constexpr int EV_TOTAL_T = 1024;
constexpr int EV_MAX_HOP = 1024;
constexpr double EV_FLOOR = 1e-3, EV_CAP = 4.0;     // -60 dB under the average level; +12 dB

constexpr int PK_TILE = 2048;                       // samples per tile
constexpr int PK_T = 256;                           // threads per workgroup: PK_S samples each in the tap sum
constexpr int PK_S = PK_TILE / PK_T;
constexpr int PK_MIN_RATE = 8000, PK_MAX_RATE = 48000;
constexpr int PK_MAX_L = 240;                       // look-ahead at PK_MAX_RATE
constexpr int PK_R = PK_TILE + 4 * PK_MAX_L;        // tile + halo

int pk_lookahead(int32_t sr) { return (sr + 100) / 200; }      // floor(0.005 sr + 0.5) in integers

// ---------------------------------------------------------------------------------------------- envelope mix
__global__ __launch_bounds__(EV_T) void ev_energy_kernel(const float* __restrict__ y, const float* __restrict__ x, long nx, int hop,
                                                        long T, double* __restrict__ bx, double* __restrict__ by) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * (EV_T / 64) + wave;
    if (j >= T) return;                              // the whole wave
    const long base = j * hop;
    double sx = 0.0, sy = 0.0;
    for (int i = lane; i < hop; i += 64) {
        const long g = base + i;
        const double v = (double)y[g], u = g < nx ? (double)x[g] : 0.0;
        sy += v * v;
        sx += u * u;
    }
    sx = wave_sum_d(sx);
    sy = wave_sum_d(sy);
    if (lane == 0) { bx[j] = sx; by[j] = sy; }
}

__device__ __forceinline__ double ev_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = EV_TOTAL_T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(EV_TOTAL_T) void ev_total_kernel(const double* __restrict__ bx, const double* __restrict__ by, long T,
                                                             double* __restrict__ tot) {
#pragma clang fp contract(off)
    __shared__ double sh[EV_TOTAL_T];
    double sx = 0.0, sy = 0.0;
    for (long j = threadIdx.x; j < T; j += EV_TOTAL_T) { sx += bx[j]; sy += by[j]; }
    sx = ev_block_sum(sx, sh);
    sy = ev_block_sum(sy, sh);
    if (threadIdx.x == 0) { tot[0] = sx; tot[1] = sy; }
}

__device__ __forceinline__ double ev_frame_gain(const double* __restrict__ bx, const double* __restrict__ by, long t, long T, double div,
                                                double Rx, double Ry, double a) {
    auto at = [&](const double* __restrict__ b, long j) { return j >= 0 && j < T ? b[j] : 0.0; };
    const double rx = sqrt(((at(bx, t - 1) + at(bx, t)) + at(bx, t + 1)) / div);
    const double ry = sqrt(((at(by, t - 1) + at(by, t)) + at(by, t + 1)) / div);
    const double px = fmax(rx / Rx, EV_FLOOR), py = fmax(ry / Ry, EV_FLOOR);
    return fmin(pow(px / py, a), EV_CAP);
}

template <bool VEC>
__global__ __launch_bounds__(EV_T) void ev_apply_kernel(const float* y, long n, int hop, long T, double a, const double* __restrict__ bx,
                                                       const double* __restrict__ by, const double* __restrict__ tot, float* out,
                                                       double* __restrict__ gains) {
#pragma clang fp contract(off)
    const long n0 = 4 * ((long)blockIdx.x * EV_T + threadIdx.x);
    if (n0 >= n) return;                             // n is a multiple of 64: a thread has all four samples or none
    float v[4];
    if (VEC) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(y + n0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = y[n0 + i];
    }
    const double Rx = sqrt(tot[0] / (double)n), Ry = sqrt(tot[1] / (double)n);
    const bool on = Rx > 0.0 && Ry > 0.0 && isfinite(Rx) && isfinite(Ry);
    const int half = hop / 2;
    // the four samples lie between the same two frame centres (half and hop are multiples of 4)
    const long fl = n0 >= half ? (n0 - half) / hop : -1;
    const long t0 = fl < 0 ? 0 : (fl > T - 1 ? T - 1 : fl), t1 = t0 + 1 < T ? t0 + 1 : T - 1;
    double g0 = 1.0, g1 = 1.0;
    if (on) {
        const double div = 3.0 * (double)hop;
        g0 = ev_frame_gain(bx, by, t0, T, div, Rx, Ry, a);
        g1 = t1 == t0 ? g0 : ev_frame_gain(bx, by, t1, T, div, Rx, Ry, a);
    }
    if (gains && n0 == t0 * hop + half) gains[t0] = g0;           // exactly one thread per frame starts on its centre
    if (on) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double p = ((double)(n0 + i) - (double)half) / (double)hop;
            const double f = fmin(fmax(p - (double)t0, 0.0), 1.0);
            v[i] = (float)((double)v[i] * (g0 + f * (g1 - g0)));
        }
    }                                                             // else: y bit for bit
    if (VEC) {
        *reinterpret_cast<f32x4*>(out + n0) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[n0 + i] = v[i];
    }
}

bool ev_hop_ok(int32_t hop) { return hop > 0 && hop <= EV_MAX_HOP && hop % 64 == 0; }

// workspace: [T] source block energies | [T] output block energies | the two totals, all doubles
size_t ev_workspace(int64_t n, int32_t hop) { return (size_t)(2 * (n / hop) + 2) * 8; }

// ---------------------------------------------------------------------------------------------- peak ceiling
__global__ void pk_stats_reset_kernel(unsigned long long* __restrict__ stats) {
    if (threadIdx.x == 0) {
        stats[0] = 0ull;
        stats[1] = (unsigned long long)__builtin_bit_cast(long, 1.0);
    }
}

// Tiles [blockIdx.x * per_group, ... + per_group) one after the other.  per_group == 1: the parallel launch.  per_group == tiles
// with ONE workgroup: the aliased call (see the head of the file); the left halo of every tile but the first then comes from
// `carry`, not from memory this workgroup has already overwritten.
__global__ __launch_bounds__(PK_T) void pk_limit_kernel(const float* y, long n, double c, int L, int K, long tiles, long per_group,
                                                       float* out, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double buf_a[PK_R], buf_b[PK_R], hw[2 * PK_MAX_L + 1], carry[2 * PK_MAX_L];
    __shared__ unsigned long long red_n[PK_T / 64];
    __shared__ double red_s[PK_T / 64];
    const int tid = threadIdx.x;
    const int taps = 2 * L + 1, R = PK_TILE + 4 * L, M = PK_TILE + 2 * L, W = 1 << K;
    for (int k = tid; k < taps; k += PK_T)            // sum over k of 1 + cos(pi k / (L + 1)) is 2L + 2 exactly (a full period less one term)
        hw[k] = (1.0 + cos(3.14159265358979323846 * (double)(k - L) / (double)(L + 1))) / (double)(2 * L + 2);
    unsigned long long cnt = 0ull;
    double smin = 1.0;
    const long first = (long)blockIdx.x * per_group, last = first + per_group < tiles ? first + per_group : tiles;
    for (long tile = first; tile < last; ++tile) {
        const long base = tile * PK_TILE;
        __syncthreads();                              // hw is written; the buffers and carry of the tile before are no longer read
        int over = 0;
        for (int i = tid; i < R; i += PK_T) {
            double r = 1.0;
            if (tile > first && i < 2 * L) {
                r = carry[i];
            } else {
                const long g = base - 2 * L + i;
                if (g >= 0 && g < n) {
                    const double v = fabs((double)y[g]);
                    if (v > c) r = c / v;             // (a NaN sample compares false: r = 1, and the sample stays NaN below)
                }
            }
            buf_a[i] = r;
            over |= r < 1.0;
        }
        over = __syncthreads_or(over);
        if (per_group > 1)
            for (int i = tid; i < 2 * L; i += PK_T) carry[i] = buf_a[PK_TILE + i];
        const int len = n - base < PK_TILE ? (int)(n - base) : PK_TILE;
        if (!over) {                                  // the whole workgroup: nothing within 2L of this tile is over the ceiling
            if (out != y)
                for (int i = tid; i < len; i += PK_T) out[base + i] = y[base + i];
            continue;
        }
        double* src = buf_a;
        double* dst = buf_b;
        for (int k = 0; k < K; ++k) {                 // src[i] = min r[i .. i + 2^k)  ->  dst[i] = min r[i .. i + 2^(k+1))
            const int d = 1 << k;
            for (int i = tid; i < R; i += PK_T) {
                const double v = src[i];
                dst[i] = i + d < R ? fmin(v, src[i + d]) : v;      // (entries whose window leaves the buffer are never used)
            }
            __syncthreads();
            double* t = src; src = dst; dst = t;
        }
        // dst[j] = 1 - m of sample base - L + j:  m = min r over 2L + 1 = two W-windows, the second ending where the first would
        for (int j = tid; j < M; j += PK_T) dst[j] = 1.0 - fmin(src[j], src[j + taps - W]);
        __syncthreads();
        double acc[PK_S];
#pragma unroll
        for (int s = 0; s < PK_S; ++s) acc[s] = 0.0;
        for (int k = 0; k < taps; ++k) {              // k ascending
            const double h = hw[k];
#pragma unroll
            for (int s = 0; s < PK_S; ++s) acc[s] += h * dst[tid + PK_T * s + k];
        }
#pragma unroll
        for (int s = 0; s < PK_S; ++s) {
            const int i = tid + PK_T * s;
            if (i < len) {
                const double sg = 1.0 - acc[s];
                out[base + i] = (float)((double)y[base + i] * sg);
                if (sg < 1.0) { ++cnt; smin = fmin(smin, sg); }
            }
        }
    }
    if (!stats) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        smin = fmin(smin, __shfl_xor(smin, o, 64));
    }
    if ((tid & 63) == 0) { red_n[tid >> 6] = cnt; red_s[tid >> 6] = smin; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PK_T / 64; ++w) { cnt += red_n[w]; smin = fmin(smin, red_s[w]); }
        if (cnt) {
            atomicAdd(&stats[0], cnt);
            atomicMin(&stats[1], (unsigned long long)__builtin_bit_cast(long, smin));     // 0 <= s <= 1: the bits order as the values
        }
    }
}

// ---------------------------------------------------------------------------------------------- mix of the voices
// The voices of a mix: host tables of device pointers and gains, handed over by value.
constexpr int MX_VOICES = KNNSVC_HARMONY_MAX_PARTS + 1;
constexpr int MX_T = 256;                            // four samples per thread
struct KnMixTable { const float* y[MX_VOICES]; double g[MX_VOICES]; };

// (float)(sum_v g[v] * (double)x[v]) over the voices whose gain is not 0, in order, every operation on its own; the sum starts with
// the first product.  (Unlike a blend's one-hot row, a single live voice is still multiplied: its gain need not be 1.)
__device__ __forceinline__ float mx_sum(const KnMixTable& mt, const float (&x)[MX_VOICES]) {
#pragma clang fp contract(off)
    double acc = 0.0;
    bool first = true;
#pragma unroll
    for (int v = 0; v < MX_VOICES; ++v) {
        if (mt.g[v] != 0.0) {
            const double p = mt.g[v] * (double)x[v];
            acc = first ? p : acc + p;
            first = false;
        }
    }
    return (float)acc;
}

// A thread reads its four samples of every live voice and then writes them: out may be one of the voices.  The gains are uniform,
// so a silent voice costs a scalar branch and no load.  VEC: every live pointer and out are 16-byte aligned; the last thread's
// quad may be short and is then done sample by sample.
template <bool VEC>
__global__ __launch_bounds__(MX_T) void mix_kernel(const KnMixTable mt, long n, float* out) {
#pragma clang fp contract(off)
    const long n0 = 4 * ((long)blockIdx.x * MX_T + threadIdx.x);
    if (n0 >= n) return;
    if (VEC && n0 + 4 <= n) {
        f32x4 xv[MX_VOICES];
#pragma unroll
        for (int v = 0; v < MX_VOICES; ++v) xv[v] = mt.g[v] != 0.0 ? *reinterpret_cast<const f32x4*>(mt.y[v] + n0) : (f32x4)(0.f);
        f32x4 vo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x[MX_VOICES] = {xv[0][e], xv[1][e], xv[2][e], xv[3][e]};
            vo[e] = mx_sum(mt, x);
        }
        *reinterpret_cast<f32x4*>(out + n0) = vo;
    } else {
        const int len = n - n0 < 4 ? (int)(n - n0) : 4;
        float r[4];
        for (int e = 0; e < len; ++e) {
            float x[MX_VOICES];
#pragma unroll
            for (int v = 0; v < MX_VOICES; ++v) x[v] = mt.g[v] != 0.0 ? mt.y[v][n0 + e] : 0.f;
            r[e] = mx_sum(mt, x);
        }
        for (int e = 0; e < len; ++e) out[n0 + e] = r[e];
    }
}
static_assert(MX_VOICES == 4, "mix_kernel spells out four voices");

}  // namespace

extern "C" int knnsvc_mix_waves(const float* const* host_y, int32_t n_voices, const double* host_gains, int64_t n, float* out,
                                void* stream) {
    KN_REQUIRE(n_voices >= 1 && n_voices <= MX_VOICES, "mix_waves: n_voices %d outside 1..%d", (int)n_voices, MX_VOICES);
    KN_REQUIRE(n >= 0 && n <= DY_MAX_N, "mix_waves: bad length %lld (0 .. 2^36)", (long long)n);
    KN_REQUIRE(host_y && host_gains && (out || n == 0), "mix_waves: null pointer");
    KnMixTable mt;
    bool vec = ((uintptr_t)out & 15) == 0, positive = false;
    for (int v = 0; v < MX_VOICES; ++v) {
        mt.y[v] = v < n_voices ? host_y[v] : nullptr;
        mt.g[v] = v < n_voices ? host_gains[v] + 0.0 : 0.0;
        if (v >= n_voices) continue;
        KN_REQUIRE(mt.g[v] >= 0.0 && mt.g[v] <= 1.79769313486231570815e308, "mix_waves: gain %d is %g, not finite and >= 0", v, mt.g[v]);
        KN_REQUIRE(mt.y[v] || n == 0, "mix_waves: null pointer for voice %d", v);
        KN_REQUIRE(n == 0 || out == mt.y[v] || out + n <= mt.y[v] || mt.y[v] + n <= out, "mix_waves: out overlaps voice %d without being it", v);
        if (mt.g[v] != 0.0) { positive = true; vec = vec && ((uintptr_t)mt.y[v] & 15) == 0; }
    }
    KN_REQUIRE(positive, "mix_waves: no positive gain");
    if (n == 0) return KNNSVC_OK;
    const dim3 grid((unsigned)cdiv64(n, 4 * MX_T));
    if (vec)
        hipLaunchKernelGGL(mix_kernel<true>, grid, dim3(MX_T), 0, (hipStream_t)stream, mt, (long)n, out);
    else
        hipLaunchKernelGGL(mix_kernel<false>, grid, dim3(MX_T), 0, (hipStream_t)stream, mt, (long)n, out);
    return knnsvc_check_launch("mix_waves");
}

extern "C" size_t knnsvc_envelope_workspace_bytes(int64_t n, int32_t hop) {
    if (!ev_hop_ok(hop)) { knnsvc_fail(KNNSVC_EINVAL, "envelope: hop %d is not a positive multiple of 64 up to %d", (int)hop, EV_MAX_HOP); return 0; }
    if (n < 0 || n > DY_MAX_N || n % hop) {
        knnsvc_fail(KNNSVC_EINVAL, "envelope: bad length %lld (a multiple of hop %d in 0 .. 2^36)", (long long)n, (int)hop);
        return 0;
    }
    return ev_workspace(n, hop);
}

extern "C" int knnsvc_envelope_mix(const float* y, int64_t n, const float* x, int64_t nx, int32_t hop, double a, float* out,
                                   double* gains, void* ws, size_t ws_bytes, void* stream) {
    KN_REQUIRE(ev_hop_ok(hop), "envelope_mix: hop %d is not a positive multiple of 64 up to %d", (int)hop, EV_MAX_HOP);
    KN_REQUIRE(n >= 0 && n <= DY_MAX_N && n % hop == 0, "envelope_mix: bad length %lld (a multiple of hop %d in 0 .. 2^36)", (long long)n,
               (int)hop);
    KN_REQUIRE(nx >= 0 && nx <= DY_MAX_N, "envelope_mix: bad source length %lld", (long long)nx);
    KN_REQUIRE(a >= 0.0 && a <= 1.0, "envelope_mix: mix %g outside [0, 1]", a);          // (false for NaN)
    KN_REQUIRE(ws && ((y && out) || n == 0) && (x || nx == 0), "envelope_mix: null pointer");
    KN_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)gains & 7) == 0, "envelope_mix: workspace and gains must be 8-byte aligned");
    KN_REQUIRE(out == y || out + n <= y || y + n <= out, "envelope_mix: out overlaps y without being y");
    const size_t need = ev_workspace(n, hop);
    if (ws_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "envelope_mix: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (n == 0) return KNNSVC_OK;
    hipStream_t st = (hipStream_t)stream;
    const long T = (long)(n / hop);
    double* bx = (double*)ws;
    double* by = bx + T;
    double* tot = by + T;
    hipLaunchKernelGGL(ev_energy_kernel, dim3((unsigned)cdiv64(T, EV_T / 64)), dim3(EV_T), 0, st, y, x, (long)nx, (int)hop, T, bx, by);
    int rc = knnsvc_check_launch("envelope_mix (block energies)");
    if (rc) return rc;
    hipLaunchKernelGGL(ev_total_kernel, dim3(1), dim3(EV_TOTAL_T), 0, st, (const double*)bx, (const double*)by, T, tot);
    if ((rc = knnsvc_check_launch("envelope_mix (totals)"))) return rc;
    const dim3 grid((unsigned)cdiv64(n, 4 * EV_T));
    if ((((uintptr_t)y | (uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL(ev_apply_kernel<true>, grid, dim3(EV_T), 0, st, y, (long)n, (int)hop, T, a, (const double*)bx, (const double*)by,
                           (const double*)tot, out, gains);
    else
        hipLaunchKernelGGL(ev_apply_kernel<false>, grid, dim3(EV_T), 0, st, y, (long)n, (int)hop, T, a, (const double*)bx, (const double*)by,
                           (const double*)tot, out, gains);
    return knnsvc_check_launch("envelope_mix (apply)");
}

extern "C" void knnsvc_peak_limit_layout(int32_t* tile, int32_t* lookahead_at_16k) {
    if (tile) *tile = PK_TILE;
    if (lookahead_at_16k) *lookahead_at_16k = pk_lookahead(16000);
}

extern "C" int knnsvc_peak_limit(const float* y, int64_t n, int32_t sample_rate, double peak_db, float* out, void* stats, void* stream) {
    KN_REQUIRE(n >= 0 && n <= DY_MAX_N, "peak_limit: bad length %lld (0 .. 2^36)", (long long)n);
    KN_REQUIRE(sample_rate >= PK_MIN_RATE && sample_rate <= PK_MAX_RATE, "peak_limit: sample rate %d outside %d .. %d", (int)sample_rate,
               PK_MIN_RATE, PK_MAX_RATE);
    KN_REQUIRE(isfinite(peak_db) && peak_db <= 0.0, "peak_limit: ceiling %g dBFS is not a finite value <= 0", peak_db);
    KN_REQUIRE((y && out) || n == 0, "peak_limit: null pointer");
    KN_REQUIRE(((uintptr_t)stats & 7) == 0, "peak_limit: stats must be 8-byte aligned");
    KN_REQUIRE(out == y || out + n <= y || y + n <= out, "peak_limit: out overlaps y without being y");
    hipStream_t st = (hipStream_t)stream;
    if (stats) {
        hipLaunchKernelGGL(pk_stats_reset_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)stats);
        const int rc = knnsvc_check_launch("peak_limit (statistics reset)");
        if (rc) return rc;
    }
    if (n == 0) return KNNSVC_OK;
    const int L = pk_lookahead(sample_rate);
    int K = 0;
    while ((2 << K) <= 2 * L + 1) ++K;               // W = 2^K <= 2L + 1 < 2W
    const double c = pow(10.0, peak_db / 20.0);
    const long tiles = (long)cdiv64(n, PK_TILE);
    const bool serial = out == y;
    hipLaunchKernelGGL(pk_limit_kernel, dim3(serial ? 1u : (unsigned)tiles), dim3(PK_T), 0, st, y, (long)n, c, L, K, tiles,
                       serial ? tiles : 1L, out, (unsigned long long*)stats);
    return knnsvc_check_launch("peak_limit");
}
