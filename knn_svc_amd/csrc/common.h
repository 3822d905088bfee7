// Shared host/device helpers for libknnsvc_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/knnsvc_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

extern thread_local char g_knnsvc_err[512];

static inline int knnsvc_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_knnsvc_err, sizeof(g_knnsvc_err), fmt, ap);
    va_end(ap);
    return code;
}

#define KN_REQUIRE(cond, ...) do { if (!(cond)) return knnsvc_fail(KNNSVC_EINVAL, __VA_ARGS__); } while (0)

static inline int knnsvc_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return knnsvc_fail(KNNSVC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return KNNSVC_OK;
}

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Segment table of the match-stage entry points (n independent sequences stacked row-wise; the single-sequence calls are n = 1):
// validated on the host, then handed to the kernels BY VALUE as a kernel argument (528 bytes) — no device-side table, no
// allocation, no copy to wait for.
struct KnSegTable { int n; long off[KNNSVC_MAX_SEGMENTS + 1]; };

static inline int kn_seg_table(const int64_t* host_seg, int32_t n_seg, const char* entry, KnSegTable* out) {
    if (!host_seg) return knnsvc_fail(KNNSVC_EINVAL, "%s: null segment table", entry);
    if (n_seg < 1 || n_seg > KNNSVC_MAX_SEGMENTS)
        return knnsvc_fail(KNNSVC_EINVAL, "%s: n_seg %d outside 1..%d", entry, (int)n_seg, KNNSVC_MAX_SEGMENTS);
    if (host_seg[0] != 0) return knnsvc_fail(KNNSVC_EINVAL, "%s: segment table must start at 0 (got %lld)", entry, (long long)host_seg[0]);
    for (int s = 0; s < n_seg; ++s)
        if (host_seg[s + 1] <= host_seg[s])
            return knnsvc_fail(KNNSVC_EINVAL, "%s: segment table must be strictly ascending (entry %d: %lld after %lld)", entry, s + 1,
                               (long long)host_seg[s + 1], (long long)host_seg[s]);
    out->n = n_seg;
    for (int s = 0; s <= KNNSVC_MAX_SEGMENTS; ++s) out->off[s] = host_seg[s < n_seg ? s : n_seg];
    return KNNSVC_OK;
}

// The table of ONE sequence of n rows: the single-sequence entry points are the one-segment case of the segmented ones.
static inline int kn_seg_one(int64_t n, const char* entry, KnSegTable* out) {
    if (n <= 0) return knnsvc_fail(KNNSVC_EINVAL, "%s: bad sizes (%lld rows)", entry, (long long)n);
    const int64_t one[2] = {0, n};
    return kn_seg_table(one, 1, entry, out);
}

// Voice blend (include/knnsvc_hip.h, "Voice blend"): the per-segment weight rows of knnsvc_blend_seg (blend.hip) and
// knnsvc_shift_f0_seg_blend (select.hip), a host table validated here and handed to the kernels by value (2 KiB beside the
// segment table).  Unused rows and voices hold 0.
struct KnBlendWeights { int nv; double w[KNNSVC_MAX_SEGMENTS][KNNSVC_BLEND_MAX_VOICES]; };

static inline int kn_blend_weights(const double* host_weights, int32_t n_seg, int32_t n_voices, const char* entry, KnBlendWeights* out) {
    if (n_voices < 2 || n_voices > KNNSVC_BLEND_MAX_VOICES)
        return knnsvc_fail(KNNSVC_EINVAL, "%s: n_voices %d outside 2..%d", entry, (int)n_voices, KNNSVC_BLEND_MAX_VOICES);
    if (!host_weights) return knnsvc_fail(KNNSVC_EINVAL, "%s: null weight table", entry);
    out->nv = n_voices;
    for (int s = 0; s < KNNSVC_MAX_SEGMENTS; ++s)
        for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v) out->w[s][v] = 0.0;
    for (int s = 0; s < n_seg; ++s) {
        double sum = 0.0;
        bool positive = false;
        for (int v = 0; v < n_voices; ++v) {
            const double a = host_weights[(size_t)s * n_voices + v];
            if (!(a >= 0.0 && a <= 1.79769313486231570815e308))
                return knnsvc_fail(KNNSVC_EINVAL, "%s: segment %d: weight %d is %g, not finite and >= 0", entry, s, v, a);
            positive = positive || a > 0.0;
            sum += a;
            out->w[s][v] = a;
        }
        if (!positive) return knnsvc_fail(KNNSVC_EINVAL, "%s: segment %d: no positive weight", entry, s);
        if (!(sum - 1.0 <= 1e-6 && 1.0 - sum <= 1e-6))
            return knnsvc_fail(KNNSVC_EINVAL, "%s: segment %d: the weights sum to %.9g, not 1 (the caller normalises)", entry, s, sum);
    }
    return KNNSVC_OK;
}

// One segment's row of the table as the mixing code wants it: w[v] (0 beyond nv) and how many are non-zero.
struct KnBlendRow { double w[KNNSVC_BLEND_MAX_VOICES]; int live; };
__device__ __forceinline__ KnBlendRow kn_blend_row(const KnBlendWeights& bw, int s) {
    KnBlendRow r;
    r.live = 0;
#pragma unroll
    for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v) {
        r.w[v] = v < bw.nv ? bw.w[s][v] : 0.0;
        if (r.w[v] != 0.0) ++r.live;
    }
    return r;
}
// (float)(sum_v w[v] * (double)x[v]) over the voices with a non-zero weight, in ascending order, every operation on its own; the
// sum starts with the first product.  x[v] of a zero-weight voice is not looked at; a single non-zero weight hands its x on as it is.
__device__ __forceinline__ float kn_blend_mix(const KnBlendRow& r, const float (&x)[KNNSVC_BLEND_MAX_VOICES]) {
#pragma clang fp contract(off)
    double acc = 0.0;
    float one = 0.f;
    bool first = true;
#pragma unroll
    for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v) {
        if (r.w[v] != 0.0) {
            const double p = r.w[v] * (double)x[v];
            acc = first ? p : acc + p;
            first = false;
            one = x[v];
        }
    }
    return r.live == 1 ? one : (float)acc;
}

// KNNSVC_MATCH_GENERIC_K=1: the match stage at k = 4 skips its fast paths and runs the K kernels as any other k (select.hip)
bool knnsvc_match_generic_k();

// A/B switches of the three host dispatchers (conv_gemm.hip, attention.hip, elementwise.hip), read from the environment ONCE — by
// the first call that looks at any of them — into this record; knnsvc_reload_knobs() re-reads them (tests that switch a route
// inside one process call it through ops.reload_knobs()).  Defaults are the product configuration; none of these changes results
// beyond what its comment says.  ONE record for the library: the definition, kn_knobs() and the reload are in api.hip.
struct KnKnobs {
    int quad = 1;                  // KNNSVC_QUAD: 0 = no 256x256 kernel, 1 = by shape (default), 2 = every qualifying launch
    bool quad_epi = true;          // KNNSVC_QUAD_EPI=0: generic epilogue behind the quad kernel (bit-identical, slower)
    bool generic_epilogue = false; // KNNSVC_EPILOGUE=g: the generic (64-bit addressed) epilogue everywhere
    bool win = true;               // KNNSVC_WIN=0: tap-major kernel instead of the windowed one (other summation order)
    bool win_wide = true;          // KNNSVC_WIN_WIDE=0: the windowed kernels keep the column-per-lane epilogue
    bool win_small = true, win_deep = true, win160 = true;      // KNNSVC_WIN_SMALL / _DEEP / WIN160 = 0: tile-shape rules off
    bool gemm_small = true;        // KNNSVC_GEMM_SMALL=0: no 64x64 tile for launches below one round of 128x128 tiles
    int attention = 2;             // KNNSVC_ATTENTION = f16x2 (2, default) | bf16x3 (3) | fp32 (0: the exact-f32 MFMA kernel)
    int conv0_rp = 2;              // KNNSVC_CONV0_RP: conv0's rows per pass, 2 (default), 4, or 1 = the shuffle-sum kernel, for A/B
    int conv0_subs = 8;            // KNNSVC_CONV0_SUBS: spans of 64 rows a conv0 workgroup walks on long inputs (1..64)
    bool loaded = false;
};
const KnKnobs& kn_knobs();

// Opt-in of KERNEL to `bytes` of dynamic LDS (a launch with more than 64 KiB fails without it).  The attribute is set once per
// kernel instantiation and process, and again only when a later call needs more.  `entry`: the API entry point, for the message.
template <auto KERNEL>
static inline int kn_lds_optin(int bytes, const char* entry) {
    static int granted = 0;
    if (bytes <= granted) return KNNSVC_OK;
    if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return knnsvc_fail(KNNSVC_EHIP, "%s: hipFuncSetAttribute failed", entry);
    granted = bytes;
    return KNNSVC_OK;
}

// A wave's TM x TN accumulator tiles of 32x32 (v_mfma_f32_32x32x*) in a block of (4 or 8 / WN) x WN waves
template <int WN, int TM, int TN>
struct Acc32 {
    // accumulator element (tile i,j; register r) of this lane -> (row, col) inside the block tile
    __device__ __forceinline__ static int acc_row(int wave, int lane, int i, int r) {
        return (wave / WN) * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    }
    __device__ __forceinline__ static int acc_col(int wave, int lane, int j) {
        return (wave % WN) * TN * 32 + j * 32 + (lane & 31);
    }
};

// acc[TM][TN] = 0 for a wave's accumulator tiles of NR floats.  A macro on purpose: the same loops behind a function call (or
// `= {}`) reach the optimiser in another order and reshuffle the scalar prologue of every kernel (tools/isa_diff.py).
#define KN_ZERO_ACC(ACC, TM, TN, NR)                                                                            \
    _Pragma("unroll") for (int i = 0; i < (TM); ++i)                                                           \
        _Pragma("unroll") for (int j = 0; j < (TN); ++j)                                                       \
            _Pragma("unroll") for (int r = 0; r < (NR); ++r) ACC[i][j][r] = 0.f;

// Zero-fill as an ORDINARY KERNEL on the caller's stream (bytes % 4 == 0).  Not hipMemsetAsync: with several generators in flight on
// several streams its fills were not ordered with the kernels that follow them on the same stream the way a kernel is (round 5:
// csrc/models.hip, zero_slots — run-to-run different samples in the dataset-mode pipeline until the memset became a kernel).
namespace {
__global__ __launch_bounds__(256) void kn_zero_kernel(unsigned* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}
}  // namespace
static inline int kn_zero_async(void* p, size_t bytes, hipStream_t st) {
    const long n = (long)(bytes / 4);
    if (n == 0) return KNNSVC_OK;
    hipLaunchKernelGGL(kn_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned*)p, n);
    return knnsvc_check_launch("zero_fill");
}

// GELU(x) = x Phi(x) (torch.nn.functional.gelu, exact erf form: wavlm/modules.py, WavLM.py feature extractor and FFN).
// Phi(-|x|) = 0.5 erfc(|x| / sqrt 2) = P(t) exp(-x^2 / 2), t = 1 / (1 + p |x| / sqrt 2), P a degree-6 polynomial (minimax fit of
// erfc(z) exp(z^2), max error 8e-9 in exact arithmetic; the family of Abramowitz & Stegun 7.1.26); Phi(|x|) = 1 - Phi(-|x|).
// 15 VALU instructions, two of them transcendental (v_rcp_f32, v_exp_f32), against ~45 for the library erff — the step evaluates
// 2.8e9 GELUs (conv feature extractor, FFN1).  Accuracy in fp32 against the exact function: rms 6e-8, max 3.8e-7 over [-8, 8]
// — torch's own fp32 GELU: rms 1.4e-7, max 1.1e-6 — and the negative tail keeps its relative accuracy (no 1 + erf
// cancellation).  -DKN_GELU_ERFF restores the library form.
__device__ __forceinline__ float kn_gelu(float x) {
#ifdef KN_GELU_ERFF
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
#else
    // contraction off: whether `1 - p * e` became one fma used to depend on the code around the call, so the same activation could
    // differ by an ulp between two kernels (or two epilogue variants of one kernel); every rounding below is now spelled out
#pragma clang fp contract(off)
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.39f, z, 1.0f));
    float p = -0.1137684788031453f;                       // 0.5 x the fitted coefficients
    p = fmaf(p, t, 0.4433318425354039f);
    p = fmaf(p, t, -0.3176995829519751f);
    p = fmaf(p, t, 0.32477925011974735f);
    p = fmaf(p, t, 0.045694387408764885f);
    p = fmaf(p, t, 0.11766258084307574f);
    p *= t;
    const float h = p * __builtin_amdgcn_exp2f(-(z * z) * 1.4426950408889634f);      // Phi(-|x|)
    return x * (x >= 0.f ? 1.0f - h : h);
#endif
}

// Two activations per instruction where the ISA has a packed fp32 form (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32; the two
// reciprocals and the two exponentials stay scalar): every component goes through exactly the roundings of kn_gelu, so the result
// is bit-identical to it — a change of instruction selection only (the conv stack's first layer evaluates 1e9 of these per step
// and is VALU-bound).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 kn_gelu2(f32x2 x) {
#ifdef KN_GELU_ERFF
    return (f32x2){kn_gelu(x[0]), kn_gelu(x[1])};
#else
#pragma clang fp contract(off)
    const f32x2 ax = {fabsf(x[0]), fabsf(x[1])};
    const f32x2 z = ax * 0.70710678118654752440f;
    const f32x2 u = __builtin_elementwise_fma((f32x2)(0.39f), z, (f32x2)(1.0f));
    const f32x2 t = {__builtin_amdgcn_rcpf(u[0]), __builtin_amdgcn_rcpf(u[1])};
    f32x2 p = (f32x2)(-0.1137684788031453f);
    p = __builtin_elementwise_fma(p, t, (f32x2)(0.4433318425354039f));
    p = __builtin_elementwise_fma(p, t, (f32x2)(-0.3176995829519751f));
    p = __builtin_elementwise_fma(p, t, (f32x2)(0.32477925011974735f));
    p = __builtin_elementwise_fma(p, t, (f32x2)(0.045694387408764885f));
    p = __builtin_elementwise_fma(p, t, (f32x2)(0.11766258084307574f));
    p = p * t;
    const f32x2 ea = (-(z * z)) * 1.4426950408889634f;
    const f32x2 h = p * (f32x2){__builtin_amdgcn_exp2f(ea[0]), __builtin_amdgcn_exp2f(ea[1])};      // Phi(-|x|)
    const f32x2 omh = 1.0f - h;
    return x * (f32x2){x[0] >= 0.f ? omh[0] : h[0], x[1] >= 0.f ? omh[1] : h[1]};
#endif
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Wave-wide sum on the VALU: four DPP adds fold each row of 16 lanes (xor 1, xor 2, half-mirror, mirror), four readlanes pick
// the row sums.  ds_bpermute-based __shfl_xor trees cost six dependent LDS round trips per value — in a frame-sequential
// kernel that is latency on the critical path of every frame.  Every lane gets the total.
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}
// the same fold for a double (two 32-bit DPP moves per step)
__device__ __forceinline__ double wave_sum_d_dpp(double v) {
#define KN_DPP_D(CTRL)                                                                                          \
    {                                                                                                          \
        const long b = __builtin_bit_cast(long, v);                                                            \
        const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, true), hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true); \
        v += __builtin_bit_cast(double, ((long)hi << 32) | (unsigned)lo);                                      \
    }
    KN_DPP_D(0xB1) KN_DPP_D(0x4E) KN_DPP_D(0x141) KN_DPP_D(0x140)
#undef KN_DPP_D
    const long b = __builtin_bit_cast(long, v);
    const int lo = (int)b, hi = (int)(b >> 32);
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r[k] = __builtin_bit_cast(double, ((long)__builtin_amdgcn_readlane(hi, 16 * k) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, 16 * k));
    return (r[0] + r[1]) + (r[2] + r[3]);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
