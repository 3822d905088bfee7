// Time scale: a stacked batch of query sequences (features and f0) re-timed along the frame axis, between the encoder and the
// match stage.  include/knnsvc_hip.h ("Time scale") is the specification; upstream's counterpart is the F.interpolate(...,
// mode='linear') of the query features in ddsp_matcher.py:545-548 (it never stretches the f0 it hands to the vocoder).
#include "common.h"

namespace {

// Per-segment c = 1 / scale_factor of knnsvc_time_scale_seg: a host table handed over by value like the segment tables.
struct KnInvScales { double c[KNNSVC_MAX_SEGMENTS]; };

constexpr int TS_ROWS = 4;     // output rows per feature workgroup (neighbouring output rows share input rows: L2 hits)

// Source rows and weights of output row j of a segment of T input rows: PyTorch's linear, align_corners=False, scale_factor-given
// source index.  The index is ONE explicit fused multiply-add, fma(c, j + 0.5, -0.5), rounded once: that is how torch's CPU kernel
// evaluates `scale * (dst + 0.5) - 0.5`, and the two-rounding form differs from it wherever the product lies just above a power
// of two (the weight by 5.7e-14 at r ~ 512).  Every other operation is an fp64 operation of its own (no contraction).
struct KnTap { long i0, i1; double l0, l1; };
__device__ __forceinline__ KnTap ts_tap(long j, long T, double c) {
#pragma clang fp contract(off)
    double r = __builtin_fma(c, (double)j + 0.5, -0.5);
    if (r < 0.0) r = 0.0;
    KnTap t;
    if (!(r < (double)T)) {                  // i0 > T - 1 (possible only through rounding); also keeps the conversion below in range
        t.i0 = t.i1 = T - 1; t.l1 = 0.0;
    } else {
        t.i0 = (long)r;
        t.i1 = t.i0 + (t.i0 < T - 1 ? 1 : 0);
        t.l1 = r - (double)t.i0;
    }
    t.l0 = 1.0 - t.l1;
    return t;
}

__device__ __forceinline__ float ts_mix(const KnTap& t, float a, float b) {
#pragma clang fp contract(off)
    const double pa = t.l0 * (double)a, pb = t.l1 * (double)b;
    return (float)(pa + pb);
}

// blockIdx.y = segment.  blockIdx.x < feat_blocks: TS_ROWS output rows of the features each (VEC: one float4 per thread and
// step, dim % 4 == 0 and both pointers 16-byte aligned); the blocks behind them: 256 output frames of f0 each.  Either part may
// be absent (feat_blocks == 0 / f0 == nullptr).  A row reads rows i0, i1 of its OWN segment only.
template <bool VEC>
__global__ __launch_bounds__(256) void time_scale_kernel(const float* __restrict__ x, int dim, const float* __restrict__ f0,
                                                         const KnSegTable seg_in, const KnSegTable seg_out, const KnInvScales inv,
                                                         int feat_blocks, float* __restrict__ x_out, float* __restrict__ f0_out) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const long oi = seg_in.off[s], T = seg_in.off[s + 1] - oi;
    const long oo = seg_out.off[s], To = seg_out.off[s + 1] - oo;
    const double c = inv.c[s];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < feat_blocks) {
        const long j0 = (long)blockIdx.x * TS_ROWS;
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r) {
            const long j = j0 + r;
            if (j >= To) break;
            const KnTap t = ts_tap(j, T, c);
            const float* __restrict__ a = x + (oi + t.i0) * (long)dim;
            const float* __restrict__ b = x + (oi + t.i1) * (long)dim;
            float* __restrict__ o = x_out + (oo + j) * (long)dim;
            if constexpr (VEC) {
                for (int col = tid * 4; col < dim; col += 1024) {
                    const f32x4 va = *(const f32x4*)(a + col), vb = *(const f32x4*)(b + col);
                    f32x4 vo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) vo[e] = ts_mix(t, va[e], vb[e]);
                    *(f32x4*)(o + col) = vo;
                }
            } else {
                for (int col = tid; col < dim; col += 256) o[col] = ts_mix(t, a[col], b[col]);
            }
        }
        return;
    }
    // f0: voicing follows the nearer frame (a tie goes left); two voiced neighbours are interpolated in log-frequency, a voiced
    // frame beside an unvoiced one is kept as it is: a note's edge never glides towards 0 Hz.
    const long j = ((long)blockIdx.x - feat_blocks) * 256 + tid;
    if (j >= To) return;
    const KnTap t = ts_tap(j, T, c);
    const float fa = f0[oi + t.i0], fb = f0[oi + t.i1];
    const float fn = t.l1 > 0.5 ? fb : fa;
    float r;
    if (fn <= 0.f) r = 0.f;
    else if (fa > 0.f && fb > 0.f) {
        const double la = t.l0 * log((double)fa), lb = t.l1 * log((double)fb);
        r = (float)exp(la + lb);
    } else r = fn;
    f0_out[oo + j] = r;
}

}  // namespace

extern "C" int knnsvc_time_scale_seg(const float* x, int32_t dim, const float* f0, const int64_t* host_seg_in,
                                     const int64_t* host_seg_out, const double* host_inv_scale, int32_t n_seg, float* x_out,
                                     float* f0_out, void* stream) {
    const char* entry = "time_scale_seg";
    KnSegTable si, so;
    if (const int rc = kn_seg_table(host_seg_in, n_seg, entry, &si)) return rc;
    if (const int rc = kn_seg_table(host_seg_out, n_seg, entry, &so)) return rc;
    KN_REQUIRE(host_inv_scale, "%s: null inv_scale table", entry);
    KN_REQUIRE((x != nullptr) == (x_out != nullptr), "%s: x and x_out must both be given or both be NULL", entry);
    KN_REQUIRE((f0 != nullptr) == (f0_out != nullptr), "%s: f0 and f0_out must both be given or both be NULL", entry);
    KN_REQUIRE(x || f0, "%s: nothing to do (no features and no f0)", entry);
    KN_REQUIRE(!x || dim > 0, "%s: bad feature dim %d", entry, (int)dim);
    KnInvScales inv;
    for (int s = 0; s < KNNSVC_MAX_SEGMENTS; ++s) inv.c[s] = 1.0;
    long longest = 0;
    for (int s = 0; s < n_seg; ++s) {
        const double c = host_inv_scale[s];
        KN_REQUIRE(c > 0.0 && c <= 1.79769313486231570815e308, "%s: segment %d: inv_scale %g is not finite and > 0", entry, s, c);
        inv.c[s] = c;
        const long To = so.off[s + 1] - so.off[s];
        longest = To > longest ? To : longest;
    }
    const long fb = x ? cdiv64(longest, TS_ROWS) : 0, pb = f0 ? cdiv64(longest, 256) : 0;
    KN_REQUIRE(fb + pb <= 0x7FFFFFFFl, "%s: %ld output rows in one segment are too many for one launch", entry, longest);
    const bool vec = x && dim % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)x_out & 15) == 0;
    const dim3 grid((unsigned)(fb + pb), (unsigned)n_seg);
    if (vec)
        hipLaunchKernelGGL(time_scale_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)dim, f0, si, so, inv, (int)fb, x_out, f0_out);
    else
        hipLaunchKernelGGL(time_scale_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)dim, f0, si, so, inv, (int)fb, x_out, f0_out);
    return knnsvc_check_launch(entry);
}
