// Voice blend: the matched frames of 2 to 4 voices (features, harmonics) mixed per segment with that segment's weights, between
// the match stage and the tail.  include/knnsvc_hip.h ("Voice blend", point 2) is the specification; upstream has no counterpart
// (it converts towards one pool).  The blended f0 median of point 3 lives in select.hip's one shift kernel.
#include "common.h"

namespace {

// The voices' stacked rows: a host table of device pointers handed over by value like the segment table.
struct KnBlendPtrs { const float* x[KNNSVC_BLEND_MAX_VOICES]; };

constexpr int BL_ROWS = 4;     // rows per workgroup

// blockIdx.y = segment, blockIdx.x = BL_ROWS rows of it (VEC: one float4 per thread, voice and step; dim % 4 == 0 and every
// pointer 16-byte aligned).  The weights of the segment are uniform over the workgroup, so a zero-weight voice costs a scalar
// branch and no load.  Memory bound: (live voices + 1) * 4 bytes per element, every access a full 16-byte lane in VEC.
template <bool VEC>
__global__ __launch_bounds__(256) void blend_kernel(const KnBlendPtrs xs, int dim, const KnSegTable seg, const KnBlendWeights bw,
                                                    float* out) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const long o = seg.off[s], T = seg.off[s + 1] - o;
    const long j0 = (long)blockIdx.x * BL_ROWS;
    if (j0 >= T) return;
    const KnBlendRow row = kn_blend_row(bw, s);
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < BL_ROWS; ++r) {
        const long j = j0 + r;
        if (j >= T) break;
        const long base = (o + j) * (long)dim;
        if constexpr (VEC) {
            for (int col = tid * 4; col < dim; col += 1024) {
                f32x4 xv[KNNSVC_BLEND_MAX_VOICES];
#pragma unroll
                for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v)
                    xv[v] = row.w[v] != 0.0 ? *(const f32x4*)(xs.x[v] + base + col) : (f32x4)(0.f);
                f32x4 vo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x[KNNSVC_BLEND_MAX_VOICES] = {xv[0][e], xv[1][e], xv[2][e], xv[3][e]};
                    vo[e] = kn_blend_mix(row, x);
                }
                *(f32x4*)(out + base + col) = vo;
            }
        } else {
            for (int col = tid; col < dim; col += 256) {
                float x[KNNSVC_BLEND_MAX_VOICES];
#pragma unroll
                for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v) x[v] = row.w[v] != 0.0 ? xs.x[v][base + col] : 0.f;
                out[base + col] = kn_blend_mix(row, x);
            }
        }
    }
}

}  // namespace

extern "C" int knnsvc_blend_seg(const float* const* host_x, int32_t n_voices, int32_t dim, const int64_t* host_seg, int32_t n_seg,
                                const double* host_weights, float* out, void* stream) {
    const char* entry = "blend_seg";
    KnSegTable seg;
    KnBlendWeights bw;
    KN_REQUIRE(host_x && out, "%s: null pointer", entry);
    if (const int rc = kn_seg_table(host_seg, n_seg, entry, &seg)) return rc;
    if (const int rc = kn_blend_weights(host_weights, n_seg, n_voices, entry, &bw)) return rc;
    KN_REQUIRE(dim > 0, "%s: bad feature dim %d", entry, (int)dim);
    KnBlendPtrs xs;
    bool vec = dim % 4 == 0 && ((uintptr_t)out & 15) == 0;
    for (int v = 0; v < KNNSVC_BLEND_MAX_VOICES; ++v) {
        xs.x[v] = v < n_voices ? host_x[v] : nullptr;
        KN_REQUIRE(v >= n_voices || xs.x[v], "%s: null pointer for voice %d", entry, v);
        vec = vec && ((uintptr_t)xs.x[v] & 15) == 0;
    }
    long longest = 0;
    for (int s = 0; s < n_seg; ++s) longest = seg.off[s + 1] - seg.off[s] > longest ? seg.off[s + 1] - seg.off[s] : longest;
    const long nb = cdiv64(longest, BL_ROWS);
    KN_REQUIRE(nb <= 0x7FFFFFFFl, "%s: %ld rows in one segment are too many for one launch", entry, longest);
    const dim3 grid((unsigned)nb, (unsigned)n_seg);
    if (vec)
        hipLaunchKernelGGL(blend_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, xs, (int)dim, seg, bw, out);
    else
        hipLaunchKernelGGL(blend_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, xs, (int)dim, seg, bw, out);
    return knnsvc_check_launch(entry);
}
