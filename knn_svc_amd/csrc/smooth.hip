// Concatenation-smoothness weight optimisation, fully on the device, for K neighbours per frame (1 <= K <= 8; the reference's 4
// is one instantiation).
// Reference: ddsp_prematch_dataset.py:574-680 (compute_wavlm_weight), :807-924
// (compute_extended_weight), :426-428 (softmax weights), :449-461 (the two MSE costs).
//
// The reference runs autograd + torch.optim.Adam(amsgrad) with a host sync per iteration and
// re-reads 3 x [N,K,D] gathered features every step.  The loss is a quadratic form in the
// softmax weights, so this implementation
//   1. reduces the features once to two 2K x 2K Gram matrices per adjacent frame pair
//      (gram_kernel<K>; vectors are centred on their mean first — the weights of each frame sum
//      to one, so centring changes neither loss nor softmax gradient but removes cancellation);
//   2. runs the whole Adam loop — loss, analytic gradient, amsgrad update, best-iterate
//      tracking and the reference's three stopping rules — inside ONE persistent workgroup,
//      O(N * (2K)^2) flops per iteration and no host round trips.
// The loop for every K is adam_k_kernel<K>: state in the workspace as [K][rows] planes.  k = 4 has two fast paths beside it, which
// KNNSVC_MATCH_GENERIC_K=1 skips: adam_reg_kernel<1|2|3> (up to 1536 rows, everything in registers) and adam_kernel (longer
// sequences, rows of float4: 33 to 55 % faster than the planes at k = 4 and not bit-identical to them, profiles/adam_long_ab.txt).
// The loop control and the per-element update are the same text in the three bodies: as shared helpers they changed the register
// loops' instruction streams, so only the bias corrections are functions (adam_step_size, adam_rbc2).
#include "common.h"

namespace {

constexpr int KW = 4;                       // neighbours per frame of the k = 4 fast paths
constexpr int GE = KW * (2 * KW - 1);       // and their Gram entries per pair (28)

// Sums over a row's K values are pairwise trees: (a + b) + (c + d) at K = 4.
template <int N>
__device__ __forceinline__ float tree_sum(const float* p) {
    if constexpr (N == 1) return p[0];
    else return tree_sum<N / 2>(p) + tree_sum<N - N / 2>(p + N / 2);
}
// Entry (i, j), i != j, of the strict upper triangle of a symmetric R x R Gram matrix, R = 2K.  The R centred vectors sum to zero,
// so every row of G sums to zero and the diagonal is implied: (G c)_i = sum_{j != i} G_ij (c_j - c_i)
template <int R>
__device__ __forceinline__ constexpr int tri_r(int i, int j) {
    return i < j ? i * (R - 1) - i * (i - 1) / 2 + (j - i - 1) : j * (R - 1) - j * (j - 1) / 2 + (i - j - 1);
}

// Floats of workspace per segment: Gram [K(2K-1)][nq] | theta, m, v, vmax, best, scratch: 6 x [K][nq] | exchange [2][K][nq] (used
// when LDS is too small).  adam_kernel (k = 4) keeps the same amounts as rows of float4.
inline size_t ws_floats_k(long nq, int k) { return (size_t)(k * (2 * k - 1)) * nq + (size_t)6 * k * nq + (size_t)2 * k * nq; }
// longest sequence whose two exchange planes fit 144 KB of LDS (4608 rows at K = 4, 2304 at K = 8)
__host__ __device__ constexpr long adam_lds_rows(int k) { return 144 * 1024 / (2 * k * 4); }

// Segments of knnsvc_smooth_weights[_seg]: row offsets, and where each segment's workspace starts, in units of 64 bytes from the
// aligned workspace base.  By value, like KnSegTable.
struct SmoothSegs { int n; long off[KNNSVC_MAX_SEGMENTS + 1]; unsigned ws64[KNNSVC_MAX_SEGMENTS]; };
// the segments one launch works on: block b -> segment id[b]
struct SegList { int n; unsigned char id[KNNSVC_MAX_SEGMENTS]; };

__device__ __forceinline__ float* seg_ws(float* base, const SmoothSegs& sg, int s) { return base + (size_t)sg.ws64[s] * 16; }

// block per frame pair t.  Both cost terms are quadratic forms in the SAME coefficient vector
// c = [w[t+1,:], -w[t,:]] (term a over rows F[idx[t+1,k]-1], F[idx[t,k]]; term b over F[idx[t+1,k]], F[idx[t,k]+1]),
// so only the sum of the two centred 2K x 2K Gram matrices is kept: its K(2K - 1) off-diagonal entries per pair.
// row_scale (optional) [nq][K]: candidate k of frame t and its +-1 neighbours are multiplied by row_scale[t][k]
// (compute_weight_with_amp, ddsp_prematch_dataset.py:684-713); the centring argument is unchanged because the
// coefficient vector still sums to zero.
// The body of gram_kernel (all pairs of all segments): idx, row_scale and gram already at the sequence, nq its length, t the pair.
template <int K>
__device__ __forceinline__ void gram_body(const long* __restrict__ idx, long nq, const float* __restrict__ pool,
                                          long np, int dim, int ld, const float* __restrict__ row_scale,
                                          float* __restrict__ gram, const long t) {
    constexpr int R = 2 * K, GEK = K * (2 * K - 1), NQ = (GEK + 3) / 4;
    constexpr bool whole = GEK % 4 == 0;    // the four waves share the entries evenly: no tail to guard (K = 4, 8)
    extern __shared__ float sm[];           // [R][dim] centred vectors of the current term
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    float rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rs[r] = row_scale ? (r < K ? row_scale[(t + 1) * K + r] : row_scale[t * K + (r - K)]) : 1.f;
    for (int term = 0; term < 2; ++term) {
        __syncthreads();
        for (int c = tid; c < dim; c += 256) {
            float v[R], mean = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                long id;
                if (r < K) id = idx[(t + 1) * K + r] + (term == 0 ? -1 : 0);
                else id = idx[t * K + (r - K)] + (term == 0 ? 0 : 1);
                id = id < 0 ? 0 : (id > np - 1 ? np - 1 : id);
                v[r] = pool[id * (long)ld + c];
                if (row_scale) v[r] *= rs[r];
                mean += v[r];
            }
            mean = mean / (float)R;
#pragma unroll
            for (int r = 0; r < R; ++r) sm[r * dim + c] = v[r] - mean;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int e = wave + 4 * q;                 // wave-uniform
            if (whole || e < GEK) {
                int i = 0, rem = e;                       // unpack e -> (i < j)
                while (rem >= R - 1 - i) { rem -= R - 1 - i; ++i; }
                const int j = i + 1 + rem;
                double s = 0.0;
                for (int c = lane; c < dim; c += 64) s += (double)sm[i * dim + c] * (double)sm[j * dim + c];
                acc[q] += wave_sum_d(s);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (whole || wave + 4 * q < GEK) gram[((long)(wave + 4 * q)) * nq + t] = (float)acc[q];
    }
}

// one launch over the adjacent pairs of all segments: segment s has len - 1 of them, pair numbers start at off[s] - s
template <int K>
__global__ __launch_bounds__(256) void gram_kernel(const long* __restrict__ idx, const SmoothSegs sg, const float* __restrict__ pool,
                                                      long np, int dim, int ld, const float* __restrict__ row_scale,
                                                      float* __restrict__ ws) {
    const long b = blockIdx.x;
    int s = 0;
    for (int j = 1; j < sg.n; ++j) if (sg.off[j] - j <= b) s = j;       // the last segment whose first pair is <= b (uniform)
    const long o = sg.off[s];
    gram_body<K>(idx + o * K, sg.off[s + 1] - o, pool, np, dim, ld, row_scale ? row_scale + o * K : row_scale, seg_ws(ws, sg, s),
                 b - (o - s));
}

// The two per-element pieces of an iteration that were IEEE divides, square roots and expf: 250 of the 410 VALU instructions a
// frame costs per iteration (one CU runs the whole loop).  Inside the loop they run on the hardware's 1-ulp v_exp_f32 / v_rcp_f32 /
// v_sqrt_f32: 4.67 -> 2.65 us per iteration.  The optimiser's trajectory is only defined up to such roundings anyway (a different
// summation order of the loss already moves the weights by 2e-4), and measured against the reference-generated fixtures the two
// forms are level: weights max|d| 3.5e-4 / 2.4e-4 (IEEE) vs 2.9e-4 / 2.8e-4 (WavLM / harmonics, g5), 1.1e-6 vs 1.2e-6
// (amplitude-scaled), the same iteration counts (201 / 201 / 401), file-level waveform rms 5.4e-7 vs 1.2e-6 on the post_opt
// fixture (bar 1e-4), everything else unchanged.  The FINAL weights (softmax of the best iterate) keep expf and the IEEE divide.
__device__ __forceinline__ f32x4 loop_softmax4(f32x4 th, float mx) {
#pragma clang fp contract(off)
    f32x4 e;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = __builtin_amdgcn_exp2f((th[k] - mx) * 1.44269504088896341f);
    const float den = (e[0] + e[1]) + (e[2] + e[3]);       // >= 1: the maximum contributes exp2(0)
    return e * __builtin_amdgcn_rcpf(den);
}
// theta + step_size * m / (sqrt(vmax) / sqrt(1 - b2^t) + eps); rbc2 = 1 / sqrt(1 - b2^t), one IEEE divide per iteration
__device__ __forceinline__ float loop_step(float th, float m, float vmax, float rbc2, float eps, float step_size) {
#pragma clang fp contract(off)
    const float denom = __builtin_amdgcn_sqrtf(vmax) * rbc2 + eps;
    return th + step_size * (m * __builtin_amdgcn_rcpf(denom));
}

// The bias corrections of iteration t (pb = beta^t, in double): the step size -lr / (1 - b1^t) with lr = 0.1, and 1 / sqrt(1 - b2^t).
// These two are all of the loop the three bodies below share as functions: the loop control and the per-element update are written
// out in each, because as helpers (by reference, by value or as a struct) they change the register loops' instruction streams.
__device__ __forceinline__ float adam_step_size(double pb1) { return (float)(-(0.1 / (1.0 - pb1))); }
__device__ __forceinline__ float adam_rbc2(double pb2) { const float bc2_sqrt = (float)sqrt(1.0 - pb2); return 1.0f / bc2_sqrt; }

// The long loop of k = 4 (more than 1536 rows): state in the workspace as rows of float4, softmax weights and gradients exchanged
// through LDS while they fit (adam_lds_rows(4) rows) and through the workspace beyond.
__device__ __forceinline__ void adam_body(long nq, int dim, float scale, int max_iter,
                                          const float* __restrict__ gram, float* __restrict__ state,
                                          float* __restrict__ xch_global, int use_lds,
                                          float* __restrict__ out_w, int* __restrict__ out_iters) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ double red[2][16];
    float* xw = use_lds ? sm : xch_global;                 // [nq][4] softmax weights
    float* xg = xw + nq * KW;                              // [nq][4] gradient w.r.t. w from the pair (t-1, t)
    f32x4* theta = (f32x4*)state;
    f32x4* m1 = theta + nq; f32x4* v2 = m1 + nq; f32x4* vmax = v2 + nq; f32x4* best = vmax + nq;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double S = (double)scale / ((double)dim * (double)(nq - 1));
    const float twoS = (float)(2.0 * S);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long t = tid; t < nq; t += 1024) { theta[t] = zero; m1[t] = zero; v2[t] = zero; vmax[t] = zero; best[t] = zero; }
    __syncthreads();

    double min_loss = 20000.0, conv_min = 20000.0;
    int since = 0, it = 0;
    const float b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
    double pb1 = 1.0, pb2 = 1.0;
    const bool forced = max_iter < 0;            // measurement mode: exactly |max_iter| iterations, stopping rules off
    const int cap = forced ? -max_iter : max_iter;
    for (it = 0; it < cap; ++it) {
        // ---- phase 1: softmax weights ---------------------------------------------------------
        for (long t = tid; t < nq; t += 1024) {
            const f32x4 th = theta[t];
            const float mx = fmaxf(fmaxf(th[0], th[1]), fmaxf(th[2], th[3]));
            *(f32x4*)&xw[t * KW] = loop_softmax4(th, mx);
        }
        __syncthreads();
        // ---- phase 2: per pair quadratic forms, gradient w.r.t. the weights ---------------------
        double lsum = 0.0;
        for (long t = tid; t < nq - 1; t += 1024) {
            const f32x4 w1 = *(const f32x4*)&xw[(t + 1) * KW], w0 = *(const f32x4*)&xw[t * KW];
            const float c[8] = {w1[0], w1[1], w1[2], w1[3], -w0[0], -w0[1], -w0[2], -w0[3]};
            float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            {
                float g[GE];
#pragma unroll
                for (int e = 0; e < GE; ++e) g[e] = gram[((long)e) * nq + t];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j != i) s += g[tri_r<8>(i, j)] * (c[j] - c[i]);
                    y[i] += s;
                }
            }
            float qf = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) qf += c[i] * y[i];
            lsum += (double)qf;
            f32x4 gf = {twoS * y[0], twoS * y[1], twoS * y[2], twoS * y[3]};
            *(f32x4*)&xg[(t + 1) * KW] = gf;                       // d/dw[t+1,:] from pair t
            // d/dw[t,:] from pair t is kept in the (unused) slot layout of the state pass below
            f32x4 gs = {-twoS * y[4], -twoS * y[5], -twoS * y[6], -twoS * y[7]};
            best[nq + t] = gs;                                     // scratch row after `best`
        }
        lsum = wave_sum_d_dpp(lsum);                  // two barriers per iteration: see adam_reg_kernel
        if (lane == 0) red[it & 1][wave] = lsum;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) tot += red[it & 1][i];
        const float loss = (float)(S * tot);
        // ---- phase 3: the reference's loop control (uniform across the block) -------------------
        if (it % 100 == 1) {
            if (!forced && fabs(min_loss - conv_min) < 1e-5) break;
            conv_min = min_loss;
        }
        const bool improved = loss < (float)min_loss;
        if (improved) { min_loss = (double)loss; since = 0; } else ++since;
        if (!forced && since >= 1000) break;
        // ---- phase 4: gradient through softmax + Adam(amsgrad) ----------------------------------
        pb1 *= 0.9; pb2 *= 0.999;
        const float step_size = adam_step_size(pb1), rbc2 = adam_rbc2(pb2);
        for (long t = tid; t < nq; t += 1024) {
            const f32x4 w = *(const f32x4*)&xw[t * KW];
            f32x4 g = zero;
            if (t >= 1) g = *(const f32x4*)&xg[t * KW];
            if (t < nq - 1) g += best[nq + t];
            const float dotwg = (w[0] * g[0] + w[1] * g[1]) + (w[2] * g[2] + w[3] * g[3]);
            f32x4 gt = w * (g - dotwg);
            f32x4 th = theta[t];
            if (improved) best[t] = th;
            f32x4 mm = m1[t], vv = v2[t], vm = vmax[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mm[k] = mm[k] + (gt[k] - mm[k]) * omb1;
                vv[k] = vv[k] * b2 + (omb2 * gt[k]) * gt[k];
                vm[k] = fmaxf(vm[k], vv[k]);
                th[k] = loop_step(th[k], mm[k], vm[k], rbc2, eps, step_size);
            }
            theta[t] = th; m1[t] = mm; v2[t] = vv; vmax[t] = vm;
        }
    }
    // softmax(best)
    __syncthreads();
    for (long t = tid; t < nq; t += 1024) {
        const f32x4 th = best[t];
        const float mx = fmaxf(fmaxf(th[0], th[1]), fmaxf(th[2], th[3]));
        f32x4 e = {expf(th[0] - mx), expf(th[1] - mx), expf(th[2] - mx), expf(th[3] - mx)};
        const float den = (e[0] + e[1]) + (e[2] + e[3]);
        *(f32x4*)&out_w[t * KW] = e / den;
    }
    if (tid == 0 && out_iters) out_iters[0] = it;
}

// block b runs the loop of segment list.id[b] in that segment's own workspace; LDS or the global exchange buffer as the segment
// would get alone
__global__ __launch_bounds__(1024) void adam_kernel(const SmoothSegs sg, const SegList list, int dim, float scale, int max_iter,
                                                       float* __restrict__ ws, float* __restrict__ out_w, int* __restrict__ out_iters) {
    const int s = list.id[blockIdx.x];
    const long o = sg.off[s], nq = sg.off[s + 1] - o;
    float* gram = seg_ws(ws, sg, s);
    float* state = gram + (size_t)GE * nq;
    adam_body(nq, dim, scale, max_iter, gram, state, state + (size_t)6 * 4 * nq, nq <= adam_lds_rows(KW), out_w + o * KW,
              out_iters ? out_iters + s : out_iters);
}

// Same loop with everything a thread needs for its (up to FPT) frames in registers: the 36-entry Gram of
// each frame pair, theta, Adam moments, amsgrad maximum and the best iterate.  Only the softmax weights and
// the gradient contribution of the left neighbour travel through LDS; an iteration costs three barriers and
// no global memory traffic (the global-state variant streams ~150 KB of Gram data per iteration through one CU).
template <int FPT>
__device__ __forceinline__ void adam_reg_body(long nq, int dim, float scale, int max_iter,
                                              const float* __restrict__ gram, float* __restrict__ out_w,
                                              int* __restrict__ out_iters) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ double red[2][8];      // by iteration parity: a fast wave may write its next sum while a slow one still reads
    float* xw = sm;                       // [nq][4]
    float* xg = sm + nq * KW;             // [nq][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double S = (double)scale / ((double)dim * (double)(nq - 1));
    const float twoS = (float)(2.0 * S);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float g[FPT][GE];
    f32x4 th[FPT], mm[FPT], vv[FPT], vm[FPT], best[FPT], gs[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
        const long t = tid + 512L * f;
        th[f] = mm[f] = vv[f] = vm[f] = best[f] = gs[f] = zero;
#pragma unroll
        for (int e = 0; e < GE; ++e) g[f][e] = (t < nq - 1) ? gram[(long)e * nq + t] : 0.f;
    }
    double min_loss = 20000.0, conv_min = 20000.0;
    int since = 0, it = 0;
    const float b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
    double pb1 = 1.0, pb2 = 1.0;
    const bool forced = max_iter < 0;            // measurement mode: exactly |max_iter| iterations, stopping rules off
    const int cap = forced ? -max_iter : max_iter;
    for (it = 0; it < cap; ++it) {
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            const long t = tid + 512L * f;
            if (t < nq) {
                const float mx = fmaxf(fmaxf(th[f][0], th[f][1]), fmaxf(th[f][2], th[f][3]));
                *(f32x4*)&xw[t * KW] = loop_softmax4(th[f], mx);
            }
        }
        __syncthreads();
        double lsum = 0.0;
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            const long t = tid + 512L * f;
            if (t < nq - 1) {
                const f32x4 w1 = *(const f32x4*)&xw[(t + 1) * KW], w0 = *(const f32x4*)&xw[t * KW];
                const float c[8] = {w1[0], w1[1], w1[2], w1[3], -w0[0], -w0[1], -w0[2], -w0[3]};
                // c[j] - c[i] once per pair: (c[i] - c[j]) is its exact negation (a free source modifier), the sums keep their order
                float dd[GE], y[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = i + 1; j < 8; ++j) dd[tri_r<8>(i, j)] = c[j] - c[i];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j != i) s = fmaf(g[f][tri_r<8>(i, j)], j > i ? dd[tri_r<8>(i, j)] : -dd[tri_r<8>(i, j)], s);
                    y[i] = s;
                }
                float qf = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) qf += c[i] * y[i];
                lsum += (double)qf;
                *(f32x4*)&xg[(t + 1) * KW] = (f32x4){twoS * y[0], twoS * y[1], twoS * y[2], twoS * y[3]};
                gs[f] = (f32x4){-twoS * y[4], -twoS * y[5], -twoS * y[6], -twoS * y[7]};
            }
            __builtin_amdgcn_sched_barrier(0);      // one frame at a time: keeps the matvec temporaries of different frames from coexisting
        }
        // Two barriers per iteration (round 3; four before): the wave sums are DPP folds instead of twelve ds_bpermute round
        // trips, every thread adds the eight wave sums itself (same order everywhere: the loss is uniform) instead of waiting
        // for thread 0, and the barrier that closed the iteration is gone — xw[t] / xg[t + 1] are only rewritten behind the
        // NEXT iteration's first barrier, which their last readers (this iteration's update phase) have to pass first.
        lsum = wave_sum_d_dpp(lsum);
        if (lane == 0) red[it & 1][wave] = lsum;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) tot += red[it & 1][i];
        const float loss = (float)(S * tot);
        if (it % 100 == 1) {
            if (!forced && fabs(min_loss - conv_min) < 1e-5) break;
            conv_min = min_loss;
        }
        const bool improved = loss < (float)min_loss;
        if (improved) { min_loss = (double)loss; since = 0; } else ++since;
        if (!forced && since >= 1000) break;
        pb1 *= 0.9; pb2 *= 0.999;
        const float step_size = adam_step_size(pb1), rbc2 = adam_rbc2(pb2);
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            const long t = tid + 512L * f;
            if (t < nq) {
                const f32x4 w = *(const f32x4*)&xw[t * KW];
                f32x4 gg = zero;
                if (t >= 1) gg = *(const f32x4*)&xg[t * KW];
                if (t < nq - 1) gg += gs[f];
                const float dotwg = (w[0] * gg[0] + w[1] * gg[1]) + (w[2] * gg[2] + w[3] * gg[3]);
                const f32x4 gt = w * (gg - dotwg);
                if (improved) best[f] = th[f];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    mm[f][k] = mm[f][k] + (gt[k] - mm[f][k]) * omb1;
                    vv[f][k] = vv[f][k] * b2 + (omb2 * gt[k]) * gt[k];
                    vm[f][k] = fmaxf(vm[f][k], vv[f][k]);
                    th[f][k] = loop_step(th[f][k], mm[f][k], vm[f][k], rbc2, eps, step_size);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int f = 0; f < FPT; ++f) {
        const long t = tid + 512L * f;
        if (t < nq) {
            const f32x4 b = best[f];
            const float mx = fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3]));
            f32x4 e = {expf(b[0] - mx), expf(b[1] - mx), expf(b[2] - mx), expf(b[3] - mx)};
            const float den = (e[0] + e[1]) + (e[2] + e[3]);
            *(f32x4*)&out_w[t * KW] = e / den;
        }
    }
    if (tid == 0 && out_iters) out_iters[0] = it;
}

template <int FPT>
__global__ __launch_bounds__(512) void adam_reg_kernel(const SmoothSegs sg, const SegList list, int dim, float scale, int max_iter,
                                                          float* __restrict__ ws, float* __restrict__ out_w, int* __restrict__ out_iters) {
    const int s = list.id[blockIdx.x];
    const long o = sg.off[s];
    adam_reg_body<FPT>(sg.off[s + 1] - o, dim, scale, max_iter, seg_ws(ws, sg, s), out_w + o * KW, out_iters ? out_iters + s : out_iters);
}

// The loop for K neighbours per frame: adam_body with its state in the workspace as [K][rows] planes (thread t touches element t of
// each plane: coalesced, and conflict-free where the exchange planes sit in LDS).  K = 1 runs the loop like any other K.
template <int K>
__device__ __forceinline__ void adam_k_body(long nq, int dim, float scale, int max_iter,
                                            const float* __restrict__ gram, float* __restrict__ state,
                                            float* __restrict__ xch_global, int use_lds,
                                            float* __restrict__ out_w, int* __restrict__ out_iters) {
    constexpr int R = 2 * K;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ double red[2][16];
    float* xw = use_lds ? sm : xch_global;                 // [K][nq] softmax weights
    float* xg = xw + nq * K;                               // [K][nq] gradient w.r.t. w from the pair (t-1, t)
    float* theta = state;                                  // [K][nq] each
    float* m1 = theta + nq * K; float* v2 = m1 + nq * K; float* vmax = v2 + nq * K; float* best = vmax + nq * K;
    float* gs = best + nq * K;                             // gradient w.r.t. w[t,:] from the pair (t, t+1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double S = (double)scale / ((double)dim * (double)(nq - 1));
    const float twoS = (float)(2.0 * S);
    for (long t = tid; t < nq; t += 1024) {
#pragma unroll
        for (int k = 0; k < K; ++k) { const long a = k * nq + t; theta[a] = 0.f; m1[a] = 0.f; v2[a] = 0.f; vmax[a] = 0.f; best[a] = 0.f; }
    }
    __syncthreads();

    double min_loss = 20000.0, conv_min = 20000.0;
    int since = 0, it = 0;
    const float b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
    double pb1 = 1.0, pb2 = 1.0;
    const bool forced = max_iter < 0;            // measurement mode: exactly |max_iter| iterations, stopping rules off
    const int cap = forced ? -max_iter : max_iter;
    for (it = 0; it < cap; ++it) {
        // ---- phase 1: softmax weights ---------------------------------------------------------
        for (long t = tid; t < nq; t += 1024) {
#pragma clang fp contract(off)
            float e[K], mx = theta[t];
#pragma unroll
            for (int k = 1; k < K; ++k) mx = fmaxf(mx, theta[k * nq + t]);
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = __builtin_amdgcn_exp2f((theta[k * nq + t] - mx) * 1.44269504088896341f);
            const float rden = __builtin_amdgcn_rcpf(tree_sum<K>(e));      // den >= 1: the maximum contributes exp2(0)
#pragma unroll
            for (int k = 0; k < K; ++k) xw[k * nq + t] = e[k] * rden;
        }
        __syncthreads();
        // ---- phase 2: per pair quadratic forms, gradient w.r.t. the weights ---------------------
        double lsum = 0.0;
        for (long t = tid; t < nq - 1; t += 1024) {
            float c[R], y[R];
#pragma unroll
            for (int k = 0; k < K; ++k) { c[k] = xw[k * nq + t + 1]; c[K + k] = -xw[k * nq + t]; }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < R; ++j) if (j != i) s += gram[(long)tri_r<R>(i, j) * nq + t] * (c[j] - c[i]);
                y[i] = s;
            }
            float qf = 0.f;
#pragma unroll
            for (int i = 0; i < R; ++i) qf += c[i] * y[i];
            lsum += (double)qf;
#pragma unroll
            for (int k = 0; k < K; ++k) { xg[k * nq + t + 1] = twoS * y[k]; gs[k * nq + t] = -twoS * y[K + k]; }
        }
        lsum = wave_sum_d_dpp(lsum);
        if (lane == 0) red[it & 1][wave] = lsum;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) tot += red[it & 1][i];
        const float loss = (float)(S * tot);
        // ---- phase 3: the reference's loop control (uniform across the block) -------------------
        if (it % 100 == 1) {
            if (!forced && fabs(min_loss - conv_min) < 1e-5) break;
            conv_min = min_loss;
        }
        const bool improved = loss < (float)min_loss;
        if (improved) { min_loss = (double)loss; since = 0; } else ++since;
        if (!forced && since >= 1000) break;
        // ---- phase 4: gradient through softmax + Adam(amsgrad) ----------------------------------
        pb1 *= 0.9; pb2 *= 0.999;
        const float step_size = adam_step_size(pb1), rbc2 = adam_rbc2(pb2);
        for (long t = tid; t < nq; t += 1024) {
            float w[K], g[K], wg[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                w[k] = xw[k * nq + t];
                float gk = 0.f;
                if (t >= 1) gk = xg[k * nq + t];
                if (t < nq - 1) gk += gs[k * nq + t];
                g[k] = gk; wg[k] = w[k] * gk;
            }
            const float dotwg = tree_sum<K>(wg);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const long a = k * nq + t;
                const float gt = w[k] * (g[k] - dotwg);
                float th = theta[a];
                if (improved) best[a] = th;
                float mm = m1[a], vv = v2[a], vm = vmax[a];
                mm = mm + (gt - mm) * omb1;
                vv = vv * b2 + (omb2 * gt) * gt;
                vm = fmaxf(vm, vv);
                th = loop_step(th, mm, vm, rbc2, eps, step_size);
                theta[a] = th; m1[a] = mm; v2[a] = vv; vmax[a] = vm;
            }
        }
    }
    // softmax(best): expf and the IEEE divide
    __syncthreads();
    for (long t = tid; t < nq; t += 1024) {
        float e[K], mx = best[t];
#pragma unroll
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, best[k * nq + t]);
#pragma unroll
        for (int k = 0; k < K; ++k) e[k] = expf(best[k * nq + t] - mx);
        const float den = tree_sum<K>(e);
#pragma unroll
        for (int k = 0; k < K; ++k) out_w[t * K + k] = e[k] / den;
    }
    if (tid == 0 && out_iters) out_iters[0] = it;
}

template <int K>
__global__ __launch_bounds__(1024) void adam_k_kernel(const SmoothSegs sg, const SegList list, int dim, float scale, int max_iter,
                                                         float* __restrict__ ws, float* __restrict__ out_w, int* __restrict__ out_iters) {
    const int s = list.id[blockIdx.x];
    const long o = sg.off[s], nq = sg.off[s + 1] - o;
    float* gram = seg_ws(ws, sg, s);
    float* state = gram + (size_t)(K * (2 * K - 1)) * nq;
    adam_k_body<K>(nq, dim, scale, max_iter, gram, state, state + (size_t)6 * K * nq, nq <= adam_lds_rows(K), out_w + o * K,
                   out_iters ? out_iters + s : out_iters);
}

// segments of one row (no adjacent pair): softmax(0) = 1 / k and zero iterations
__global__ void fill_uniform_kernel(const SmoothSegs sg, const SegList list, int k, float* __restrict__ out_w, int* __restrict__ out_iters) {
    const int s = list.id[blockIdx.x];
    if ((int)threadIdx.x < k) out_w[sg.off[s] * k + threadIdx.x] = 1.0f / (float)k;
    if (threadIdx.x == 0 && out_iters) out_iters[s] = 0;
}

// bytes of segment workspace: what the segment needs alone, rounded up to 64
inline size_t seg_ws_bytes(long nq, int k = KW) { return (ws_floats_k(nq, k) * 4 + 64 + 63) & ~(size_t)63; }

}  // namespace

extern "C" size_t knnsvc_smooth_workspace_bytes(int64_t nq) { return nq > 0 ? ws_floats_k(nq, KW) * 4 + 64 : 0; }

// row offsets and workspace placement of a validated table; *bytes: the workspace of the segmented call
static int smooth_segs(const KnSegTable& t, const char* entry, SmoothSegs* sg, size_t* bytes, int k = KW) {
    sg->n = t.n;
    size_t at = 0;
    for (int s = 0; s <= KNNSVC_MAX_SEGMENTS; ++s) {
        sg->off[s] = t.off[s];
        if (s < KNNSVC_MAX_SEGMENTS) sg->ws64[s] = (unsigned)(at / 64);
        if (s < t.n) at += seg_ws_bytes(t.off[s + 1] - t.off[s], k);
    }
    if (at / 64 > 0xFFFFFFFFull) return knnsvc_fail(KNNSVC_EINVAL, "%s: segments too long", entry);
    *bytes = at;
    return KNNSVC_OK;
}

// The argument checks, the class-by-length choice and the launches, once.  `need`: the workspace size the entry point documents
// (knnsvc_smooth_workspace_bytes for the single call, knnsvc_smooth_seg_workspace_bytes[_k] for the segmented ones); `entry`: its
// name, for the messages.  Every check runs before the first HIP call.
// One-row segments are filled with 1 / k, one Gram launch covers the pairs of all segments, then one loop launch per loop variant
// present, each over the list of segments that would get that variant alone.  The k = 4 fast paths (`fast`: k = 4 without
// KNNSVC_MATCH_GENERIC_K=1) are the register loops up to 1536 rows and adam_kernel beyond; everything else runs adam_k_kernel<k>.
static int smooth_weights_launch(const SmoothSegs& sg, size_t need, const char* entry, int k, const int64_t* idx, const float* pool,
                                 int64_t np, int32_t dim, int32_t ld, float scale, const float* row_scale, int32_t max_iter,
                                 float* out_w, int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream) {
    KN_REQUIRE(k >= 1 && k <= 8, "%s: k = %d outside 1..8", entry, k);
    KN_REQUIRE(idx && pool && out_w && workspace, "%s: null pointer", entry);
    KN_REQUIRE(np > 0 && dim > 0 && ld >= dim && max_iter != 0, "%s: bad sizes", entry);
    const bool fast = k == KW && !knnsvc_match_generic_k();
    // the fast paths write rows of float4, adam_k_kernel float by float
    KN_REQUIRE(((uintptr_t)out_w & (fast ? 15 : 3)) == 0, "%s: out_w must be %d-byte aligned", entry, fast ? 16 : 4);
    const size_t gl = (size_t)2 * k * dim * 4;
    KN_REQUIRE(gl <= 150 * 1024, "%s: feature dim %d too large for LDS at k = %d", entry, (int)dim, k);
    if (workspace_bytes < need) return knnsvc_fail(KNNSVC_EWORKSPACE, "%s: workspace %zu < %zu bytes", entry, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
    // the loop variant each segment would get alone: 0 one row (no adjacent pair: the reference's loss is NaN and never improves ->
    // softmax(0), no loop), 1..3 adam_reg_kernel<1|2|3> (fast only), 4 the long loop
    SegList cls[5];
    long longest[5] = {0, 0, 0, 0, 0}, lds_rows = 0;
    for (int c = 0; c < 5; ++c) cls[c].n = 0;
    for (int s = 0; s < sg.n; ++s) {
        const long nq = sg.off[s + 1] - sg.off[s];
        const int c = nq < 2 ? 0 : (!fast || nq > 1536 ? 4 : (nq <= 512 ? 1 : (nq <= 1024 ? 2 : 3)));
        cls[c].id[cls[c].n++] = (unsigned char)s;
        if (nq > longest[c]) longest[c] = nq;
        if (c == 4 && nq <= adam_lds_rows(k) && nq > lds_rows) lds_rows = nq;
    }
    int rc;
    if (cls[0].n) {
        hipLaunchKernelGGL(fill_uniform_kernel, dim3((unsigned)cls[0].n), dim3(64), 0, st, sg, cls[0], k, out_w, out_iters);
        if ((rc = knnsvc_check_launch(entry))) return rc;
    }
    const long pairs = sg.off[sg.n] - sg.n;
    if (pairs == 0) return KNNSVC_OK;
#define KN_GRAM_K(KK)                                                                                                                \
    case KK:                                                                                                                         \
        if ((rc = kn_lds_optin<gram_kernel<KK>>((int)gl, entry))) return rc;                                                         \
        hipLaunchKernelGGL(gram_kernel<KK>, dim3((unsigned)pairs), dim3(256), gl, st, (const long*)idx, sg, pool, (long)np, dim, ld, \
                           row_scale, base);                                                                                         \
        break;
    switch (k) { KN_GRAM_K(1) KN_GRAM_K(2) KN_GRAM_K(3) KN_GRAM_K(4) KN_GRAM_K(5) KN_GRAM_K(6) KN_GRAM_K(7) KN_GRAM_K(8) }
#undef KN_GRAM_K
    if ((rc = knnsvc_check_launch(entry))) return rc;
#define KN_ADAM_SEG(F)                                                                                                               \
    if (cls[F].n) {                                                                                                                  \
        if ((rc = kn_lds_optin<adam_reg_kernel<F>>(65536, entry))) return rc;                                                        \
        hipLaunchKernelGGL(adam_reg_kernel<F>, dim3((unsigned)cls[F].n), dim3(512), (size_t)longest[F] * 2 * KW * 4, st, sg, cls[F], dim, scale, \
                           max_iter, base, out_w, out_iters);                                                                        \
        if ((rc = knnsvc_check_launch(entry))) return rc;                                                                            \
    }
    KN_ADAM_SEG(1) KN_ADAM_SEG(2) KN_ADAM_SEG(3)
#undef KN_ADAM_SEG
    if (!cls[4].n) return KNNSVC_OK;
    const size_t al = (size_t)lds_rows * 2 * k * 4;              // of the segments that exchange through LDS; the others take none
#define KN_ADAM_LONG(KERNEL)                                                                                                         \
    if ((rc = kn_lds_optin<KERNEL>((int)al, entry))) return rc;                                                                      \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)cls[4].n), dim3(1024), al, st, sg, cls[4], dim, scale, max_iter, base, out_w, out_iters);
#define KN_ADAM_K(KK) case KK: KN_ADAM_LONG(adam_k_kernel<KK>) break;
    if (fast) {
        KN_ADAM_LONG(adam_kernel)
    } else {
        switch (k) { KN_ADAM_K(1) KN_ADAM_K(2) KN_ADAM_K(3) KN_ADAM_K(4) KN_ADAM_K(5) KN_ADAM_K(6) KN_ADAM_K(7) KN_ADAM_K(8) }
    }
#undef KN_ADAM_K
#undef KN_ADAM_LONG
    return knnsvc_check_launch(entry);
}

extern "C" int knnsvc_smooth_weights(const int64_t* idx, int64_t nq, const float* pool, int64_t np, int32_t dim,
                                     int32_t ld, float scale, const float* row_scale, int32_t max_iter, float* out_w,
                                     int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream) {
    KnSegTable t; SmoothSegs sg; size_t seg_bytes = 0;
    int rc;
    if ((rc = kn_seg_one(nq, "smooth_weights", &t)) || (rc = smooth_segs(t, "smooth_weights", &sg, &seg_bytes))) return rc;
    // Its own size, not seg_bytes (which rounds up to 64): the one segment starts at the 64-byte-aligned base, at most 63 bytes
    // into the workspace, and ends ws_floats_k(nq, 4) * 4 bytes later.
    return smooth_weights_launch(sg, knnsvc_smooth_workspace_bytes(nq), "smooth_weights", KW, idx, pool, np, dim, ld, scale, row_scale,
                                 max_iter, out_w, out_iters, workspace, workspace_bytes, stream);
}

extern "C" size_t knnsvc_smooth_seg_workspace_bytes(const int64_t* host_seg, int32_t n_seg) {
    KnSegTable t; SmoothSegs sg; size_t bytes = 0;
    if (kn_seg_table(host_seg, n_seg, "smooth_seg_workspace_bytes", &t) || smooth_segs(t, "smooth_seg_workspace_bytes", &sg, &bytes)) return 0;
    return bytes;
}

extern "C" int knnsvc_smooth_weights_seg(const int64_t* idx, const int64_t* host_seg, int32_t n_seg, const float* pool, int64_t np,
                                         int32_t dim, int32_t ld, float scale, const float* row_scale, int32_t max_iter, float* out_w,
                                         int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream) {
    KnSegTable t; SmoothSegs sg; size_t need = 0;
    int rc;
    if ((rc = kn_seg_table(host_seg, n_seg, "smooth_weights_seg", &t)) || (rc = smooth_segs(t, "smooth_weights_seg", &sg, &need))) return rc;
    return smooth_weights_launch(sg, need, "smooth_weights_seg", KW, idx, pool, np, dim, ld, scale, row_scale, max_iter, out_w, out_iters,
                                 workspace, workspace_bytes, stream);
}

// ---- the segmented calls for k neighbours per frame (1 <= k <= 8); the ones above are k = 4 ------------------------------------
extern "C" size_t knnsvc_smooth_seg_workspace_bytes_k(const int64_t* host_seg, int32_t n_seg, int32_t k) {
    KnSegTable t; SmoothSegs sg; size_t bytes = 0;
    if (k < 1 || k > 8) { knnsvc_fail(KNNSVC_EINVAL, "smooth_seg_workspace_bytes_k: k = %d outside 1..8", (int)k); return 0; }
    if (kn_seg_table(host_seg, n_seg, "smooth_seg_workspace_bytes_k", &t) || smooth_segs(t, "smooth_seg_workspace_bytes_k", &sg, &bytes, k))
        return 0;
    return bytes;
}

extern "C" int knnsvc_smooth_weights_seg_k(const int64_t* idx, int32_t k, const int64_t* host_seg, int32_t n_seg, const float* pool,
                                           int64_t np, int32_t dim, int32_t ld, float scale, const float* row_scale, int32_t max_iter,
                                           float* out_w, int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream) {
    KnSegTable t; SmoothSegs sg; size_t need = 0;
    int rc;
    if ((rc = kn_seg_table(host_seg, n_seg, "smooth_weights_seg_k", &t))) return rc;
    KN_REQUIRE(k >= 1 && k <= 8, "smooth_weights_seg_k: k = %d outside 1..8", (int)k);
    if ((rc = smooth_segs(t, "smooth_weights_seg_k", &sg, &need, k))) return rc;
    return smooth_weights_launch(sg, need, "smooth_weights_seg_k", k, idx, pool, np, dim, ld, scale, row_scale, max_iter, out_w, out_iters,
                                 workspace, workspace_bytes, stream);
}
