/*
 * libknnsvc_hip.so — C ABI of the MI355X (gfx950) kNN-SVC inference kernels.
 *
 * The reference (SmoothKen/knn-svc) has no FFI: its seams are Python callables
 * executed by PyTorch ATen.  Each entry point below replaces one of those
 * callables; the comment above it cites the reference file:line.  A maintainer
 * binds them with ctypes (see INTEGRATION.md for the stubs).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named host_*;
 *   - activations are channel-last: a [T, C] matrix with row stride `ld*` (floats);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); nothing synchronises, nothing allocates — callers own every buffer and
 *     workspace, so each call is hipGraph-capturable;
 *   - return value: 0 on success, a KNNSVC_E* code otherwise; knnsvc_last_error()
 *     gives the thread-local message.
 */
#ifndef KNNSVC_HIP_H
#define KNNSVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNNSVC_OK        0
#define KNNSVC_EINVAL    1   /* bad shape / alignment / argument          */
#define KNNSVC_EWORKSPACE 2  /* workspace too small                        */
#define KNNSVC_EHIP      3   /* a HIP runtime call failed                  */
#define KNNSVC_ENAN      4   /* NaN distance (the reference sys.exit()s)   */

#define KNNSVC_ABI_VERSION 21

int knnsvc_abi_version(void);
const char* knnsvc_last_error(void);
/* Short tag of the kernel the calling thread's last knnsvc_conv_gemm dispatched to ("F128a2", "W64", "G128v8", ...):
 * measurement hook (bench.py attributes HIP-event times to kernels with it); "" before the first call. */
const char* knnsvc_conv_gemm_last_kernel(void);
/* ... and which epilogue that launch took: "patch" (LDS patches, 16-byte stores: conv_epilogue_wide32), "lane" (column per lane) or
 * "" (kernels with an epilogue of their own: the 256x256-tile kernel, fp32, bf16x3); after a grid of several
 * descriptors (knnsvc_conv_gemm_multi): the first descriptor's.  Test hook. */
const char* knnsvc_conv_gemm_last_epilogue(void);
/* The dispatchers' A/B switches (KNNSVC_QUAD, KNNSVC_QUAD_EPI, KNNSVC_EPILOGUE, KNNSVC_WIN, KNNSVC_WIN_SMALL, KNNSVC_WIN_DEEP,
 * KNNSVC_WIN160, KNNSVC_WIN_WIDE, KNNSVC_GEMM_SMALL of knnsvc_conv_gemm, KNNSVC_ATTENTION of knnsvc_wavlm_attention, KNNSVC_CONV0_RP and
 * KNNSVC_CONV0_SUBS of knnsvc_wavlm_conv0) are read from the environment once, by the first call that looks at one of them; this
 * re-reads them all (tests and A/B runs that switch a route inside one process). */
int knnsvc_reload_knobs(void);
/* Stream-placement probe: `blocks` one-wave workgroups that spin for `spin` shader-clock ticks each (nothing is read or written).
 * The host side (knn_svc_amd/pipeline.py) times it on two streams at once to MEASURE whether they share a hardware queue or
 * dispatch pipe, instead of trusting the stream -> queue mapping. */
int knnsvc_probe_dispatch(int32_t blocks, int32_t spin, void* stream);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces F.conv1d / F.conv_transpose1d / F.linear as used by
 *   wavlm/WavLM.py:401,514-527 (feature extractor, pos_conv), wavlm/WavLM.py:347-348, 671-672,
 *   wavlm/modules.py:540-563 (q/k/v/out projections),
 *   hifigan/ddsp_models.py:113-168,176-233 (every conv of the Generator), :416 (sin_prenet).
 *
 *   out[b,g][m, n] = epilogue( sum_{tap,c} A(m,tap,c) * W[g][n][tap*cin + c] )
 *   A(m,tap,c)     = lrelu_{a_slope}( X[b,g][m*stride + tap*dil - pad][c] )   (0 outside [0,t_in))
 *   epilogue(v)    = ((act(v + bias[n % bias_period]) + resid[m,n]) + (accumulate ? out[m,n] : 0)) / div
 * With convt_u > 0 the output element (m, n) is scattered to row m*convt_u + n/convt_cout - convt_pad,
 * column n % convt_cout (rows outside [0,t_out) dropped): a stride-u transposed convolution whose
 * kernel is taps*u wide, written as one GEMM over K = taps*cin, N = u*cout.
 * X rows are ldx floats apart; ldx >= cin, except that taps == 1 also accepts overlapping rows (ldx < cin):
 * the framed view of a signal, row t = x[t*ldx .. t*ldx + cin) — how the 400-point STFT (hop 320) is a GEMM.
 * ------------------------------------------------------------------------------------------ */
enum { KNNSVC_ACT_NONE = 0, KNNSVC_ACT_GELU = 1, KNNSVC_ACT_LRELU = 2, KNNSVC_ACT_TANH = 3 };

typedef struct knnsvc_conv_desc {
    const float* x;  int64_t x_bstride; int64_t x_gstride; int32_t ldx; int32_t t_in;
    int32_t cin; int32_t taps; int32_t stride; int32_t dil; int32_t pad;
    float a_slope;                     /* 1.0f = no prologue activation                   */
    const float* w;  int64_t w_gstride; int32_t n;
    const float* bias; int64_t bias_gstride; int32_t bias_period;   /* bias may be NULL  */
    float* out; int64_t o_bstride; int64_t o_gstride; int32_t ldo; int32_t m;
    int32_t act; float act_slope;
    const float* resid; int64_t r_bstride; int64_t r_gstride; int32_t ldr;   /* may be NULL */
    int32_t accumulate; float div;     /* div == 1.0f = off                               */
    int32_t batches; int32_t groups;
    int32_t convt_u; int32_t convt_cout; int32_t convt_pad; int32_t t_out;
    const void* w_bf16x3;              /* optional: w pre-split by knnsvc_split_weight_bf16x3 (NULL = fp32 MFMA) */
    const void* w_f16x2;               /* optional: w pre-split by knnsvc_split_weight_f16x2; wins over w_bf16x3 */
    float w_f16x2_scale;               /* the power-of-two scale w_f16x2 was split with                         */
    float a_f16x2_scale;               /* power-of-two activation pre-scale of the f16x2 path; 0 = default 16    */
    int32_t x_f16x2;                   /* 1: x already is in the f16x2 split layout (see below), split with            */
                                       /*    a_f16x2_scale (0 = 16) or with the scale x_absmax implies               */
    int32_t out_f16x2;                 /* 1: write out in the f16x2 split layout (scale 16) for the next GEMM;      */
                                       /* c >= 32 (multiple of 32): only columns >= c are split (QKV: K,V blocks)   */
    /* Range of the f16x2 path without host round trips (all optional, NULL / 0 = off; ignored by the fp32 / bf16x3 paths):
     * A RANGE SLOT is 2048 DEVICE floats (8 KiB) used as 64 stripes of one 128-byte cache line each (float 32 i is stripe i):
     * a producer block folds max|.| into stripe (block id % 64) with one atomicMax — atomics that meet on a cache line
     * serialise, and a launch's first round of blocks all find the slot empty — and consumers use the maximum of the 64.
     * Its content is a pure function of the data (max is order-independent).
     *   x_absmax / w_absmax: range slots holding an upper bound of |x| over the A operand / of |w| over the split
     *     weights; the kernel then derives the operand's power-of-two scale itself — the largest s with bound * s < 2^15
     *     (knnsvc_split_f16x2_dyn splits with the same rule, so a pre-split operand and its consumer agree by sharing a
     *     slot) — instead of a_f16x2_scale / w_f16x2_scale.  No activation range can overflow fp16 this way, and tiny
     *     tensors are lifted into the range instead of losing bits.
     *   out_absmax: range slot; the epilogue folds max|out| over everything this launch stores into it with atomicMax
     *     (on the bit pattern: a NaN output makes the slot NaN).  The caller zeroes the slot; it is the next launch's
     *     x_absmax.
     *   out_f16x2_scale: scale of the split layout written under out_f16x2 (0 = 16); the consumer passes the same value
     *     as its a_f16x2_scale.
     *   x_bound_mul / x_bound_add (0 / 0 = 1 / 0): the A operand's bound is x_bound_mul * max(x_absmax) + x_bound_add — for an
     *     input that was not measured itself but whose bound follows from ITS producer's measured input and weights
     *     (|conv(x)| <= max_n sum_k |w[n,k]| * max|x| + max|b|; activations that do not grow their argument change nothing):
     *     publishing costs short-lived blocks ~1 us each, so only every other tensor of a conv chain is measured. */
    const float* x_absmax; const float* w_absmax; float* out_absmax; float out_f16x2_scale;
    /* Dynamic length (optional; NULL = off): n_dyn is a DEVICE int32 holding a count n (frames); the kernel then uses
     *   t_in = n * dyn_t_in_mul + dyn_t_in_add,  m = n * dyn_m_mul + dyn_m_add,  t_out = n * dyn_t_out_mul (transposed mode)
     * instead of the fields above, which become the MAXIMA the launch is sized for (grid, 31-bit offsets).  Input rows
     * >= t_in read as zero (the convolution's own zero padding at the sequence end), output rows >= m are not written.
     * One launch — one captured hipGraph — thus serves every sequence length up to its bucket with the results of an
     * exact-length launch: the generator's frame-count buckets (hifigan/ddsp_models.py:176-233 is fully convolutional). */
    const int32_t* n_dyn; int32_t dyn_t_in_mul; int32_t dyn_t_in_add; int32_t dyn_m_mul; int32_t dyn_m_add; int32_t dyn_t_out_mul;
    float x_bound_mul; float x_bound_add;
    /* 2: always the 256x256-tile kernel (Gemm2QuadS; needs x_f16x2, n % 4 == 0, 16-byte rows) — what the kNN's dot-matrix
     * route sets, so that it sums over K exactly as the fused screen kernel does.
     * 1: always the 128x128-tile kernel, whatever the launch size.  The default picks the 256x256-tile kernel for large
     * launches; the two sum over K in different groupings, so a row's result would depend (in the last bit) on how many other
     * rows and columns the launch has.  The distance GEMM of the kNN sets this: a pool shard of any size gives the distances the
     * whole pool gives (device-count invariance of the sharded search, lib_ongaku_test.py:148-175 is one formula). */
    int32_t fixed_tile;
} knnsvc_conv_desc;

int knnsvc_conv_gemm(const knnsvc_conv_desc* d, void* stream);

/* `count` (1..4) convolutions of the same output shape [m, n] in ONE launch (hifigan/ddsp_models.py:206-227: the three
 * ResBlock branches of a generator stage — kernel sizes 3 / 7 / 11 — only share their input; the reference runs them one
 * after the other and averages).  When every descriptor takes the windowed kernel (stride 1, >= 3 taps, fp32 input, split
 * weights, (taps - 1) * dil <= 64, batches = groups = 1) the descriptors become the y dimension of one grid: the branches
 * fill the chip together without streams of their own.  Otherwise: one knnsvc_conv_gemm per descriptor, in order.  Results
 * are bit-identical to separate launches either way.  Put the descriptor with the most taps first. */
int knnsvc_conv_gemm_multi(const knnsvc_conv_desc* descs, int32_t count, void* stream);

/* What the dispatcher decides for `count` (1..4) descriptors, without a launch: host code only, no GPU and no stream; the operand
 * pointers are looked at (null, alignment) but never followed.  count == 1: the tag knnsvc_conv_gemm_last_kernel() reports after
 * knnsvc_conv_gemm of the descriptor, and the epilogue tag; both "" for m == 0 (nothing is launched).  count > 1: the tag of the
 * one grid knnsvc_conv_gemm_multi launches ("W128Dx", ...) and the first descriptor's epilogue, or "" where it launches the
 * descriptors one by one.  `tag` and `epilogue` hold `cap` >= 16 bytes each.  Returns what the launch entry returns for a
 * descriptor that does not validate. */
int knnsvc_conv_gemm_route(const knnsvc_conv_desc* descs, int32_t count, char* tag, char* epilogue, int32_t cap);
/* Every tag the dispatcher can report, separated by blanks, into `out` (`cap` bytes; 256 are enough). */
int knnsvc_conv_gemm_tags(char* out, int32_t cap);

/* One ResBlock1 iteration of the generator in one launch (hifigan/ddsp_models.py:13-44):
 *     t1 = lrelu(conv1d(lrelu(x), w1, dilation = dil) + b1);   out = conv1d(t1, w2) + b2 + x
 * x, out: channel-last [t, channels] fp32 (row pitches ldx / ldo), both convolutions `taps` wide with "same" zero padding; the
 * inner activation t1 lives only in LDS.  Weights as for knnsvc_conv_gemm: packed [channels, taps * channels] and pre-split
 * (knnsvc_split_weight_f16x2) with their power-of-two scales.  Activation scales as in "Range": x_absmax is x's range slot
 * (t1 is bounded by t1_bound_mul * max|x| + t1_bound_add, as knnsvc_conv_desc.x_bound_*), or fixed a1_scale / a2_scale.
 * out_absmax (optional): max |out| is folded into that slot.  n_dyn (optional): the valid length is n_dyn[0] * dyn_mul <= t.
 * Results are bit-identical to the two knnsvc_conv_gemm launches.  channels = 32 or 64. */
typedef struct knnsvc_pair_desc {
    const float* x; int32_t ldx; int32_t t; int32_t channels; int32_t taps; int32_t dil;
    const void* w1_f16x2; float w1_scale; const float* b1;
    const void* w2_f16x2; float w2_scale; const float* b2;
    float* out; int32_t ldo;
    float slope;
    const float* x_absmax; float t1_bound_mul; float t1_bound_add; float a1_scale; float a2_scale;
    float* out_absmax;
    const int32_t* n_dyn; int32_t dyn_mul;
} knnsvc_pair_desc;
int knnsvc_resblock_pair(const knnsvc_pair_desc* d, void* stream);
/* The pairs of `count` (1..4) ResBlock branches (same channels and length, any odd taps) in one launch: see knnsvc_conv_gemm_multi. */
int knnsvc_resblock_pair_multi(const knnsvc_pair_desc* descs, int32_t count, void* stream);

/* out = alpha * x (accumulate = 0) or out + alpha * x (accumulate = 1) over n floats (n % 4 == 0): one term of the layer
 * weighting `(feats * w[:, None]).sum(0)` over WavLM's layer outputs (ddsp_prematch_dataset.py:349-350) when w is not one-hot
 * (terms are added in ascending layer order, each product rounded on its own, as torch evaluates it). */
int knnsvc_axpy(const float* x, int64_t n, float alpha, int32_t accumulate, float* out, void* stream);

/* out = (c + (b + a)) / div, elementwise over n floats (n % 4 == 0), max |out| folded into the range slot out_absmax (may be
 * NULL): the mean of the parallel ResBlock branches of a generator stage (hifigan/ddsp_models.py:218-227).  n_dyn (optional,
 * device int32): only the first n_dyn * dyn_mul floats are touched (bucketed sequence lengths, see "Dynamic length"). */
int knnsvc_mean3(const float* a, const float* b, const float* c, int64_t n, float div, float* out, float* out_absmax,
                 const int32_t* n_dyn, int64_t dyn_mul, void* stream);

/* Split fp32 weights [rows, K] (K % 32 == 0) into three truncated bf16 planes, layout [rows][K/32][3][32]
 * (6 bytes per weight).  With w_bf16x3 set and cin % 32 == 0, knnsvc_conv_gemm evaluates every fp32
 * product as six bf16 MFMAs (a0b0+a0b1+a1b0+a0b2+a2b0+a1b1, fp32 accumulate): fp32-level accuracy at
 * 6/16 of the fp32-MFMA cost.  Activations are split on the fly inside the kernel. */
int knnsvc_split_weight_bf16x3(const float* w, int64_t rows, int32_t K, void* out, void* stream);

/* Split scale*w (scale = a power of two that puts max|w| in [2^13, 2^14)) into two round-to-nearest fp16
 * planes, layout [rows][K/32][2][32] (4 bytes per weight).  With w_f16x2 set and cin % 32 == 0,
 * knnsvc_conv_gemm evaluates every fp32 product as three fp16 MFMAs (lo*hi + hi*lo + hi*hi, fp32
 * accumulate; activations are scaled by 16 and split on the fly, the epilogue undoes both scales exactly):
 * fp32-GEMM accuracy at 3/16 of the fp32-MFMA cost.  a_f16x2_scale * |activation| must stay below 65504
 * (default scale 16: |x| < 4094) or the output turns NaN (never silently wrong); activations whose rms is
 * below ~0.2 / a_f16x2_scale lose relative accuracy (absolute floor 3e-8 / a_f16x2_scale per element). */
int knnsvc_split_weight_f16x2(const float* w, int64_t rows, int32_t K, float scale, void* out, void* stream);

/* The same split with the scale taken from a range slot (8 KiB, see knnsvc_conv_desc): scale = the largest power of two with max(slot) * scale < 2^15
 * (what knnsvc_conv_gemm derives from x_absmax / w_absmax).  For operands whose range is only known on the device — the
 * kNN's query and pool features (lib_ongaku_test.py:148-175 takes whatever WavLM produced). */
int knnsvc_split_f16x2_dyn(const float* w, int64_t rows, int32_t K, const float* absmax, void* out, void* stream);

/* Folds max |x[r, c]| over a [rows, cols] matrix with row pitch ld into the range slot (8 KiB; atomicMax on the bit
 * pattern, NaN wins); the caller zeroes the slot.  Feeds x_absmax / w_absmax for tensors that no GEMM epilogue produced. */
int knnsvc_absmax(const float* x, int64_t rows, int32_t cols, int32_t ld, float* slot, void* stream);

/* Activations in the f16x2 split layout ("A2"): a [rows, C] matrix (C % 32 == 0, row pitch ld floats, ld % 32 == 0)
 * occupies the same bytes as fp32, but every group of 32 channels is stored as 32 fp16 `hi` values followed by
 * 32 fp16 `lo` values with 16*x = hi + lo (round to nearest twice): element (r, c) -> byte r*ld*4 + (c/32)*128 +
 * plane*64 + (c%32)*2.  Producers that feed ONLY GEMMs write it (out_f16x2 here, the split flags of
 * knnsvc_layernorm / knnsvc_wavlm_conv0 / knnsvc_wavlm_attention), consumers set x_f16x2: the GEMM then stages A with
 * plain copies instead of splitting it once per column tile. */

/* ------------------------------------------------------------------------------------------
 * Row-wise layer norm over the last dim (eps 1e-5, affine), optional exact-erf GELU after it.
 * Replaces F.layer_norm at wavlm/WavLM.py:342, 415 (+nn.GELU :418), 692, 706.  In place allowed.
 * ------------------------------------------------------------------------------------------ */
/* flags: bit 0 = GELU after the norm, bit 1 = write the f16x2 split layout (dim % 32 == 0, ldo % 32 == 0). */
int knnsvc_layernorm(const float* x, int64_t rows, int32_t dim, int32_t ldx, const float* gamma,
                     const float* beta, int32_t flags, float* out, int32_t ldo, void* stream);

/* Layer 0 of the conv feature extractor fused: Conv1d(1->C, k, stride, no bias) -> LayerNorm(C) -> GELU
 * (wavlm/WavLM.py:401-419 with in_d = 1).  x [batches, L] -> out [batches * T, C], T = (L-k)/stride + 1,
 * w [C, k].  C in {64,128,256,512}, k <= 16, stride <= 8. */
int knnsvc_wavlm_conv0(const float* x, int32_t batches, int64_t L, const float* w, int32_t channels, int32_t k,
                       int32_t stride, const float* gamma, const float* beta, float* out, int32_t out_f16x2,
                       void* stream);
/* The launch shape knnsvc_wavlm_conv0 takes for `batches` inputs of T output frames each, without a launch (host code only):
 * rows per pass (KNNSVC_CONV0_RP: 2, 4 or 1) and the spans of 64 rows a workgroup walks (KNNSVC_CONV0_SUBS on long inputs, else 1). */
int knnsvc_wavlm_conv0_route(int32_t batches, int64_t T, int32_t* rows_per_pass, int32_t* spans);
/* ... and what the calling thread's last knnsvc_wavlm_conv0 launched with (0, 0 before the first launch).  Test hook. */
void knnsvc_wavlm_conv0_last_route(int32_t* rows_per_pass, int32_t* spans);

/* Gated relative-position multiplier, wavlm/modules.py:523-533:
 *   gate[row, h] = ga*(gb*grep_a[h] - 1) + 2, (ga, gb) = sigmoid(W2 @ xn[row, h*hd:(h+1)*hd] + b2)
 * where W2 [2, hd] / b2 [2] are grep_linear's weight rows / bias summed in groups of four. */
int knnsvc_wavlm_gate(const float* xn, int64_t rows, int32_t heads, int32_t head_dim, int32_t ldx,
                      const float* w2, const float* b2, const float* grep_a, float* gate, int32_t x_f16x2,
                      void* stream);

/* Fused bidirectional self-attention with the gated bucketed relative-position bias
 * (wavlm/modules.py:504-506, 533-563 -> F.multi_head_attention_forward, need_weights=False):
 *   O[b, i, h, :] = softmax_j( q_i.k_j * head_dim^-0.5 + gate[b,i,h] * table[h][j - i + T - 1] ) @ V
 * qkv is [batches*T, 3*E] (q | k | v column blocks, E = heads*64), table is [heads][2T-1]
 * (bucket LUT already applied), gate [batches*T, heads], out [batches*T, E].  head_dim must be 64.
 * Nothing of size T x T is ever written to HBM. */
/* kv_f16x2: the K and V column blocks of `qkv` (columns E..3E) already hold the f16x2 split layout, written by the QKV
 * projection with knnsvc_conv_desc.out_f16x2 = E (split from column E on); Q stays fp32.  f16x2 kernel only.
 * out_f16x2 is a flag word: bit 0 = write the output in the split layout; bit 2 (value 4) = wide range: Q, K or V may
 * exceed what the f16x2 kernel's fixed operand scales hold (|k|, |v| < 4094, |q| < ~20000 — the caller decides this
 * once, from bounds implied by the weights), so the bf16x3 kernel (fp32 exponent range) runs instead; fp32 in and out. */
/* kv_len (may be NULL): DEVICE int32 [batches] — batch row b attends to its first kv_len[b] keys only (clamped to 1..T):
 * WavLM's key_padding_mask for a chunk that sits zero-padded inside a longer, bucketed sequence (wavlm/WavLM.py:311-321;
 * F.multi_head_attention_forward masks padded keys with -inf).  The table stays indexed with the bucket's T.  Read on the
 * device at launch time, so one captured hipGraph serves every length of its bucket.  Query rows >= kv_len[b] still get
 * (finite, unused) outputs.  A batch row with ONE visible key (T = 1, kv_len[b] <= 1) gets that key's V row itself, bit for bit,
 * from every kernel (with kv_f16x2: what its split holds). */
int knnsvc_wavlm_attention(const float* qkv, const float* gate, const float* table, int32_t batches,
                           int32_t T, int32_t heads, float* out, int32_t out_f16x2, int32_t kv_f16x2, const int32_t* kv_len,
                           void* stream);
/* Tag of the kernel the calling thread's last knnsvc_wavlm_attention launched: "wavlm_attention2" (f16x2, 128 queries per
 * workgroup), "wavlm_attention2q" (256), "wavlm_attention2w" (512, eight waves), "wavlm_attention3" (bf16x3), "wavlm_attention"
 * (fp32); "" before the first launch, unchanged by a refused call.  Measurement and test hook. */
const char* knnsvc_wavlm_attention_last_kernel(void);
/* The kernel knnsvc_wavlm_attention launches for these sizes and flags under the knobs as they are (KNNSVC_ATTENTION as last read,
 * KNNSVC_ATT_QB / KNNSVC_ATT_NW now), without a launch: host code only, no GPU and no stream.  -> its tag (`cap` >= 24 bytes) and
 * its dynamic LDS in bytes; a call the launch entry refuses for its sizes, its flags or a T too long for the LDS bias table is
 * refused here with the same code and message. */
int knnsvc_wavlm_attention_route(int32_t batches, int32_t T, int32_t heads, int32_t out_f16x2, int32_t kv_f16x2, char* tag,
                                 int32_t cap, int64_t* lds_bytes);

/* x[b, t, :] = 0 for t >= lens[b] on a [batches, T, dim] activation (row pitch ld): WavLM's `x[padding_mask] = 0`
 * (wavlm/WavLM.py:353, 574-575) in front of the positional convolution, for chunks padded up to a bucket length. */
int knnsvc_mask_rows(float* x, int32_t batches, int32_t T, int32_t dim, int32_t ld, const int32_t* lens, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-model entry points (round 5): ONE call enqueues the layer sequence of a network on the caller's stream.
 * A handle holds a copy of the descriptor — packed weights, their f16x2 splits and scales, LayerNorm vectors, the
 * range plan decided at load — i.e. POINTERS to device memory the caller keeps alive until *_free; the library
 * allocates nothing on the device and nothing at all inside the hot call (hipGraph-capturable), activations live in
 * a caller-provided workspace.  The sequence is the one knn_svc_amd/wavlm.py issued launch by launch until round 4:
 * same kernels, same arguments, same bits.
 * ------------------------------------------------------------------------------------------ */
typedef struct knnsvc_weight {            /* a packed GEMM weight matrix [n, K] and its split (knnsvc_split_weight_f16x2) */
    const float* w; const void* w_f16x2; float w_f16x2_scale; int32_t pad_;
} knnsvc_weight;

typedef struct knnsvc_wavlm_conv {        /* one layer of the conv feature extractor (wavlm/WavLM.py:401-419, 485-504) */
    knnsvc_weight w;                      /* [dim, k * cin] (layer 0 with cin = 1: [dim, k], fp32 only)                  */
    const float* ln_g; const float* ln_b; /* LayerNorm(dim) behind it (extractor_mode "layer_norm")                        */
    int32_t dim, k, stride, cin;
    int32_t out_split;                    /* the activation behind this layer may travel in the f16x2 split layout (load-time range plan) */
    int32_t pad_;
} knnsvc_wavlm_conv;

typedef struct knnsvc_wavlm_layer {       /* TransformerSentenceEncoderLayer, layer_norm_first (wavlm/WavLM.py:691-714) */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    knnsvc_weight wqkv; const float* bqkv;          /* q | k | v fused: [3E, E]                                            */
    knnsvc_weight wo;   const float* bo;
    knnsvc_weight w1;   const float* b1;            /* fc1 [ffn, E] */
    knnsvc_weight w2;   const float* b2;            /* fc2 [E, ffn] */
    const float *gate_w, *gate_b, *grep_a;          /* grep_linear summed to [2, 64] / [2]; grep_a [H] (wavlm/modules.py:523-533) */
    int32_t xn_split, xn2_split, h_split, attn_f16; /* range plan: which activations fit the fixed-scale split layout      */
} knnsvc_wavlm_layer;

typedef struct knnsvc_wavlm_desc {
    int32_t n_conv; int32_t n_layers;
    const knnsvc_wavlm_conv* conv; const knnsvc_wavlm_layer* layers;      /* HOST arrays, copied by knnsvc_wavlm_create    */
    const float *ln_g, *ln_b; int32_t feats_split; int32_t pad_;          /* layer_norm over the extractor's output (WavLM.py:342) */
    knnsvc_weight proj; const float* proj_b;                               /* post_extract_proj (:347-348)                  */
    knnsvc_weight pos; const float* pos_b; int32_t pos_groups, pos_k;      /* pos_conv, weight norm folded, packed per group (:514-527) */
    float pos_a_scale;                    /* fixed activation scale of the positional conv from the load-time bound (0: a range slot) */
    int32_t E, H, ffn;
    const float* layer_mix;               /* HOST [n_layers + 1] weights of a general layer weighting, NULL = the output of layer n_layers */
} knnsvc_wavlm_desc;

int knnsvc_wavlm_create(const knnsvc_wavlm_desc* d, void** handle);
int knnsvc_wavlm_free(void* handle);
/* frames of one chunk of L samples; bytes of workspace knnsvc_wavlm_encode needs for [batches, L] */
int64_t knnsvc_wavlm_frames(const void* handle, int64_t L);
size_t knnsvc_wavlm_workspace_bytes(const void* handle, int32_t batches, int64_t L);
/* WavLM.extract_features up to layer n_layers (wavlm/WavLM.py:323-375, 572-612) for [batches, L] equal-length chunks:
 * wav -> out [batches * T, E].  lens (may be NULL): DEVICE int32 [batches], valid frames per chunk (WavLM's padding mask:
 * rows >= lens[b] zeroed in front of the positional conv, excluded as attention keys).  table: [H][2T - 1] relative
 * position bias with the bucket LUT applied (host-built: wavlm/modules.py:417-455).  Everything is enqueued on `stream`. */
int knnsvc_wavlm_encode(const void* handle, const float* wav, int32_t batches, int64_t L, const int32_t* lens,
                        const float* table, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* The conditioned HiFi-GAN generator behind one call: SynthesizerTrn.forward + Generator.forward
 * (hifigan/ddsp_models.py:108-233, 405-493 'mix'; hifigan/ddsp_models_f0.py:106-216, 320-381 'f0').  Weights are
 * packed as knn_svc_amd/vocoder.py packs them (weight norm folded; conv [Cout, k*Cin]; transposed conv [u*Cout, (k/u)*Cin]),
 * each with its f16x2 split.  Three ResBlocks per stage (resblock_kernel_sizes has three entries), three dilations each. */
typedef struct knnsvc_gen_pair {          /* one iteration of ResBlock1.forward (hifigan/ddsp_models.py:13-44) */
    knnsvc_weight w1; const float* b1; knnsvc_weight w2; const float* b2;
    int32_t dil; float t1_bound_mul, t1_bound_add;   /* |convs1(lrelu(x)) + b1| <= mul * max|x| + add (from the weights, at load) */
    int32_t pad_;
} knnsvc_gen_pair;
typedef struct knnsvc_gen_stage {
    knnsvc_weight up; const float* up_b; int32_t u, k, cin, cout;      /* ups[i]: ConvTranspose1d(cin -> cout, k, stride u)            */
    knnsvc_weight ccv;                                                 /* concat_conv[i] (k = 3, no bias)                               */
    int32_t res_k[3]; int32_t pad_; knnsvc_gen_pair res[3][3];         /* resblocks[3 i + j]: kernel size res_k[j], pairs res[j][0..2]  */
    knnsvc_weight down; const float* down_b; int32_t down_k, down_u;   /* downs[i]: strided conv of the side path                       */
    knnsvc_weight rbd; const float* rbd_b;                             /* resblocks_downs[i].convs[0] (k = 3)                           */
} knnsvc_gen_stage;
typedef struct knnsvc_generator_desc {
    int32_t kind;                         /* 0 = 'mix' (additive-synth excitation, harmonic amplitudes), 1 = 'f0' (sine excitation) */
    int32_t n_up, hop, sample_rate, n_harm_in, uic, hubert_dim, hifi_dim;      /* lin_pre: hubert_dim -> hifi_dim; conv_pre: hifi_dim -> uic */
    int32_t side[8];                      /* channels of the side path's levels: side[0] = condition, side[i + 1] = output of down stage i */
    knnsvc_weight lin; const float* lin_b; knnsvc_weight pre; const float* pre_b;       /* lin_pre, conv_pre (k = 7)              */
    knnsvc_weight cpre; const float* cpre_b; knnsvc_weight post;                        /* concat_pre (k = 3), conv_post (k = 7)  */
    const float *prenet_w, *prenet_b;                                                   /* sin_prenet: Conv1d(1 -> side[0], 3)     */
    const knnsvc_gen_stage* stages;       /* HOST array [n_up], copied by knnsvc_generator_create */
} knnsvc_generator_desc;

int knnsvc_generator_create(const knnsvc_generator_desc* d, void** handle);
int knnsvc_generator_free(void* handle);
size_t knnsvc_generator_workspace_bytes(const void* handle, int64_t frames);
/* c [frames, hubert_dim], f0 [frames], harm [frames, n_harm_in] (NULL for kind 1) -> out [frames * hop].  n_dyn (may be NULL):
 * DEVICE int32 holding the valid frame count <= frames — the launch sequence is laid out for `frames` (a length bucket) and
 * computes exactly what an exact-length run computes (knnsvc_conv_desc, "Dynamic length").  Enqueues only; capturable. */
int knnsvc_generator_forward(const void* handle, const float* c, const float* f0, const float* harm, int64_t frames,
                             const int32_t* n_dyn, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cosine-distance kNN (lib_ongaku_test.py:148-175 fast_cosine_dist + Tensor.topk(k, largest=False),
 * driver loop ddsp_prematch_dataset.py:1195-1210).
 * ------------------------------------------------------------------------------------------ */
/* norm[r] = sqrt(sum x^2) (torch.norm, lib_ongaku_test.py:150-151); sq[r] = sum x^2 (cdist's own term).
 * max_slot (may be NULL): range slot (8 KiB), folded with the largest row norm (atomicMax on the bit pattern; the caller
 * zeroes it) — an upper bound of max|x| that costs no extra pass: the range slot the kNN's f16x2 GEMM scales by. */
int knnsvc_row_norms(const float* x, int64_t rows, int32_t dim, int32_t ldx, float* norm, float* sq, float* max_slot,
                     void* stream);

size_t knnsvc_knn_workspace_bytes(int64_t nq, int64_t np, int32_t k);

/* Wide lists and the exact re-score (round 5).  "Bit-exact top-k indices" is defined against the reference's fp32 formula
 * (lib_ongaku_test.py:162-165) evaluated on ITS matrix product; whatever product a GPU kernel forms (here: fp16-split MFMAs with 96
 * fp32 roundings along K, or fp32 MFMAs) differs from it in the last bits, and neighbours closer together than those bits swap.
 * The selection kernels below therefore only PICK candidates: each keeps, per query row, a WIDE list of up to 64 keys
 * (uint64: order-preserving bits of the screening distance << 32 | pool row) — the k best and every pair within the guard band
 * of the k-th (4e-6 on the f16x2 routes; 5e-7 sqrt(dim), at least 4e-6, on knnsvc_knn_topk's fp32-MFMA tile) — and
 * knnsvc_knn_rescore recomputes q.p for exactly those pairs in fp64 from the fp32 operands, rounds once to fp32,
 * replays the reference's formula and sorts by (distance bits, lower index first).  A CROWDED row — all 64 places filled, the
 * 64th key still inside the band: exact top-k members may have been cut — is re-scored against every one of the np pool rows
 * instead, so the result is the exact top-k either way.  What is left between this order and the
 * reference's is the reference's own BLAS rounding.  exact = 0 passes the screening order through (A/B aid).
 * wide: [nq][64] keys ascending, unused places 0xFFFF...F; out_idx / out_dist: [nq][k], indices + idx_offset; a row with fewer
 * than k finite distances (a NaN row) is filled with VALID row indices and NaN distances.  [mask_lo, mask_hi) as below. */
int knnsvc_knn_rescore(const void* wide, int64_t nq, int32_t k, const float* q, const float* q_norm, const float* q_sq,
                       const float* pool, const float* p_norm, const float* p_sq, int64_t np, int32_t dim,
                       int64_t idx_offset, int64_t mask_lo, int64_t mask_hi, int32_t exact,
                       int64_t* out_idx, float* out_dist, void* stream);

/* Ascending top-k of d(q_i, p_j) per query row, d evaluated with the reference's operation
 * sequence on top of an fp32-MFMA dot product (candidates), then re-scored exactly (rescore != 0: knnsvc_knn_rescore).
 * Ties: lower pool index first.  Indices are written
 * as idx_offset + j (so that a pool shard reports global rows).  k <= 32.
 * [mask_lo, mask_hi): local pool rows whose distance is replaced by exactly 1 before selection — the
 * self-matching rule of per_spk_extract (ddsp_prematch_dataset.py:1606-1607, `dists[:, start:end] = 1`);
 * mask_lo >= mask_hi disables it. */
int knnsvc_knn_topk(const float* q, const float* q_norm, const float* q_sq, int64_t nq,
                    const float* pool, const float* p_norm, const float* p_sq, int64_t np,
                    int32_t dim, int32_t k, int64_t idx_offset, int64_t mask_lo, int64_t mask_hi,
                    int64_t* out_idx, float* out_dist, void* workspace, size_t workspace_bytes,
                    int32_t* nan_flag, int32_t rescore, void* stream);

/* Second half of the two-kernel kNN route: `dots`[nq, np] (row pitch ld) holds q.p^T computed by knnsvc_conv_gemm
 * on the emulated-fp32 matrix-core path (q as the A operand, the pool rows as pre-split "weights"); this replays the
 * reference's distance formula (lib_ongaku_test.py:148-175) on every entry and keeps each row's WIDE list (wide_out [nq][64],
 * see knnsvc_knn_rescore, which turns it into the top-k) with the same (distance, lower index) order and NaN flag
 * semantics as knnsvc_knn_topk. */
int knnsvc_knn_select(const float* dots, int64_t ld, const float* q_norm, const float* q_sq, int64_t nq,
                      const float* p_norm, const float* p_sq, int64_t np, int32_t k,
                      int64_t mask_lo, int64_t mask_hi,
                      void* wide_out, int32_t* nan_flag, void* stream);

/* Fused route (no [nq, np] dot matrix in HBM; lib_ongaku_test.py:148-175 + ddsp_prematch_dataset.py:1195-1210: the reference's
 * 20-row cdist + topk loop over the whole pool).  The caller walks the pool's rows in EPOCHS [p_base, p_base + np) of growing
 * size (knn_svc_amd/ops.py: knn_epochs); each epoch is one knnsvc_knn_screen + one knnsvc_knn_refine.
 * knnsvc_knn_screen: q.p^T on the f16x2 matrix-core path (both operands pre-split by knnsvc_split_f16x2_dyn with the range
 * slots q_absmax / p_absmax; p_f16x2 / p_norm / p_sq point at the epoch's first row), every product screened in registers: first
 * conservatively against the row's threshold, then — the few survivors — exactly: the reference's distance of the pair as a
 * (distance, pool index) key.
 *   thr == thr_idx == NULL (the first epoch): every 256 x 256 tile bounds its rows itself — at least 32 of its columns lie at
 *     or below the bound it derives, so no row's top-k (k <= 32) can lie beyond it;
 *   otherwise (thr[row], thr_idx[row]) = the row's threshold key over the rows searched so far (knnsvc_knn_refine's thr_out /
 *     thr_idx_out: the k-th best distance + the guard band of the exact re-score; the index in the chunk's index space, i.e.
 *     without idx_offset): exactly the pairs with key <= it pass.
 * Survivors are appended to cand[row][0 .. cap) as (pool index = p_base + row in epoch, order-preserving bits of the distance;
 * 0xFFFFFFFF = NaN), 8 bytes each; cand_count[row] counts them (the caller zeroes cand_count and the flag once; refine
 * resets the counts).  Bit 1 of *overflow_flag set afterwards: some row had more than cap survivors — the caller must fall
 * back to the dot-matrix route (the same word and bit as knnsvc_knn_refine's `flags`: one flag per search).  mask_lo / mask_hi: chunk rows [lo, hi) compete at distance exactly 1.
 * cold_ws (first epoch only, else NULL; nq * (1 + 2 * ceil(np / 256)) + 32 * ceil(nq / 256) words the caller zeroes): [nq] the best
 * bound found for each row — knnsvc_knn_refine's row_bound: it starts from it and drops the survivors of weaker tiles unseen —,
 * then the per-half-tile bounds and arrival counters through which the tiles of a row tile, running side by side, tighten each
 * other's bounds (a bounded wait; only tightness depends on it, never the result).
 * knnsvc_knn_refine: the row's wide list so far (`wide` [nq][64], read when has_prev != 0: the previous refine's output) + the
 * candidates -> the wide list, written back to `wide` — after the last epoch identical to knnsvc_knn_select's over every
 * pair; knnsvc_knn_rescore turns it into the top-k.  flags: bit 0 = a NaN distance was met, bit 1 (final_pass only) = a row
 * ended with fewer than k entries although no NaN was seen (the caller repeats the search on the dot-matrix route).
 * thr_out / thr_idx_out (NULL after the last epoch): the next epoch's thresholds (the k-th distance + the guard band).
 * nq * dim and np * dim below 2^28 per call (chunk larger searches).
 * max_blocks: the screen kernel is persistent (a block walks tiles); 0 = one block per CU, otherwise at most this many blocks
 * (rounded down to a multiple of 8), so that a search inside a stream pipeline leaves CUs to the other streams' kernels. */
int knnsvc_knn_screen(const void* q_f16x2, const float* q_absmax, const float* q_norm, const float* q_sq, int64_t nq,
                      const void* p_f16x2, const float* p_absmax, const float* p_norm, const float* p_sq, int64_t np,
                      int32_t dim, const float* thr, const int64_t* thr_idx, int64_t mask_lo, int64_t mask_hi, int64_t p_base,
                      int32_t* cand_count, void* cand, int32_t cap, uint32_t* cold_ws, int32_t* overflow_flag, int32_t max_blocks,
                      void* stream);
int knnsvc_knn_refine(int32_t* cand_count, const void* cand, int32_t cap, int64_t nq, int32_t k,
                      const uint32_t* row_bound, int32_t has_prev, void* wide, float* thr_out,
                      int64_t* thr_idx_out, int32_t final_pass, int32_t* flags, void* stream);

/* Merge `parts` per-shard top-k lists ([parts][nq][k], e.g. after an RCCL all-gather) into one. */
int knnsvc_knn_merge(const float* part_dist, const int64_t* part_idx, int32_t parts, int64_t nq,
                     int32_t k, int64_t* out_idx, float* out_dist, void* stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour post-processing.
 * ------------------------------------------------------------------------------------------ */
/* lower median of log(f0) over voiced frames (torch.median, ddsp_prematch_dataset.py:1224-1225);
 * result[0] = median, result[1] = voiced count (as float).  workspace: n floats. */
int knnsvc_log_f0_median(const float* f0, int64_t n, float* result, float* workspace, void* stream);

/* shifted[i] = f0[i] ? exp(log f0[i] + (pool_median - query_median)) : 0   (:1232-1233).  The one-segment case of
 * knnsvc_shift_f0_seg_mode with MEDIAN / 0 ("Pitch control" below: the three entries share one kernel). */
int knnsvc_shift_f0(const float* f0, int64_t n, const float* query_median, const float* pool_median,
                    float* shifted, void* stream);

/* sort_by_f0_compatibility (ddsp_prematch_dataset.py:954-1016): stable ascending re-order of each
 * row's k neighbours by |log2(pool_f0[idx]+1e-5) - log2(shifted[i]+1e-5)|. k <= 64. */
int knnsvc_f0_rerank(const int64_t* nn_idx, int64_t nq, int32_t k, const float* shifted_f0,
                     const float* pool_f0, int64_t* out_idx, void* stream);

/* knn_with_concat_cost (lib_ongaku_test.py:270-369), frame-sequential, one workgroup per sequence.
 * idx_in/out [nq, 4]; use_f0 selects the pitched variant. */
int knnsvc_concat_reselect(const int64_t* idx_in, const float* q, const float* q_norm, int64_t nq,
                           const float* pool, const float* p_norm, int64_t np, int32_t dim,
                           const float* shifted_f0, const float* pool_f0, int32_t use_f0,
                           float concat_weight, int64_t* idx_out, void* stream);

/* compute_wavlm_weight / compute_extended_weight (ddsp_prematch_dataset.py:574-680, 807-924):
 * Adam(amsgrad) on softmax weights with the reference's stopping rules, run entirely on the
 * device (no per-iteration host sync).  scale = 0.1 (WavLM) or 1000 (harmonics).
 * out_w [nq,4]; out_iters[0] = iterations executed.  workspace from knnsvc_smooth_workspace_bytes.
 * max_iter > 0: the reference's cap (100 000 there).  max_iter < 0 (measurement aid): exactly -max_iter iterations
 * with the stopping rules switched off (bench.py's sensitivity figure for data on which the loops run long). */
/* row_scale (may be NULL) [nq,4]: compute_weight_with_amp (ddsp_prematch_dataset.py:684-804) — candidate k of
 * frame t and its two neighbours are multiplied by row_scale[t,k] (the amp_ratio of per_spk_extract) before the
 * loss is formed; with scale = 1000 this is the prematch weight optimisation. */
size_t knnsvc_smooth_workspace_bytes(int64_t nq);
int knnsvc_smooth_weights(const int64_t* idx, int64_t nq, const float* pool, int64_t np, int32_t dim,
                          int32_t ld, float scale, const float* row_scale, int32_t max_iter, float* out_w,
                          int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The match stage for n_seg independent sequences in one launch sequence.  Every per-row array is the
 * sequences' arrays stacked in order; host_seg is a HOST array int64 [n_seg + 1] of row offsets: host_seg[0] == 0,
 * strictly ascending (no empty segment), host_seg[n_seg] = total rows, 1 <= n_seg <= KNNSVC_MAX_SEGMENTS.  It is
 * validated on the host, sizes the grids and reaches the kernels by value as a kernel argument: no device-side
 * table, no allocation, no synchronisation; the calls stay hipGraph-capturable.  One workgroup per segment; the
 * single-sequence entry points above are the one-segment case (the same kernels and host path with a table
 * {0, n}), so every output row of segment s, and its result / out_iters entry, is bit-identical to that entry
 * point called on the segment's rows alone.  All argument checks run before the first HIP call.
 * ------------------------------------------------------------------------------------------ */
#define KNNSVC_MAX_SEGMENTS 64
/* knnsvc_log_f0_median per segment (ddsp_prematch_dataset.py:1224-1225).  result [n_seg][2]: (lower median of
 * log f0 over voiced rows — NaN if there is none —, voiced count); workspace: total floats. */
int knnsvc_log_f0_median_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, float* result, float* workspace, void* stream);

/* knnsvc_shift_f0 per segment (:1232-1233).  query_median [n_seg][2] (the above), pool_median [2].
 * knnsvc_shift_f0_seg_mode with NULL tables and a NULL shift_semitones, under this entry's name in the messages. */
int knnsvc_shift_f0_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, const float* query_median,
                        const float* pool_median, float* shifted, void* stream);

/* Pitch control (an extension; upstream knows only the median shift): knnsvc_shift_f0_seg with a MODE and a TRANSPOSE t
 * (semitones, finite, |t| <= KNNSVC_F0_TRANSPOSE_MAX) per segment.  This restatement is the specification, and the one kernel
 * and host path behind it also serve knnsvc_shift_f0 and knnsvc_shift_f0_seg (all MEDIAN, all 0).
 *   L = log_rn(f): the fp32 log evaluated in fp64 and rounded once, as in knnsvc_shift_f0; qm, pm: the fp32 lower medians
 *   (query_median[s][0], pool_median[0]); LN2 = fp64 ln 2, S = LN2 / 12, d = (double)pm - (double)qm; rint rounds half to
 *   even; no floating-point contraction anywhere.  Shifted log f0 of a voiced frame:
 *     KNNSVC_F0_SHIFT_MEDIAN   (0)  v = (L + pm) - qm in fp32, knnsvc_shift_f0's expression; when t != 0: v + (float)(t * S)
 *     KNNSVC_F0_SHIFT_OCTAVE   (1)  L + (float)(LN2 * rint(d / LN2) + t * S)   pitch classes kept, register moved to the pool's
 *     KNNSVC_F0_SHIFT_SEMITONE (2)  L + (float)(S * rint(d / S) + t * S)       stays on the source's equal-tempered grid
 *     KNNSVC_F0_SHIFT_NONE     (3)  L + (float)(t * S)                         the medians are NOT READ
 *   shifted = exp_rn of that value; an unvoiced frame (f == 0) is copied bit for bit.  MEDIAN with t == 0 is upstream's
 *   shift.  A NaN median (no voiced frame on either side) propagates in the three modes that read the medians.
 *   shift_semitones (device float [n_seg], may be NULL) receives the interval applied, in semitones: d / S + t (MEDIAN),
 *   (quantised + t * S) / S (OCTAVE, SEMITONE), t (NONE).
 * host_modes (int32 [n_seg]) and host_transposes (float [n_seg]) are HOST tables read by the call and handed to the kernel
 * by value like host_seg; NULL = all MEDIAN / all 0.  The interval is chosen on the device by every thread of the segment:
 * no host read of the medians, one launch, hipGraph-capturable.  Refused before the launch, with a message: a bad table, a
 * null f0 / query_median / pool_median / shifted, a mode outside 0..3, a transpose that is NaN, infinite or beyond the bound. */
#define KNNSVC_F0_SHIFT_MEDIAN 0
#define KNNSVC_F0_SHIFT_OCTAVE 1
#define KNNSVC_F0_SHIFT_SEMITONE 2
#define KNNSVC_F0_SHIFT_NONE 3
#define KNNSVC_F0_TRANSPOSE_MAX 36.0f
int knnsvc_shift_f0_seg_mode(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_modes,
                             const float* host_transposes, const float* query_median, const float* pool_median,
                             float* shifted, float* shift_semitones, void* stream);

/* knnsvc_concat_reselect per segment (lib_ongaku_test.py:270-369): every segment is a sequence of its own — its
 * frame 0 keeps its neighbours, the walk never looks across a boundary.  idx_in/out [total, 4]. */
int knnsvc_concat_reselect_seg(const int64_t* idx_in, const float* q, const float* q_norm, const int64_t* host_seg, int32_t n_seg,
                               const float* pool, const float* p_norm, int64_t np, int32_t dim, const float* shifted_f0,
                               const float* pool_f0, int32_t use_f0, float concat_weight, int64_t* idx_out, void* stream);

/* knnsvc_smooth_weights per segment (ddsp_prematch_dataset.py:574-680, 807-924): one Gram launch over the adjacent
 * pairs of all segments (a pair never spans a boundary), then one launch per loop variant present, each segment on the
 * variant it would get alone.  out_w [total][4]; out_iters [n_seg] (may be NULL); row_scale (may be NULL) [total][4].
 * A segment of one row gets 0.25 and 0 iterations.  The workspace is the sum of the per-segment needs
 * (knnsvc_smooth_workspace_bytes), each rounded up to 64 bytes; 0 for an invalid table. */
size_t knnsvc_smooth_seg_workspace_bytes(const int64_t* host_seg, int32_t n_seg);
int knnsvc_smooth_weights_seg(const int64_t* idx, const int64_t* host_seg, int32_t n_seg, const float* pool, int64_t np,
                              int32_t dim, int32_t ld, float scale, const float* row_scale, int32_t max_iter, float* out_w,
                              int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream);

/* The three segmented calls above that carry a [.., 4], for k neighbours per frame (topk), 1 <= k <= 8: idx_in / idx_out /
 * idx / out_w / row_scale are [total, k].  The entry points above are the k = 4 call of the same launchers.  Each stage
 * is one K-templated kernel for every k (a four-wave walk over 2k candidates per frame in (4k + 2) * dim * 4 bytes of LDS;
 * a Gram of k(2k - 1) entries per frame pair; one Adam loop with its state in the workspace, exchanging weights and
 * gradients through LDS while 2 * k * 4 * rows bytes fit 144 KB), and k = 4 has fast paths beside them: the pipelined
 * walk (dim <= 1024), the register-resident Adam loops (<= 1536 rows) and a float4 Adam loop for longer sequences.
 * KNNSVC_MATCH_GENERIC_K=1 (read per call) makes k = 4 skip them.  A one-row segment gets 1 / k and 0 iterations.  Refused before the first HIP call: k outside 1..8
 * (KNNSVC_EINVAL; the workspace size is then 0), an LDS need above 150 KB, misaligned q / pool / out_w, a workspace below
 * knnsvc_smooth_seg_workspace_bytes_k (KNNSVC_EWORKSPACE).  At k = 4 that size equals knnsvc_smooth_seg_workspace_bytes. */
int knnsvc_concat_reselect_seg_k(const int64_t* idx_in, int32_t k, const float* q, const float* q_norm, const int64_t* host_seg,
                                 int32_t n_seg, const float* pool, const float* p_norm, int64_t np, int32_t dim,
                                 const float* shifted_f0, const float* pool_f0, int32_t use_f0, float concat_weight,
                                 int64_t* idx_out, void* stream);
size_t knnsvc_smooth_seg_workspace_bytes_k(const int64_t* host_seg, int32_t n_seg, int32_t k);
int knnsvc_smooth_weights_seg_k(const int64_t* idx, int32_t k, const int64_t* host_seg, int32_t n_seg, const float* pool, int64_t np,
                                int32_t dim, int32_t ld, float scale, const float* row_scale, int32_t max_iter, float* out_w,
                                int32_t* out_iters, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Time scale (makes upstream's target_duration work, ddsp_matcher.py:524-548): n_seg stacked query sequences re-timed
 * along the frame axis, in front of the whole match stage.  x [seg_in[n_seg], dim] -> x_out [seg_out[n_seg], dim] and
 * f0 [seg_in[n_seg]] -> f0_out [seg_out[n_seg]]; x / x_out may both be NULL (f0 only), f0 / f0_out may both be NULL
 * (features only).  host_seg_in / host_seg_out are HOST row-offset tables as for the *_seg calls above (segment s: T =
 * seg_in[s+1] - seg_in[s] >= 1 input rows, T' = seg_out[s+1] - seg_out[s] >= 1 output rows); host_inv_scale (HOST double
 * [n_seg]) holds c = 1 / scale_factor per segment, finite and > 0.  The caller decides T' and c; the kernel applies them.
 * This restatement is the specification.  All arithmetic is fp64 and no operation is contracted with another, with ONE
 * stated exception: the source index is a single fused multiply-add, rounded once, because that is how PyTorch's CPU
 * kernel evaluates the same expression (the two-rounding form differs from it wherever c * (j + 0.5) lies just above a
 * power of two and r below it, by up to an ulp of the product).  For output row j of a segment:
 *     r  = fma(c, (double)j + 0.5, -0.5);  r < 0 becomes 0
 *     i0 = (int64)r;  i1 = i0 + (i0 < T-1 ? 1 : 0);  l1 = r - (double)i0;  l0 = 1.0 - l1
 *     i0 > T-1 (possible only through rounding): i0 = i1 = T-1, l1 = 0
 *   which is PyTorch's `linear`, align_corners=False, scale_factor-given source index with c = 1 / scale_factor, the call
 *   upstream makes.
 *   features  x_out[j][d] = (float)(l0 * (double)x[i0][d] + l1 * (double)x[i1][d]): two multiplies, one add, one rounding
 *             to fp32.  With c == 1 every l1 is 0 and finite rows come back bit for bit.
 *   f0        (upstream has no rule) voiced means > 0; near = (l1 > 0.5) ? i1 : i0, a tie goes left.  f0[near] <= 0 -> 0;
 *             else both neighbours voiced -> (float)exp(l0 * log((double)f0[i0]) + l1 * log((double)f0[i1])) (interpolation
 *             in log-frequency, the domain the match stage works in); else f0[near] unchanged.  Voicing follows the nearer
 *             frame and a note's edge never glides towards 0 Hz.
 * A row never reads across its segment's boundary, and the result of segment s does not depend on what else is in the call.
 * One launch on `stream` (256-thread workgroups: four feature rows each, 16-byte accesses when dim % 4 == 0 and x, x_out are
 * 16-byte aligned, else scalar; the f0 frames in a tail of the grid), no atomics, no workspace, hipGraph-capturable.
 * Refused before the launch, with a message: a bad table, a null / non-finite / non-positive inv_scale, x without x_out
 * (or f0 without f0_out) and the reverse, neither pair given, dim <= 0 with features.
 * ------------------------------------------------------------------------------------------ */
int knnsvc_time_scale_seg(const float* x, int32_t dim, const float* f0, const int64_t* host_seg_in, const int64_t* host_seg_out,
                          const double* host_inv_scale, int32_t n_seg, float* x_out, float* f0_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voice blend (an extension; upstream converts towards one pool): a conversion towards a weighted mix of V voices,
 * 2 <= V <= KNNSVC_BLEND_MAX_VOICES, with weights a_0 .. a_{V-1} per segment (source item).  This restatement is the
 * specification.
 *   1. Per voice the match stage runs exactly as for a single target, against that voice's pool with the item's f0 shift
 *      mode, transpose and k: voice v's features x_v and harmonics are bit-identical to the single-target conversion
 *      towards v.  The per-voice shifted f0 is used inside that voice's match only.
 *   2. Features and harmonics are mixed linearly in fp64 and rounded once:
 *          out[i][c] = (float)( sum_v a_v * (double)x_v[i][c] )
 *      over the voices in ascending order.  Every product and every sum is an fp64 operation of its own (no contraction);
 *      the sum starts with the first product (nothing is added to a zero).  A voice whose weight is exactly 0 is NOT READ:
 *      a NaN in it does not reach the output.  When only one weight of the row is non-zero, that voice's values are copied
 *      bit for bit.
 *   3. The output f0 is ONE shift towards the blended register, not a mix of shifted tracks: the pool median of the segment
 *      is pm = (float)( sum_v a_v * (double)pm_v ) over the voices' fp32 lower medians of log f0 (pool_medians[v][0]), with
 *      the zero-skip and single-term-copy rules of 2.  After that the arithmetic of "Pitch control" applies unchanged, in
 *      all four modes and with the transpose: OCTAVE and SEMITONE keep their grid guarantee under a blend, MEDIAN moves
 *      the source to the weighted mean of the voices' log medians, NONE reads no median.  A NaN median of a voice with a
 *      non-zero weight propagates.  (Mixing the per-voice shifted tracks instead would put an OCTAVE blend of two voices
 *      an octave apart half an octave — a tritone — off the source's pitch classes.)
 *   4. Weights: every entry finite and >= 0, at least one > 0, |sum - 1| <= 1e-6 (summed in order in fp64).  The library
 *      does not normalise: the caller divides by the sum, so that a one-hot row stays exactly one-hot.
 * knnsvc_blend_seg: point 2 for n_seg stacked segments.  host_x: a HOST array of n_voices device pointers, each to the
 * stacked [host_seg[n_seg], dim] rows of one voice; host_weights: HOST double [n_seg][n_voices]; both tables are read by
 * the call and reach the kernel by value like host_seg.  out [host_seg[n_seg], dim] may be one of the inputs, and may not
 * overlap one otherwise.  One launch on `stream` (256-thread workgroups, four rows each; 16-byte accesses when dim % 4 == 0
 * and every pointer is 16-byte aligned, else scalar), no device table, no allocation, no synchronisation,
 * hipGraph-capturable; the result of segment s does not depend on what else is in the call.
 * knnsvc_shift_f0_seg_blend: knnsvc_shift_f0_seg_mode with pool_medians (device float [n_voices][2], the results of
 * knnsvc_log_f0_median per voice), n_voices and host_weights [n_seg][n_voices] in place of pool_median: point 3.  The same
 * kernel and host path as the other three shift entries; the blended median is formed by every thread of the segment
 * from the device medians: no host read, no extra launch.
 * Both refuse before the first HIP call, with a message: a null pointer, n_voices outside 2..KNNSVC_BLEND_MAX_VOICES, a bad
 * segment table, a weight row that breaks point 4 (naming the segment), dim <= 0; the shift entry also what
 * knnsvc_shift_f0_seg_mode refuses.
 * ------------------------------------------------------------------------------------------ */
#define KNNSVC_BLEND_MAX_VOICES 4
int knnsvc_blend_seg(const float* const* host_x, int32_t n_voices, int32_t dim, const int64_t* host_seg, int32_t n_seg,
                     const double* host_weights, float* out, void* stream);
int knnsvc_shift_f0_seg_blend(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_modes,
                              const float* host_transposes, const float* query_median, const float* pool_medians,
                              int32_t n_voices, const double* host_weights, float* shifted, float* shift_semitones,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * Pitch correction (an extension; upstream has none): the shifted f0 of n_seg stacked segments snapped towards the notes of
 * a key, behind knnsvc_shift_f0_seg[_mode|_blend] and in front of everything that reads the shifted track (f0 re-rank,
 * pitched concat re-selection, vocoder).  This restatement is the specification.
 * Per segment s:  x[i] fp32, the f0 as the shift returns it;  mask (int) 12 bits, bit k = pitch class k is allowed, C = 0;
 * sigma (fp64) in [0, 1], the strength;  a (fp64) in (0, 1], the retune coefficient per frame;  log_ref (fp64), the natural
 * log of the tuning frequency of A4.  mask == 0 or sigma == 0: the segment is OFF, its output is the input bit for bit and
 * its notes are -1.  Constants: S = LN2 / 12 (the fp64 LN2 of "Pitch control"), H = 5, HYST = 0.25.  All arithmetic is fp64
 * with contraction off, every step rounded on its own; the output is rounded once.
 *   1. Pitched frames.  A frame is pitched iff 0 < x[i] < +inf.  Every other frame (0, NaN, negative, inf) keeps its bits,
 *      gets note -1 and ends a run.  A run is a maximal stretch of consecutive pitched frames WITHIN ONE SEGMENT; nothing
 *      below looks across a run's ends or a segment's ends.
 *   2. Pitch in semitones.  l[i] = log((double)x[i]);  m[i] = (l[i] - log_ref) / S + 69.0.
 *   3. Centre.  c[i] = the lower median (element (cnt - 1) / 2 of the sorted values) of m[lo..hi], lo = max(b, i - H),
 *      hi = min(e - 1, i + H) for the run [b, e): selection only, no arithmetic.  It follows note steps and rides through
 *      vibrato.
 *   4. Note, sequential along the run.  near(c) = the integer k with bit ((k mod 12) + 12) mod 12 of mask set that minimises
 *      |(double)k - c|; of two equally near, the lower.  n[b] = near(c[b]); for i > b, with cand = near(c[i]):
 *      n[i] = cand if |c[i] - cand| + HYST < |c[i] - n[i-1]|, else n[i-1].  The hysteresis keeps vibrato from flipping
 *      between two notes.
 *   5. Correction, sequential along the run.  e[i] = (double)n[i] - m[i] (the raw pitch, not the centre);  g[b] = e[b],
 *      g[i] = g[i-1] + a * (e[i] - g[i-1]).
 *   6. Output.  y[i] = (float)exp(l[i] + (sigma * g[i]) * S);  notes[i] = n[i] (int32).
 * a = 1 is a hard snap: every pitched frame lands on its note and vibrato is gone.  A small a (slow retune) moves each
 * note's centre onto the grid and leaves vibrato alone.  A caller that thinks in milliseconds uses
 * a = -expm1(-20 / retune_ms) in fp64 (20 ms frames; retune_ms = 0: a = 1).  The tie rules make the specification total; an
 * exact tie cannot be reached from fp32 inputs through a log.
 * knnsvc_tune_f0_seg: host_mask (int32), host_sigma, host_alpha, host_log_ref (double), each [n_seg], are HOST tables read
 * by the call and handed to the kernel by value like host_seg (64 x 28 bytes beside the segment table).  out [total] may not
 * be f0; notes (int32 [total]) may be NULL.  ws: knnsvc_tune_f0_workspace_bytes(total, n_seg) bytes, 8-byte aligned (32
 * bytes per frame: m, c, g and the note between the phases).  One launch on `stream`, one workgroup per segment in three
 * phases separated by workgroup barriers: (A) a thread per frame: m, the centre, near(c) and its distance; (B) the thread
 * whose frame starts a run walks that run alone through 4 and 5 — runs side by side, the order inside a run is the
 * specification's, so nothing depends on scheduling; (C) a thread per frame: the exponential.  No allocation, no
 * synchronisation, no floating-point atomics, hipGraph-capturable.  A segment's output is bit-identical whether it is
 * launched alone or stacked with others, and from call to call; an off segment is never read beyond copying its bits; rows
 * outside the table are not written.
 * Refused before the first HIP call, with a message: a bad table, a null table, a mask outside 0..0xFFF, a sigma that is not
 * a number in [0, 1], an alpha that is not a number in (0, 1], a log_ref that is not finite (on and off segments alike), a
 * null f0 / out / ws, out == f0, a misaligned workspace, a workspace below the size (KNNSVC_EWORKSPACE).  The size is 0,
 * with a message, for n_seg outside 1..KNNSVC_MAX_SEGMENTS or fewer rows than segments.
 * ------------------------------------------------------------------------------------------ */
size_t knnsvc_tune_f0_workspace_bytes(int64_t n_total, int32_t n_seg);
int knnsvc_tune_f0_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_mask,
                       const double* host_sigma, const double* host_alpha, const double* host_log_ref, float* out,
                       int32_t* notes, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Harmony voice (an extension; upstream has none): the f0 contour of a harmony PART derived from the lead's, for n_seg
 * stacked segments: every note of the lead moved by a number of scale DEGREES (a third above in C major is 4 semitones
 * over C and 3 over D), the lead's own deviation from its note (vibrato, drift, phrasing) carried over unchanged.  It
 * stands behind knnsvc_shift_f0_seg* and, when on, knnsvc_tune_f0_seg, and in front of everything that reads the f0 (f0
 * re-rank, pitched concat re-selection, vocoder), so a part's pool frames are chosen at the part's pitch.  This
 * restatement is the specification.
 * Per segment s:  x[i] fp32, the lead's final f0;  mask (int) 12 bits as in "Pitch correction";  steps (int) scale degrees,
 * -KNNSVC_HARMONY_MAX_STEPS..KNNSVC_HARMONY_MAX_STEPS;  a (fp64) in (0, 1], the glide coefficient per frame;  log_ref
 * (fp64), the natural log of the tuning frequency of A4.  mask == 0 or steps == 0: the segment is OFF, its output is the
 * input bit for bit, its notes are -1 and nothing else of it is read.  Constants S, H, HYST as there.  All arithmetic is
 * fp64 with contraction off, every step rounded on its own; the output is rounded once.
 *   1-4. Steps 1 to 4 of "Pitch correction", word for word: pitched frames and runs, l[i] and m[i], the centre c[i], the
 *      note n[i] with its hysteresis.  (One copy of the device code serves both kernels.)
 *   5. Degree move.  p_0 < ... < p_{d-1}: the allowed pitch classes, d = popcount(mask).  n[i] is allowed by construction;
 *      j: the index of its pitch class, o = (n[i] - p_j) / 12 (exact), J = j + steps.
 *      t[i] = 12 * (o + floordiv(J, d)) + p_{floormod(J, d)}: floor division and the non-negative remainder, for negative
 *      J and negative notes (below 8.18 Hz at 440) too.  D[i] = t[i] - n[i], a whole number of semitones.
 *   6. Glide, sequential along the run.  h[b] = (double)D[b];  h[i] = h[i-1] + a * ((double)D[i] - h[i-1]).  A part's
 *      interval changes where the lead changes note; a = 1 makes that a jump, a smaller a a short portamento.
 *   7. Output.  y[i] = (float)exp(l[i] + h[i] * S);  notes[i] = t[i] (int32), -1 for an unpitched frame, which keeps its
 *      bits.  (A part's note may itself be -1, below 8.18 Hz; the lead's frame is then pitched.)
 * With the chromatic mask D == steps: a parallel part, y = (float)exp(l + steps * S).  steps = +-d gives D == +-12.  The
 * part keeps the lead's deviation from its note to the cent.  A caller that thinks in milliseconds uses
 * a = -expm1(-20 / glide_ms) (glide_ms = 0: a = 1).
 * knnsvc_harmony_f0_seg: host_mask, host_steps (int32), host_alpha, host_log_ref (double), each [n_seg], are HOST tables
 * handed to the kernel by value.  Workspace (knnsvc_tune_f0_workspace_bytes), launch shape (one workgroup per segment,
 * phases A / B / C) and promises are those of knnsvc_tune_f0_seg: one launch, no allocation, no synchronisation, no
 * floating-point atomics, hipGraph-capturable; a segment's output is bit-identical whether it is launched alone or
 * stacked, and from call to call; rows outside the table are not written.
 * Refused before the first HIP call, with a message that names the segment: what knnsvc_tune_f0_seg refuses (steps in
 * the place of sigma: outside -24..24).
 * ------------------------------------------------------------------------------------------ */
#define KNNSVC_HARMONY_MAX_STEPS 24
#define KNNSVC_HARMONY_MAX_PARTS 3
int knnsvc_harmony_f0_seg(const float* f0, const int64_t* host_seg, int32_t n_seg, const int32_t* host_mask,
                          const int32_t* host_steps, const double* host_alpha, const double* host_log_ref, float* out,
                          int32_t* notes, void* ws, size_t ws_bytes, void* stream);

/* out[i,:] = sum_k w[i,k] * pool[idx[i,k], :]   (ddsp_prematch_dataset.py:1358, 1444).  w NULL = uniform weights:
 * mean_mode 0 multiplies every row by 1.0f / k (softmax(ones), :1361-1364), mean_mode 1 sums in order and divides by k
 * (torch.mean, harmonics :1446); any k >= 1, the two are bit-identical when k is a power of two. */
int knnsvc_weighted_gather(const int64_t* idx, const float* w, int64_t nq, int32_t k, const float* pool,
                           int32_t dim, int32_t ld, int32_t mean_mode, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prematch (training-pool generation, ddsp_prematch_dataset.py:1464-1772 per_spk_extract).
 * ------------------------------------------------------------------------------------------ */
/* out = float(half(x)) element-wise, round-to-nearest-even (`.half().float()`, :1509, 1561, 1592) */
int knnsvc_round_f16(const float* x, int64_t n, float* out, void* stream);
/* amp_ratio[t,k] = ||spec_q[t,:]||_1 / (||spec_pool[idx[t,k],:]||_1 + 1e-5)   (:1657-1660) */
int knnsvc_amp_ratio(const float* spec_q, int32_t ld_q, const float* spec_pool, int32_t ld_pool, int64_t np,
                     const int64_t* idx, int64_t nq, int32_t k, int32_t bins, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * f0 front end.  The reference runs pyworld.harvest(f0_floor 65, f0_ceil 1047, frame period 20 ms) and
 * zeroes values below 80 Hz when no `<stem>_f0.npy` exists (ddsp_prematch_dataset.py:121-128, 376-379).
 * ------------------------------------------------------------------------------------------ */
/* Harvest (M. Morise, Interspeech 2017) — what pyworld.harvest computes where the reference calls it
 * (ddsp_prematch_dataset.py:121-128: fs = 16000, f0_floor = 65, f0_ceil = 1047, frame_period = 20 ms, then `f0[f0 < 80] = 0`;
 * :376-379 when `<stem>_f0.npy` is missing).  x: [L] fp32 at 16 kHz on the device; f0: [n_frames] fp32,
 * n_frames = (int)(1000 L / fs / frame_period) + 1, 0 = unvoiced.  All stages run in fp64 on `stream` inside `workspace`
 * (256-byte aligned device memory of at least the size knnsvc_f0_harvest_workspace reports: ~35 MB per second of audio);
 * no host synchronisation.  status (device int32, may be NULL): 0, or a bit mask if a fixed-capacity list overflowed
 * (1: more than 16 candidates in a frame, 2 / 4: section storage) — the track is then incomplete.
 * Both entries serve 64.59286 <= f0_floor < f0_ceil <= 1600 (below that floor the longest band-pass filter does not fit the
 * bank kernel's tile: "f0_floor too low"), frame_period >= 1 ms, 1600 <= L < 2^30.
 * Restates the published algorithm, pinned by oracle/f0_ref.py on the reference's two shipped harvest tracks. */
int knnsvc_f0_harvest_workspace(int64_t L, int32_t sample_rate, float f0_floor, float f0_ceil, float frame_period,
                                int64_t* n_frames, int64_t* bytes);
int knnsvc_f0_harvest(const float* x, int64_t L, int32_t sample_rate, float f0_floor, float f0_ceil, float frame_period,
                      float zero_below, float* f0, int64_t n_frames, void* workspace, int64_t workspace_bytes,
                      int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC container (HOST functions: plain pointers into host memory, no stream, no GPU).  The reference reads .flac through
 * torchaudio.load (ddsp_prematch_dataset.py:332; its prematch builder globs *.wav and *.flac, :1469-1473) and writes .flac
 * through pydub / ffmpeg (lib_ongaku_test.py:122-143).  RFC 9639; every frame's CRC-8 / CRC-16 is verified while decoding.
 * ------------------------------------------------------------------------------------------ */
/* STREAMINFO of a FLAC file image: sample rate, channels, bits per sample, samples per channel, MD5 of the PCM (16 bytes, may be NULL) */
int knnsvc_flac_info(const uint8_t* data, int64_t size, int32_t* sample_rate, int32_t* channels, int32_t* bits,
                     int64_t* total_samples, uint8_t* md5);
/* decode into out[channels][capacity] (planar, sign-extended to int32); *decoded = samples per channel */
int knnsvc_flac_decode(const uint8_t* data, int64_t size, int32_t* out, int64_t capacity, int64_t* decoded);
/* encode pcm[channels][n] (`bits`-bit signed samples in int32; bits in {8, 12, 16, 20, 24}) with fixed predictors + Rice coding,
 * block size 4096; md5: 16 bytes for STREAMINFO or NULL (= unknown); *size = bytes written to out (capacity: 5 n channels + 8192 is safe) */
int knnsvc_flac_encode(const int32_t* pcm, int32_t channels, int64_t n, int32_t bits, int32_t sample_rate, const uint8_t* md5,
                       uint8_t* out, int64_t capacity, int64_t* size);

/* ------------------------------------------------------------------------------------------
 * Pool side features and the additive synthesiser.
 * ------------------------------------------------------------------------------------------ */
/* reflect-pad by `pad` samples each side (torch.stft center=True) : out[n + 2*pad] */
int knnsvc_reflect_pad(const float* x, int64_t n, int32_t pad, float* out, void* stream);
/* the same for a batch of signals packed back to back: item b = x[offs[b] .. offs[b+1]) (offs: device int64 [batches+1]) ->
 * row b of out [batches, stride], zero from n_b + 2*pad on.  One launch per pool instead of one per file
 * (ddsp_prematch_dataset.py:361 runs torchaudio's Spectrogram file by file). */
int knnsvc_reflect_pad_batch(const float* x, const int64_t* offs, int32_t batches, int32_t pad, float* out, int64_t stride,
                             void* stream);
/* knnsvc_complex_mag + knnsvc_harmonic_amps in one pass over the DFT product (ddsp_prematch_dataset.py:361, 391-404):
 * reim [rows, ld >= 2*bins], f0 [rows] -> spec [rows, bins], harm [rows, n_harm]; results identical to the two calls. */
int knnsvc_spec_harm(const float* reim, int64_t rows, int32_t bins, int32_t ld, const float* f0, int32_t n_harm,
                     float* spec, float* harm, void* stream);
/* |re + i im| of a [rows, 2*bins] (cos block | sin block) DFT product -> [rows, bins] */
int knnsvc_complex_mag(const float* reim, int64_t rows, int32_t bins, int32_t ld, float* out, void* stream);
/* harmonic amplitudes (ddsp_prematch_dataset.py:391-404): spec [T,200], f0 [T] -> harm [T,49] */
int knnsvc_harmonic_amps(const float* spec, const float* f0, int64_t T, int32_t bins, int32_t n_harm,
                         float* harm, void* stream);
/* get_bulk_dsp_choral (ddsp_prematch_dataset.py:165-208) fused with sin_prenet
 * (hifigan/ddsp_models.py:416,476): f0 [N], amp [N,H] -> cond [N*hop, n_ch] channel-last, and
 * optionally the raw excitation exc [N*hop].  mode 0 = additive (mix), 1 = plain sine of f0
 * (hifigan/ddsp_models_f0.py:348-356; amp ignored).  frame_phase: N doubles of workspace. */
/* n_dyn (may be NULL): DEVICE int32 — the valid frame count (<= N): amplitude taps clamp at frame n - 1 and samples past n * hop
 * are left alone, so a launch sized for a bucket of N frames reproduces the exact-length result (see knnsvc_conv_desc.n_dyn). */
int knnsvc_additive_synth(const float* f0, const float* amp, int64_t N, int32_t H, int32_t hop,
                          int32_t sample_rate, int32_t mode, const float* prenet_w, const float* prenet_b,
                          int32_t n_ch, float* cond, int32_t ld_cond, float* exc, double* frame_phase,
                          const int32_t* n_dyn, void* stream);

/* ------------------------------------------------------------------------------------------
 * Output loudness (csrc/loudness.hip).  The reference documents tgt_loudness_db as "float db used to normalize the output
 * volume" and does gain(prediction, tgt - torchaudio.functional.loudness(prediction)) (ddsp_matcher.py:533, 947; live in its
 * `match`, commented out in special_match :997-1003).
 * ------------------------------------------------------------------------------------------ */
/* Integrated loudness (LKFS) of a mono fp32 signal wav[0..n) on the device, after ITU-R BS.1770-4 with the constants and biquad
 * forms of torchaudio.functional.loudness:
 *   K-weighting  two biquads in cascade, direct form  y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2],  zero initial
 *                state, coefficients computed in fp64 and divided by a0, intermediate signals NOT clamped:
 *                high-shelf +4 dB at 1500 Hz, Q = 1/sqrt 2 (w0 = 2 pi 1500 / sr, A = 10^(4/40), alpha = sin w0 / (2Q),
 *                  b = [A((A+1)+(A-1)cos w0+2 sqrt(A) alpha), -2A((A-1)+(A+1)cos w0), A((A+1)+(A-1)cos w0-2 sqrt(A) alpha)],
 *                  a = [(A+1)-(A-1)cos w0+2 sqrt(A) alpha, 2((A-1)-(A+1)cos w0), (A+1)-(A-1)cos w0-2 sqrt(A) alpha]),  then
 *                high-pass at 38 Hz, Q = 0.5 (b = [(1+cos w0)/2, -(1+cos w0), (1+cos w0)/2], a = [1+alpha, -2 cos w0, 1-alpha]);
 *   blocks       G = 0.4 sr samples every S = G/4 (sample_rate must be a multiple of 10, 8000 .. 768000): nb = (n - G) / S + 1
 *                blocks when n >= G, else none (a trailing partial step is ignored);  e_j = mean(y^2) over block j,
 *                l_j = -0.691 + 10 log10 e_j;
 *   gating       keep l_j > -70;  Gamma = -0.691 + 10 log10(mean of the kept e_j) - 10;  keep l_j > Gamma as well;
 *                result = -0.691 + 10 log10(mean of the twice-kept e_j), -inf without blocks or when a gate leaves nothing.
 * All arithmetic between the samples and the result is fp64 in a fixed order (bit-stable from run to run).
 * lkfs: ONE device float.  counts (device int32 [3], may be NULL): blocks, blocks kept by the absolute gate, blocks kept by both.
 * n == 0 and n < G are valid; n may not exceed 2^36 samples (the block counts are int32; the functions below refuse more).
 * Two of the four launches are a single workgroup whose serial work per thread grows linearly with n (negligible for clips and
 * for hours of audio, see csrc/loudness.hip).  workspace: 8-byte aligned device memory of at least knnsvc_loudness_workspace_bytes(n, sample_rate)
 * bytes (a HOST function; 0 with knnsvc_last_error() set for n < 0 or a bad rate); a smaller one is refused before anything is
 * launched.  Asynchronous on `stream`, no allocation, no host synchronisation, capturable. */
size_t knnsvc_loudness_workspace_bytes(int64_t n, int32_t sample_rate);
/* HOST: the lengths at which the measure changes path: samples per lane (`chunk`; the filter state crosses these boundaries)
 * and samples per workgroup (`group`).  Tests take their edge lengths from here; either pointer may be NULL. */
void knnsvc_loudness_layout(int32_t* chunk, int32_t* group);
int knnsvc_loudness(const float* wav, int64_t n, int32_t sample_rate, float* lkfs, int32_t* counts, void* workspace,
                    size_t workspace_bytes, void* stream);
/* out[i] = wav[i] * g,  g = (float)10^((target_db - *lkfs) / 20) evaluated in fp64 on the device from the DEVICE float lkfs
 * (what knnsvc_loudness wrote); g = 1 when *lkfs is -inf, +inf or NaN (silence stays silence, a NaN waveform stays as it is for
 * the caller's finiteness check).  out may alias wav. */
int knnsvc_loudness_gain(float* wav, int64_t n, const float* lkfs, float target_db, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voice-activity trimming of pool recordings (csrc/vad.hip).  The reference documents vad_trigger_level on get_features
 * ("optionally perform VAD trimming on start/end", ddsp_matcher.py:438-491: torchaudio's Vad on the signal, then on the flipped
 * remainder, every cut extended to a whole number of 320-sample hops) and passes 7 for the target pool
 * (ddsp_prematch_dataset.py:1131), where get_complete_spk_pool drops it.
 * ------------------------------------------------------------------------------------------ */
/* Where speech starts and ends in each of n_seg mono fp32 recordings stacked in wav (recording s = wav[host_seg[s] ..
 * host_seg[s + 1]); host_seg_offsets is a HOST table as for the *_seg calls above, 1 <= n_seg <= KNNSVC_MAX_SEGMENTS).  The
 * algorithm is the sox `vad` effect with torchaudio's default parameters AS RESTATED HERE (and in fp64 numpy in
 * tests/vad_oracle.py); this restatement is the specification - parity with torchaudio's own code is not pinned.
 *   constants    (in brackets: at 16 kHz)  measure_len = int(sr 0.1 + .5) [1600];  dft_len = 16 doubled until >= measure_len [2048];
 *                period = int(sr / 20 + .5) [800];  spectrum bins [s0, s1): s0 = max(1, int(50 / sr dft_len + .5)) [6],
 *                s1 = min(int(6000 / sr dft_len + .5), dft_len / 2) [768];  cepstrum bins [c0, c1): c0 = ceil(sr / 2 / 2000) [4],
 *                c1 = min(floor(sr / 2 / 150), dft_len / 4) [53];  smooth = exp(-1/8), up = exp(-1/2), down = exp(-5),
 *                trig = exp(-1/5);  periodic Hann windows win[i] = 2 / sqrt(measure_len) (0.5 - 0.5 cos(2 pi i / measure_len)),
 *                cwin[i] = 2 / sqrt(s1 - s0) (0.5 - 0.5 cos(2 pi i / (s1 - s0))).
 *   measures     measurement m covers samples [m period, m period + measure_len): M = (L - measure_len) / period + 1 of them, none
 *                when L < measure_len.  With S = N = 0 before the first:  a_k = |rfft(win frame, zero-padded to dft_len)_k| for k
 *                in [s0, s1);  m < 6 (boot): b = m + 1, S = b/(1+b) S + 1/(1+b) a, d = S^2, N = d;  later: S = smooth S +
 *                (1 - smooth) a, d = S^2, N = mu N + (1 - mu) d with mu_k = up if d_k > N_k else down;  e = sqrt(max(0, d - 1.35 N));
 *                c = zeros(dft_len / 2), c[s0:s1] = e cwin;  r = sum over q in [c0, c1) of |rfft(c)_q|^2;
 *                meas_m = max(0, 21 + ln(r / (c1 - c0))) if r > 0 else 0.
 *   trigger      mean = trig mean + (1 - trig) meas_m from mean = 0; the first m with mean >= trigger_level fires.  Walk back over
 *                meas_m, meas_(m-1), ... for j = 0 .. 19 (before the recording: 0) from jT = jZ = 20:  meas >= level and
 *                j <= jT + 5: jZ = jT = j;  else meas == 0 and jT >= jZ: jZ = j.  start = max(0, m - min(20, jZ)) period; -1 when
 *                nothing fires.
 *   both ends    lstrip = start rounded up to a multiple of 320.  The same procedure on the time-reversed signal, over the
 *                measurements that fit in L - lstrip samples, gives rstrip (rounded up likewise).  The kept range is
 *                [lstrip, L - rstrip).  A recording that does not fire in one of the two directions, or whose kept range is shorter
 *                than measure_len, is dropped.
 * out_strip: device int64 [n_seg][2] = (lstrip, rstrip), (-1, -1) for a dropped recording.  out_measures (may be NULL): device
 * double [2][rows], rows = host_seg[n_seg] / period + 1: measure m of recording s is [host_seg[s] / period + m] of the forward half
 * and of the reversed half (all M of them, also those behind the trigger); the entries between recordings are not written.
 * sample_rate 8000 .. 20000 (the transform of dft_len <= 2048 points runs in LDS); trigger_level finite and > 0.  All arithmetic
 * between the samples and the cut points is fp64 in a fixed order: bit-stable from run to run, and a recording's result does not
 * depend on the others in the call.  workspace: 8-byte aligned device memory of at least
 * knnsvc_vad_workspace_bytes(host_seg[n_seg], n_seg, sample_rate) bytes (a HOST function; 0 with knnsvc_last_error() set for bad
 * arguments; about 2 x 762 doubles per 50 ms of audio at 16 kHz); a smaller one is refused before anything is launched.
 * Asynchronous on `stream`, no allocation, no host synchronisation, capturable. */
size_t knnsvc_vad_workspace_bytes(int64_t total_samples, int32_t n_seg, int32_t sample_rate);
int knnsvc_vad_trim_seg(const float* wav, const int64_t* host_seg_offsets, int32_t n_seg, int32_t sample_rate,
                        double trigger_level, int64_t* out_strip, double* out_measures, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Output dynamics (csrc/dynamics.hip): two stages behind the generator, both extensions without a counterpart in the reference.
 * Their place in the tail is fixed: generator -> envelope mix -> loudness normalisation -> peak ceiling -> finiteness check.
 * Both are restated in fp64 numpy in tests/dynamics_oracle.py; the text here is the specification.  All arithmetic between the
 * fp32 samples and the fp32 result is fp64 in a fixed order (bit-stable from run to run).  n may not exceed 2^36 samples.
 * ------------------------------------------------------------------------------------------ */
/* Envelope mix: the SHAPE of the source's volume envelope put back on the generated waveform y[0..n), n = T hop.  x[0..nx) is the
 * source as the encoder received it (16 kHz mono), zero-extended or cut to n samples; sample i of y corresponds to sample i of x.
 *   block energies   bx[j] = sum of x[i]^2, by[j] = sum of y[i]^2 over i in [j hop, (j + 1) hop), j = 0 .. T - 1; 0 outside that range
 *   frame RMS        rx[t] = sqrt((bx[t-1] + bx[t] + bx[t+1]) / (3 hop)), ry[t] likewise (the same divisor at the edges)
 *   global RMS       Rx = sqrt(sum of bx / n), Ry likewise.  Rx == 0, Ry == 0 or either not finite: out = y bit for bit, G = 1
 *   relative         px[t] = max(rx[t] / Rx, 1e-3), py[t] = max(ry[t] / Ry, 1e-3)          (floor: 60 dB under the average level)
 *   frame gain       G[t] = min((px[t] / py[t])^a, 4)                                      (cap: +12 dB)
 *   sample gain      linear between frame centres: p = (i - hop/2) / hop, t0 = clamp(floor p, 0, T-1), t1 = min(t0 + 1, T-1),
 *                    f = clamp(p - t0, 0, 1), g[i] = G[t0] + f (G[t1] - G[t0]); constant before the first and after the last centre
 *   result           out[i] = (float)(y[i] g[i]), rounded once.
 * The division by the global RMS is deliberate: the envelope's shape is transferred, not the recording level (a source recorded
 * 20 dB low gives the same result).  a in [0, 1] (0: G = 1).  hop: a positive multiple of 64, at most 1024; n a multiple of hop;
 * anything else is KNNSVC_EINVAL before a launch.  x may be NULL when nx == 0.  gains (may be NULL): T device doubles, receives G.
 * out may be y itself (no other overlap).  workspace: 8-byte aligned device memory of at least
 * knnsvc_envelope_workspace_bytes(n, hop) bytes (a HOST function; 0 with knnsvc_last_error() set for bad arguments); a smaller one
 * is refused before anything is launched.  Three launches, no floating-point atomics, asynchronous on `stream`, no allocation,
 * no host synchronisation, capturable. */
size_t knnsvc_envelope_workspace_bytes(int64_t n, int32_t hop);
int knnsvc_envelope_mix(const float* y, int64_t n, const float* x, int64_t nx, int32_t hop, double a, float* out, double* gains,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Peak ceiling: a look-ahead limiter without recursion on SAMPLE peaks (true-peak, i.e. oversampled, limiting is out of scope:
 * the reconstructed signal between two samples may pass the ceiling).  It does not bring the loudness back: behind
 * knnsvc_loudness_gain the integrated loudness can end below the target; the statistics say when the limiter engaged.
 *   constants        c = 10^(peak_db / 20), L = floor(0.005 sample_rate + 0.5)             (80 at 16 kHz)
 *   required gain    r[i] = c / |y[i]| where |y[i]| > c, else 1; 1 outside [0, n)
 *   sliding minimum  m[j] = min r[j - L .. j + L]
 *   weights          h[k] = (1 + cos(pi k / (L + 1))) / (2L + 2), k = -L .. L: a strictly positive Hann; the divisor is the sum
 *   smoothed gain    s[i] = 1 - sum over k ascending of h[k] (1 - m[i + k])
 *   result           out[i] = (float)(y[i] s[i]).
 * Ceiling: every m[i + k] is a minimum over a window that contains i, so s[i] <= r[i] and |out[i]| <= c (1 + 2^-23) after the
 * one fp32 rounding.  Identity: where nothing within 2L samples exceeds c, s[i] is exactly 1 and out[i] == y[i] bit for bit.
 * A NaN sample stays NaN, an infinite one becomes NaN (its r is 0): the caller's finiteness check still fires.
 * sample_rate 8000 .. 48000, peak_db finite and <= 0; anything else is KNNSVC_EINVAL before a launch.  stats (may be NULL): 16
 * bytes of 8-byte aligned device memory = { int64 number of samples with s < 1, double smallest s (1 when none) }, reset by the
 * call (integer atomics: order-independent).  out may be y itself (no other overlap); the aliased call runs ONE workgroup over
 * the tiles in order (a parallel launch could overwrite a neighbour's look-ahead samples before they are read), same bits,
 * slower.  One launch (two with stats), asynchronous on `stream`, no allocation, no host synchronisation, capturable. */
int knnsvc_peak_limit(const float* y, int64_t n, int32_t sample_rate, double peak_db, float* out, void* stats, void* stream);
/* HOST: samples per workgroup tile and L at 16 kHz; tests take their edge lengths from here; either pointer may be NULL. */
void knnsvc_peak_limit_layout(int32_t* tile, int32_t* lookahead_at_16k);
/* Mix of the voices of one output (the lead and its harmony parts; "Harmony voice"), between the per-voice half of the tail
 * (generator, envelope mix) and the per-output half (loudness, ceiling):
 *     out[i] = (float)( sum_v g_v * (double)y_v[i] )
 * over the voices in order.  Every product and every sum is an fp64 operation of its own (no contraction), the sum starts
 * with the first product that is read, the result is rounded once.  A voice whose gain is exactly 0 is NOT READ: a NaN in
 * it does not reach the output.  host_y: a HOST array of n_voices device pointers to n samples each; host_gains: HOST
 * double [n_voices], finite and >= 0, at least one > 0 (a caller in dB uses 10^(dB / 20)); both reach the kernel by value.
 * n_voices 1..KNNSVC_HARMONY_MAX_PARTS + 1.  out may be one of the inputs and may not overlap one otherwise.  One launch on
 * `stream` (four samples per thread; 16-byte accesses when out and every voice that is read are 16-byte aligned, else
 * scalar), enqueue only: no allocation, no synchronisation, capturable.  Anything else is KNNSVC_EINVAL before a launch. */
int knnsvc_mix_waves(const float* const* host_y, int32_t n_voices, const double* host_gains, int64_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KNNSVC_HIP_H */
