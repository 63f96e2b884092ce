/* diamond_hip.h -- C ABI of libdiamond_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for DIAMOND's imagined-rollout hot path.  The reference
 * (eloialonso/diamond) has no FFI: every op below replaces a chain of ATen calls issued by
 * the cited reference Python lines.  All pointers are DEVICE pointers (HBM) unless noted,
 * all floating-point tensors are fp32, activations are NHWC, every entry point is
 * asynchronous on the given hipStream_t, allocates nothing, synchronises nothing and is
 * graph-capturable.  Return value: 0 = launched, non-zero = invalid arguments (message via
 * dmd_last_error()).  No exceptions cross this boundary.
 */
#ifndef DIAMOND_HIP_H
#define DIAMOND_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dmd_stream_t; /* hipStream_t */

#define DMD_PROLOGUE_NONE 0      /* conv consumes the source as stored                       */
#define DMD_PROLOGUE_NORM_SILU 1 /* GroupNorm(+FiLM|affine) then SiLU fused into the load    */
#define DMD_PROLOGUE_NORM 2      /* GroupNorm(+affine) only (attention pre-norm)             */

#define DMD_GN_GROUP 32 /* models/blocks.py:12 GN_GROUP_SIZE */

/* GroupNorm statistics travel between kernels as per-tile partial sums in fp64:
 * stats[((n * G + g) * T + t) * 2 + {0: sum x, 1: sum x^2}], T = producer tiles per image.
 * The consumer reduces the T partials in a fixed order (deterministic).
 * Grouping rule (models/blocks.py:27,38): C channels form G = max(1, C / 32) groups of C / G channels -- 32 whenever
 * C % 32 == 0, else e.g. 16, 48, 40, 36 channels at C = 16, 48, 80, 144.  A normalised width must be C % 32 == 0, or
 * C <= 256 with C % 16 == 0, C % G == 0 and C / G a multiple of 4.  dmd_conv2d emits out_stats for Cout % 32 == 0 only
 * (other widths: dmd_gn_stats on its output).  dmd_conv2d_wgrad normalises the real channels [0, cin_real) of its source in
 * groups of that rule applied to cin_real where those differ from min(C, 32) channels of src.C (then: one whole group,
 * zero-padded to Cout = C = 64). */
typedef struct dmd_norm {
  const double* stats;   /* NULL <=> no normalisation                                  */
  int32_t stat_tiles;    /* T                                                          */
  int32_t mul_plus_one;  /* 1: y = xn * (1 + mul) + add  (AdaGroupNorm, blocks.py:41-45) */
                         /* 0: y = xn * mul + add        (nn.GroupNorm affine, :28-31)  */
  const float* mul;      /* [n * mul_stride + c]                                       */
  const float* add;      /* [n * add_stride + c]                                       */
  int64_t mul_stride;    /* 0 for per-channel parameters shared by the batch           */
  int64_t add_stride;
} dmd_norm;

typedef struct dmd_conv_src {
  const float* x;   /* NHWC (N, Hs, Ws, C) */
  int32_t C;        /* channels, multiple of 16 */
  int32_t prologue; /* DMD_PROLOGUE_* */
  dmd_norm norm;
} dmd_conv_src;

/* dmd_conv2d: 3x3 (pad 1, stride 1|2) or 1x1 convolution as an implicit GEMM on
 * v_mfma_f32_16x16x4_f32 (exact fp32 fma chain), with
 *   - channel concatenation of up to two sources       (torch.cat, blocks.py:174; inner_model.py:46)
 *   - nearest x2 upsampling folded into the gather      (Upsample.forward blocks.py:108-110)
 *   - GroupNorm/AdaGroupNorm + SiLU fused into the load (blocks.py:143-144; inner_model.py:48)
 *   - bias, residual add (optionally of the normalised residual, blocks.py:72) in the epilogue
 *   - GroupNorm partial statistics of the OUTPUT emitted by the epilogue.
 * Replaces F.conv2d call sites blocks.py:18-19,96,109,119,133-138 / inner_model.py:36,41. */
typedef struct dmd_conv_params {
  int32_t N, H, W;   /* batch and OUTPUT spatial size (H, W multiples of 8)            */
  int32_t Cout;      /* real output channels                                           */
  int32_t CoutPad;   /* Cout rounded up to 16/32/64-channel groups (weights are padded) */
  int32_t taps;      /* 9: 3x3 pad 1;  1: 1x1 pad 0                                    */
  int32_t stride;    /* 1 or 2 (taps == 9 only)                                        */
  int32_t upsample;  /* 1: sources stored at (H/2, W/2), nearest x2 before the conv    */
  int32_t nsrc;      /* 1 or 2                                                         */
  dmd_conv_src src[2];
  const float* w;    /* packed [Cin_total/16][taps][CoutPad][16]  (see dmd_pack_conv_weight) */
  const float* bias; /* [CoutPad] or NULL                                               */
  const float* residual; /* NHWC (N, H, W, Cout) or NULL                                */
  dmd_norm residual_norm; /* optional GroupNorm(+affine) applied to the residual        */
  float* out;        /* NHWC (N, H, W, Cout), or NCHW (N, Cout, H, W) if out_nchw       */
  int32_t out_nchw;
  int32_t precision; /* DMD_PRECISION_*: arithmetic of the contraction (see below)       */
  double* out_stats; /* (N, Cout/32, T, 2) partial sums of the output, or NULL          */
  const void* w_f16; /* dmd_pack_conv_weight_f16x2 layout, or NULL (needed for F16X2)    */
  /* Optional FUSED SKIP PROJECTION (ResBlock.forward, blocks.py:133,147: `self.proj(x) + conv2(...)` with
   * x = cat(x_up, skip)): a 1x1 convolution of proj_nsrc raw NHWC sources of the OUTPUT's N, H, W, accumulated into the
   * same fp32 accumulators as the 3x3 contraction -- the (N, H, W, Cout) projection is never written to or read from
   * HBM.  Honoured only where dmd_conv2d_proj_eligible() says so; dmd_conv2d fails loudly otherwise. */
  int32_t proj_nsrc;      /* 0: none; 2: two sources                                     */
  int32_t proj_C[2];      /* channels of each source                                     */
  int32_t proj_reserved;
  const float* proj_x[2]; /* NHWC (N, H, W, proj_C[i]), no prologue                      */
  const void* proj_w_f16; /* dmd_pack_conv_weight_f16x2(k = 1) of the (Cout, sum C, 1, 1) weights */
  const float* proj_bias; /* [Cout] or NULL                                              */
  /* VALID EXTENT (ABI v6).  The kernels tile in 8 / 16-pixel blocks; the reference's U-Net runs on any size that is a
   * multiple of 2^num_down (it pads to that and crops, blocks.py:227-229,247), e.g. 72x72 with levels 72/36/18/9.  Such a
   * tensor is stored inside a larger (N, H, W, C) buffer whose H, W satisfy the tiling rule, and (valid_h, valid_w) <= (H, W)
   * is the part that exists: conv-input positions outside the valid extent read as ZERO (like the convolution's own
   * padding, whatever the buffer holds there and before any fused normalisation), GroupNorm counts and the emitted
   * partial statistics cover the valid extent only.  Everything is still WRITTEN for the whole (H, W) buffer: positions
   * outside the valid extent hold unspecified values that no consumer reads unmasked.  The valid extent is the OUTPUT's;
   * a source's is (2 valid_h, 2 valid_w) at stride 2 and (valid_h / 2, valid_w / 2) under `upsample`.  0, 0 = (H, W). */
  int32_t valid_h, valid_w;
} dmd_conv_params;

/* DMD_PRECISION_F32:   v_mfma_f32_16x16x4_f32, bit-for-bit a k-ordered fp32 fma chain.
 * DMD_PRECISION_F16X2: fp32 operands split into two fp16 pieces each (x = h + l), three
 *   v_mfma_f32_32x32x16_f16 per product into an fp32 accumulator: fp32-class accuracy
 *   (representation error <= max(2^-22 |x|, 2^-25)), 16x the MFMA rate.  Range contract: finite operands must
 *   be inside the fp16 range (|x| < 65520); nothing is clamped, an operand beyond it makes every output it
 *   touches NaN (loud, never a silently wrong finite value), NaN / Inf inputs stay non-finite.  Honoured only
 *   where dmd_conv2d_f16x2_eligible() says so (3x3 / 1x1 stride 1, Cout in {32, 64}, Cin <= 128 / 64, NHWC
 *   out, or the few-channel NCHW head); everything else uses the exact kernel.
 *   GROUPNORM CONTRACT of that kernel (conv_f16ws_kernel; tests/test_groupnorm_precision.py walks its edges, measured table in
 *   profiles/groupnorm_precision.txt).  Everywhere else GroupNorm is (x - mean) * a + add on float64 sums.
 *   (1) Prologue: a normalised source is evaluated as fma(x, a, b), b = add - mean * a rounded to fp32, so every normalised
 *       value of a channel carries half an ulp of b: up to delta = 2^-24 (|mean| rstd |mul'| + |add|).  Up to |mean| rstd = 32
 *       (mean = 30 sigma included) that stays inside fp32-class accuracy of the output; a group CONSTANT at v != 0 (variance
 *       0, rstd = 316) is |mean| rstd = 316 |v|: its output is `add` only to 1.9e-5 |v mul'| (the (x - mean) * a paths give
 *       `add` exactly).  Measured on the MI355X at v = -3.25: 0.8 .. 1.6e-5 of the convolution's output scale, 0.2 .. 1.37 of
 *       the root-sum-square of delta through the weights; the tests allow 2 x that root-sum-square beyond the edge.
 *   (2) Epilogue: out_stats are float64 sums of fp32 partial sums -- of a lane's 16 outputs in the 16x16 geometries, of its
 *       32 .. 64 in the 8x8 and fused-projection ones (at the register cap) -- so the consumer's rstd is that of a mean square
 *       rounded once to fp32: off by up to 2^-24 (1 + r^2), r = |mean| / sigma of the output group (measured 0.27 of that:
 *       1.7e-5 at r = 30, 4e-6 at r = 15).  The next prologue holds its fp32-class bound up to r = 30 on the 16x16 and
 *       fused-projection geometries and up to r = 15 on the 8x8 ones; an output with a larger offset that needs float64
 *       statistics takes dmd_gn_stats of it instead. */
#define DMD_PRECISION_F32 0
#define DMD_PRECISION_F16X2 1
int dmd_conv2d_f16x2_eligible(const dmd_conv_params* p);
/* 1: dmd_conv2d can fuse the skip projection described by the proj_* fields into this launch (split-fp16 3x3 stride 1,
 * one 64-channel
 * source, Cout == 64, H, W multiples of 16, two 64-channel projection sources, no other residual) */
int dmd_conv2d_proj_eligible(const dmd_conv_params* p);
/* 1: dmd_conv2d runs these parameters on the streaming 1x1 kernel (exact fp32; taps == 1, Cout == 64, no
 * prologue / residual / statistics, Cin in {32, 64, 128}): blocks.py:120,133 skip projections */
int dmd_conv1x1_stream_eligible(const dmd_conv_params* p);
/* OIHW (Cout in {32, 64}, Cin, k, k) fp32, k in {1, 3} -> [CinPad/16][k*k][h|l][2][Cout][8] fp16 pieces */
int dmd_pack_conv_weight_f16x2(const float* oihw, void* packed, int Cout, int Cin, int k, int CinPad, dmd_stream_t stream);

/* Every kernel-layout copy of a model's convolution parameters in ONE launch (a training step changes all of them:
 * trainer.py:366-388).  A job = one copy; the table lives in DEVICE memory and is reusable as long as the pointers are.
 *   kind DMD_PACK_F32   : dmd_pack_conv_weight's layout        kind DMD_PACK_F16X2: dmd_pack_conv_weight_f16x2's
 *   kind DMD_PACK_BIAS  : (CoutPad) fp32 <- bias (Cout), zero beyond
 *   transposed = 1      : the weight of the data-gradient convolution restricted to input channels [c0, c1):
 *                         W'[ci - c0][co][ky][kx] = W[co][ci][k-1-ky][k-1-kx]; CoutPad / CinPad then refer to W'
 *                         (outputs c1 - c0, inputs Cout zero-padded to CinPad).
 * max_elems = the largest job's element count (fp32: CinPad * taps * CoutPad, f16x2: CinPad * taps * CoutPad, bias: CoutPad). */
#define DMD_PACK_F32 0
#define DMD_PACK_F16X2 1
#define DMD_PACK_BIAS 2
typedef struct dmd_pack_job {
  const float* src;      /* OIHW (Cout, Cin, k, k) fp32, or the bias (Cout) */
  void* dst;
  int32_t Cout, Cin, k;  /* of src */
  int32_t kind, transposed, c0, c1;
  int32_t CoutPad, CinPad; /* of the packed (possibly transposed) weight */
  int32_t reserved;
} dmd_pack_job;
int dmd_pack_jobs(const dmd_pack_job* jobs_device, int njobs, int64_t max_elems, dmd_stream_t stream);

/* ABI v9: fingerprints of parameter storage, for the always-on audit of the packed copies (engine.WeightAudit): a copy is keyed on
 * the parameter's version counter and storage pointer, and a write that changes neither (`p.data.copy_`, a collective on
 * `.data`) must not go unnoticed.  out[j * DMD_CHECKSUM_PARTS + b] = the sum, in 64 bits, of the 32-bit words w of jobs[j].src
 * (as signed integers) with (w / 256) % DMD_CHECKSUM_PARTS == b: exact and independent of the launch.  No reference
 * counterpart (torch keeps no second copy of a parameter: F.conv2d reads the parameter itself, /root/reference/src/models/blocks.py:18-31). */
#define DMD_CHECKSUM_PARTS 8
typedef struct dmd_checksum_job {
  const void* src;
  int64_t words; /* 32-bit words */
} dmd_checksum_job;
int dmd_checksums(const dmd_checksum_job* jobs_device, int njobs, long long* out_device, dmd_stream_t stream);

int dmd_conv2d(const dmd_conv_params* p, dmd_stream_t stream);
/* name of the kernel instantiation dmd_conv2d launches for these parameters, spelled like rocprofv3's kernel trace
 * (e.g. "conv_f16ws_kernel<WsGeom<false, 2, 9>>"): measurement plumbing for bench.py / profiles */
int dmd_conv2d_kernel_name(const dmd_conv_params* p, char* buf, int buf_len);
/* number of GroupNorm stat tiles per image a dmd_conv2d with output (H, W) emits */
int dmd_conv_stat_tiles(int H, int W);
/* OIHW (Cout, Cin, k, k) fp32 -> packed layout; Cin padded to 16, Cout padded to CoutPad. */
int dmd_pack_conv_weight(const float* oihw, float* packed, int Cout, int Cin, int k, int CoutPad, int CinPad,
                         dmd_stream_t stream);

/* Debug/verification twin of dmd_conv2d: one thread per output element, plain fp32 fma
 * loops, identical parameters and semantics (used by tests to localise MFMA-path bugs). */
int dmd_conv2d_naive(const dmd_conv_params* p, dmd_stream_t stream);

/* dmd_linear: C[M,N] (+)= A[M,K] . W[N,K]^T + bias[N], optional SiLU.  nn.Linear call sites:
 * AdaGroupNorm.linear blocks.py:39,44 (all of a forward batched into one call), cond_proj
 * inner_model.py:31-35, LSTM gates, actor/critic heads actor_critic.py:47-48,73. */
typedef struct dmd_linear_params {
  int32_t M, N, K;   /* any K > 0; K % 16 == 0 with K-contiguous 16-byte-aligned rows: the 16-byte-load kernel */
  const float* A; int64_t lda;
  const float* W; int64_t ldw;
  const float* bias; /* [N] or NULL */
  float* C; int64_t ldc;
  int32_t accumulate; /* 1: C += ... */
  int32_t silu;       /* 1: C = silu(...) */
  /* Operands in either storage order (the backward's data / weight gradient GEMMs): trans_a = 1: A is given as (K, M) row-major,
   * lda = the stride between its K rows; trans_w = 1: W is given as (K, N) row-major likewise.  The instance that reads them also
   * runs K-contiguous operands whose K is no multiple of 16 (the tail is masked: exact zeros), whose lda / ldw is no multiple
   * of 4, or whose A / W pointer is not 16-byte aligned (any 4-byte-aligned pointer is a legal operand: the host looks at the
   * pointers, the 16-byte loads are never issued on a misaligned row).  The result is BITWISE the plain call on aligned
   * K-contiguous copies zero-padded to K rounded up to 16: same 16-wide steps, same four MFMAs per step, and the split-K route
   * is chosen by the rounded K: Kp >= 512 and Kp % 64 == 0 split (four K quarters, summed ((w0 + w1) + w2) + w3); every other K
   * -- 496, 528, 608, 1008 among them -- is ONE chain of Kp and on the interpreter about 2x less accurate than K = 512
   * (profiles/linear_precision.txt).  A weight gradient whose K = (T - 1) * B falls there; moving the rule changes bits. */
  int32_t trans_a, trans_w;
} dmd_linear_params;
int dmd_linear(const dmd_linear_params* p, dmd_stream_t stream);

/* dmd_attention: softmax(q k^T / sqrt(d)) v per (image, head) over T tokens (T % 64 == 0), K / V tiles of 256 keys staged in
 * LDS.  qkv is NHWC (N, T, 3C): q | k | v channel thirds, head h = channels [h*d, (h+1)*d) of each third (blocks.py:66-71).
 * d == 8.  Which kernel runs depends on T alone:
 *   T % 256 != 0 (64, 192, 320 ...: the 8x8 level)   attention_kernel: fp32 operands on the fp32 MFMAs, online softmax (running
 *       maximum, rescale per 16-key block).  IEEE fp32 throughout: full fp32 range, no floor; NaN / +-Inf operands give what an
 *       fp32 evaluation of the formula gives.
 *   T % 256 == 0 (256 = the default denoiser's 16x16 level, 1024 / 4096 = the 256x256 configuration)   attention_f16x2_kernel:
 *       SPLIT-fp16 operands on the f16 MFMAs in TWO passes over the keys (row maxima, then weights / sums / PV).  The forward of
 *       the TRAINING step takes it too, so by default the attention backward differentiates around a split-fp16 y.
 *       dmd_attention_valid never takes it.
 * The precision switch is the CALLER's: dmd_attention itself keeps choosing by T alone.  DIAMOND_CONV_PRECISION=f32 does not reach
 * attention; DIAMOND_ATTN_PRECISION=f32 (engine.attention's `precision`, the `attn_precision` keyword of the denoiser's inference
 * and training paths) does: every attention core then runs on exact fp32 operands -- dmd_attention_f32 below from
 * ATTN_F32_TILED_MIN_T valid tokens on, attention_kernel (through dmd_attention_valid) below that -- and the training backward
 * differentiates around that exact y.  Reference-width arithmetic needs BOTH switches.  (The 8x8 dmd_lowres_chain / chain32
 * launches carry their own attention core, which is on fp32 operands already.)
 * PRECISION CONTRACT of the two-pass kernel (tests/test_attention_precision.py walks its edges; measured table in
 * profiles/attention_precision.txt):
 *   * operands: k, v and q' = q * log2(e) / sqrt(d) are each held as two fp16 pieces x = h + l: off by at most
 *     max(2^-22 |x|, 2^-25).  The relative part applies from |x| >= 2^-3 on; below, the ABSOLUTE floor 2^-25 does.  Scores keep the
 *     three products q'_h k_h + q'_h k_l + q'_l k_h in fp32: their error is about 2^-22 sum_i |q'_i k_i| (it scales with the
 *     products' magnitudes, not with the score differences), plus 2^-25 sum_i |k_i| once q' is below 2^-3 and 2^-25 sum_i |q'_i|
 *     once k is.  When EVERY q' of a workgroup's 256 queries is below 2^-3, the kernel multiplies them by the power of two that
 *     brings the largest into [1, 2) and its copy of the keys by the inverse (exact; the factor is 1 otherwise and no bit
 *     changes), so tiny queries against keys near 65504 keep the relative error.  Within about 4x of an fp32 evaluation of the
 *     formula on every input family of the test file.  v far below 2^-3 is NOT rebalanced: outputs are off by up to 2^-24
 *     absolute whatever their size (scale v up by a power of two first).
 *   * range: up to the end of fp16 (65504) for k, v and q'.  NOTHING IS CLAMPED: a finite operand beyond it is LOUD and
 *     CONFINED: the split gives h = +-Inf, l = -+Inf, so a k element makes every output of its (image, head) NaN, a q element
 *     every output of its query row, a v element every output of its dim in its (image, head); every other output keeps its
 *     bits.  Never finite and wrong.  NaN and +-Inf operands give the non-finite pattern of an fp32 evaluation: an infinite k
 *     element is held as h = 0, l = +-Inf, so its key drops out of the rows whose score against it is -Inf and makes the rows
 *     NaN whose score is +Inf (or 0 * Inf).
 *   * weights: p = 2^(s - max + 13) as two fp16 pieces, divided by their fp32 sum: a weight below 2^-38 of its row's largest is
 *     dropped (pieces stop at 2^-25 of 2^13), each weight is off by at most 2^-22 of itself or 2^-38 of the largest. */
int dmd_attention(const float* qkv, float* out, int N, int T, int C, int head_dim, dmd_stream_t stream);
/* ... over an (H, W) token grid of which only (valid_h, valid_w) exists (see dmd_conv_params: VALID EXTENT): keys outside it
 * do not take part in the softmax; outputs of queries outside it are unspecified */
int dmd_attention_valid(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                        dmd_stream_t stream);
/* (ABI v11 addition) The exact forward for long token grids: attention_f32_tiled_kernel, exact fp32 operands on
 * v_mfma_f32_16x16x4_f32, fp32 throughout (IEEE arithmetic; the exponential is v_exp_f32, about 1 ulp), TWO passes over the keys (row maximum of the raw q . k, then
 * p = 2^((q . k - m) log2(e) / sqrt(d)), row sum, O += P V; out = O / l), K / V tiles of 256 keys double-buffered in LDS, no online
 * rescale, no atomics: run-to-run bitwise, and an (image, head)'s output does not depend on N or on the other heads.
 * Extent convention of dmd_attention_bwd_mfma: tokens are addressed by their valid index li <-> (li / valid_w) * W + li % valid_w,
 * the work is sized by valid_h * valid_w, nothing outside the extent is read (the margins of qkv may hold anything, NaN / Inf
 * included) and the rows of `out` outside the extent are written as +0.  The full grid of T tokens is H = 1, W = T,
 * valid = (1, T); the whole-grid call (H, W, H, W) is bitwise that one.  Any valid token count >= 1 (no T % 64 condition).  d == 8.
 * PRECISION CONTRACT, beside the two-pass split kernel's above: operands are the fp32 numbers themselves -- the full fp32 range,
 * no floor, no rebalancing; a finite operand beyond 65504 is simply computed; NaN / +-Inf operands give what an fp32 evaluation of
 * the formula gives (a key whose score is -Inf drops out of its row; +Inf or NaN scores make their row NaN; a non-finite v element
 * stays in its dim).  Error against float64 within K_TILED x that of a float32 CPU evaluation per (image, head)
 * (tests/test_attention_f32_tiled.py, profiles/attention_f32_tiled_precision.txt); differs from attention_kernel in rounding only. */
int dmd_attention_f32(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                      dmd_stream_t stream);
/* (ABI v11 addition) The split-fp16 two-pass kernel (attention_f16x2_kernel, dmd_attention's at T % 256 == 0) over ANY valid
 * extent: arguments, checks and extent convention are dmd_attention_f32's -- tokens addressed by their valid index, the work sized
 * by valid_h * valid_w (ceil(tv / 256) workgroups per (image, head), as many key tiles), any valid token count >= 1, nothing outside
 * the extent read (the margins of qkv may hold anything, NaN / Inf included), the rows of `out` outside the extent written as +0.
 * Whole key tiles run dmd_attention's inner loops; only a partial last tile is masked: its keys behind the extent are staged as
 * zeros, their scores are REPLACED by -inf in both passes (a selection: a zero key against an infinite query makes no NaN) and they
 * add exactly 0 to the row sum and to the output.  Asynchronous, allocates nothing, graph-capturable.  What engine.attention calls
 * in default precision for valid extents and for whole grids with T % 256 != 0, from ATTN_F16X2_EXTENT_MIN_T valid tokens on
 * (DIAMOND_ATTN_F16X2_MIN_T); dmd_attention and dmd_attention_valid keep their routing and their bits.
 * PRECISION CONTRACT: the two-pass kernel's above, per (query, key) pair -- the same split operands, products, weights, range and
 * non-finite behaviour.  REBALANCING is decided per workgroup of 256 queries IN VALID-INDEX ORDER (queries 256 b .. 256 b + 255 of
 * the extent, the last workgroup's over its valid queries only).  Bitwise: the extent (1, T, 1, T) with T % 256 == 0 is
 * dmd_attention; (H, W, vh, vw) is the flat call (1, tv, 1, tv) on the compacted tokens; run-to-run equal; an (image, head)'s output
 * does not depend on N or on the other heads.  d == 8. */
int dmd_attention_f16x2(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                        dmd_stream_t stream);
/* Backward of dmd_attention (autograd of blocks.py:66-71 under the denoiser training loss, denoiser.py:93-122):
 * y = the forward's output, dy its gradient -> dqkv (N, T, 3C) in the qkv layout.  workspace: dmd_attention_bwd_workspace_floats.
 * Any T > 0.  dmd_attention_bwd and dmd_attention_bwd_valid launch ONE pair of scalar kernels (attention_bwd_rows_kernel,
 * attention_bwd_cols_kernel, one thread per valid token): the whole grid of T tokens is the extent (1, T, 1, T) of a (1, T) grid. */
int64_t dmd_attention_bwd_workspace_floats(int N, int T, int C);
int dmd_attention_bwd(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int T, int C,
                      int head_dim, dmd_stream_t stream);
/* (ABI v11 addition) Backward of dmd_attention_valid over the (valid_h, valid_w) part of an (H, W) token grid (dmd_conv_params:
 * VALID EXTENT): only tokens with row < valid_h and column < valid_w take part, as queries and as keys, and nothing outside the
 * extent is read -- the margins of qkv, y and dy may hold anything, NaN / Inf included.  The dqkv rows outside the extent are
 * written as ZERO in all three thirds.  The work is sized by the valid token count; every way of writing the same
 * tokens -- (H, W, H, W), (1, H W, 1, H W), dmd_attention_bwd(N, H W) -- gives bitwise the same result (same kernels, same summation
 * order).  workspace: dmd_attention_bwd_workspace_floats(N, H * W, C). */
int dmd_attention_bwd_valid(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int H, int W,
                            int valid_h, int valid_w, int C, int head_dim, dmd_stream_t stream);
/* (ABI v11 addition) The same gradient on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 operands), for long token
 * grids: two tiled kernels of 64 queries (64 keys) per workgroup that stream the other side in LDS tiles of 256 tokens, two
 * passes over the keys for the row maximum and the weights, no atomics, every sum in a fixed order (run-to-run bitwise).
 * Arguments, extent convention, margins (never read; dqkv written as ZERO there) and workspace size are dmd_attention_bwd_valid's;
 * the full grid of T tokens is H = 1, W = T, valid = (1, T), and the whole-grid call (H, W, H, W) is bitwise that one.  The
 * result differs from dmd_attention_bwd's in rounding only (weights by exp2 of the fp32 score difference; same error against
 * float64: profiles/attention_bwd_mfma_precision.txt).  Any valid token count >= 1. */
int dmd_attention_bwd_mfma(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int H, int W,
                           int valid_h, int valid_w, int C, int head_dim, dmd_stream_t stream);

/* ---- dmd_lowres_chain: a whole chain of ResBlocks at the 8x8 level of the denoiser's U-Net in ONE launch ----
 * Replaces, for H = W = 8 and 64 channels, the launches of the deepest level of UNet.forward (reference blocks.py:232-246:
 * d_blocks[-1], mid_blocks, u_blocks[0]) -- per ResBlock (blocks.py:141-147): optional 1x1 `proj` of the raw (concatenated)
 * input, conv1(SiLU(AdaGN1(cat(x, skip)))), conv2(SiLU(AdaGN2(h))) + r, optional SelfAttention2d (blocks.py:62-72).
 * One workgroup per image keeps every activation of the chain in LDS (64 pixels x 64 channels = 16 KiB per tensor); the
 * convolutions use the split-fp16 MFMA arithmetic of dmd_conv2d's DMD_PRECISION_F16X2 path and the same packed weights
 * (dmd_pack_conv_weight_f16x2).  At batch 256 these launches are latency chains of ~25 us each for 1.2 GFLOP. */
#define DMD_CHAIN_MAX_BLOCKS 8
typedef struct dmd_chain_block {
  int32_t skip_slot;    /* -1: the block's input is x;  0..2: cat(x, saved[skip_slot]) (128 input channels)            */
  int32_t save_slot;    /* -1, or 0..2: keep the block's OUTPUT in this slot for a later concatenation                  */
  int32_t film1_mul[2]; /* FiLM-table column of AdaGN1's `scale` for the x part / the skip part                          */
  int32_t film1_add[2]; /* ... of `shift`                                                                                */
  int32_t film2_mul, film2_add;
  int32_t has_attn, reserved;
  const void* w1;       /* conv1 3x3, Cin 64 | 128 -> 64, dmd_pack_conv_weight_f16x2 layout                              */
  const void* w2;       /* conv2 3x3, 64 -> 64                                                                           */
  const void* wproj;    /* 1x1 128 -> 64 (f16x2 pack) or NULL (identity skip)                                            */
  const float* b1;      /* (64)                                                                                          */
  const float* b2;      /* (64)                                                                                          */
  const float* bproj;   /* (64) or NULL                                                                                  */
  const float* gn_gamma; /* attention: nn.GroupNorm affine (64), (64)                                                    */
  const float* gn_beta;
  const void* wq;       /* attention: 1x1 64 -> 64 packs of the q | k | v thirds of qkv_proj and of out_proj             */
  const void* wk;
  const void* wv;
  const void* wo;
  const float* bqkv;    /* (192) */
  const float* bo;      /* (64)  */
} dmd_chain_block;

typedef struct dmd_lowres_chain_params {
  int32_t N;                 /* images                                                            */
  int32_t nblocks;           /* <= DMD_CHAIN_MAX_BLOCKS                                           */
  int32_t input_save_slot;   /* -1, or the slot that keeps the chain INPUT for a later concatenation */
  int32_t reserved;
  const float* x;            /* NHWC (N, 8, 8, 64)                                                */
  float* out;                /* NHWC (N, 8, 8, 64)                                                */
  const float* table;        /* FiLM table (N, table_stride): every AdaGroupNorm.linear(cond) of the network, concatenated */
  int64_t table_stride;
  dmd_chain_block blocks[DMD_CHAIN_MAX_BLOCKS];
} dmd_lowres_chain_params;
int dmd_lowres_chain(const dmd_lowres_chain_params* p, dmd_stream_t stream);
/* The same for the 8x8 x 32-channel tail of the reward / end model's encoder (reference rew_end_model.py:93-133: the last
 * level's ResBlocks and the final attention ResBlocks; no concatenated inputs): x / out are NHWC (N, 8, 8, 32), packs are the
 * 32-cout form of dmd_pack_conv_weight_f16x2, q | k | v are 32-channel thirds (4 heads). */
int dmd_lowres_chain32(const dmd_lowres_chain_params* p, dmd_stream_t stream);

/* ---- EDM preconditioning / sampler pointwise (denoiser.py:74-84, diffusion_sampler.py:45-56) ---- */
/* The four EDM conditioners (c_in, c_out, c_skip, c_noise; compute_conditioners denoiser.py:66-72)
 * are four scalars per sample: the host evaluates them with the reference's own fp32 op order
 * (bit-exact; v_sqrt_f32 is not correctly rounded) and hands them over as a device array
 * cond[n * cond_stride + {0: c_in, 1: c_out, 2: c_skip, 3: c_noise}], cond_stride in {0, 4}. */

/* cat(obs / sigma_data, x * c_in) -> NHWC with CPad channels (zero padded).
 * x (N, Cx, H, W), obs (N, Cobs, H, W) NCHW.  obs may be a RING of T conditioning frames (N, T, Cobs / T, H, W):
 * logical frame t is stored at slot (head + t) % T, so that WorldModelEnv.step never rolls its context
 * (world_model_env.py:74-75).  T = 1, head = 0: plain tensor. */
int dmd_edm_pack_input(const float* x, const float* obs, const float* cond, int cond_stride, float sigma_data,
                       float* out_nhwc, int N, int Cx, int Cobs, int H, int W, int CPad, int T, int head,
                       dmd_stream_t stream);
/* cond input: fourier(c_noise) + flatten(embedding(act))  (blocks.py:84-87, inner_model.py:27-30,45);
 * act is a ring of T actions per sample starting at act_head (0: plain (N, T) tensor); A = rows of act_emb
 * (indices are clamped to [0, A) for memory safety -- validating them is the caller's job) */
int dmd_cond_embed(const float* cond, int cond_stride, const float* fourier_w /*[half]*/,
                   const int64_t* act /*(N, T)*/, const float* act_emb /*(A, E)*/, float* out /*(N, 2*half)*/, int N,
                   int half, int T, int E, int act_head, int A, dmd_stream_t stream);
/* denoised = quantise(c_skip * x + c_out * F)  (denoiser.py:81-83); all NCHW, elementwise */
int dmd_edm_denoised(const float* x, const float* model_out, const float* cond, int cond_stride,
                     float* denoised, int N, int64_t per_sample, dmd_stream_t stream);
/* x_out = x + ((x - denoised) / sigma_hat) * dt   (diffusion_sampler.py:45-49) */
int dmd_euler_step(const float* x, const float* denoised, float sigma_hat, float dt, float* x_out, int64_t n,
                   dmd_stream_t stream);
/* Heun combine, diffusion_sampler.py:52-56: d = (x - D) / sigma_hat, d_2 = (x_2 - D_2) / sigma_next,
 * x_out = x + ((d + d_2) / 2) * dt   (same fp32 op order as the reference) */
int dmd_heun_step(const float* x, const float* denoised, const float* x_2, const float* denoised_2, float sigma_hat,
                  float sigma_next, float dt, float* x_out, int64_t n, dmd_stream_t stream);

/* ---- device-resident uint8 pool of initial conditions (world_model_env.py:107-139; frames are uint8 on disk,
 *      data/episode.py:36-50, and `x.div(255).mul(2).sub(1)` when loaded) ------------------------------------- */
/* q = round((x + 1) / 2 * 255); *off_grid (device int, zeroed by the caller) becomes 1 if some x is not exactly the
 * dequantisation of its level -- such a pool cannot be kept as uint8 without changing results. */
int dmd_quantize_u8(const float* x, uint8_t* q, int* off_grid, int64_t n, dmd_stream_t stream);
/* dst ring row rows[i] (NULL: i), slot (head + t) % T  <-  (pool[idx[i]][t] / 255) * 2 - 1   for i < M, t < T.
 * pool (P, T, per_frame) uint8, dst (B, T, per_frame) fp32, per_frame = C * H * W (multiple of 4). */
int dmd_dequant_gather(const uint8_t* pool, const int64_t* idx, const int64_t* rows, float* dst, int M, int T,
                       int64_t per_frame, int head, dmd_stream_t stream);
/* ABI v9: the rest of a reset (envs/world_model_env.py:56-62 `reset_dead`) in one launch, for i < count, r = rows[i], q = idx[i]:
 * act_ring[r][(head + t) % T] = pool_act[q][t] (int64 (B, T) / (P, T)); hx[r] = pool_hx[q], cx[r] = pool_cx[q] ((B, hd) / (P, hd)
 * fp32: the reward/end LSTM state); ep_len[r] = 0. */
int dmd_reset_state(const int64_t* idx, const int64_t* rows, int count, const int64_t* pool_act, int64_t* act_ring, int T, int head,
                    const float* pool_hx, const float* pool_cx, float* hx, float* cx, int hd, int64_t* ep_len, dmd_stream_t stream);

/* ---- ABI v11: the deaths of an imagined step resolved on the device -----------------------------------------------------
 * Replaces the reference's per-step host round trip `if dead.any(): reset_dead(dead)` (envs/world_model_env.py:77-83, :56-62) and
 * what coroutines/env_loop.py:45-56 does with its answer: the step works on K SLOTS chosen by the host BEFORE it knows the step's
 * deaths; dead rows take slots in ascending row order (the order of the reference's boolean masks and of its pool,
 * world_model_env.py:133-139), unused slots are -1, and the host reads `report` one step late.
 *   ep_len[r] += 1; trunc[r] = ep_len[r] >= horizon (:71-72); dead[r] = end[r] | trunc[r]; ep_len[r] = 0 where dead (:61)
 *   slot_row (K) int64: j-th dead row or -1;  row_slot (B) int32: slot of a dead row, -1 if alive (or no slot was left)
 *   report (B + 4) int32: dead[0..B), k = number of dead rows, rows with end != 0, k > K (slot overflow), K */
int dmd_resolve_deaths(const int64_t* end, int64_t* ep_len, int horizon, int64_t* trunc, uint8_t* dead, int B, int K,
                       int64_t* slot_row, int32_t* row_slot, int32_t* report, dmd_stream_t stream);

/* Ring advance (world_model_env.py:74-75, as a ring: the oldest slot receives the imagined frame), reset of the slots' rows
 * from pool rows pool_base + j (:56-62: context frames, actions, reward/end LSTM state), and the policy's next input
 * enc_in (B + T * K, per_frame) = [ newest frame of every env (a reset row: of its NEW episode)
 *                                  | final observation of slot j (env_loop.py:49)
 *                                  | burn-in frame t of slot j, frame-major, t < T - 1 (env_loop.py:53-56) ]
 * in one call (two launches).  head = the ring's head AFTER the advance.  A pool round: frames (P, T, per_frame) uint8 (dequantised
 * as dmd_dequant_gather does; pad (P, T) uint8, optional: frames that are exact zeros) or fp32 (is_f32), act (P, T) int64, hx / cx
 * (P, hd) fp32.  TWO rounds may be given: the reference drops the rest of a round and preloads the next one when a request does not
 * fit (world_model_env.py:133-139) -- a decision that depends on the step's number of deaths, which only the device knows at launch
 * time: with pool[1].frames and num_dead set, the slots are served from pool[1] rows 0.. iff pool_base + *num_dead > pool[0].rows.
 * Unused slots produce copies of row 0's imagined frame in enc_in and touch nothing else. */
typedef struct dmd_pool_round {
  const void* frames;
  const uint8_t* pad;
  const int64_t* act;
  const float* hx;
  const float* cx;
  int32_t is_f32, rows;
} dmd_pool_round;
typedef struct dmd_reset_slots_params {
  int32_t B, K, T, head;
  int64_t per_frame; /* C * H * W, a multiple of 4 */
  int32_t hd, reserved; /* hd: width of the reward/end LSTM state */
  dmd_pool_round pool[2];
  int64_t pool_base;       /* first row of pool[0] this step would be served from */
  const int32_t* num_dead; /* device: the step's number of dead rows (dmd_resolve_deaths' report + B); NULL with one round */
  const int64_t* slot_row; /* (K), from dmd_resolve_deaths */
  const int32_t* row_slot; /* (B) */
  const float* next_obs;   /* (B, per_frame): the imagined frames of this step */
  float* ctx;              /* (B, T, per_frame) context ring */
  int64_t* act_ring;       /* (B, T) */
  float* hx;               /* (B, hd) reward/end LSTM state */
  float* cx;
  float* enc_in;           /* (B + T * K, per_frame) */
} dmd_reset_slots_params;
int dmd_reset_slots(const dmd_reset_slots_params* p, dmd_stream_t stream);

/* ---- device-resident replay store: a whole (B, T) training batch gathered from a uint8 arena in ONE launch ---------------------
 * (additive to ABI v11.)  Replaces the reference's per-sample CPU pipeline (data/dataset.py:47-49 `__getitem__`,
 * data/utils.py:12-41 `make_segment` / `collate_segments_to_batch`, then an fp32 upload of the batch).
 * Arena (device): frames (F, per_frame) uint8 levels, act (F) int64, rew (F) fp32, end / trunc (F) uint8, the episodes' steps
 * back to back; finals (E, per_frame) uint8: the episodes' final observations (may be NULL when there are none).
 * seg (B, 4) int64 on the device, per sample: first = arena index of the episode's step 0, start = the segment's first step (may
 * be negative: left padding), len = the episode's length, final_row = row of `finals` or -1.
 * For sample b, position t, step s = start + t, valid = 0 <= s < len:
 *   valid:   out_obs[b][t] = (frames[first + s] / 255) * 2 - 1 (the bits of dmd_dequant_gather and of data/episode.py:36-43),
 *            out_act / out_rew / out_end / out_trunc [b][t] = the arena's values at first + s, out_mask[b][t] = 1
 *   invalid: exact zeros everywhere, nothing is read (never an out-of-range address), out_mask[b][t] = 0
 *   put_back_final != 0: at the one position with s == len, t >= 1, end[first + len - 1] != 0 and final_row >= 0, out_obs[b][t]
 *            is the dequantised final observation instead of zeros (where models/rew_end_model.py:65-69 writes it); the mask stays 0
 *   out_final[b] = dequantised finals[final_row], or zeros when final_row < 0.
 * Every out_* may be NULL (not written).  out_end / out_trunc hold flag_size-byte integers: 1 (uint8) or 8 (int64).
 * Any per_frame >= 1: 16-byte stores where per_frame % 4 == 0, frames / finals are 4-byte and out_obs / out_final 16-byte aligned
 * (16 levels per lane where per_frame % 16 == 0, else 4); one level per lane otherwise. */
typedef struct dmd_segment_gather_params {
  int32_t B, T;
  int64_t per_frame;       /* C * H * W */
  int32_t flag_size;       /* bytes per element of out_end / out_trunc: 1 or 8 */
  int32_t put_back_final;
  const uint8_t* frames;   /* (F, per_frame) */
  const int64_t* act;      /* (F) */
  const float* rew;        /* (F) */
  const uint8_t* end;      /* (F) */
  const uint8_t* trunc;    /* (F) */
  const uint8_t* finals;   /* (E, per_frame) or NULL */
  const int64_t* seg;      /* (B, 4): first, start, len, final_row */
  float* out_obs;          /* (B, T, per_frame) */
  int64_t* out_act;        /* (B, T) */
  float* out_rew;          /* (B, T) */
  void* out_end;           /* (B, T) of flag_size bytes */
  void* out_trunc;         /* (B, T) of flag_size bytes */
  uint8_t* out_mask;       /* (B, T): mask_padding */
  float* out_final;        /* (B, per_frame) */
} dmd_segment_gather_params;
int dmd_segment_gather(const dmd_segment_gather_params* p, dmd_stream_t stream);

/* ---- device-resident replay store: a window of env steps written INTO the arena in ONE launch ----------------------------------
 * (additive to ABI v11.)  Replaces the reference collector's path for collected steps (coroutines/collector.py:53-106: a host
 * Episode concatenated per step, the whole grown episode handed over again) -- the frames are on the device when the env loop
 * yields them.
 * Sources (device): obs (steps, per_frame) fp32 in [-1, 1], act (steps) int64, rew (steps) fp32, end / trunc (steps) integers of
 * flag_size bytes (1 or 8) -- the env loop's stacked (B, T, ...) tensors, steps = B * T, flattened index b * T + t -- and
 * final_obs (K, per_frame) fp32 (NULL with K == 0).  Destinations: the arena arrays of dmd_segment_gather, F rows, and finals, E rows.
 * runs (R, 4) int64 on the device, per run (kind, src, n, dst):
 *   kind 0   the n consecutive source steps src ... src + n - 1 (one env's: src = b * T + t0) -> arena rows dst ... dst + n - 1, all
 *            five fields: frames as levels, act and rew copied, end / trunc stored as (value != 0)
 *   kind 1   final_obs[src] -> finals[dst], as levels (n = 1)
 *   kind 2   arena rows src ... src + n - 1 -> arena rows dst ... dst + n - 1, all five fields, byte for byte (an episode that has
 *            outgrown its slot moves)
 * A level is clamp(rint((v + 1) / 2 * 255), 0, 255), dmd_quantize_u8's expression; *off_grid (int32, zeroed by the caller) becomes 1
 * when some value is not bitwise (level / 255) * 2 - 1, that kernel's rule, and is not written otherwise.
 * The caller guarantees: total == the sum of the runs' n; the source and destination rows of a kind-2 run do not overlap; no
 * destination row of the launch is another run's source or destination.  The entry checks what it can see on the host (below);
 * on the device a run with n < 1, an unknown kind, or rows outside steps / K / F / E is skipped whole: nothing outside the arrays
 * is read or written.
 * One workgroup per 256 x W levels of ONE frame (what it copies is uniform over it; the runs are read through scalar loads), the
 * five small fields in workgroups of their own: the launched work is proportional to `total`.  W = 16 where per_frame % 16 == 0
 * (four 16-byte fp32 loads 4 KiB apart in flight per lane, 4-byte packed stores), W = 4 where per_frame % 4 == 0 -- both need obs /
 * final_obs 16-byte and frames / finals 4-byte aligned --, one level per lane otherwise: any per_frame >= 1, any alignment.
 * R == 0 or total == 0 launches nothing and returns 0.  Refused (non-zero, dmd_last_error): a NULL array, runs or off_grid;
 * flag_size other than 1 or 8; K > 0 without final_obs or finals; negative R, total, steps, K, F or E; per_frame < 1; a grid
 * beyond one launch. */
typedef struct dmd_record_window_params {
  int32_t R;               /* runs */
  int32_t flag_size;       /* bytes per element of the source end / trunc: 1 or 8 */
  int64_t per_frame;       /* C * H * W */
  int64_t total;           /* sum of the runs' n: the frames this launch writes */
  int64_t steps;           /* B * T: rows of obs / act / rew / end / trunc */
  int64_t K;               /* rows of final_obs */
  int64_t F;               /* rows of the arena */
  int64_t E;               /* rows of finals */
  const float* obs;        /* (steps, per_frame) */
  const int64_t* act;      /* (steps) */
  const float* rew;        /* (steps) */
  const void* end;         /* (steps) of flag_size bytes */
  const void* trunc;       /* (steps) of flag_size bytes */
  const float* final_obs;  /* (K, per_frame) or NULL */
  uint8_t* frames;         /* (F, per_frame) */
  int64_t* arena_act;      /* (F) */
  float* arena_rew;        /* (F) */
  uint8_t* arena_end;      /* (F) */
  uint8_t* arena_trunc;    /* (F) */
  uint8_t* finals;         /* (E, per_frame) or NULL */
  const int64_t* runs;     /* (R, 4): kind, src, n, dst */
  int32_t* off_grid;
} dmd_record_window_params;
int dmd_record_window(const dmd_record_window_params* p, dmd_stream_t stream);

/* ---- open-loop world-model evaluation against the replay arena: one step closed on the device in ONE launch ------------------
 * (additive to ABI v11.)  The sampler has produced `pred` from the context rings; this call compares it with what the arena
 * recorded and advances the rings, from the prediction (free running) or from the recording (teacher forced).
 * Arena and descriptor: those of dmd_segment_gather.  For sample b the predicted frame is episode step s = start + T + step, it
 * belongs to transition j = s - 1.
 *   target   frames[first + s] when 0 <= s < len; finals[final_row] when s == len, final_row >= 0 and end[first + len - 1] != 0
 *            (the put_back_final rule of dmd_segment_gather); otherwise the frame is INVALID
 *   metrics  q = level(pred) = clamp(rint((v + 1) / 2 * 255), 0, 255) (dmd_quantize_u8's expression), d = q - target, in uint8 levels:
 *            metrics[b] = { sum d^2, sum |d|, max |d|, count of d != 0 }; zeros for an invalid frame.  Exact integers.
 *   truth    out_rew[b] = rew[first + j], out_end[b] = end[first + j] when 0 <= j < len, else zeros
 *   flags    out_valid[b] = { frame valid, transition valid }
 *   rings    ctx_obs[b][head] = pred[b]; with teacher_forced and a valid frame: the dequantised target, (u8 / 255) * 2 - 1 with the
 *            bits of dmd_segment_gather.  ctx_act[b][head] = act[first + s] when 0 <= s < len, else 0.  `head` is the ring slot
 *            the new frame goes to: the oldest one (the convention of dmd_edm_pack_input and dmd_reset_slots).
 *   out_levels (optional, may be NULL) receives q.
 * Nothing outside the episode is read (never an out-of-range address).  One workgroup per sample; the sums are reduced in a fixed
 * order (and are integers).  Any per_frame >= 1: 16-byte accesses of pred / ctx_obs where per_frame % 4 == 0 and the pointers are
 * aligned (pred / ctx_obs 16 bytes, frames / finals / out_levels 4; 16 levels per lane and pass where per_frame % 16 == 0, else 4);
 * one level per lane otherwise. */
typedef struct dmd_openloop_params {
  int32_t B, T;
  int64_t per_frame;       /* C * H * W */
  int32_t step, head;      /* the evaluated step i >= 0; ring slot of the new frame, 0 <= head < T */
  int32_t teacher_forced;  /* 0 or 1 */
  int32_t reserved;
  const uint8_t* frames;   /* (F, per_frame) */
  const int64_t* act;      /* (F) */
  const float* rew;        /* (F) */
  const uint8_t* end;      /* (F) */
  const uint8_t* finals;   /* (E, per_frame) or NULL */
  const int64_t* seg;      /* (B, 4): first, start, len, final_row */
  const float* pred;       /* (B, per_frame) */
  float* ctx_obs;          /* (B, T, per_frame) ring */
  int64_t* ctx_act;        /* (B, T) ring */
  int64_t* metrics;        /* (B, 4) */
  float* out_rew;          /* (B) */
  uint8_t* out_end;        /* (B) */
  uint8_t* out_valid;      /* (B, 2) */
  uint8_t* out_levels;     /* (B, per_frame) or NULL */
} dmd_openloop_params;
int dmd_openloop_step(const dmd_openloop_params* p, dmd_stream_t stream);

/* ---- open-loop evaluation: what moved in the recording, what the prediction moved, what copying a frame would score -----------
 * (additive to ABI v11.)  One launch per evaluated step, issued BEFORE that step's dmd_openloop_step: it reads the ring as it
 * stands before the advance and writes nothing but `out` and `out_valid`.  Arena, descriptor, T, step and head: those of
 * dmd_openloop_step.  For sample b, with s = start + T + step, in uint8 levels, level(v) = clamp(rint((v + 1) / 2 * 255), 0, 255)
 * (dmd_quantize_u8's expression, the one device function dmd_openloop_step compares with):
 *   y   the target by dmd_openloop_step's rule: frames[first + s] when 0 <= s < len; finals[final_row] when s == len, final_row >= 0
 *       and end[first + len - 1] != 0; otherwise the frame is INVALID: all eight outputs and all three flags are 0
 *   r   the previous recorded frame, frames[first + s - 1]; valid when the frame is valid and s >= 1
 *   a   the anchor, the context's last frame, frames[first + start + T - 1]; valid when the frame is valid and 0 <= start + T - 1 < len
 *   q   level(pred[b])
 *   m   level(ctx_obs[b][(head + T - 1) % T]): the ring's NEWEST slot, the frame the model itself saw last (free running from step 1
 *       on: its own previous prediction; at step 0 or teacher forced: the recording).  No other slot of the ring is read.
 *   out[b] = { sum (y - r)^2,  sum (y - a)^2,  #{y != r},  #{q != m},  #{y != r and q != m},  sum over {y != r} of (q - y)^2,
 *              #{y != r and q == y},  0 }
 *            entries 0, 2, 4, 5, 6 are 0 where r is not valid, entry 1 is 0 where a is not valid, entry 3 counts every valid frame.
 *   out_valid[b] = { frame valid, r valid, a valid }
 * Exact integers, 64-bit from the lane's partial sum to `out` (a 256 x 256 x 3 frame exceeds 2^32 in entries 0, 1 and 5).  Nothing
 * outside the episode is read (never an out-of-range address); r and a are not read where they are not valid, an invalid frame
 * reads neither pred nor the ring.  One workgroup per sample; the sums are reduced in a fixed order (and are integers).  Any
 * per_frame >= 1: 16-byte loads of pred / ctx_obs where per_frame % 4 == 0 and the pointers are aligned (pred / ctx_obs 16 bytes,
 * frames / finals 4; 16 levels per lane and pass where per_frame % 16 == 0, else 4); one level per lane otherwise.
 * Refused (non-zero, dmd_last_error): NULL frames / end / seg / pred / ctx_obs / out / out_valid; B < 0, T < 1, per_frame < 1,
 * step < 0, head outside [0, T).  finals may be NULL (final_row is then never followed).  B == 0 returns 0 and launches nothing. */
typedef struct dmd_openloop_motion_params {
  int32_t B, T;
  int64_t per_frame;       /* C * H * W */
  int32_t step, head;      /* as dmd_openloop_params: the evaluated step, the ring's OLDEST slot (where that step's frame will go) */
  const uint8_t* frames;   /* (F, per_frame) */
  const uint8_t* end;      /* (F) */
  const uint8_t* finals;   /* (E, per_frame) or NULL */
  const int64_t* seg;      /* (B, 4): first, start, len, final_row */
  const float* pred;       /* (B, per_frame) */
  const float* ctx_obs;    /* (B, T, per_frame) ring BEFORE the advance */
  int64_t* out;            /* (B, 8) */
  uint8_t* out_valid;      /* (B, 3): frame, previous, anchor */
} dmd_openloop_motion_params;
int dmd_openloop_motion(const dmd_openloop_motion_params* p, dmd_stream_t stream);

/* ---- per-frame SSIM of uint8 levels, in fp64, on the device ---------------------------------------------------------------------
 * (additive to ABI v11.)  Wang et al. 2004 as the common implementations compute it: operands are levels 0 ... 255 as fp64, a
 * window of 11 taps per axis with weight win[i] * win[j] at tap (i, j), and only the positions whose window lies wholly inside the
 * frame: (H - 10) * (W - 10) per channel.  Per position and channel, with x from `a` and y from `b`:
 *   mx = sum w x, my = sum w y, sxx = sum w x^2 - mx^2, syy = sum w y^2 - my^2, sxy = sum w x y - mx my
 *   cs = (2 sxy + c2) / (sxx + syy + c2)          ssim = (2 mx my + c1) / (mx^2 + my^2 + c1) * cs
 *   out[n] = { mean ssim, mean cs } over the C * (H - 10) * (W - 10) positions of frame n.
 * win, c1 and c2 come from the host (the kernel holds no exp): diamond_amd/metrics.py forms the normalised Gaussian and
 * c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2.
 * Operand a: N frames (N, C, H, W) contiguous, through EXACTLY ONE of a_f32 (values in [-1, 1]; the level is
 *   clamp(rint((v + 1) / 2 * 255), 0, 255), the expression dmd_openloop_step compares with and dmd_quantize_u8 stores) and a_u8 (levels).
 * Operand b, one of two modes:
 *   direct  exactly one of b_f32 / b_u8, N contiguous frames; every arena field NULL
 *   arena   b_f32 = b_u8 = NULL; frames, end, seg (and finals, which may be NULL) are those of dmd_openloop_step, and the target of
 *           sample n is resolved by ITS rule: arena row first + s with
 *           s = start + T + step when 0 <= s < len; finals[final_row] when s == len, final_row >= 0 and end[first + len - 1] != 0;
 *           otherwise the sample has no target and out[n] = { NaN, NaN }.  Nothing outside the episode is read.
 * Arithmetic: fp64 throughout, no atomics, ONE summation order, so a shape's result is bitwise the same from run to run:
 *   the window sum is SEPARABLE -- a workgroup takes one channel's tile of 16 x 16 positions, stages the 26 x 26 levels of both
 *   operands in LDS, forms the five horizontal sums (x, y, x^2, y^2, x y; taps 0 ... 10 ascending, from 0.0) for its 26 x 16 (row,
 *   position column) pairs into LDS, then each lane the five vertical sums of its position (taps ascending, from 0.0);
 *   the tile's ssim / cs sums: a __shfl_xor butterfly over each wave (offsets 32, 16, ... 1), then waves 0 ... 3 in order; positions
 *   beyond the frame's last contribute +0.0.  The pair goes to workspace[((n * C + c) * tiles + tile)] (tile = ty * tiles_x + tx).
 *   A second launch of the same call: one wave per frame, lane l adds the frame's partials l, l + 64, ... in ascending order, the
 *   same butterfly follows, and lane 0 divides by the count.  x and y go through identical operations: identical frames give
 *   exactly { 1.0, 1.0 }.
 * workspace: dmd_ssim_workspace_doubles(N, C, H, W) doubles (2 * N * C * ceil((H - 10) / 16) * ceil((W - 10) / 16); 0 for sizes
 * the entry refuses), overwritten by every call.  Any C >= 1, any H, W >= 11, any alignment (levels are read byte by byte).
 * Refused (non-zero, dmd_last_error): H or W below 11; both or neither pointer of an operand; a direct b together with an arena
 * field; an arena without frames / end / seg; T < 0 or step < 0; NULL out or workspace.  N == 0 returns 0 and launches nothing. */
#define DMD_SSIM_TAPS 11
typedef struct dmd_ssim_params {
  int32_t N, C, H, W;
  const float* a_f32;      /* (N, C, H, W) in [-1, 1], or NULL */
  const uint8_t* a_u8;     /* (N, C, H, W) levels, or NULL */
  const float* b_f32;      /* direct mode: as a */
  const uint8_t* b_u8;
  const uint8_t* frames;   /* arena mode: (F, C * H * W) */
  const uint8_t* finals;   /* (E, C * H * W) or NULL */
  const uint8_t* end;      /* (F) */
  const int64_t* seg;      /* (N, 4): first, start, len, final_row */
  int32_t T, step;         /* arena mode: context length, evaluated step >= 0 */
  double win[DMD_SSIM_TAPS];
  double c1, c2;
  double* workspace;       /* dmd_ssim_workspace_doubles(N, C, H, W) doubles */
  double* out;             /* (N, 2): mean ssim, mean cs */
} dmd_ssim_params;
int64_t dmd_ssim_workspace_doubles(int N, int C, int H, int W);
int dmd_frame_ssim(const dmd_ssim_params* p, dmd_stream_t stream);

/* out[r] = row_slot[r] >= 0 ? slots[row_slot[r]] : base[r]  (rows of D floats): the burnt-in policy LSTM state of the reset rows
 * merged into the batch's state (env_loop.py:51-56), and the transposed operation for its backward:
 * d_base[r] = row_slot[r] >= 0 ? 0 : d_out[r] (d_base may be NULL);  d_slots[j] = slot_row[j] >= 0 ? d_out[slot_row[j]] : 0 */
int dmd_merge_slots(const float* base, const float* slots, const int32_t* row_slot, float* out, int B, int D, dmd_stream_t stream);
int dmd_merge_slots_bwd(const float* d_out, const int32_t* row_slot, const int64_t* slot_row, float* d_base, float* d_slots, int B, int K,
                        int D, dmd_stream_t stream);

/* NCHW (N, C, H, W) -> NHWC (N, H, W, CPad), zero padded channels */
int dmd_nchw_to_nhwc(const float* in, float* out, int N, int C, int H, int W, int CPad, dmd_stream_t stream);
int dmd_nhwc_to_nchw(const float* in, float* out, int N, int C, int H, int W, int CPad, dmd_stream_t stream);

/* GroupNorm partial statistics of an NHWC tensor (one tile per image): for tensors that
 * no dmd_* kernel produced. */
int dmd_gn_stats(const float* x, double* stats, int N, int HW, int C, dmd_stream_t stream);
/* ... of the (valid_h, valid_w) part of an (N, H, W, C) buffer (dmd_conv_params: VALID EXTENT) */
int dmd_gn_stats_valid(const float* x, double* stats, int N, int H, int W, int valid_h, int valid_w, int C, dmd_stream_t stream);

/* 2x2 max pooling, NHWC, also emits GroupNorm stats of the pooled output and the argmax
 * (0..3) for the backward pass (actor_critic.py:108-109). */
int dmd_maxpool2(const float* x, float* out, uint8_t* argmax, double* out_stats, int N, int H, int W, int C,
                 dmd_stream_t stream);

/* LSTM cell pointwise: gates (N, 4*Hd) in i,f,g,o order -> h, c (nn.LSTMCell, actor_critic.py:46,72) */
int dmd_lstm_pointwise(const float* gates, const float* c_prev, float* h, float* c, int N, int Hd,
                       dmd_stream_t stream);

/* backward of dmd_lstm_pointwise: gates = the forward's pre-activations, dh / dc = gradients w.r.t. the new h / c
 * (NULL = zero) -> dgates (N, 4*Hd), dc_prev (N, Hd)   (autograd of nn.LSTMCell, actor_critic.py:46,72) */
int dmd_lstm_pointwise_bwd(const float* gates, const float* c_prev, const float* c_new, const float* dh, const float* dc,
                           float* dgates, float* dc_prev, int N, int Hd, dmd_stream_t stream);
/* TD(lambda) targets of the actor-critic loss (reference actor_critic.py:116-143), one launch: rew / val_bootstrap / ret are
 * (B, T) fp32, end / trunc (B, T) int64, all contiguous.  The fp32 operations of the reference's expressions in their order
 * (no fused multiply-add); gamma, one_minus_lambda (= 1 - lambda formed in double) and lambda are the scalars rounded to fp32. */
int dmd_lambda_returns(const float* rew, const int64_t* end, const int64_t* trunc, const float* val_bootstrap, float* ret, int B, int T,
                       float gamma, float one_minus_lambda, float lambda, dmd_stream_t stream);

/* argmax(softmax(logits) / E) with injected exponential draws E == Categorical(logits).sample()
 * (env_loop.py:32, world_model_env.py:103-104). */
int dmd_categorical_sample(const float* logits, const float* expo, int64_t* out, int N, int A, dmd_stream_t stream);

/* (ABI v11 addition) The reward / end training loss (rew_end_model.py:72-88) in ONE launch of one workgroup, with nothing
 * data-dependent on the host (capturable).  logits (R, 5) fp32 contiguous: columns 0-2 the reward head, 3-4 the end head; rew (R)
 * fp32; end (R) int64; mask (R) one byte per row (0 = padding).  With n = the number of masked rows:
 *   losses[0]  mean over the masked rows of the cross-entropy of logits[:, 0:3] against class sign(rew) + 1 (-0.0, 0.0: class 1)
 *   losses[1]  the same of logits[:, 3:5] against class (end != 0)
 *   dlogits    (R, 5): gradient of losses[0] + losses[1], (softmax - onehot) / n per head; exact zeros on unmasked rows
 *   counts     int64 [13]: the confusion matrices [true][argmax] of the masked rows, 3 x 3 then 2 x 2, row-major; argmax ties go
 *              to the lowest index
 * n == 0: both losses NaN (the mean of an empty selection), dlogits and counts all zero.  fp32 log-soft-max with the row maximum
 * subtracted; fp64 loss sums and integer counts in a fixed order (no atomics): bitwise reproducible.  1 <= R <= 2^20. */
int dmd_rew_end_loss(const float* logits, const float* rew, const int64_t* end, const uint8_t* mask, float* losses, float* dlogits,
                     int64_t* counts, int R, dmd_stream_t stream);

/* ---- actor-critic encoder backward (what ATen autograd does for actor_critic.py:101-113 /
 *      blocks.py:116-123 under loss.backward(), trainer.py:366) ------------------------------ */

/* dx (N, H, W, C) <- scatter of dpooled (N, H/2, W/2, C) by the argmax dmd_maxpool2 saved */
int dmd_maxpool2_bwd(const float* dpooled, const uint8_t* argmax, float* dx, int N, int H, int W, int C,
                     dmd_stream_t stream);

/* Backward of a = act(GroupNorm(x) * mul' + add), act = SiLU or identity (mul' = mul or 1 + mul, as in dmd_norm):
 *   dx = d a / d x applied to da (+ dskip, the gradient of the residual branch around the block)
 *   dmul[n][c] = sum_hw du * xhat,  dadd[n][c] = sum_hw du   (the caller sums over n for affine
 *   parameters shared by the batch). */
typedef struct dmd_gn_bwd_params {
  int32_t N, HW, C;
  int32_t identity_activation; /* 0: a = SiLU(u) (AdaGroupNorm / SmallResBlock); 1: a = u (attention pre-norm, blocks.py:64) */
  const float* x;      /* NHWC input of the GroupNorm                          */
  dmd_norm norm;       /* its statistics + multiplicative/additive parameters  */
  const float* da;     /* gradient w.r.t. the activated tensor                 */
  const float* dskip;  /* NULL or NHWC, added to dx                            */
  float* dx;
  void* workspace;     /* dmd_gn_bwd_workspace_bytes(N, HW, C) bytes           */
  float* dmul;         /* (N, C) */
  float* dadd;         /* (N, C) */
  /* VALID EXTENT (ABI v8; all 0: the whole tensor): x is (N, HW / W, W, C) of which rows < valid_h, columns < valid_w exist.
   * Only those pixels enter the sums and the GroupNorm count; dx is written as ZERO outside (so that what consumes it --
   * max-pool backward, the next weight gradient -- sees no contribution from there). */
  int32_t W, valid_h, valid_w, reserved;
} dmd_gn_bwd_params;
int64_t dmd_gn_bwd_workspace_bytes(int N, int HW, int C);
int dmd_gn_silu_bwd(const dmd_gn_bwd_params* p, dmd_stream_t stream);

/* Weight/bias gradient of a stride-1 dmd_conv2d (3x3 pad 1 or 1x1) with a single source:
 *   dw[co][ci][ky][kx] = sum_{n,y,x} dy[n,y,x,co] * a[n, y+ky-1, x+kx-1, ci],  db[co] = sum dy,
 * a = the conv's (prologue-activated) input, recomputed from src exactly as the forward does. */
typedef struct dmd_wgrad_params {
  int32_t N, H, W;
  int32_t Cout;        /* multiple of 16 */
  int32_t taps;        /* 9 | 1 */
  int32_t cin_real;    /* input channels of the OIHW gradient (<= src.C, the padded count) */
  dmd_conv_src src;
  const float* dy;     /* NHWC (N, H, W, Cout) */
  float* workspace;    /* dmd_wgrad_workspace_floats(p) floats */
  float* dw;           /* OIHW (Cout, cin_real, k, k) */
  float* dbias;        /* (Cout) or NULL */
  int32_t precision;   /* DMD_PRECISION_F32 (exact fp32 fma chains of at most 2,048 pixels) | DMD_PRECISION_F16X2 (split-fp16 operands, fp32 accumulate) */
  /* DMD_PRECISION_F16X2, the OPERAND CONTRACT (tests/test_wgrad_precision.py pins every sentence):
   *  - both operands -- dy, and the source after its prologue -- enter as h + l, h = fp16(x), l = fp16(x - h), |x| < 65520:
   *    |x - (h + l)| <= e(x) = max(2^-22 |x|, 2^-25); an exact zero stays exact.  The kernels sum all four products, l l + h l + l h + h h,
   *    so ONE product is within 2^-21 |dy a| where both operands are >= 2^-3, and an element within
   *    sum_pixels e(dy) |a| + |dy| e(a) + e(dy) e(a) of the fp32-class result.
   *  - a FINITE operand beyond the range splits into h = inf, l = -inf: such a dy[.., co] makes the whole row dw[co][*][*] NaN,
   *    such a source value a[.., ci] the whole column dw[*][ci][*]; every other row and column is untouched, and none is a
   *    finite wrong number.  NaN / Inf operands do the same.  db is summed from the RAW fp32 dy on both routes: finite, fp32-class.
   *  - PER ROW: dw[co] is a sum over pixels of dy[.., co] alone, and one scalar (grad_ops.pow2_scaled) scales the whole launch
   *    to O(1).  A row whose dy is >= 2^-3 of that has l a normal fp16 and is fp32-class (within 30 x the fp32 reference, like
   *    the exact route).  Below 2^-3, l is a fp16 subnormal and the operand error an ABSOLUTE 2^-25: the row's relative error
   *    grows as the inverse of its scale.  Measured on the MI355X (profiles/wgrad_precision.txt; max |err| / max |dw| of the row,
   *    N = 3 at 8x16, 64 -> 64 3x3, source 1.3 N(0, 1) + 0.2, wgrad_ps_kernel; the exact route stays at 1e-7 .. 7e-7 on every line):
   *      dy channel scale   2^0     2^-4    2^-6    2^-10   2^-14   2^-20   2^-26
   *      row error          1.5e-7  3.2e-7  8.9e-7  1.9e-5  2.7e-4  1.9e-2  0.91
   *    An output channel at about 2^-13 (1.2e-4) of the launch's largest gradient loses the 1e-4 bar (5.4e-5 at 2^-12, 1.4e-4 at
   *    2^-13); at 2^-26 the row is flushed. */
  /* VALID EXTENT (ABI v8; both 0: the whole tensor): rows < valid_h, columns < valid_w of src and dy exist; positions outside are
   * the convolution's zero padding (input, after the prologue) / contribute nothing (dy), GroupNorm counts the valid pixels. */
  int32_t valid_h, valid_w;
  /* ABI v10 (was reserved, 0): 1 = stop after the per-workgroup partials; they stay in `workspace` (which the caller keeps alive)
   * until a dmd_wgrad_reduce_jobs launch sums them into dw / dbias -- the job comes from dmd_wgrad_job(p). */
  int32_t defer_reduce;
} dmd_wgrad_params;
int64_t dmd_wgrad_workspace_floats(const dmd_wgrad_params* p);
int dmd_conv2d_wgrad(const dmd_wgrad_params* p, dmd_stream_t stream);

/* Deferred reductions of weight gradients (ABI v10).  The reference leaves every weight gradient to autograd's per-layer kernels
 * (src/models/diffusion/denoiser.py:93-122 -> loss.backward(), src/trainer.py:349-388); here the partial sums of ALL layers of a
 * backward are reduced by one launch per 32 gradients once the last dmd_conv2d_wgrad(defer_reduce = 1) is issued.  The sums are
 * formed in the order of the undeferred call: the gradients are bit-identical.  A job names where its gradient lands:
 * element (co, ci, tap) -> dw[(co * ld_cin + c0 + ci) * taps + tap], so the sources of a convolution over concatenated inputs
 * (ld_cin = all input channels, c0 = this source's first) and the 64-channel pieces of a wide output (dw offset by whole rows)
 * fill ONE OIHW tensor.  The table is HOST memory: it travels in the kernel arguments. */
typedef struct dmd_wgrad_reduce_job {
  const float* partials; /* the workspace of the deferred dmd_conv2d_wgrad */
  float* dw;
  float* dbias;          /* or NULL */
  int32_t num_wg, NB, NCO, NCI, taps, cin_real; /* filled by dmd_wgrad_job */
  int32_t ld_cin, c0;    /* dmd_wgrad_job: cin_real, 0 */
  /* DEVICE pointer to one float, or NULL (dmd_wgrad_job: NULL): every element leaves as (float)sum * *scale.  The backward of the
   * actor-critic encoder runs on a gradient scaled by 2^k and hands its 2^-k here: a power of two, so the result is bitwise the
   * unscaled reduction followed by a multiplication, without that pass. */
  const float* scale;
  /* DMD_REDUCE_WGRAD (dmd_wgrad_job), or DMD_REDUCE_COLSUM: the GroupNorm PARAMETER gradients of a block in the same launch --
   * partials = the (2, N, C) per-(sample, channel) gradients [dmul; dadd] of dmd_gn_silu_bwd, num_wg = N, cin_real = C, the other
   * counts unused; dw[c] = sum_n dmul[n][c] (dgamma), dbias[c] = sum_n dadd[n][c] (dbeta), both required.  Order: ascending n,
   * accumulated in fp64, rounded to fp32 once (then scaled): deterministic, and at least as accurate as an fp32 sum. */
  int32_t kind, reserved;
} dmd_wgrad_reduce_job;
#define DMD_REDUCE_WGRAD 0
#define DMD_REDUCE_COLSUM 1
/* The job of dmd_conv2d_wgrad(p, defer_reduce = 1): its pointers are p's (which may still be null -- a deferred call needs only
 * num_wg * (NB * NCO * 256 + NCO * 16) floats of workspace, less than dmd_wgrad_workspace_floats, and the caller may size it from
 * the job before it sets p->workspace and job->partials). */
int dmd_wgrad_job(const dmd_wgrad_params* p, dmd_wgrad_reduce_job* job);
int dmd_wgrad_reduce_jobs(const dmd_wgrad_reduce_job* jobs, int njobs, dmd_stream_t stream);

/* (ABI v11 addition) Image gradients: the data gradient of a network's FIRST convolution (3x3, stride 1, pad 1: conv_in of the
 * denoiser, of the actor-critic encoder and of the reward / end encoder), written straight into the caller's cropped NCHW
 * tensors -- what ATen autograd returns for `torch.autograd.grad(out, image)` in the reference (inner_model.py:46,
 * denoiser.py:74-77, actor_critic.py:105, rew_end_model.py:37).  ONE launch, no workspace:
 *   dx[n, c, y, x] = (post * sum_{co, ky, kx} dy[n, y + 1 - ky, x + 1 - kx, co] * w[co, c, ky, kx]) * s(n, c)
 *       for 0 <= y < valid_h, 0 <= x < valid_w, 0 <= c < cin
 * dy is the (valid_h, valid_w) extent of an (N, H, W, Cout) buffer (dmd_conv_params: VALID EXTENT; 0, 0 = (H, W); any H, W >= 1):
 * its margins are never loaded (they may hold NaN) and count as zero, like the pixels outside the buffer.  w is the convolution's
 * own OIHW (Cout, cin, 3, 3) parameter: no packed copy exists.  Channels [0, c_split) go to dx_a (N, c_split, valid_h, valid_w),
 * channels [c_split, cin) to dx_b (N, cin - c_split, valid_h, valid_w), both contiguous; either may be NULL (its channels are
 * then not written), nothing else is written.
 * ORDER OF THE TWO MULTIPLICATIONS: the sum is multiplied by *post first (the 2^-k of a backward that ran on a gradient scaled by
 * 2^k: exact, the true gradient of the convolution's input), the product then by s(n, c) (the chain rule of how the caller built
 * that input from its images): s = scale_a[n * stride_a] for the channels of dx_a and scale_b for those of dx_b; with swap_scales
 * the other way round (the denoiser packs obs / sigma_data BEFORE noisy * c_in[n]: dmd_edm_pack_input).  NULL post / scale_a = 1.
 * Cout: any multiple of 16.  1 <= cin <= 64 (16 channels per workgroup).  Exact fp32 operands on v_mfma_f32_16x16x4_f32 with fp32
 * accumulation, whatever precision the rest of the backward runs in.  No atomics, one fixed summation order: an image's result
 * depends on that image alone (not on N, its position in the batch or the launch geometry) and is run-to-run bitwise. */
typedef struct dmd_dgrad_input_params {
  int32_t N, H, W;          /* dy's buffer                                                    */
  int32_t valid_h, valid_w; /* 0, 0 = (H, W)                                                  */
  int32_t Cout;             /* channels of dy = rows of w, a multiple of 16                   */
  int32_t cin, c_split;     /* w's input channels; the first c_split of them are dx_a's       */
  const float* dy;          /* NHWC (N, H, W, Cout), 8-byte aligned                           */
  const float* w;           /* OIHW (Cout, cin, 3, 3)                                         */
  float* dx_a;              /* NCHW (N, c_split, valid_h, valid_w) or NULL                    */
  float* dx_b;              /* NCHW (N, cin - c_split, valid_h, valid_w) or NULL              */
  const float* scale_a;     /* DEVICE, [n * stride_a], or NULL (1)                            */
  int32_t stride_a;         /* 0 | 1                                                          */
  float scale_b;            /* host scalar                                                    */
  const float* post;        /* DEVICE, one float, or NULL (1)                                 */
  int32_t swap_scales;      /* 1: scale_a applies to dx_b's channels, scale_b to dx_a's       */
  int32_t reserved;
} dmd_dgrad_input_params;
int dmd_conv2d_dgrad_input(const dmd_dgrad_input_params* p, dmd_stream_t stream);

const char* dmd_last_error(void);
int dmd_abi_version(void);
/* The library reads its DIAMOND_* switches from the environment once; this makes it read them again (test hook). */
void dmd_reload_env(void);

#ifdef __cplusplus
}
#endif
#endif /* DIAMOND_HIP_H */
