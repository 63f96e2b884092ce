// Attention of SelfAttention2d (models/blocks.py:62-72): softmax(q k^T / sqrt(d)) v and its gradient, head_dim d = 8 (ATTN_HEAD_DIM,
// blocks.py:14).  qkv / dqkv are NHWC (N, T, 3C): q | k | v channel thirds, head h = channels [8h, 8h + 8).  Precision contracts:
// include/diamond_hip.h; which entry point the host calls: engine.attention (forward), grad_ops.attention_bwd (backward).
//   entry point              kernel(s)                                      when
//   dmd_attention            attention_f16x2_kernel<false>                  T % 256 == 0: split-fp16 operands, two passes over the keys
//                            attention_kernel                               any other T % 64 == 0: exact fp32, online softmax
//   dmd_attention_valid      attention_kernel                               always; keys outside the extent are masked
//   dmd_attention_f32        attention_f32_tiled_kernel                     always: exact fp32, two passes, over the valid tokens
//   dmd_attention_f16x2      attention_f16x2_kernel<true>                   always: split-fp16 operands, two passes, over the valid tokens
//   dmd_attention_bwd        attention_bwd_rows_kernel + _cols_kernel       always: the extent (1, T, 1, T) of a (1, T) grid
//   dmd_attention_bwd_valid  attention_bwd_rows_kernel + _cols_kernel       always: the extent as given
//   dmd_attention_bwd_mfma   attention_bwd_mfma_q_kernel + _k_kernel        always: fp32 matrix cores, the extent as given
// EXTENT CONVENTION of every kernel but the first two: only rows < vh, columns < vw of a row-major (H, W) token grid exist
// (dmd_conv_params: VALID EXTENT); tokens are addressed by their valid index (ab_token), nothing outside the extent is read, and the
// whole grid of T tokens is the extent (1, T, 1, T) of a (1, T) grid.
//
// attention_kernel:
// Layout trick: compute the TRANSPOSED score block S^T[key][query] = K Q^T so that a lane
// (j = lane & 15, kg = lane >> 4) owns 4 keys {4 kg + r} of ONE query j:
//   * the softmax statistics of query j live in the 4 lanes {j, j+16, j+32, j+48}
//     (two __shfl_xor to combine),
//   * those same 4 registers are exactly the MFMA B operand of O^T[d][query] += V^T P^T
//     (k-remap: MFMA t contracts keys {4 k' + t}), so P never moves between lanes,
//   * O^T's D layout again has the query in the column (lane & 15): the running rescale
//     exp(m_old - m_new) is a per-lane scalar.
// One workgroup = 4 waves = 64 queries of one (image, head); keys stream in tiles of 256.
#include <stdlib.h>

#include "dmd_common.h"

#define ATT_KB 256          // keys per LDS tile
#define ATT_VSTRIDE (ATT_KB + 16)

// token of valid index li: the li-th token, in row-major order, of the (vh, vw) extent of an (H, W) grid
__device__ __forceinline__ int ab_token(int li, int W, int vw) {
  const int r = li / vw;
  return r * W + (li - r * vw);
}
// the m-th token OUTSIDE the extent, m < H W - vh vw: rows < vh, columns >= vw first, then the rows >= vh (vw == W: side is 0 and
// nothing divides by W - vw)
__device__ __forceinline__ int ab_margin_token(int m, int W, int vh, int vw) {
  const int side = vh * (W - vw);
  if (m >= side) return vh * W + (m - side);
  const int r = m / (W - vw);
  return r * W + vw + (m - r * (W - vw));
}

// The argument checks the entry points share (`who` names the entry point in the message); one over T tokens with no grid of its
// own passes the whole-grid extent (1, T, 1, T).  0 if they hold.
static int att_check_args(const char* who, bool pointers, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim) {
  DMD_CHECK_ARG(pointers, "%s: null", who);
  DMD_CHECK_ARG(head_dim == 8, "%s: head_dim must be 8 (ATTN_HEAD_DIM), got %d", who, head_dim);
  DMD_CHECK_ARG(C > 0 && C % 8 == 0 && N > 0 && H > 0 && W > 0, "%s: need C %% 8 == 0, N, H, W > 0 (N=%d H=%d W=%d C=%d)", who, N, H, W, C);
  DMD_CHECK_ARG(valid_h > 0 && valid_h <= H && valid_w > 0 && valid_w <= W, "%s: valid extent %d x %d of %d x %d", who, valid_h, valid_w,
                H, W);
  return 0;
}

// Wp > 0 (dmd_attention_valid): the T tokens are a row-major (T / Wp) x Wp grid of which only rows < hv, columns < wv
// exist; the other keys get the score -inf (token 0 always exists, so the running maximum is finite from the first block on).
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T,
                                                        int C, float inv_scale_den, int Wp, int hv, int wv) {
  __shared__ float Ks[ATT_KB][8];
  __shared__ float Vt[8][ATT_VSTRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kg = lane >> 4;
  const int n = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 64 + wave * 16;
  const size_t row = (size_t)3 * C;
  const float* base = qkv + (size_t)n * T * row;

  // Q fragment (B operand of S^T = K Q^T): lane (query j, k' = kg), step s uses dim 2 kg + s
  const float* qp = base + (size_t)(q0 + j) * row + h * 8 + 2 * kg;
  const float qa = qp[0], qb = qp[1];

  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};  // O^T[dd = 4 kg + r][query j]  (kg >= 2: padding rows)
  float m_run = -INFINITY, l_run = 0.f;

  for (int kt = 0; kt < T; kt += ATT_KB) {
    const int nk = (T - kt) < ATT_KB ? (T - kt) : ATT_KB;
    __syncthreads();
    if (tid < nk) {
      const float* kp = base + (size_t)(kt + tid) * row + C + h * 8;
      const float* vp = kp + C;
      const f32x4 k0 = *(const f32x4*)kp, k1 = *(const f32x4*)(kp + 4);
      const f32x4 v0 = *(const f32x4*)vp, v1 = *(const f32x4*)(vp + 4);
      *(f32x4*)&Ks[tid][0] = k0;
      *(f32x4*)&Ks[tid][4] = k1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Vt[e][tid] = v0[e];
        Vt[4 + e][tid] = v1[e];
      }
    }
    __syncthreads();
    for (int k0 = 0; k0 < nk; k0 += 16) {
      // S^T block: A = K[key i = lane & 15][dim], B = Q[dim][query j]
      const float ka = Ks[k0 + j][2 * kg], kb = Ks[k0 + j][2 * kg + 1];
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
      s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, qa, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x4f32(kb, qb, s, 0, 0, 0);
      // s[r] = q_j . k_{k0 + 4 kg + r}
      float bmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[r] = s[r] / inv_scale_den;  // (q @ k^T) / sqrt(d), blocks.py:68
        if (Wp > 0) {
          const int key = kt + k0 + 4 * kg + r, ky = key / Wp, kx = key - ky * Wp;
          if (ky >= hv || kx >= wv) s[r] = -INFINITY;
        }
        bmax = fmaxf(bmax, s[r]);
      }
      bmax = fmaxf(bmax, __shfl_xor(bmax, 16, 64));
      bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
      const float m_new = fmaxf(m_run, bmax);
      const float alpha = expf(m_run - m_new);
      f32x4 pr;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pr[r] = expf(s[r] - m_new);
        psum += pr[r];
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l_run = alpha * l_run + psum;
      m_run = m_new;
      acc *= alpha;
      // O^T += V^T P^T : A = V^T[dd i = lane & 15][key 4 kg + t], B = P^T[key][query j] = pr[t]
      f32x4 vf = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (j < 8) vf = *(const f32x4*)&Vt[j][k0 + 4 * kg];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[t], pr[t], acc, 0, 0, 0);
    }
  }
  if (kg < 2) {
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = acc[r] / l_run;
    *(f32x4*)(out + ((size_t)n * T + q0 + j) * C + h * 8 + 4 * kg) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// attention_f16x2_kernel -- the same attention for T a multiple of 256 (256 tokens at the default denoiser's 16x16 level, in
// sampling and in the training step's forward; 1024 / 4096 tokens at the 32x32 / 64x64 levels of the 256x256 configuration) on the
// f16 matrix cores with SPLIT fp32 operands (x = h + l, fp16 pieces, as in dmd_conv_f16ws.hip: each operand off by at most
// max(2^-22 |x|, 2^-25), usable up to the end of fp16, nothing clamped -- a finite operand whose h piece overflows makes the
// outputs it feeds NaN; NaN / +-Inf operands behave as in fp32, af_split8).  With head_dim 8 a (query, key) pair costs 16 MACs and one exponential: the kernel is bound by
// the vector unit's issue port (v_exp_f32 takes two of its slots: 8 cycles per wave64 instruction, additive with plain VALU work,
// tools/probe/trans_probe.hip / profiles/r04_trans_probe.txt), so everything else is taken off it:
//   * TWO passes over the keys instead of an online softmax.  Pass 1: S^T = K Q^T blocks and a running per-lane maximum
//     (one cross-lane reduction per query at its end).  Pass 2: the score MFMA starts from the accumulator -m_q + 13, so
//     its output is directly the exponent: p = 2^(s - m + 13) -- no subtraction, no per-block maximum, no rescaling of O,
//     and exactly softmax's x - max(x) (blocks.py:69).  The 2^13 moves the split's absolute floor (2^-25) to 2^-38 of the
//     largest weight and cancels in O / l.
//   * log2(e) / sqrt(d) is folded into Q once per query (p = exp2: one v_exp_f32 per pair, no expf range code).
//   * one v_mfma_f32_16x16x32_f16 per 16 keys x 16 queries does the whole split product q_h k_h + q_h k_l + q_l k_h:
//     the K = 32 slots are {k_h | k_l | k_h | 0} against {q_h | q_h | q_l | 0} (8 dims each).
//   * O^T[dim][query] += V^T P^T with A = [v_h ; v_l] stacked in the 16 rows and B = p_h, then p_l: two MFMAs per
//     32 keys give (p_h + p_l)(v_h + v_l); rows dim and 8 + dim are added once at the end.  P never moves between lanes:
//     the score MFMA leaves lane (j = lane & 15, kg = lane >> 4) with keys {4 kg + r} of a 16-key block for query j,
//     and the P^T operand's k-slots are simply DEFINED as those keys (A reads V^T with the same map).
// One workgroup = 4 waves x 64 queries (4 groups of 16) of one (image, head); K / V^T tiles of 256 keys are split once per
// workgroup while staging and double-buffered in LDS.
// ------------------------------------------------------------------------------------------------
typedef _Float16 att_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 att_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 att_h2 __attribute__((ext_vector_type(2)));
// lw = {fp16(p0 - h0), fp16(p1 - h1)} for hw = {h0, h1}: one mixed-precision fma per element (tests/simt, the host build of
// these sources, defines the macro with the same arithmetic in C++ before this point)
#ifndef ATT_SPLIT_LOW_PAIR
#define ATT_SPLIT_LOW_PAIR(lw, p0, p1, hw)                                          \
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"       \
      "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"           \
      : "=&v"(lw)                                                                   \
      : "v"(p0), "v"(p1), "v"(hw))
#endif

// max(a, b, c) as ONE v_max3_f32.  Pairwise fmaxf() trees made hipcc quiet every MFMA output first (v_max_f32 v, v, v: 72 of the
// 92 vector instructions of pass 1's inner loop, which made that pass VALU-bound instead of MFMA-bound); the three-input form
// needs no quieting.  (Not inline asm: the compiler has to see the MFMA -> VALU dependency to place the wait states.)
__device__ __forceinline__ float af_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// lab builds only (tools/build_attention_ablations.sh; WRONG results): timing proxies, bits: 1 no pass 1, 2 no exponentials,
// 4 no l-piece of P, 8 no row sums, 16 no PV MFMAs, 32 no score MFMAs in pass 2, 64 tiles staged once
#if defined(DMD_LAB) && defined(AF_ABL)
#define AF_LAB(bit) ((AF_ABL) & (bit))
#else
#define AF_LAB(bit) 0
#endif

#define AF_KT 256                   // keys per LDS tile
#define AF_VS (AF_KT + 8)           // V^T row stride in halfs (+16 bytes: rows start on different banks)
#define AF_QG 4                     // 16-query groups per wave
#define AF_SHIFT 13.0f              // exponent offset of the weights (see above)

struct AfTile {
  att_h8 kh[AF_KT];       // [key] dims 0..7, h pieces
  att_h8 kl[AF_KT];       // l pieces
  _Float16 vt[16][AF_VS];  // rows 0..7: v_h[dim][key], rows 8..15: v_l[dim][key]
};

// INF_IN_L (the keys): an infinite element is held as h = 0, l = +-Inf instead of h = +-Inf, l = Inf - Inf = NaN.  The score's
// slots are then q_h * 0 + q_h * (+-Inf) + q_l * 0 (+ 0 * 0 in the unused group) = sign(q) * Inf, fp32's q * k: a key whose score is
// -Inf drops out of its row, one whose score is +Inf makes the row NaN, and q = 0 against it is NaN, as in fp32.  With h = +-Inf
// the q_l * k_h slot (q_l takes either sign) and the unused group's k_h * 0 made every score of that key NaN.  A FINITE element
// beyond fp16 still splits into h = +-Inf, l = -+Inf: NaN, nothing is clamped.
template <bool INF_IN_L = false>
__device__ __forceinline__ void af_split8(const f32x4& a, const f32x4& b, att_h8& h, att_h8& l) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (INF_IN_L && __builtin_isinf(a[e])) ? (_Float16)0.f : (_Float16)a[e];
    l[e] = (_Float16)(a[e] - (float)h[e]);
    h[4 + e] = (INF_IN_L && __builtin_isinf(b[e])) ? (_Float16)0.f : (_Float16)b[e];
    l[4 + e] = (_Float16)(b[e] - (float)h[4 + e]);
  }
}

// the scores of the keys behind the tile's nk valid ones become -inf: s0[r] is key kb + r of the tile, s1[r] key kb + 16 + r.  A
// SELECTION, not arithmetic: those keys are staged as zeros, and 0 against an infinite query is NaN
__device__ __forceinline__ void af_mask_keys(f32x4& s0, f32x4& s1, int kb, int nk) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s0[r] = kb + r < nk ? s0[r] : -INFINITY;
    s1[r] = kb + 16 + r < nk ? s1[r] : -INFINITY;
  }
}
// The two inner loop bodies, 32 keys from k0 of tile `tl`: each is expanded twice in the kernel, plain (MASK = (void)0) and with
// af_mask_keys on the partial last tile of an extent.  Macros, not lambdas or helpers: either of those changed the on-grid
// kernel's instruction stream; this way the compiler is given exactly the text it had.
#define AF_PASS1_BLOCK(MASK)                                                                                          \
  {                                                                                                                   \
    const att_h8 ka0 = k_frag(tl, k0), ka1 = k_frag(tl, k0 + 16);                                                     \
    _Pragma("unroll") for (int g = 0; g < AF_QG; ++g) {                                                               \
      f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka0, bq[g], zero4, 0, 0, 0);                                  \
      f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka1, bq[g], zero4, 0, 0, 0);                                  \
      MASK;                                                                                                           \
      mx[g] = af_max3(af_max3(mx[g], s0[0], s0[1]), af_max3(s0[2], s0[3], s1[0]), af_max3(s1[1], s1[2], s1[3]));      \
    }                                                                                                                 \
  }
/* V^T operand: lane (row i = lane & 15, kg): k-slots 0..3 = keys k0 + 4 kg + (0..3), 4..7 = keys k0 + 16 + 4 kg + (0..3);
   p = h + l: packed fp16 conversion for h, one mixed-precision fma per element for l = fp16(p - h) */
#define AF_PASS2_BLOCK(MASK)                                                                                          \
  {                                                                                                                   \
    const att_h8 ka0 = k_frag(tl, k0), ka1 = k_frag(tl, k0 + 16);                                                     \
    const att_h4 va = *(const att_h4*)&tl.vt[j][k0 + 4 * kg], vb = *(const att_h4*)&tl.vt[j][k0 + 16 + 4 * kg];       \
    const att_h8 vf = (att_h8){va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};                               \
    _Pragma("unroll") for (int g = 0; g < AF_QG; ++g) {                                                               \
      f32x4 s0 = AF_LAB(32) ? negm[g] + oacc[g] : __builtin_amdgcn_mfma_f32_16x16x32_f16(ka0, bq[g], negm[g], 0, 0, 0); \
      f32x4 s1 = AF_LAB(32) ? negm[g] - oacc[g] : __builtin_amdgcn_mfma_f32_16x16x32_f16(ka1, bq[g], negm[g], 0, 0, 0); \
      MASK;                                                                                                           \
      float p[8];                                                                                                     \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                 \
        p[r] = AF_LAB(2) ? s0[r] : __builtin_amdgcn_exp2f(s0[r]);                                                     \
        p[4 + r] = AF_LAB(2) ? s1[r] : __builtin_amdgcn_exp2f(s1[r]);                                                 \
      }                                                                                                               \
      if (!AF_LAB(8)) lsum[g] += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));                   \
      unsigned hw[4], lw[4];                                                                                          \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                 \
        hw[r] = __builtin_bit_cast(unsigned, (att_h2){(_Float16)p[2 * r], (_Float16)p[2 * r + 1]});                   \
        if (AF_LAB(4))                                                                                                \
          lw[r] = hw[r];                                                                                              \
        else                                                                                                          \
          ATT_SPLIT_LOW_PAIR(lw[r], p[2 * r], p[2 * r + 1], hw[r]);                                                   \
      }                                                                                                               \
      typedef unsigned att_u4 __attribute__((ext_vector_type(4)));                                                    \
      const att_h8 ph = __builtin_bit_cast(att_h8, (att_u4){hw[0], hw[1], hw[2], hw[3]});                             \
      const att_h8 pl = __builtin_bit_cast(att_h8, (att_u4){lw[0], lw[1], lw[2], lw[3]});                             \
      if (AF_LAB(16)) { /* (keeps the operands alive: 8 plain adds) */                                                \
        oacc[g] += __builtin_bit_cast(f32x4, ph) + __builtin_bit_cast(f32x4, pl);                                     \
      } else {                                                                                                        \
        oacc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, ph, oacc[g], 0, 0, 0);                                   \
        oacc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pl, oacc[g], 0, 0, 0);                                   \
      }                                                                                                               \
    }                                                                                                                 \
  }

// EXTENT (dmd_attention_f16x2): the same body over the V = vh vw tokens of the (vh, vw) extent of a (T / W, W) grid, addressed by
// their valid index (EXTENT CONVENTION above): ceil(V / 256) workgroups per (image, head), blockIdx.x < nbv, and as many key tiles.
//   * whole key tiles run the inner loops of the on-grid kernel (the same macro, unmasked, constant trip count); only a partial LAST tile runs the
//     masked copy of them (af_mask_keys), over its 32-key blocks that hold a valid key.  Its keys behind V are not loaded: K and V
//     are staged as zeros, their scores are -inf in both passes, p = 2^-inf = 0 exactly, so they add 0 to l and 0 * 0 to O.
//   * queries behind V (the last workgroup's) are not loaded: their Q operand is zero, which leaves them out of the workgroup's
//     qmax, and they are not stored.
//   * BARRIERS: the only exit before the end is that of the workgroups blockIdx.x >= nbv, which leave as a whole before the first
//     barrier (they write the rows of `out` outside the extent as +0).  In a workgroup blockIdx.x < nbv every thread, with or
//     without a valid query (V = 323: the second workgroup has 67 valid queries, its waves 2 and 3 none), runs every statement
//     below but the final store: ntiles, nk and the choice between the two copies of the inner loops depend on V and t alone, so
//     all 256 threads stage their key of every tile, execute the same MFMAs and reach the same __syncthreads() the same number of
//     times.
// EXTENT = false is the on-grid kernel as it was (the same instruction stream): W, vh, vw, nbv are not read.  The extent form needs
// 146 VGPRs against 128 (the valid-index arithmetic and the second copy of the loops): three workgroups per CU, asked for by its
// launch bound (left at two it takes 174 registers), where the on-grid kernel has four.
template <bool EXTENT>
__global__ __launch_bounds__(256, EXTENT ? 3 : 2) void attention_f16x2_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int C,
                                                              float qscale, int W, int vh, int vw, int nbv) {
  __shared__ AfTile tiles[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kg = lane >> 4;
  const int n = blockIdx.z, h = blockIdx.y;
  const int V = EXTENT ? vh * vw : T;
  if constexpr (EXTENT) {
    if ((int)blockIdx.x >= nbv) {  // the whole workgroup: no barrier has been reached
      const int m = ((int)blockIdx.x - nbv) * 256 + tid;
      if (m >= T - V) return;
      float* o = out + ((size_t)n * T + ab_margin_token(m, W, vh, vw)) * C + h * 8;
      *(f32x4*)o = (f32x4){0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(o + 4) = (f32x4){0.f, 0.f, 0.f, 0.f};
      return;
    }
  }
  const int q0 = blockIdx.x * (64 * 4) + wave * 64;
  const size_t row = (size_t)3 * C;
  const float* base = qkv + (size_t)n * T * row;
  const int ntiles = EXTENT ? (V + AF_KT - 1) / AF_KT : T / AF_KT;

  // Q operand of S^T = K Q^T, per 16-query group: k-slots {q_h | q_h | q_l | 0}, scaled by log2(e) / sqrt(d).
  // REBALANCING: the fp16 pieces carry 2^-22 of an operand only from 2^-3 upwards (below, their absolute floor 2^-25).  When every
  // q' of the workgroup's 256 queries is below 2^-3 -- tiny queries against keys near the end of fp16 -- q' is multiplied by the
  // power of two that brings the largest into [1, 2) and the workgroup's copy of K (split while staging) by its inverse, < 2^-3:
  // the scores are the same numbers, the keys cannot overflow.  Otherwise the factor is 1 and every bit is as without it.
  f32x4 qa[AF_QG], qb[AF_QG];
  float qmax = 0.f;
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) {
    const int lq = q0 + g * 16 + j;
    qa[g] = qb[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (!EXTENT || lq < V) {
      const float* qp = base + (size_t)(EXTENT ? ab_token(lq, W, vw) : lq) * row + h * 8;
      qa[g] = *(const f32x4*)qp;
      qb[g] = *(const f32x4*)(qp + 4);
    }
    qa[g] *= qscale;
    qb[g] *= qscale;
#pragma unroll
    for (int e = 0; e < 4; ++e) qmax = fmaxf(qmax, fmaxf(fabsf(qa[g][e]), fabsf(qb[g][e])));
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) qmax = fmaxf(qmax, __shfl_xor(qmax, o, 64));
  float* red = (float*)&tiles[1];  // free until pass 1 stages its second tile, behind the next barrier
  if (lane == 0) red[wave] = qmax;
  __syncthreads();
  qmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float kscale = 1.f, qs = 1.f;
  if (qmax < 0.125f && qmax > 1e-30f) {
    const unsigned pw = __builtin_bit_cast(unsigned, qmax) & 0x7f800000u;  // 2^floor(log2 qmax)
    kscale = __builtin_bit_cast(float, pw);
    qs = __builtin_bit_cast(float, 0x7f000000u - pw);
  }
  att_h8 bq[AF_QG];
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) {
    att_h8 qh, ql;
    af_split8(qa[g] * qs, qb[g] * qs, qh, ql);
    att_h8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.f;
    bq[g] = kg < 2 ? qh : (kg == 2 ? ql : z);
  }

  // staging of one key tile: thread = key; K always, V^T in pass 2
  f32x4 sk0, sk1, sv0, sv1;
  auto stage_load = [&](int t, bool with_v) {
    const int lk = t * AF_KT + tid;
    if constexpr (EXTENT) {
      sk0 = sk1 = sv0 = sv1 = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (lk >= V) return;
    }
    const float* kp = base + (size_t)(EXTENT ? ab_token(lk, W, vw) : lk) * row + C + h * 8;
    sk0 = *(const f32x4*)kp;
    sk1 = *(const f32x4*)(kp + 4);
    if (with_v) {
      sv0 = *(const f32x4*)(kp + C);
      sv1 = *(const f32x4*)(kp + C + 4);
    }
  };
  auto stage_store = [&](AfTile& tl, bool with_v) {
    att_h8 hh, ll;
    af_split8<true>(sk0 * kscale, sk1 * kscale, hh, ll);
    tl.kh[tid] = hh;
    tl.kl[tid] = ll;
    if (with_v) {
      af_split8(sv0, sv1, hh, ll);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        tl.vt[e][tid] = hh[e];
        tl.vt[8 + e][tid] = ll[e];
      }
    }
  };
  // A operand of a score block: lane (key i = lane & 15, kg): slots {k_h | k_l | k_h | (k_h x 0)}
  auto k_frag = [&](const AfTile& tl, int k0) -> att_h8 { return kg == 1 ? tl.kl[k0 + j] : tl.kh[k0 + j]; };

  // ---------------- pass 1: row maxima ----------------
  float mx[AF_QG];
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) mx[g] = -INFINITY;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  stage_load(0, false);
  stage_store(tiles[0], false);
  __syncthreads();
  for (int t = 0; t < (AF_LAB(1) ? 1 : ntiles); ++t) {
    const AfTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1, false);
    const int nk = !EXTENT || V - t * AF_KT > AF_KT ? AF_KT : V - t * AF_KT;
    if (!EXTENT || nk == AF_KT) {
#pragma unroll 2
      for (int k0 = 0; k0 < AF_KT; k0 += 32) AF_PASS1_BLOCK((void)0)
    } else {  // the partial last tile of an extent: its 32-key blocks that hold a valid key
      for (int k0 = 0; k0 < nk; k0 += 32) AF_PASS1_BLOCK(af_mask_keys(s0, s1, k0 + 4 * kg, nk))
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1], false);
    __syncthreads();
  }
  f32x4 negm[AF_QG];
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) {
    float m = mx[g];
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float c = AF_SHIFT - m;
    negm[g] = (f32x4){c, c, c, c};
  }

  // ---------------- pass 2: weights, row sums, O^T = V^T P^T ----------------
  f32x4 oacc[AF_QG];
  float lsum[AF_QG];
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) {
    oacc[g] = zero4;
    lsum[g] = 0.f;
  }
  stage_load(0, true);
  stage_store(tiles[0], true);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AfTile& tl = tiles[AF_LAB(64) ? 0 : (t & 1)];
    if (t + 1 < ntiles && !AF_LAB(64)) stage_load(t + 1, true);
    const int nk = !EXTENT || V - t * AF_KT > AF_KT ? AF_KT : V - t * AF_KT;
    if (!EXTENT || nk == AF_KT) {
#pragma unroll 2
      for (int k0 = 0; k0 < AF_KT; k0 += 32) AF_PASS2_BLOCK((void)0)
    } else {
      for (int k0 = 0; k0 < nk; k0 += 32) AF_PASS2_BLOCK(af_mask_keys(s0, s1, k0 + 4 * kg, nk))
    }
    if (t + 1 < ntiles && !AF_LAB(64)) stage_store(tiles[(t + 1) & 1], true);
    __syncthreads();
  }
  // rows dim (v_h) and 8 + dim (v_l) live in lanes kg and kg + 2; the row sum is spread over the 4 kg lanes of a query
#pragma unroll
  for (int g = 0; g < AF_QG; ++g) {
    float l = lsum[g];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 o = oacc[g];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] += __shfl_xor(o[r], 32, 64);
    const int lq = q0 + g * 16 + j;
    if (kg < 2 && (!EXTENT || lq < V)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = o[r] / l;
      // (the on-grid sum is kept term by term: as one int it costs the on-grid instantiation 6 VGPRs and a wave of occupancy)
      const size_t tok = EXTENT ? (size_t)n * T + ab_token(lq, W, vw) : (size_t)n * T + q0 + g * 16 + j;
      *(f32x4*)(out + tok * C + h * 8 + 4 * kg) = o;
    }
  }
}

extern "C" int dmd_attention(const float* qkv, float* out, int N, int T, int C, int head_dim, dmd_stream_t stream) {
  if (att_check_args("attention", qkv && out, N, 1, T, 1, T, C, head_dim)) return 1;
  DMD_CHECK_ARG(T % 64 == 0, "attention: need T %% 64 == 0 (T=%d)", T);
  if (T % 256 == 0) {
    // whole 256-key tiles (256 tokens of the default 16x16 level, 1024 / 4096 of the 256x256 configuration): split-fp16 two-pass kernel
    hipLaunchKernelGGL(attention_f16x2_kernel<false>, dim3(T / 256, C / 8, N), dim3(256), 0, (hipStream_t)stream, qkv, out, T, C,
                       1.4426950408889634f / sqrtf((float)head_dim), 0, 0, 0, 0);
    DMD_LAUNCH_CHECK();
    return 0;
  }
  dim3 grid(T / 64, C / 8, N);
  hipLaunchKernelGGL(attention_kernel, grid, dim3(256), 0, (hipStream_t)stream, qkv, out, T, C, sqrtf((float)head_dim), 0, 0, 0);
  DMD_LAUNCH_CHECK();
  return 0;
}

// The same over an (H, W) token grid of which only (valid_h, valid_w) exists (dmd_conv_params: VALID EXTENT): keys outside
// it do not take part in the softmax; the outputs of queries outside it are unspecified.
extern "C" int dmd_attention_valid(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                                   dmd_stream_t stream) {
  if (att_check_args("attention_valid", qkv && out, N, H, W, valid_h, valid_w, C, head_dim)) return 1;
  const int T = H * W;
  DMD_CHECK_ARG(T % 64 == 0, "attention_valid: need H W %% 64 == 0 (H=%d W=%d)", H, W);
  dim3 grid(T / 64, C / 8, N);
  hipLaunchKernelGGL(attention_kernel, grid, dim3(256), 0, (hipStream_t)stream, qkv, out, T, C, sqrtf((float)head_dim), W, valid_h, valid_w);
  DMD_LAUNCH_CHECK();
  return 0;
}

// The split-fp16 two-pass kernel over the (valid_h, valid_w) extent of an (H, W) grid, any valid token count >= 1 (engine.attention
// in default precision from ATTN_F16X2_EXTENT_MIN_T valid tokens on: valid extents, and whole grids with T % 256 != 0 as the extent
// (1, T, 1, T)).  Asynchronous, no allocation.
extern "C" int dmd_attention_f16x2(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                                   dmd_stream_t stream) {
  if (att_check_args("attention_f16x2", qkv && out, N, H, W, valid_h, valid_w, C, head_dim)) return 1;
  const int T = H * W, V = valid_h * valid_w;
  const int nbv = (V + AF_KT - 1) / AF_KT, nbm = (T - V + 255) / 256;
  hipLaunchKernelGGL(attention_f16x2_kernel<true>, dim3(nbv + nbm, C / 8, N), dim3(256), 0, (hipStream_t)stream, qkv, out, T, C,
                     1.4426950408889634f / sqrtf((float)head_dim), W, valid_h, valid_w, nbv);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Attention backward (denoiser training step, denoiser.py:93-122 -> autograd of blocks.py:66-71).
//   P = softmax(q k^T / sqrt(d)),  y = P v.   Given dy:
//   D_i = dy_i . y_i ;  dP_ij = dy_i . v_j ;  dS_ij = P_ij (dP_ij - D_i)
//   dq_i = sum_j dS_ij k_j / sqrt(d) ;  dk_j = sum_i dS_ij q_i / sqrt(d) ;  dv_j = sum_i P_ij dy_i
// ONE pair of kernels, fp32 VALU, one thread per valid query (key) sweeping all valid keys (queries) serially: the SMALL-T path (64
// tokens at the 8x8 level, 256 at the default denoiser's 16x16 level, valid extents off the tile grid), where a step is bound by its
// launches rather than by these FLOPs.  Long token grids (1024 / 4096 tokens of the 256x256 configuration) take
// dmd_attention_bwd_mfma further down; grad_ops.attention_bwd chooses by the valid token count (ATTN_BWD_MFMA_MIN_T).
//   rows kernel: one thread per query row i -- softmax statistics (m_i, l_i) by a first sweep over the keys, then dq_i;
//                writes (m_i, l_i, D_i) for the second kernel, indexed by the valid token; its workgroups behind the valid ones
//                (blockIdx.x >= nbv) write the dqkv rows outside the extent as zero;
//   cols kernel: one thread per key row j -- dk_j, dv_j by a sweep over the queries.
// Thread li <-> valid token (li / vw, li % vw); the sweeps walk the valid rows and columns in token order, so every way of writing
// the same tokens -- (H, W, H, W), or dmd_attention_bwd's (1, T, 1, T), one outer iteration and a flat sweep -- forms every sum in
// the same order (bitwise the same result).  Nothing outside the extent is read (the margins of qkv / y / dy are unspecified, NaN
// included).
// ------------------------------------------------------------------------------------------------
struct f8 {
  float v[8];
};
__device__ __forceinline__ f8 ld8(const float* p) {
  f8 r;
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r.v[e] = a[e];
    r.v[4 + e] = b[e];
  }
  return r;
}
__device__ __forceinline__ float dot8(const f8& a, const f8& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s = __builtin_fmaf(a.v[e], b.v[e], s);
  return s;
}

__global__ __launch_bounds__(64) void attention_bwd_rows_kernel(const float* __restrict__ qkv, const float* __restrict__ y,
                                                                const float* __restrict__ dy, float* __restrict__ dqkv,
                                                                float* __restrict__ rowstat, int T, int W, int vh, int vw, int C,
                                                                int nbv) {
  const int h = blockIdx.y, n = blockIdx.z, NH = C / 8, V = vh * vw;
  if ((int)blockIdx.x >= nbv) {
    const int m = ((int)blockIdx.x - nbv) * 64 + threadIdx.x;
    if (m >= T - V) return;
    float* o = dqkv + ((size_t)n * T + ab_margin_token(m, W, vh, vw)) * 3 * C + h * 8;
    const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      *(f32x4*)(o + t * C) = z;
      *(f32x4*)(o + t * C + 4) = z;
    }
    return;
  }
  const int li = blockIdx.x * 64 + threadIdx.x;
  if (li >= V) return;
  const int i = ab_token(li, W, vw);
  const float scale = 0.35355339059327373f;  // 1 / sqrt(8)
  const size_t row = ((size_t)n * T + i);
  const f8 q = ld8(qkv + row * 3 * C + h * 8);
  const f8 yo = ld8(y + row * C + h * 8), dyo = ld8(dy + row * C + h * 8);
  const float D = dot8(dyo, yo);
  const float* kbase = qkv + (size_t)n * T * 3 * C + C + h * 8;
  const float* vbase = kbase + C;
  float m = -INFINITY, l = 0.f;
  for (int jr = 0; jr < vh; ++jr) {
    const float* krow = kbase + (size_t)jr * W * 3 * C;
    for (int jc = 0; jc < vw; ++jc) {
      const float s = dot8(q, ld8(krow + (size_t)jc * 3 * C)) * scale;
      const float mn = fmaxf(m, s);
      l = l * expf(m - mn) + expf(s - mn);
      m = mn;
    }
  }
  f8 dq;
#pragma unroll
  for (int e = 0; e < 8; ++e) dq.v[e] = 0.f;
  for (int jr = 0; jr < vh; ++jr) {
    const float* krow = kbase + (size_t)jr * W * 3 * C;
    const float* vrow = vbase + (size_t)jr * W * 3 * C;
    for (int jc = 0; jc < vw; ++jc) {
      const f8 k = ld8(krow + (size_t)jc * 3 * C);
      const float s = dot8(q, k) * scale;
      const float p = expf(s - m) / l;
      const float ds = p * (dot8(dyo, ld8(vrow + (size_t)jc * 3 * C)) - D);
#pragma unroll
      for (int e = 0; e < 8; ++e) dq.v[e] = __builtin_fmaf(ds * scale, k.v[e], dq.v[e]);
    }
  }
  float* o = dqkv + row * 3 * C + h * 8;
  *(f32x4*)o = (f32x4){dq.v[0], dq.v[1], dq.v[2], dq.v[3]};
  *(f32x4*)(o + 4) = (f32x4){dq.v[4], dq.v[5], dq.v[6], dq.v[7]};
  float* rs = rowstat + (((size_t)n * NH + h) * V + li) * 4;
  rs[0] = m;
  rs[1] = l;
  rs[2] = D;
}

__global__ __launch_bounds__(64) void attention_bwd_cols_kernel(const float* __restrict__ qkv, const float* __restrict__ dy,
                                                                const float* __restrict__ rowstat, float* __restrict__ dqkv, int T,
                                                                int W, int vh, int vw, int C) {
  const int lj = blockIdx.x * 64 + threadIdx.x, h = blockIdx.y, n = blockIdx.z, NH = C / 8, V = vh * vw;
  if (lj >= V) return;
  const int j = ab_token(lj, W, vw);
  const float scale = 0.35355339059327373f;
  const size_t row = ((size_t)n * T + j);
  const f8 k = ld8(qkv + row * 3 * C + C + h * 8), v = ld8(qkv + row * 3 * C + 2 * C + h * 8);
  const float* qbase = qkv + (size_t)n * T * 3 * C + h * 8;
  const float* dybase = dy + (size_t)n * T * C + h * 8;
  const float* rs = rowstat + ((size_t)n * NH + h) * V * 4;
  f8 dk, dv;
#pragma unroll
  for (int e = 0; e < 8; ++e) dk.v[e] = dv.v[e] = 0.f;
  for (int ir = 0; ir < vh; ++ir) {
    const float* qrow = qbase + (size_t)ir * W * 3 * C;
    const float* dyrow = dybase + (size_t)ir * W * C;
    const float* rsr = rs + (size_t)ir * vw * 4;
    for (int ic = 0; ic < vw; ++ic) {
      const f8 q = ld8(qrow + (size_t)ic * 3 * C);
      const f8 dyo = ld8(dyrow + (size_t)ic * C);
      const float s = dot8(q, k) * scale;
      const float p = expf(s - rsr[4 * ic]) / rsr[4 * ic + 1];
      const float ds = p * (dot8(dyo, v) - rsr[4 * ic + 2]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dk.v[e] = __builtin_fmaf(ds * scale, q.v[e], dk.v[e]);
        dv.v[e] = __builtin_fmaf(p, dyo.v[e], dv.v[e]);
      }
    }
  }
  float* o = dqkv + row * 3 * C + C + h * 8;
  *(f32x4*)o = (f32x4){dk.v[0], dk.v[1], dk.v[2], dk.v[3]};
  *(f32x4*)(o + 4) = (f32x4){dk.v[4], dk.v[5], dk.v[6], dk.v[7]};
  o += C;
  *(f32x4*)o = (f32x4){dv.v[0], dv.v[1], dv.v[2], dv.v[3]};
  *(f32x4*)(o + 4) = (f32x4){dv.v[4], dv.v[5], dv.v[6], dv.v[7]};
}

extern "C" int64_t dmd_attention_bwd_workspace_floats(int N, int T, int C) { return (int64_t)N * (C / 8) * T * 4; }

// the scalar pair over the (vh, vw) extent of an (H, W) grid; vw == W, vh == H: no margin workgroup (nbm == 0)
static int att_bwd_scalar(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int H, int W, int vh,
                          int vw, int C, hipStream_t st) {
  const int T = H * W, V = vh * vw;
  const int nbv = (V + 63) / 64, nbm = (T - V + 63) / 64;
  hipLaunchKernelGGL(attention_bwd_rows_kernel, dim3(nbv + nbm, C / 8, N), dim3(64), 0, st, qkv, y, dy, dqkv, workspace, T, W, vh, vw, C,
                     nbv);
  hipLaunchKernelGGL(attention_bwd_cols_kernel, dim3(nbv, C / 8, N), dim3(64), 0, st, qkv, dy, (const float*)workspace, dqkv, T, W, vh,
                     vw, C);
  DMD_LAUNCH_CHECK();
  return 0;
}

// any T > 0: the whole grid is the extent (1, T, 1, T) of a (1, T) grid
extern "C" int dmd_attention_bwd(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int T,
                                 int C, int head_dim, dmd_stream_t stream) {
  if (att_check_args("attention_bwd", qkv && y && dy && dqkv && workspace, N, 1, T, 1, T, C, head_dim)) return 1;
  return att_bwd_scalar(qkv, y, dy, dqkv, workspace, N, 1, T, 1, T, C, (hipStream_t)stream);
}

// the gradient of dmd_attention_valid; the dqkv rows outside the extent are written as zero
extern "C" int dmd_attention_bwd_valid(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int H,
                                       int W, int valid_h, int valid_w, int C, int head_dim, dmd_stream_t stream) {
  if (att_check_args("attention_bwd_valid", qkv && y && dy && dqkv && workspace, N, H, W, valid_h, valid_w, C, head_dim)) return 1;
  return att_bwd_scalar(qkv, y, dy, dqkv, workspace, N, H, W, valid_h, valid_w, C, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// dmd_attention_bwd_mfma -- the same gradient (formulae above attention_bwd_rows_kernel) for LONG token grids, on
// v_mfma_f32_16x16x4_f32 with exact fp32 operands (dy has no bounded range: no split-fp16 here).  The structure mirrors the scalar
// pair -- a query-side kernel that owns dq and the row statistics, a key-side kernel that owns dk and dv -- so there are no
// atomics and every sum has a fixed order.  Tokens are addressed by their VALID index li <-> token (li / vw) * W + li % vw of an
// (H, W) grid (dmd_attention_bwd_valid's convention; the full grid is H = 1, W = T): nothing outside the extent is read, and the
// whole-grid call walks the tokens exactly as the (1, T, 1, T) call does.
//   attention_bwd_mfma_q_kernel: 4 waves x 16 queries; K / V tiles of 256 keys double-buffered in LDS.  attention_kernel's
//     layout trick: S^T[key][query] = K Q^T and dP^T = V dY^T leave lane (j = lane & 15, kg = lane >> 4) with keys {4 kg + r} of
//     ONE query j, so m, D and 1 / l are per-lane scalars and the four p~ (dP - D) are directly the B operand of
//     dq^T[dim][query] += K^T dS~^T.  TWO passes over the keys: the first finds the row maximum m of the raw dot products q . k,
//     the second forms p~ = 2^((q . k - m) log2(e) / sqrt(d)) (one subtraction, one multiplication, one v_exp_f32 per pair; exactly
//     softmax's x - max(x)), the row sum l and dq~; dq = dq~ / l / sqrt(d).  Keys behind the last valid one get the score -inf
//     (their LDS rows are zero).  Writes (m, l, D, 0) per valid query into the workspace.  Its workgroups behind the valid ones
//     write the dqkv rows outside the extent as zero.
//   attention_bwd_mfma_k_kernel: 4 waves x 16 keys, k and v of the lane's key in registers; tiles of 128 queries (q, dy, both
//     also transposed, and (m, 1 / l, D)) double-buffered in LDS.  S[query][key] and dP = dY V^T have the key in the lane's column;
//     dk^T[dim][key] += Q^T dS, dv^T[dim][key] += dY^T P.  Query rows behind the last valid one are zero with 1 / l = 0.
// Lanes of a partial last block compute on the last valid token and write nothing.
// ------------------------------------------------------------------------------------------------
#define AB_KT 256                 // keys per LDS tile of the query-side kernel
#define AB_QT 128                 // queries per LDS tile of the key-side kernel
#define AB_PAD 16                 // row padding of the transposed copies
#define AB_EXP_SCALE 0.51006973f  // log2(e) / sqrt(8)
#define AB_SCALE 0.35355339059327373f

struct AbKeyTile {
  float k[AB_KT][8];
  float v[AB_KT][8];
  float kt[8][AB_KT + AB_PAD];  // K^T[dim][key]
};

struct AbQueryTile {
  float q[AB_QT][8];
  float dy[AB_QT][8];
  float qt[8][AB_QT + AB_PAD];   // Q^T[dim][query]
  float dyt[8][AB_QT + AB_PAD];  // dY^T[dim][query]
  f32x4 st[AB_QT];               // m, 1 / l, D, 0
};

__global__ __launch_bounds__(256) void attention_bwd_mfma_q_kernel(const float* __restrict__ qkv, const float* __restrict__ y,
                                                                   const float* __restrict__ dy, float* __restrict__ dqkv,
                                                                   float* __restrict__ rowstat, int T, int W, int vh, int vw, int C,
                                                                   int nbv) {
  __shared__ AbKeyTile tiles[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kg = lane >> 4;
  const int n = blockIdx.z, h = blockIdx.y, NH = C / 8, V = vh * vw;
  const size_t row = (size_t)3 * C;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x >= nbv) {
    const int m = ((int)blockIdx.x - nbv) * 256 + tid;
    if (m >= T - V) return;
    float* o = dqkv + ((size_t)n * T + ab_margin_token(m, W, vh, vw)) * row + h * 8;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      *(f32x4*)(o + t * C) = zero4;
      *(f32x4*)(o + t * C + 4) = zero4;
    }
    return;
  }
  const float* base = qkv + (size_t)n * T * row;
  const int lq = blockIdx.x * 64 + wave * 16 + j;
  const size_t qtok = (size_t)n * T + ab_token(lq < V ? lq : V - 1, W, vw);
  // B operands of S^T = K Q^T and dP^T = V dY^T: lane (query j, k' = kg), step s uses dim 2 kg + s
  const float* qp = qkv + qtok * row + h * 8 + 2 * kg;
  const float* dyp = dy + qtok * C + h * 8 + 2 * kg;
  const float* yp = y + qtok * C + h * 8 + 2 * kg;
  const float qa = qp[0], qb = qp[1], da = dyp[0], db = dyp[1];
  float D = __builtin_fmaf(db, yp[1], da * yp[0]);
  D += __shfl_xor(D, 16, 64);
  D += __shfl_xor(D, 32, 64);

  const int ntiles = (V + AB_KT - 1) / AB_KT;
  f32x4 sk0, sk1, sv0, sv1;
  auto stage_load = [&](int t, bool with_v) {
    const int lk = t * AB_KT + tid;
    sk0 = sk1 = sv0 = sv1 = zero4;
    if (lk < V) {
      const float* kp = base + (size_t)ab_token(lk, W, vw) * row + C + h * 8;
      sk0 = *(const f32x4*)kp;
      sk1 = *(const f32x4*)(kp + 4);
      if (with_v) {
        sv0 = *(const f32x4*)(kp + C);
        sv1 = *(const f32x4*)(kp + C + 4);
      }
    }
  };
  auto stage_store = [&](AbKeyTile& tl, bool with_v) {
    *(f32x4*)&tl.k[tid][0] = sk0;
    *(f32x4*)&tl.k[tid][4] = sk1;
    if (with_v) {
      *(f32x4*)&tl.v[tid][0] = sv0;
      *(f32x4*)&tl.v[tid][4] = sv1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        tl.kt[e][tid] = sk0[e];
        tl.kt[4 + e][tid] = sk1[e];
      }
    }
  };
  // S^T block of 16 keys from k0: s[r] = q_j . k_{k0 + 4 kg + r}, -inf behind the tile's nk keys
  auto scores = [&](const AbKeyTile& tl, int k0, int nk) -> f32x4 {
    f32x4 s = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.k[k0 + j][2 * kg], qa, zero4, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.k[k0 + j][2 * kg + 1], qb, s, 0, 0, 0);
    if (k0 + 16 > nk) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (k0 + 4 * kg + r >= nk) s[r] = -INFINITY;
    }
    return s;
  };

  // ---------------- pass 1: row maxima of q . k ----------------
  float m = -INFINITY;
  stage_load(0, false);
  stage_store(tiles[0], false);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AbKeyTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1, false);
    const int nk = (V - t * AB_KT) < AB_KT ? (V - t * AB_KT) : AB_KT;
    for (int k0 = 0; k0 < nk; k0 += 16) {
      const f32x4 s = scores(tl, k0, nk);
      m = fmaxf(fmaxf(fmaxf(m, s[0]), fmaxf(s[1], s[2])), s[3]);
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1], false);
    __syncthreads();
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---------------- pass 2: weights, row sum, dq~^T[dim][query] += K^T dS~^T ----------------
  f32x4 acc = zero4;  // dq~^T[dd = 4 kg + r][query j]  (kg >= 2: padding rows)
  float l = 0.f;
  stage_load(0, true);
  stage_store(tiles[0], true);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AbKeyTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1, true);
    const int nk = (V - t * AB_KT) < AB_KT ? (V - t * AB_KT) : AB_KT;
    for (int k0 = 0; k0 < nk; k0 += 16) {
      const f32x4 s = scores(tl, k0, nk);
      f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.v[k0 + j][2 * kg], da, zero4, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.v[k0 + j][2 * kg + 1], db, dp, 0, 0, 0);
      f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = __builtin_amdgcn_exp2f((s[r] - m) * AB_EXP_SCALE);
        ds[r] = p[r] * (dp[r] - D);
      }
      l += (p[0] + p[1]) + (p[2] + p[3]);
      // A = K^T[dd i = lane & 15][key 4 kg + t], B = dS~^T[key][query j] = ds[t]
      f32x4 kf = zero4;
      if (j < 8) kf = *(const f32x4*)&tl.kt[j][k0 + 4 * kg];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[u], ds[u], acc, 0, 0, 0);
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1], true);
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (lq < V) {
    if (kg < 2) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = acc[r] / l * AB_SCALE;
      *(f32x4*)(dqkv + qtok * row + h * 8 + 4 * kg) = o;
    }
    if (kg == 0) *(f32x4*)(rowstat + (((size_t)n * NH + h) * V + lq) * 4) = (f32x4){m, l, D, 0.f};
  }
}

__global__ __launch_bounds__(256) void attention_bwd_mfma_k_kernel(const float* __restrict__ qkv, const float* __restrict__ dy,
                                                                   const float* __restrict__ rowstat, float* __restrict__ dqkv,
                                                                   int T, int W, int vh, int vw, int C) {
  __shared__ AbQueryTile tiles[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kg = lane >> 4;
  const int n = blockIdx.z, h = blockIdx.y, NH = C / 8, V = vh * vw;
  const size_t row = (size_t)3 * C;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int lk = blockIdx.x * 64 + wave * 16 + j;
  const size_t ktok = (size_t)n * T + ab_token(lk < V ? lk : V - 1, W, vw);
  // B operands of S = Q K^T and dP = dY V^T: lane (key j, k' = kg), step s uses dim 2 kg + s
  const float* kp = qkv + ktok * row + C + h * 8 + 2 * kg;
  const float ka = kp[0], kb = kp[1], va = kp[C], vb = kp[C + 1];
  const float* rs = rowstat + ((size_t)n * NH + h) * V * 4;

  // staging of one query tile: threads 0..127 the q row of query tid, threads 128..255 the dy row and the statistics
  const int srow = tid & (AB_QT - 1), shalf = tid >> 7;
  const int ntiles = (V + AB_QT - 1) / AB_QT;
  f32x4 s0, s1, sst;
  auto stage_load = [&](int t) {
    const int li = t * AB_QT + srow;
    s0 = s1 = sst = zero4;
    if (li < V) {
      const size_t tok = (size_t)n * T + ab_token(li, W, vw);
      const float* p = shalf ? dy + tok * C + h * 8 : qkv + tok * row + h * 8;
      s0 = *(const f32x4*)p;
      s1 = *(const f32x4*)(p + 4);
      if (shalf) {
        const f32x4 st = *(const f32x4*)(rs + (size_t)li * 4);
        sst = (f32x4){st[0], 1.0f / st[1], st[2], 0.f};
      }
    }
  };
  auto stage_store = [&](AbQueryTile& tl) {
    float(*rows)[8] = shalf ? tl.dy : tl.q;
    float(*cols)[AB_QT + AB_PAD] = shalf ? tl.dyt : tl.qt;
    *(f32x4*)&rows[srow][0] = s0;
    *(f32x4*)&rows[srow][4] = s1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cols[e][srow] = s0[e];
      cols[4 + e][srow] = s1[e];
    }
    if (shalf) tl.st[srow] = sst;
  };

  f32x4 dk = zero4, dv = zero4;  // dk~^T / dv^T[dd = 4 kg + r][key j]  (kg >= 2: padding rows)
  stage_load(0);
  stage_store(tiles[0]);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AbQueryTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1);
    const int nq = (V - t * AB_QT) < AB_QT ? (V - t * AB_QT) : AB_QT;
    for (int i0 = 0; i0 < nq; i0 += 16) {
      // S[query 4 kg + r][key j]: A = Q[query i = lane & 15][dim], B = K^T[dim][key j]
      f32x4 s = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.q[i0 + j][2 * kg], ka, zero4, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.q[i0 + j][2 * kg + 1], kb, s, 0, 0, 0);
      f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.dy[i0 + j][2 * kg], va, zero4, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x4f32(tl.dy[i0 + j][2 * kg + 1], vb, dp, 0, 0, 0);
      f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 st = tl.st[i0 + 4 * kg + r];
        p[r] = __builtin_amdgcn_exp2f((s[r] - st[0]) * AB_EXP_SCALE) * st[1];
        ds[r] = p[r] * (dp[r] - st[2]);
      }
      // A = Q^T / dY^T[dd i = lane & 15][query 4 kg + u], B = dS / P[query][key j]
      f32x4 qf = zero4, df = zero4;
      if (j < 8) {
        qf = *(const f32x4*)&tl.qt[j][i0 + 4 * kg];
        df = *(const f32x4*)&tl.dyt[j][i0 + 4 * kg];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dk = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[u], ds[u], dk, 0, 0, 0);
        dv = __builtin_amdgcn_mfma_f32_16x16x4f32(df[u], p[u], dv, 0, 0, 0);
      }
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1]);
    __syncthreads();
  }
  if (lk < V && kg < 2) {
    float* o = dqkv + ktok * row + C + h * 8 + 4 * kg;
    *(f32x4*)o = dk * AB_SCALE;
    *(f32x4*)(o + C) = dv;
  }
}

extern "C" int dmd_attention_bwd_mfma(const float* qkv, const float* y, const float* dy, float* dqkv, float* workspace, int N, int H,
                                      int W, int valid_h, int valid_w, int C, int head_dim, dmd_stream_t stream) {
  if (att_check_args("attention_bwd_mfma", qkv && y && dy && dqkv && workspace, N, H, W, valid_h, valid_w, C, head_dim)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const int T = H * W, V = valid_h * valid_w;
  const int nbv = (V + 63) / 64, nbm = (T - V + 255) / 256;
  hipLaunchKernelGGL(attention_bwd_mfma_q_kernel, dim3(nbv + nbm, C / 8, N), dim3(256), 0, st, qkv, y, dy, dqkv, workspace, T, W,
                     valid_h, valid_w, C, nbv);
  hipLaunchKernelGGL(attention_bwd_mfma_k_kernel, dim3(nbv, C / 8, N), dim3(256), 0, st, qkv, dy, (const float*)workspace, dqkv, T, W,
                     valid_h, valid_w, C);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// dmd_attention_f32 -- the EXACT forward for long token grids (engine.attention under DIAMOND_ATTN_PRECISION=f32, from
// ATTN_F32_TILED_MIN_T valid tokens on): softmax(q k^T / sqrt(d)) v on v_mfma_f32_16x16x4_f32 with exact fp32 operands, fp32
// throughout (IEEE subtraction, multiplication, sums and division; the exponential is v_exp_f32, about 1 ulp, as in
// attention_bwd_mfma_q_kernel).  attention_f32_tiled_kernel is attention_bwd_mfma_q_kernel's forward half: 4 waves x AT_QG groups of 16 queries, K
// (pass 2: K and V^T) tiles of 256 keys double-buffered in LDS and staged by all 256 threads (the next tile is loaded into
// registers before the compute loop and stored behind it), tokens addressed by their VALID index (ab_token), S^T = K Q^T so that
// lane (j = lane & 15, kg = lane >> 4) owns keys {4 kg + r} of ONE query j.  TWO passes over the keys: the first finds the row
// maximum m of the raw q . k, the second forms p = 2^((q . k - m) log2(e) / sqrt(d)), the row sum l (per lane in key order, the
// four lanes of a query combined once at the end) and O^T[dim][query] += V^T P^T with the four p directly as the B operand
// (attention_kernel's k-remap); out = O / l.  Inside the key loop there is no rescale, no shuffle, no division and no integer
// division; no atomics anywhere: every sum has a fixed order that depends on the (image, head)'s own tokens only.  Keys behind the
// last valid one get the score -inf (their LDS rows are zero).  The workgroups behind the valid ones write the rows of `out` outside
// the extent as +0.  Lanes of a partial last block compute on the last valid token and write nothing.
// AT_QG (16-query groups per wave, which share the wave's LDS reads of K and V^T) and AT_UNROLL (16-key blocks of a whole tile per
// loop iteration; 1 = the rolled loop) were measured side by side: profiles/attention_f32_tiled.json, "query_groups_per_wave";
// HISTORY.md has the figures, what made a difference (whole tiles have a loop of their own: constant trip count, no key mask) and
// what did not (the unroll factor).
// ------------------------------------------------------------------------------------------------
#ifndef AT_QG
#define AT_QG 2
#endif
#ifndef AT_UNROLL
#define AT_UNROLL 4  // 16-key blocks of a whole tile per loop iteration
#endif

struct AtKeyTile {
  float k[AB_KT][8];
  float vt[8][AB_KT + AB_PAD];  // V^T[dim][key]
};

__global__ __launch_bounds__(256) void attention_f32_tiled_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int W,
                                                                  int vh, int vw, int C, int nbv) {
  __shared__ AtKeyTile tiles[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kg = lane >> 4;
  const int n = blockIdx.z, h = blockIdx.y, V = vh * vw;
  const size_t row = (size_t)3 * C;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x >= nbv) {
    const int m = ((int)blockIdx.x - nbv) * 256 + tid;
    if (m >= T - V) return;
    float* o = out + ((size_t)n * T + ab_margin_token(m, W, vh, vw)) * C + h * 8;
    *(f32x4*)o = zero4;
    *(f32x4*)(o + 4) = zero4;
    return;
  }
  const float* base = qkv + (size_t)n * T * row;
  // B operand of S^T = K Q^T per 16-query group: lane (query j, k' = kg), step s uses dim 2 kg + s
  int lq[AT_QG];
  size_t qtok[AT_QG];
  float qa[AT_QG], qb[AT_QG];
#pragma unroll
  for (int g = 0; g < AT_QG; ++g) {
    lq[g] = (blockIdx.x * 4 + wave) * (16 * AT_QG) + g * 16 + j;
    qtok[g] = (size_t)n * T + ab_token(lq[g] < V ? lq[g] : V - 1, W, vw);
    const float* qp = qkv + qtok[g] * row + h * 8 + 2 * kg;
    qa[g] = qp[0];
    qb[g] = qp[1];
  }

  const int ntiles = (V + AB_KT - 1) / AB_KT;
  f32x4 sk0, sk1, sv0, sv1;
  auto stage_load = [&](int t, bool with_v) {
    const int lk = t * AB_KT + tid;
    sk0 = sk1 = sv0 = sv1 = zero4;
    if (lk < V) {
      const float* kp = base + (size_t)ab_token(lk, W, vw) * row + C + h * 8;
      sk0 = *(const f32x4*)kp;
      sk1 = *(const f32x4*)(kp + 4);
      if (with_v) {
        sv0 = *(const f32x4*)(kp + C);
        sv1 = *(const f32x4*)(kp + C + 4);
      }
    }
  };
  auto stage_store = [&](AtKeyTile& tl, bool with_v) {
    *(f32x4*)&tl.k[tid][0] = sk0;
    *(f32x4*)&tl.k[tid][4] = sk1;
    if (with_v) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        tl.vt[e][tid] = sv0[e];
        tl.vt[4 + e][tid] = sv1[e];
      }
    }
  };
  // S^T block of 16 keys: s[r] = q_j . k_{k0 + 4 kg + r} from the lane's K fragment, -inf behind the tile's nk keys
  auto scores = [&](float ka, float kb, int g, int k0, int nk) -> f32x4 {
    f32x4 s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, qa[g], zero4, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kb, qb[g], s, 0, 0, 0);
    if (k0 + 16 > nk) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (k0 + 4 * kg + r >= nk) s[r] = -INFINITY;
    }
    return s;
  };

  // ---------------- pass 1: row maxima of q . k ----------------
  float m[AT_QG];
#pragma unroll
  for (int g = 0; g < AT_QG; ++g) m[g] = -INFINITY;
  stage_load(0, false);
  stage_store(tiles[0], false);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AtKeyTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1, false);
    const int nk = (V - t * AB_KT) < AB_KT ? (V - t * AB_KT) : AB_KT;
    auto block = [&](int k0, int nk) {
      const float ka = tl.k[k0 + j][2 * kg], kb = tl.k[k0 + j][2 * kg + 1];
#pragma unroll
      for (int g = 0; g < AT_QG; ++g) {
        const f32x4 s = scores(ka, kb, g, k0, nk);
        m[g] = af_max3(af_max3(m[g], s[0], s[1]), s[2], s[3]);
      }
    };
    if (nk == AB_KT) {  // a whole tile: constant trip count, no key mask (the same operations in the same order)
#pragma unroll AT_UNROLL
      for (int k0 = 0; k0 < AB_KT; k0 += 16) block(k0, AB_KT);
    } else {
      for (int k0 = 0; k0 < nk; k0 += 16) block(k0, nk);
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1], false);
    __syncthreads();
  }
#pragma unroll
  for (int g = 0; g < AT_QG; ++g) {
    m[g] = fmaxf(m[g], __shfl_xor(m[g], 16, 64));
    m[g] = fmaxf(m[g], __shfl_xor(m[g], 32, 64));
  }

  // ---------------- pass 2: weights, row sums, O^T[dim][query] += V^T P^T ----------------
  f32x4 acc[AT_QG];  // O~^T[dd = 4 kg + r][query j]  (kg >= 2: padding rows)
  float l[AT_QG];
#pragma unroll
  for (int g = 0; g < AT_QG; ++g) {
    acc[g] = zero4;
    l[g] = 0.f;
  }
  stage_load(0, true);
  stage_store(tiles[0], true);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const AtKeyTile& tl = tiles[t & 1];
    if (t + 1 < ntiles) stage_load(t + 1, true);
    const int nk = (V - t * AB_KT) < AB_KT ? (V - t * AB_KT) : AB_KT;
    auto block = [&](int k0, int nk) {
      const float ka = tl.k[k0 + j][2 * kg], kb = tl.k[k0 + j][2 * kg + 1];
      // A = V^T[dd i = lane & 15][key 4 kg + u], B = P^T[key][query j] = p[u]
      f32x4 vf = zero4;
      if (j < 8) vf = *(const f32x4*)&tl.vt[j][k0 + 4 * kg];
#pragma unroll
      for (int g = 0; g < AT_QG; ++g) {
        const f32x4 s = scores(ka, kb, g, k0, nk);
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f((s[r] - m[g]) * AB_EXP_SCALE);
        l[g] += (p[0] + p[1]) + (p[2] + p[3]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[u], p[u], acc[g], 0, 0, 0);
      }
    };
    if (nk == AB_KT) {
#pragma unroll AT_UNROLL
      for (int k0 = 0; k0 < AB_KT; k0 += 16) block(k0, AB_KT);
    } else {
      for (int k0 = 0; k0 < nk; k0 += 16) block(k0, nk);
    }
    if (t + 1 < ntiles) stage_store(tiles[(t + 1) & 1], true);
    __syncthreads();
  }
#pragma unroll
  for (int g = 0; g < AT_QG; ++g) {
    float ls = l[g];
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    if (lq[g] < V && kg < 2) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = acc[g][r] / ls;
      *(f32x4*)(out + qtok[g] * C + h * 8 + 4 * kg) = o;
    }
  }
}

extern "C" int dmd_attention_f32(const float* qkv, float* out, int N, int H, int W, int valid_h, int valid_w, int C, int head_dim,
                                 dmd_stream_t stream) {
  if (att_check_args("attention_f32", qkv && out, N, H, W, valid_h, valid_w, C, head_dim)) return 1;
  const int T = H * W, V = valid_h * valid_w;
  const int nbv = (V + 64 * AT_QG - 1) / (64 * AT_QG), nbm = (T - V + 255) / 256;
  hipLaunchKernelGGL(attention_f32_tiled_kernel, dim3(nbv + nbm, C / 8, N), dim3(256), 0, (hipStream_t)stream, qkv, out, T, W, valid_h,
                     valid_w, C, nbv);
  DMD_LAUNCH_CHECK();
  return 0;
}
