// dmd_linear -- C[M,N] (+)= A[M,K] . W[N,K]^T + bias, optional SiLU, on v_mfma_f32_16x16x4_f32.
//
// nn.Linear call sites of the hot path: the 44 AdaGroupNorm linears of a denoiser forward
// batched into ONE (B,256)x(256,7168) call (blocks.py:39,44 share `cond`, blocks.py:171-177),
// cond_proj (inner_model.py:31-35), LSTM gate GEMMs (actor_critic.py:46,72;
// rew_end_model.py:34,53), heads (actor_critic.py:47-48; rew_end_model.py:35-39).
//
// Both operands are K-contiguous ("NT" GEMM), so MFMA fragments are plain 16-byte global
// loads: lane (i = lane & 15, kg = lane >> 4) reads A[m0 + i][k0 + 4 kg .. +3] and
// W[n0 + i][k0 + 4 kg .. +3]; the four components feed four MFMAs (k-remap, same trick as
// dmd_conv).  W is the MFMA A operand (rows = n), activations the B operand (cols = m), so a
// lane owns 4 consecutive n of one m -> 16-byte stores of C rows.
// These GEMMs are < 2 % of the step FLOPs and are L2-resident; no LDS staging.
#include "dmd_common.h"

// SPLITK = false: workgroup = 4 waves = 64 (m) x 64 (n) outputs, wave = 32 x 32 (2 x 2 MFMA blocks) over the whole K.
// SPLITK = true (deep-K GEMMs with few output tiles: the LSTM gate GEMMs, (256, 2048) x (2048, 2048)^T is only 128 tiles
// of 64 x 64 on 256 CUs, each a serial chain of 128 L2 round trips): workgroup = ONE 32 x 32 tile, wave w accumulates
// the K quarter [w K/4, (w + 1) K/4); the four partial tiles are added through LDS in the fixed order
// ((w0 + w1) + w2) + w3 -- deterministic, no atomics -- and wave 0 runs the epilogue.
// K loop: DEPTH fragment sets in flight (these GEMMs are L2-resident and latency-bound: a set is reloaded right after
// the MFMAs that consumed it have issued, DEPTH - 1 steps before it is needed again).
#define LIN_DEPTH 4

// One fragment (4 consecutive k of one row) of an operand in either storage order, TRANS instances only: element (row, k)
// lives at base[row * rs + k * ks] -- K-contiguous: rs = ld, ks = 1; given as (K, rows) row-major: rs = 1, ks = ld, where the
// 16 lanes of a row group read 16 consecutive floats per k (coalesced).  k >= K: the address is clamped and the value is an
// exact zero, which is what a zero-padded copy holds there.
__device__ __forceinline__ f32x4 lin_frag(const float* rowp, size_t ks, int k, int K) {
  f32x4 v;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int kk = k + t;
    const float x = rowp[(size_t)(kk < K ? kk : K - 1) * ks];
    v[t] = kk < K ? x : 0.f;
  }
  return v;
}

// TRANS = false: both operands K-contiguous, K a multiple of 16, 16-byte loads (every forward call site).
// TRANS = true: p.trans_a / p.trans_w say which operand is given transposed ((K, M) / (K, N) row-major, ld = its row stride);
// any K > 0, the loop runs over K rounded up to 16 with the tail masked.  Same lanes, same values, same MFMA order: bitwise
// the TRANS = false result on materialised K-contiguous, zero-padded copies.
template <bool SPLITK, bool TRANS>
__device__ __forceinline__ void linear_mfma_body(const dmd_linear_params& p) {
  __shared__ f32x4 part[SPLITK ? 3 : 1][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kg = lane >> 4;
  const int m0 = SPLITK ? blockIdx.x * 32 : blockIdx.x * 64 + (wave >> 1) * 32;
  const int n0 = SPLITK ? blockIdx.y * 32 : blockIdx.y * 64 + (wave & 1) * 32;
  const int Kp = TRANS ? (p.K + 15) & ~15 : p.K;
  const int kq = SPLITK ? Kp >> 2 : Kp;  // K range of this wave
  const int kbase = SPLITK ? wave * kq : 0;
  const int nsteps = kq >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const size_t a_rs = TRANS && p.trans_a ? 1 : (size_t)p.lda, a_ks = TRANS && p.trans_a ? (size_t)p.lda : 1;
  const size_t w_rs = TRANS && p.trans_w ? 1 : (size_t)p.ldw, w_ks = TRANS && p.trans_w ? (size_t)p.ldw : 1;
  const float* arow[2];
  const float* wrow[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    int m = m0 + 16 * b + i;
    m = m < p.M ? m : p.M - 1;  // clamp: duplicates are never stored
    int n = n0 + 16 * b + i;
    n = n < p.N ? n : p.N - 1;
    if (TRANS) {  // (row base only: the k offset goes through lin_frag's mask)
      arow[b] = p.A + (size_t)m * a_rs;
      wrow[b] = p.W + (size_t)n * w_rs;
    } else {
      arow[b] = p.A + (size_t)m * p.lda + kbase + 4 * kg;
      wrow[b] = p.W + (size_t)n * p.ldw + kbase + 4 * kg;
    }
  }
  const int kl = kbase + 4 * kg;  // first k of this lane's fragments (TRANS)
  f32x4 af[LIN_DEPTH][2], wf[LIN_DEPTH][2];
#pragma unroll
  for (int d = 0; d < LIN_DEPTH; ++d) {
    const int ks = (d < nsteps ? d : nsteps - 1) * 16;  // short K: harmless reload of the last step
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (TRANS) {
        af[d][b] = lin_frag(arow[b], a_ks, kl + ks, p.K);
        wf[d][b] = lin_frag(wrow[b], w_ks, kl + ks, p.K);
      } else {
        af[d][b] = *(const f32x4*)(arow[b] + ks);
        wf[d][b] = *(const f32x4*)(wrow[b] + ks);
      }
    }
  }
  for (int s0 = 0; s0 < nsteps; s0 += LIN_DEPTH) {
#pragma unroll
    for (int d = 0; d < LIN_DEPTH; ++d) {
      if (s0 + d < nsteps) {  // wave-uniform
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc[nb][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[d][nb][t], af[d][mb][t], acc[nb][mb], 0, 0, 0);
        const int sn = s0 + d + LIN_DEPTH;
        const int ks = (sn < nsteps ? sn : nsteps - 1) * 16;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          if (TRANS) {
            af[d][b] = lin_frag(arow[b], a_ks, kl + ks, p.K);
            wf[d][b] = lin_frag(wrow[b], w_ks, kl + ks, p.K);
          } else {
            af[d][b] = *(const f32x4*)(arow[b] + ks);
            wf[d][b] = *(const f32x4*)(wrow[b] + ks);
          }
        }
      }
    }
  }
  if (SPLITK) {
    if (wave) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) part[wave - 1][nb * 2 + mb][lane] = acc[nb][mb];
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) acc[nb][mb] += part[w][nb * 2 + mb][lane];
  }
  // D rows = n (4*kg + r), cols = m (i)
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int m = m0 + 16 * mb + i;
      const int n = n0 + 16 * nb + 4 * kg;
      if (m >= p.M) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (n + r >= p.N) continue;
        float v = acc[nb][mb][r];
        if (p.bias) v += p.bias[n + r];
        float* c = p.C + (size_t)m * p.ldc + n + r;
        if (p.accumulate) v += *c;
        if (p.silu) v = dmd_silu(v);
        *c = v;
      }
    }
}

template <bool SPLITK>
__global__ __launch_bounds__(256) void linear_mfma_kernel(const dmd_linear_params p) {
  linear_mfma_body<SPLITK, false>(p);
}

// either-storage-order instance (the backward's weight / data gradient GEMMs: no transposed or padded copies)
template <bool SPLITK>
__global__ __launch_bounds__(256) void linear_mfma_t_kernel(const dmd_linear_params p) {
  linear_mfma_body<SPLITK, true>(p);
}

extern "C" int dmd_linear(const dmd_linear_params* p, dmd_stream_t stream) {
  DMD_CHECK_ARG(p && p->A && p->W && p->C, "linear: null");
  DMD_CHECK_ARG(p->M > 0 && p->N > 0 && p->K > 0, "linear: bad M/N/K %d %d %d", p->M, p->N, p->K);
  DMD_CHECK_ARG((p->trans_a | p->trans_w | 1) == 1, "linear: trans_a / trans_w are 0 or 1");
  // the either-storage-order instance wherever the 16-byte loads cannot run: a transposed operand, a K tail, unaligned rows
  // (a row stride that is no multiple of 4 floats, or an operand that does not begin on a 16-byte boundary)
  const bool trans = p->trans_a || p->trans_w || p->K % 16 != 0 || p->lda % 4 != 0 || p->ldw % 4 != 0 ||
                     (uintptr_t)p->A % 16 != 0 || (uintptr_t)p->W % 16 != 0;
  // the choice depends on K alone -- not on M (the batch), the data or the device: an output row is summed in the same
  // order whatever the batch size it is computed in.  With a masked tail it is K rounded up to 16: the route of the call on
  // the zero-padded copy.
  const int Kp = (p->K + 15) / 16 * 16;
  const bool splitk = Kp >= 512 && Kp % 64 == 0;
  const dim3 grid = splitk ? dim3((p->M + 31) / 32, (p->N + 31) / 32) : dim3((p->M + 63) / 64, (p->N + 63) / 64);
  if (trans) {
    if (splitk)
      hipLaunchKernelGGL(linear_mfma_t_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    else
      hipLaunchKernelGGL(linear_mfma_t_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  } else if (splitk)
    hipLaunchKernelGGL(linear_mfma_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(linear_mfma_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  DMD_LAUNCH_CHECK();
  return 0;
}
