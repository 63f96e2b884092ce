// Pointwise / small kernels of the imagined-rollout path: EDM preconditioning and sampler
// updates (denoiser.py:66-84, diffusion_sampler.py:45-56), the cond embedding
// (blocks.py:84-87, inner_model.py:27-30), layout shuffles at the NCHW API boundary,
// GroupNorm partial statistics, 2x2 max-pool (actor_critic.py:108-109), the LSTM cell
// nonlinearity and Categorical sampling with injected exponential draws.
// All HBM-bound: coalesced, 16-byte accesses where the layout allows, one pass.
#include "dmd_common.h"

// ---- cat(obs / sigma_data, x * c_in) : NCHW -> NHWC(CPad) ------------------------------------
// One thread per (pixel, channel quad): the NCHW reads of a wave are 16 consecutive pixels of 4 x 4 planes (64-byte
// segments), the NHWC writes of a wave are 1 KiB contiguous (16 bytes per lane, consecutive lanes).
// The conditioning frames may live in a RING of T frames of Cobs / T channels each: logical frame t is stored at
// physical slot (head + t) % T (WorldModelEnv keeps its context that way instead of rolling it every step,
// world_model_env.py:74-75); T = 1, head = 0 is a plain (N, Cobs, H, W) tensor.
__global__ void edm_pack_input_kernel(const float* __restrict__ x, const float* __restrict__ obs,
                                      const float* __restrict__ cond, int cond_stride, float sd,
                                      float* __restrict__ out, int N, int Cx, int Cobs, int HW, int CPad, int T, int head) {
  // thread = (4 consecutive pixels, 4 consecutive output channels): four 16-byte plane reads (a wave reads 256 contiguous
  // bytes of each of its 4 planes), a 4x4 transpose in registers, four 16-byte NHWC stores
  const int Q = CPad >> 2, HW4 = HW >> 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * HW4 * Q) return;
  const int qd = idx % Q;
  const size_t npq = idx / Q;
  const int n = npq / HW4;
  const int pix0 = 4 * (int)(npq - (size_t)n * HW4);
  const float c_in = cond[(size_t)n * cond_stride + 0];
  const int cimg = Cobs / T;
  f32x4 t[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int cc = qd * 4 + e;
    t[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (cc < Cobs) {
      const int fr = cc / cimg, ci = cc - fr * cimg;
      int slot = fr + head;
      slot = slot >= T ? slot - T : slot;
      const f32x4 v = *(const f32x4*)(obs + ((size_t)n * Cobs + slot * cimg + ci) * HW + pix0);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[e][j] = v[j] / sd;  // rescaled_obs = obs / sigma_data, denoiser.py:75
    } else if (cc < Cobs + Cx) {
      const f32x4 v = *(const f32x4*)(x + ((size_t)n * Cx + (cc - Cobs)) * HW + pix0);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[e][j] = v[j] * c_in;  // denoiser.py:76
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *(f32x4*)(out + ((size_t)n * HW + pix0 + j) * CPad + qd * 4) = (f32x4){t[0][j], t[1][j], t[2][j], t[3][j]};
}

// ---- cond input: [cos(f) | sin(f)] + flatten(Embedding(act)),  f = 2 pi c_noise w -----------
__global__ void cond_embed_kernel(const float* __restrict__ cond, int cond_stride,
                                  const float* __restrict__ fw, const int64_t* __restrict__ act,
                                  const float* __restrict__ emb, float* __restrict__ out, int N, int half, int T, int E,
                                  int act_head, int A) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int D = 2 * half;
  if (idx >= N * D) return;
  const int n = idx / D, jj = idx - n * D;
  const float c_noise = cond[(size_t)n * cond_stride + 3];
  // blocks.py:86: f = 2 * math.pi * input.unsqueeze(1) @ weight   (left to right: (2 pi c) * w)
  const float two_pi_c = (float)(2.0 * 3.141592653589793) * c_noise;
  const int k = jj < half ? jj : jj - half;
  const float f = two_pi_c * fw[k];
  float v = jj < half ? cosf(f) : sinf(f);
  const int t = jj / E, e = jj - t * E;  // flatten (T, E) -> T*E == D
  int slot = t + act_head;  // logical step t of a ring of T actions starting at act_head
  slot = slot >= T ? slot - T : slot;
  int64_t a = act[(size_t)n * T + slot];
  a = a < 0 ? 0 : (a >= A ? A - 1 : a);  // memory safety only: nn.Embedding raises on an out-of-range index, the host checks it in debug mode
  v += emb[(size_t)a * E + e];
  out[idx] = v;
}

// ---- denoised = quantise(c_skip * x + c_out * F) (denoiser.py:81-83) -------------------------
__device__ __forceinline__ float dmd_quantise(float d) {
  d = fminf(fmaxf(d, -1.0f), 1.0f);       // clamp(-1, 1)
  d = d + 1.0f;                           // add(1)
  d = d / 2.0f;                           // div(2)
  d = d * 255.0f;                         // mul(255)
  const float q = (float)(uint8_t)d;      // byte(): truncation toward zero, value in [0, 255]
  return (q / 255.0f) * 2.0f - 1.0f;      // div(255).mul(2).sub(1)
}

__global__ void edm_denoised_kernel(const float* __restrict__ x, const float* __restrict__ f,
                                    const float* __restrict__ cond, int cond_stride,
                                    float* __restrict__ den, int N, int64_t per_sample) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)N * per_sample) return;
  const int n = idx / per_sample;
  const float c_out = cond[(size_t)n * cond_stride + 1], c_skip = cond[(size_t)n * cond_stride + 2];
  const float a = c_skip * x[idx];
  const float b = c_out * f[idx];
  den[idx] = dmd_quantise(a + b);
}

__global__ void euler_step_kernel(const float* __restrict__ x, const float* __restrict__ den, float sigma_hat, float dt,
                                  float* __restrict__ xo, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float xv = x[idx];
  const float d = (xv - den[idx]) / sigma_hat;  // diffusion_sampler.py:45
  xo[idx] = xv + d * dt;                        // :49
}

// Heun (2nd order) update, diffusion_sampler.py:52-56, same fp32 op order:
//   d = (x - D) / sigma_hat;  d_2 = (x_2 - D_2) / sigma_next;  x_out = x + ((d + d_2) / 2) * dt
__global__ void heun_step_kernel(const float* __restrict__ x, const float* __restrict__ den, const float* __restrict__ x2,
                                 const float* __restrict__ den2, float sigma_hat, float sigma_next, float dt,
                                 float* __restrict__ xo, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float xv = x[idx];
  const float d = (xv - den[idx]) / sigma_hat;
  const float d2 = (x2[idx] - den2[idx]) / sigma_next;
  const float dp = (d + d2) / 2.0f;
  xo[idx] = xv + dp * dt;
}

// ---- NCHW <-> NHWC(CPad) ---------------------------------------------------------------------
// one thread per (pixel, channel quad): 1 KiB contiguous NHWC writes per wave
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int C, int HW, int CPad) {
  const int Q = CPad >> 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * HW * Q) return;
  const int qd = idx % Q;
  const size_t np = idx / Q;
  const int n = np / HW;
  const int pix = np - (size_t)n * HW;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (qd * 4 + e) < C ? in[((size_t)n * C + qd * 4 + e) * HW + pix] : 0.f;
  *(f32x4*)(out + np * CPad + qd * 4) = v;
}

// ---- uint8 frame pool (episode frames are uint8 on disk, data/episode.py:36-50) ----------------
// u8 = round((x + 1) / 2 * 255) of frames in [-1, 1]; *off_grid is set when a value is not exactly the
// dequantisation of its level (such a pool must stay fp32).
// the level of a value in [-1, 1] (values outside are clamped), as a float 0 ... 255
__device__ __forceinline__ float dmd_level(float v) {
  const float lv = rintf((v + 1.0f) / 2.0f * 255.0f);
  return fminf(fmaxf(lv, 0.0f), 255.0f);
}

__global__ void quantize_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ q, int* __restrict__ off_grid, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float v = x[idx];
  const float lc = dmd_level(v);
  q[idx] = (uint8_t)lc;
  const float back = (lc / 255.0f) * 2.0f - 1.0f;  // Episode.load: .div(255).mul(2).sub(1)
  if (!(back == v)) *off_grid = 1;                 // benign race: every writer stores 1
}

// dst[row[i]] frames (logical order, ring slot (head + t) % T) <- dequantised pool frames src[idx[i]]
// per_frame = C * H * W; one thread per 4 consecutive values
__global__ void dequant_gather_kernel(const uint8_t* __restrict__ pool, const int64_t* __restrict__ idx,
                                      const int64_t* __restrict__ rows, float* __restrict__ dst, int M, int T,
                                      int64_t per_frame, int head) {
  const int64_t q4 = per_frame >> 2;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)M * T * q4) return;
  const int64_t e4 = gid % q4;
  const int64_t mt = gid / q4;
  const int t = mt % T;
  const int m = mt / T;
  const int64_t src = idx ? idx[m] : m;
  const int64_t row = rows ? rows[m] : m;
  int slot = t + head;
  slot = slot >= T ? slot - T : slot;
  const uint32_t pk = *(const uint32_t*)(pool + (src * T + t) * per_frame + e4 * 4);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = ((float)((pk >> (8 * e)) & 0xff) / 255.0f) * 2.0f - 1.0f;
  *(f32x4*)(dst + (row * T + slot) * per_frame + e4 * 4) = v;
}

__global__ void nhwc_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int C, int HW, int CPad) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * HW) return;
  const int n = idx / HW;
  const int pix = idx - (size_t)n * HW;
  const float* i = in + idx * CPad;
  for (int ch = 0; ch < C; ++ch) out[((size_t)n * C + ch) * HW + pix] = i[ch];
}

// ---- GroupNorm partial statistics of an NHWC tensor: one tile per image ----------------------
// grid (G, N), 256 threads: thread -> (pixel stripe, channel quad of the group)
// W > 0: the HW pixels are an (HW / W) x W grid of which only rows < hv, columns < wv are counted (VALID EXTENT)
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ stats, int HW, int C, int W, int hv,
                                                       int wv) {
  __shared__ double red[4][2];
  const int g = blockIdx.x, n = blockIdx.y, G = gridDim.x;
  const int tid = threadIdx.x;
  const int quad = tid & 7;  // 8 quads = 32 channels
  double s = 0.0, ss = 0.0;
  for (int pix = tid >> 3; pix < HW; pix += 32) {
    if (W > 0) {
      const int py = pix / W;
      if (py >= hv || pix - py * W >= wv) continue;
    }
    const f32x4 v = *(const f32x4*)(x + ((size_t)n * HW + pix) * C + g * DMD_GN_GROUP + quad * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)v[e];
      s += d;
      ss += d * d;
    }
  }
  s = dmd_wave_sum(s);
  ss = dmd_wave_sum(ss);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s;
    red[tid >> 6][1] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < 4; ++w) {
      a += red[w][0];
      b += red[w][1];
    }
    stats[((size_t)n * G + g) * 2] = a;
    stats[((size_t)n * G + g) * 2 + 1] = b;
  }
}

// ---- the same statistics for groups of any size the grouping rule gives (dmd_gn_group_size: 16, 48, 40, 36 ... channels, a
// multiple of 4): grid (G, N), 256 threads, thread -> (pixel, channel quad of the group) in a flat walk; same layout, fp64 sums
__global__ __launch_bounds__(256) void gn_stats_any_kernel(const float* __restrict__ x, double* __restrict__ stats, int HW, int C, int W,
                                                           int hv, int wv) {
  __shared__ double red[4][2];
  const int g = blockIdx.x, n = blockIdx.y, G = gridDim.x;
  const int tid = threadIdx.x;
  const int gq = C / G / 4;  // channel quads per group
  double s = 0.0, ss = 0.0;
  for (int i = tid; i < HW * gq; i += 256) {
    const int pix = i / gq, quad = i - pix * gq;
    if (W > 0) {
      const int py = pix / W;
      if (py >= hv || pix - py * W >= wv) continue;
    }
    const f32x4 v = *(const f32x4*)(x + ((size_t)n * HW + pix) * C + g * gq * 4 + quad * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)v[e];
      s += d;
      ss += d * d;
    }
  }
  s = dmd_wave_sum(s);
  ss = dmd_wave_sum(ss);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s;
    red[tid >> 6][1] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < 4; ++w) {
      a += red[w][0];
      b += red[w][1];
    }
    stats[((size_t)n * G + g) * 2] = a;
    stats[((size_t)n * G + g) * 2 + 1] = b;
  }
}

// ---- 2x2 max pool, NHWC; one thread per (output pixel, channel quad) ---------------------------
// argmax: index 0..3 (dy*2+dx) of the FIRST maximum in scan order (ATen max_pool2d picks the
// first max it meets scanning h then w; ties only matter for the backward routing).
__global__ void maxpool2_kernel(const float* __restrict__ x, float* __restrict__ out, uint8_t* __restrict__ argmax, int N,
                                int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, Cq = C / 4;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * Ho * Wo * Cq) return;
  const int cq = idx % Cq;
  const size_t op = idx / Cq;
  const int ox = op % Wo;
  const int oy = (op / Wo) % Ho;
  const int n = op / ((size_t)Wo * Ho);
  f32x4 best;
  int bi[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int iy = oy * 2 + (k >> 1), ix = ox * 2 + (k & 1);
    const f32x4 v = *(const f32x4*)(x + (((size_t)n * H + iy) * W + ix) * C + cq * 4);
    if (k == 0)
      best = v;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e] || v[e] != v[e]) {  // NaN propagates like ATen
          best[e] = v[e];
          bi[e] = k;
        }
    }
  }
  *(f32x4*)(out + op * C + cq * 4) = best;
  if (argmax) {
    uint32_t packed = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    *(uint32_t*)(argmax + op * C + cq * 4) = packed;
  }
}

// ---- LSTM cell nonlinearity (gate order i, f, g, o) --------------------------------------------
__global__ void lstm_pointwise_kernel(const float* __restrict__ gates, const float* __restrict__ c_prev,
                                      float* __restrict__ h, float* __restrict__ c, int N, int Hd) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * Hd) return;
  const int n = idx / Hd, k = idx - n * Hd;
  const float* gr = gates + (size_t)n * 4 * Hd;
  const float ig = dmd_sigmoid(gr[k]);
  const float fg = dmd_sigmoid(gr[Hd + k]);
  const float gg = tanhf(gr[2 * Hd + k]);
  const float og = dmd_sigmoid(gr[3 * Hd + k]);
  const float cn = fg * c_prev[idx] + ig * gg;
  c[idx] = cn;
  h[idx] = og * tanhf(cn);
}

// LSTM cell backward (autograd of nn.LSTMCell under the actor-critic loss, actor_critic.py:46,72 / trainer.py:366):
// gates = pre-activations (i, f, g, o) saved by the forward, dh / dc = gradients w.r.t. the new h / c (either may be NULL)
// -> dgates (N, 4 Hd), dc_prev (N, Hd)
__global__ void lstm_pointwise_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ c_prev,
                                          const float* __restrict__ c_new, const float* __restrict__ dh,
                                          const float* __restrict__ dc, float* __restrict__ dgates, float* __restrict__ dc_prev,
                                          int N, int Hd) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * Hd) return;
  const int n = idx / Hd, k = idx - n * Hd;
  const float* gr = gates + (size_t)n * 4 * Hd;
  const float ig = dmd_sigmoid(gr[k]);
  const float fg = dmd_sigmoid(gr[Hd + k]);
  const float gg = tanhf(gr[2 * Hd + k]);
  const float og = dmd_sigmoid(gr[3 * Hd + k]);
  const float tc = tanhf(c_new[idx]);
  const float dhv = dh ? dh[idx] : 0.f;
  const float dcv = (dc ? dc[idx] : 0.f) + dhv * og * (1.0f - tc * tc);
  float* dg = dgates + (size_t)n * 4 * Hd;
  dg[k] = dcv * gg * ig * (1.0f - ig);
  dg[Hd + k] = dcv * c_prev[idx] * fg * (1.0f - fg);
  dg[2 * Hd + k] = dcv * ig * (1.0f - gg * gg);
  dg[3 * Hd + k] = dhv * tc * og * (1.0f - og);
  dc_prev[idx] = dcv * fg;
}

// ---- Categorical(logits).sample() with injected E ~ Exp(1): argmax(softmax(logits) / E) -------
__global__ void categorical_sample_kernel(const float* __restrict__ logits, const float* __restrict__ expo,
                                          int64_t* __restrict__ out, int N, int A) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* l = logits + (size_t)n * A;
  const float* e = expo + (size_t)n * A;
  // torch: Categorical(logits=l) keeps ln = l - logsumexp(l); probs = softmax(ln)
  float m = -INFINITY;
  for (int a = 0; a < A; ++a) m = fmaxf(m, l[a]);
  float sum = 0.f;
  for (int a = 0; a < A; ++a) sum += expf(l[a] - m);
  const float lse = m + logf(sum);
  float m2 = -INFINITY;
  for (int a = 0; a < A; ++a) m2 = fmaxf(m2, l[a] - lse);
  float sum2 = 0.f;
  for (int a = 0; a < A; ++a) sum2 += expf((l[a] - lse) - m2);
  float best = -INFINITY;
  int bi = 0;
  for (int a = 0; a < A; ++a) {
    const float p = expf((l[a] - lse) - m2) / sum2;
    const float v = p / e[a];
    if (v > best) {
      best = v;
      bi = a;
    }
  }
  out[n] = bi;
}

// ------------------------------------------------------------------------------------------------
static inline unsigned nblk(size_t n, int b) { return (unsigned)((n + b - 1) / b); }

extern "C" int dmd_edm_pack_input(const float* x, const float* obs, const float* cond, int cond_stride, float sigma_data,
                                  float* out, int N, int Cx, int Cobs, int H, int W, int CPad, int T, int head,
                                  dmd_stream_t stream) {
  DMD_CHECK_ARG(x && obs && cond && out, "edm_pack_input: null");
  DMD_CHECK_ARG(CPad % 4 == 0 && CPad >= Cx + Cobs, "edm_pack_input: CPad");
  DMD_CHECK_ARG((H * W) % 4 == 0, "edm_pack_input: H * W must be a multiple of 4 (16-byte plane reads)");
  DMD_CHECK_ARG(T >= 1 && Cobs % T == 0 && head >= 0 && head < T, "edm_pack_input: ring T %d head %d Cobs %d", T, head, Cobs);
  hipLaunchKernelGGL(edm_pack_input_kernel, dim3(nblk((size_t)N * (H * W / 4) * (CPad / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                     x, obs, cond, cond_stride, sigma_data, out, N, Cx, Cobs, H * W, CPad, T, head);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_cond_embed(const float* cond, int cond_stride, const float* fw, const int64_t* act,
                              const float* emb, float* out, int N, int half, int T, int E, int act_head, int A,
                              dmd_stream_t stream) {
  DMD_CHECK_ARG(cond && fw && act && emb && out, "cond_embed: null");
  DMD_CHECK_ARG(T * E == 2 * half, "cond_embed: T*E (%d) != cond channels (%d)", T * E, 2 * half);
  DMD_CHECK_ARG(act_head >= 0 && act_head < T && A > 0, "cond_embed: act_head %d outside [0, %d) or A %d", act_head, T, A);
  hipLaunchKernelGGL(cond_embed_kernel, dim3(nblk((size_t)N * 2 * half, 256)), dim3(256), 0, (hipStream_t)stream, cond,
                     cond_stride, fw, act, emb, out, N, half, T, E, act_head, A);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_edm_denoised(const float* x, const float* f, const float* cond, int cond_stride,
                                float* den, int N, int64_t per_sample, dmd_stream_t stream) {
  DMD_CHECK_ARG(x && f && cond && den, "edm_denoised: null");
  hipLaunchKernelGGL(edm_denoised_kernel, dim3(nblk((size_t)N * per_sample, 256)), dim3(256), 0, (hipStream_t)stream, x, f,
                     cond, cond_stride, den, N, per_sample);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_euler_step(const float* x, const float* den, float sigma_hat, float dt, float* xo, int64_t n,
                              dmd_stream_t stream) {
  DMD_CHECK_ARG(x && den && xo, "euler_step: null");
  hipLaunchKernelGGL(euler_step_kernel, dim3(nblk((size_t)n, 256)), dim3(256), 0, (hipStream_t)stream, x, den, sigma_hat, dt,
                     xo, n);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_heun_step(const float* x, const float* den, const float* x2, const float* den2, float sigma_hat,
                             float sigma_next, float dt, float* xo, int64_t n, dmd_stream_t stream) {
  DMD_CHECK_ARG(x && den && x2 && den2 && xo, "heun_step: null");
  hipLaunchKernelGGL(heun_step_kernel, dim3(nblk((size_t)n, 256)), dim3(256), 0, (hipStream_t)stream, x, den, x2, den2,
                     sigma_hat, sigma_next, dt, xo, n);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_quantize_u8(const float* x, uint8_t* q, int* off_grid, int64_t n, dmd_stream_t stream) {
  DMD_CHECK_ARG(x && q && off_grid, "quantize_u8: null");
  hipLaunchKernelGGL(quantize_u8_kernel, dim3(nblk((size_t)n, 256)), dim3(256), 0, (hipStream_t)stream, x, q, off_grid, n);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_dequant_gather(const uint8_t* pool, const int64_t* idx, const int64_t* rows, float* dst, int M, int T,
                                  int64_t per_frame, int head, dmd_stream_t stream) {
  DMD_CHECK_ARG(pool && dst, "dequant_gather: null");
  DMD_CHECK_ARG(per_frame % 4 == 0 && T >= 1 && head >= 0 && head < T, "dequant_gather: per_frame %% 4, ring");
  if (M == 0) return 0;
  hipLaunchKernelGGL(dequant_gather_kernel, dim3(nblk((size_t)M * T * (per_frame / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                     pool, idx, rows, dst, M, T, per_frame, head);
  DMD_LAUNCH_CHECK();
  return 0;
}

// The small state of a reset in ONE launch (reference world_model_env.py:56-62 `reset_dead`: act_buffer[dead] = act,
// hx_rew_end[:, dead] = hx, cx likewise, ep_len[dead] = 0 -- four indexed assignments, ~12 launches of torch glue on the step's
// critical path, right behind its host synchronisation): block i handles env row rows[i] <- pool row idx[i].
__global__ __launch_bounds__(256) void reset_state_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ rows,
                                                          const int64_t* __restrict__ pool_act, int64_t* __restrict__ act_ring, int T, int head,
                                                          const float* __restrict__ pool_hx, const float* __restrict__ pool_cx,
                                                          float* __restrict__ hx, float* __restrict__ cx, int hd, int64_t* __restrict__ ep_len) {
  const int64_t q = idx[blockIdx.x], r = rows[blockIdx.x];
  for (int j = threadIdx.x; j < hd; j += 256) {
    hx[r * hd + j] = pool_hx[q * hd + j];
    cx[r * hd + j] = pool_cx[q * hd + j];
  }
  if ((int)threadIdx.x < T) act_ring[r * T + (head + threadIdx.x) % T] = pool_act[q * T + threadIdx.x];
  if (threadIdx.x == 0) ep_len[r] = 0;
}

extern "C" int dmd_reset_state(const int64_t* idx, const int64_t* rows, int count, const int64_t* pool_act, int64_t* act_ring, int T,
                               int head, const float* pool_hx, const float* pool_cx, float* hx, float* cx, int hd, int64_t* ep_len,
                               dmd_stream_t stream) {
  DMD_CHECK_ARG(idx && rows && pool_act && act_ring && pool_hx && pool_cx && hx && cx && ep_len, "reset_state: null");
  DMD_CHECK_ARG(T >= 1 && T <= 256 && head >= 0 && head < T && hd >= 1, "reset_state: T %d, head %d, hd %d", T, head, hd);
  if (count == 0) return 0;
  hipLaunchKernelGGL(reset_state_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, idx, rows, pool_act, act_ring, T, head,
                     pool_hx, pool_cx, hx, cx, hd, ep_len);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- the deaths of an imagined step resolved ON THE DEVICE (ABI v11) -----------------------------------------------------
// The reference asks the host once per step which episodes ended (`if dead.any()`, world_model_env.py:77; env_loop.py:45) and
// shapes what follows by the answer.  Here the answer stays on the device: the step works on K SLOTS (K chosen by the host
// before it knows the step's deaths), the dead rows are assigned to slots in ascending row order -- the order in which the
// reference's boolean masks enumerate them and its pool serves them (world_model_env.py:56-57,133-139) -- and everything
// downstream is fixed-shape over the slots; an unused slot is marked -1.  The host reads `report` one step LATE (episode-length
// mirror, pool cursor, slot overflow), behind a full step of queued work.
//   per row r:  ep_len[r] += 1; trunc[r] = ep_len[r] >= horizon; dead[r] = end[r] | trunc[r]; ep_len[r] = 0 where dead
//   slot_row[j] = j-th dead row (-1: unused slot);  row_slot[r] = slot of a dead row (-1: alive, or no slot left)
//   report = {dead[0..B) as int32, k = number of dead rows, number of rows with end != 0, k > K, K}
__global__ __launch_bounds__(256) void resolve_deaths_kernel(const int64_t* __restrict__ end, int64_t* __restrict__ ep_len, int horizon,
                                                             int64_t* __restrict__ trunc, uint8_t* __restrict__ dead, int B, int K,
                                                             int64_t* __restrict__ slot_row, int32_t* __restrict__ row_slot,
                                                             int32_t* __restrict__ report) {
  __shared__ int flag[256];
  __shared__ int eflag[256];
  const int tid = threadIdx.x;
  int base = 0, ends = 0;
  for (int r0 = 0; r0 < B; r0 += 256) {
    const int r = r0 + tid;
    bool d = false, e = false;
    if (r < B) {
      const int64_t l = ep_len[r] + 1;
      const bool t = l >= (int64_t)horizon;
      e = end[r] != 0;
      d = e || t;
      trunc[r] = t ? 1 : 0;
      dead[r] = d ? 1 : 0;
      ep_len[r] = d ? 0 : l;
      report[r] = d ? 1 : 0;
    }
    flag[tid] = d ? 1 : 0;
    eflag[tid] = e ? 1 : 0;
    __syncthreads();
    int before = 0, total = 0, etotal = 0;  // (256 LDS reads per thread: a one-workgroup kernel of a few microseconds)
    for (int i = 0; i < 256; ++i) {
      before += i < tid ? flag[i] : 0;
      total += flag[i];
      etotal += eflag[i];
    }
    if (r < B) {
      const int slot = base + before;
      const bool has = d && slot < K;
      row_slot[r] = has ? slot : -1;
      if (has) slot_row[slot] = r;
    }
    base += total;
    ends += etotal;
    __syncthreads();
  }
  for (int j = base + tid; j < K; j += 256) slot_row[j] = -1;
  if (tid == 0) {
    report[B] = base;
    report[B + 1] = ends;
    report[B + 2] = base > K ? 1 : 0;
    report[B + 3] = K;
  }
}

extern "C" int dmd_resolve_deaths(const int64_t* end, int64_t* ep_len, int horizon, int64_t* trunc, uint8_t* dead, int B, int K,
                                  int64_t* slot_row, int32_t* row_slot, int32_t* report, dmd_stream_t stream) {
  DMD_CHECK_ARG(end && ep_len && trunc && dead && row_slot && report && (slot_row || K == 0), "resolve_deaths: null");
  DMD_CHECK_ARG(B >= 1 && K >= 0 && horizon >= 1, "resolve_deaths: B %d, K %d, horizon %d", B, K, horizon);
  hipLaunchKernelGGL(resolve_deaths_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, end, ep_len, horizon, trunc, dead, B, K, slot_row,
                     row_slot, report);
  DMD_LAUNCH_CHECK();
  return 0;
}

// Ring advance + reset of the dead rows + the policy's next input, one launch over B + T * K frames (grid.y):
//   frame f <  B          env row f: its newest frame -- the imagined one, or (dead row with a slot) the newest frame of its NEW
//                         episode -- into enc_in[f] AND into the ring slot the advance frees (logical T - 1 at the new head)
//   frame f <  B + K      slot j = f - B: the FINAL observation of the ended episode (the imagined frame of row slot_row[j])
//   frame f >= B + K      burn-in frame t of slot j (frame-major: f = B + K + t * K + j, t < T - 1): the new episode's context
//                         frame t, into enc_in[f] AND into ring slot (head + t) % T of the row
// A slot's new episode is row base + j of a pool round (dequantised: (u8 / 255) * 2 - 1, exact zeros where `pad` marks a padded
// frame; or an fp32 round).  Which round: pool[0] from pool_base on, or -- when the step's deaths do not fit what is left of it,
// the reference's rule (world_model_env.py:133-139) -- pool[1] from row 0 (ws_pool_select: the count is on the device only).
// Unused slots (slot_row -1) receive copies of row 0's imagined frame: finite values nobody reads.
__device__ __forceinline__ int ws_pool_select(const dmd_reset_slots_params& p, int64_t* base) {
  const bool second = p.pool[1].frames && p.num_dead && (p.pool_base + (int64_t)*p.num_dead > (int64_t)p.pool[0].rows);
  *base = second ? 0 : p.pool_base;
  return second ? 1 : 0;
}

__global__ __launch_bounds__(256) void reset_slot_frames_kernel(dmd_reset_slots_params p) {
  const int64_t q4 = p.per_frame >> 2;
  const int64_t e4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e4 >= q4) return;
  const int f = blockIdx.y;
  const int B = p.B, K = p.K, T = p.T;
  int64_t base = 0;
  const dmd_pool_round& pool = p.pool[K > 0 ? ws_pool_select(p, &base) : 0];
  int64_t pool_row = -1, obs_row = 0, ring_row = -1;
  int pool_t = 0, ring_slot = 0;
  if (f < B) {
    const int s = p.row_slot[f];
    ring_row = f;
    ring_slot = (p.head + T - 1) % T;
    if (s >= 0) {
      pool_row = base + s;
      pool_t = T - 1;
    } else {
      obs_row = f;
    }
  } else if (f < B + K) {
    const int64_t r = p.slot_row[f - B];
    obs_row = r >= 0 ? r : 0;
  } else {
    const int g = f - B - K;
    const int t = g / K, j = g - t * K;
    const int64_t r = p.slot_row[j];
    if (r >= 0) {
      pool_row = base + j;
      pool_t = t;
      ring_row = r;
      ring_slot = (p.head + t) % T;
    }
  }
  f32x4 v;
  if (pool_row >= 0) {
    const int64_t pf = pool_row * T + pool_t;
    if (!pool.is_f32) {
      const uint32_t pk = *(const uint32_t*)((const uint8_t*)pool.frames + pf * p.per_frame + e4 * 4);
      const bool pad = pool.pad && pool.pad[pf];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = pad ? 0.0f : ((float)((pk >> (8 * e)) & 0xff) / 255.0f) * 2.0f - 1.0f;
    } else {
      v = *(const f32x4*)((const float*)pool.frames + pf * p.per_frame + e4 * 4);
    }
  } else {
    v = *(const f32x4*)(p.next_obs + obs_row * p.per_frame + e4 * 4);
  }
  *(f32x4*)(p.enc_in + (int64_t)f * p.per_frame + e4 * 4) = v;
  if (ring_row >= 0) *(f32x4*)(p.ctx + (ring_row * T + ring_slot) * p.per_frame + e4 * 4) = v;
}

// the small state of the slots' resets: action ring, reward/end LSTM state (reset_state_kernel with the slot indirection;
// ep_len was zeroed by resolve_deaths_kernel)
__global__ __launch_bounds__(256) void reset_slot_state_kernel(dmd_reset_slots_params p) {
  const int j = blockIdx.x;
  const int64_t r = p.slot_row[j];
  if (r < 0) return;
  int64_t base;
  const dmd_pool_round& pool = p.pool[ws_pool_select(p, &base)];
  const int64_t q = base + j;
  const int hd = p.hd, T = p.T;
  for (int i = threadIdx.x; i < hd; i += 256) {
    p.hx[r * hd + i] = pool.hx[q * hd + i];
    p.cx[r * hd + i] = pool.cx[q * hd + i];
  }
  if ((int)threadIdx.x < T) p.act_ring[r * T + (p.head + threadIdx.x) % T] = pool.act[q * T + threadIdx.x];
}

extern "C" int dmd_reset_slots(const dmd_reset_slots_params* pp, dmd_stream_t stream) {
  const dmd_reset_slots_params& p = *pp;
  DMD_CHECK_ARG(p.B >= 1 && p.K >= 0 && p.T >= 1 && p.T <= 256 && p.head >= 0 && p.head < p.T && p.per_frame > 0 && p.per_frame % 4 == 0,
                "reset_slots: B %d, K %d, T %d, head %d, per_frame %lld", p.B, p.K, p.T, p.head, (long long)p.per_frame);
  DMD_CHECK_ARG(p.row_slot && p.next_obs && p.ctx && p.enc_in, "reset_slots: null");
  const dmd_pool_round& p0 = p.pool[0];
  DMD_CHECK_ARG(p.K == 0 || (p.slot_row && p0.frames && p0.act && p0.hx && p0.cx && p.act_ring && p.hx && p.cx && p.hd >= 1 && p.pool_base >= 0),
                "reset_slots: null pool / state argument with K = %d slots", p.K);
  const dmd_pool_round& p1 = p.pool[1];
  DMD_CHECK_ARG(p.K == 0 || !p1.frames || (p.num_dead && p1.act && p1.hx && p1.cx && p0.rows >= 1), "reset_slots: second pool round without "
                "its actions / states, the first round's row count or the device's death count");
  const int frames = p.B + p.T * p.K;
  DMD_CHECK_ARG(frames <= 65535, "reset_slots: %d frames in one launch", frames);
  const dim3 grid((unsigned)nblk((size_t)(p.per_frame / 4), 256), (unsigned)frames);
  hipLaunchKernelGGL(reset_slot_frames_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
  DMD_LAUNCH_CHECK();
  if (p.K > 0) {
    hipLaunchKernelGGL(reset_slot_state_kernel, dim3((unsigned)p.K), dim3(256), 0, (hipStream_t)stream, p);
    DMD_LAUNCH_CHECK();
  }
  return 0;
}

// out[r] = alive row ? base[r] : slots[row_slot[r]]   (rows of D floats): the burnt-in LSTM state of the reset rows merged into
// the batch's state (reference env_loop.py:51-56: gate to zero, then burn in) -- and its transpose for the backward:
// d_base[r] = alive ? d_out[r] : 0;  d_slots[j] = slot used ? d_out[slot_row[j]] : 0
__global__ void merge_slots_kernel(const float* __restrict__ base, const float* __restrict__ slots, const int32_t* __restrict__ row_slot,
                                   float* __restrict__ out, int B, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * D) return;
  const int r = i / D, c = i - (int64_t)r * D;
  const int s = row_slot[r];
  out[i] = s >= 0 ? slots[(int64_t)s * D + c] : base[i];
}

__global__ void merge_slots_bwd_kernel(const float* __restrict__ d_out, const int32_t* __restrict__ row_slot, const int64_t* __restrict__ slot_row,
                                       float* __restrict__ d_base, float* __restrict__ d_slots, int B, int K, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)B * D) {
    const int r = i / D;
    if (d_base) d_base[i] = row_slot[r] >= 0 ? 0.0f : d_out[i];
  } else if (i < (int64_t)(B + K) * D) {
    const int64_t k = i - (int64_t)B * D;
    const int j = k / D, c = k - (int64_t)j * D;
    const int64_t r = slot_row[j];
    d_slots[k] = r >= 0 ? d_out[r * D + c] : 0.0f;
  }
}

// TD(lambda) targets of the actor-critic loss (reference actor_critic.py:116-143; diamond_amd/actor_critic.py
// compute_lambda_returns): one thread per env row runs the backward recursion over the T steps of the window, which the host code
// spells as a Python loop of four (B,) launches per step.  The fp32 operations are those of the torch expressions, in their order
// (the file is compiled with -ffp-contract=off: no product is fused into an add):
//   ret[t]  = sign(rew) + ((float(1 - end) * g) * ((float(1 - trunc) * (1 - lambda)) + float(trunc))) * v[t]
//   ret[t] += ((alive * g) * lambda) * last,   last = v[T - 1], then ret[t + 1];   alive = !min(end + trunc, 1)
// g, 1 - lambda (formed in double by the host, like Python does) and lambda arrive rounded to fp32, as torch rounds a Python scalar.
__global__ void lambda_returns_kernel(const float* __restrict__ rew, const int64_t* __restrict__ end, const int64_t* __restrict__ trunc,
                                      const float* __restrict__ vb, float* __restrict__ ret, int B, int T, float g,
                                      float one_minus_lambda, float lambda) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t row = (size_t)b * T;
  float last = vb[row + T - 1];
  for (int t = T - 1; t >= 0; --t) {
    const float r = rew[row + t];
    const int64_t e = end[row + t], tr = trunc[row + t];
    const float sgn = (float)((0.f < r) - (r < 0.f));
    const float x1 = (float)(1 - e) * g;
    const float x2 = (float)(1 - tr) * one_minus_lambda;
    const float x3 = x2 + (float)tr;
    const float x4 = x1 * x3;
    const float x5 = x4 * vb[row + t];
    float v = sgn + x5;
    const int64_t d = e + tr;
    const float alive = (d < 1 ? d : 1) == 0 ? 1.f : 0.f;
    const float a1 = alive * g;
    const float a2 = a1 * lambda;
    const float a3 = a2 * last;
    v = v + a3;
    ret[row + t] = v;
    last = v;
  }
}

extern "C" int dmd_merge_slots(const float* base, const float* slots, const int32_t* row_slot, float* out, int B, int D, dmd_stream_t stream) {
  DMD_CHECK_ARG(base && slots && row_slot && out && B >= 1 && D >= 1, "merge_slots: args");
  hipLaunchKernelGGL(merge_slots_kernel, dim3(nblk((size_t)B * D, 256)), dim3(256), 0, (hipStream_t)stream, base, slots, row_slot, out, B, D);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_merge_slots_bwd(const float* d_out, const int32_t* row_slot, const int64_t* slot_row, float* d_base, float* d_slots, int B,
                                   int K, int D, dmd_stream_t stream) {
  DMD_CHECK_ARG(d_out && row_slot && slot_row && d_slots && B >= 1 && K >= 1 && D >= 1, "merge_slots_bwd: args");
  hipLaunchKernelGGL(merge_slots_bwd_kernel, dim3(nblk((size_t)(B + K) * D, 256)), dim3(256), 0, (hipStream_t)stream, d_out, row_slot,
                     slot_row, d_base, d_slots, B, K, D);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_nchw_to_nhwc(const float* in, float* out, int N, int C, int H, int W, int CPad, dmd_stream_t stream) {
  DMD_CHECK_ARG(in && out && CPad % 4 == 0 && CPad >= C, "nchw_to_nhwc: args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblk((size_t)N * H * W * (CPad / 4), 256)), dim3(256), 0, (hipStream_t)stream, in,
                     out, N, C, H * W, CPad);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_nhwc_to_nchw(const float* in, float* out, int N, int C, int H, int W, int CPad, dmd_stream_t stream) {
  DMD_CHECK_ARG(in && out && CPad >= C, "nhwc_to_nchw: args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblk((size_t)N * H * W, 256)), dim3(256), 0, (hipStream_t)stream, in, out, N, C,
                     H * W, CPad);
  DMD_LAUNCH_CHECK();
  return 0;
}

// groups of 32: gn_stats_kernel; any other width the grouping rule allows (dmd_gn_width_ok): gn_stats_any_kernel
extern "C" int dmd_gn_stats(const float* x, double* stats, int N, int HW, int C, dmd_stream_t stream) {
  DMD_CHECK_ARG(x && stats && dmd_gn_width_ok(C), "gn_stats: C %d (needs C %% 32 == 0, or C <= 256, C %% 16 == 0 and groups of a multiple of 4)", C);
  if (C % DMD_GN_GROUP == 0)
    hipLaunchKernelGGL(gn_stats_kernel, dim3(C / DMD_GN_GROUP, N), dim3(256), 0, (hipStream_t)stream, x, stats, HW, C, 0, 0, 0);
  else
    hipLaunchKernelGGL(gn_stats_any_kernel, dim3(dmd_gn_groups(C), N), dim3(256), 0, (hipStream_t)stream, x, stats, HW, C, 0, 0, 0);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_gn_stats_valid(const float* x, double* stats, int N, int H, int W, int valid_h, int valid_w, int C, dmd_stream_t stream) {
  DMD_CHECK_ARG(x && stats && dmd_gn_width_ok(C), "gn_stats: C %d (needs C %% 32 == 0, or C <= 256, C %% 16 == 0 and groups of a multiple of 4)", C);
  DMD_CHECK_ARG(valid_h > 0 && valid_h <= H && valid_w > 0 && valid_w <= W, "gn_stats: valid extent %d x %d of %d x %d", valid_h, valid_w, H, W);
  if (C % DMD_GN_GROUP == 0)
    hipLaunchKernelGGL(gn_stats_kernel, dim3(C / DMD_GN_GROUP, N), dim3(256), 0, (hipStream_t)stream, x, stats, H * W, C, W, valid_h, valid_w);
  else
    hipLaunchKernelGGL(gn_stats_any_kernel, dim3(dmd_gn_groups(C), N), dim3(256), 0, (hipStream_t)stream, x, stats, H * W, C, W, valid_h,
                       valid_w);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_maxpool2(const float* x, float* out, uint8_t* argmax, double* out_stats, int N, int H, int W, int C,
                            dmd_stream_t stream) {
  DMD_CHECK_ARG(x && out && H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "maxpool2: args");
  hipLaunchKernelGGL(maxpool2_kernel, dim3(nblk((size_t)N * (H / 2) * (W / 2) * (C / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, x, out, argmax, N, H, W, C);
  DMD_LAUNCH_CHECK();
  if (out_stats) return dmd_gn_stats(out, out_stats, N, (H / 2) * (W / 2), C, stream);
  return 0;
}

extern "C" int dmd_lstm_pointwise(const float* gates, const float* c_prev, float* h, float* c, int N, int Hd,
                                  dmd_stream_t stream) {
  DMD_CHECK_ARG(gates && c_prev && h && c, "lstm_pointwise: null");
  hipLaunchKernelGGL(lstm_pointwise_kernel, dim3(nblk((size_t)N * Hd, 256)), dim3(256), 0, (hipStream_t)stream, gates, c_prev,
                     h, c, N, Hd);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_lstm_pointwise_bwd(const float* gates, const float* c_prev, const float* c_new, const float* dh,
                                      const float* dc, float* dgates, float* dc_prev, int N, int Hd, dmd_stream_t stream) {
  DMD_CHECK_ARG(gates && c_prev && c_new && dgates && dc_prev, "lstm_pointwise_bwd: null");
  hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3(nblk((size_t)N * Hd, 256)), dim3(256), 0, (hipStream_t)stream, gates,
                     c_prev, c_new, dh, dc, dgates, dc_prev, N, Hd);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_lambda_returns(const float* rew, const int64_t* end, const int64_t* trunc, const float* val_bootstrap, float* ret, int B,
                                  int T, float gamma, float one_minus_lambda, float lambda, dmd_stream_t stream) {
  DMD_CHECK_ARG(rew && end && trunc && val_bootstrap && ret && B >= 1 && T >= 1, "lambda_returns: args");
  hipLaunchKernelGGL(lambda_returns_kernel, dim3(nblk((size_t)B, 64)), dim3(64), 0, (hipStream_t)stream, rew, end, trunc, val_bootstrap,
                     ret, B, T, gamma, one_minus_lambda, lambda);
  DMD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmd_categorical_sample(const float* logits, const float* expo, int64_t* out, int N, int A,
                                      dmd_stream_t stream) {
  DMD_CHECK_ARG(logits && expo && out && A > 0, "categorical_sample: args");
  hipLaunchKernelGGL(categorical_sample_kernel, dim3(nblk((size_t)N, 64)), dim3(64), 0, (hipStream_t)stream, logits, expo, out,
                     N, A);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- reward / end training loss (reference rew_end_model.py:72-88) as ONE launch of one workgroup ------------------------------
// logits (R, 5): columns 0-2 the reward head, 3-4 the end head.  Over the rows with mask != 0 (n of them):
//   losses[0] = mean cross-entropy of the reward head against class sign(rew) + 1 (-0.0 and 0.0: class 1)
//   losses[1] = mean cross-entropy of the end head against class (end != 0)
//   dlogits   = d(losses[0] + losses[1]) / dlogits = (softmax - onehot) / n per head, exact zeros on the other rows
//   counts    = the two confusion matrices [true][argmax] (3 x 3, then 2 x 2; ties: the lowest index)
// n == 0: 0.0 / 0 = NaN losses (the mean of an empty selection), dlogits and counts all zero.
// Deterministic: thread t walks rows t, t + 256, ... in ascending order (fp64 loss sums, integer counts), the 256 partials are
// added in ascending thread order from LDS; no atomics.  log-soft-max in fp32 with the row maximum subtracted.
#define DMD_REL_THREADS 256
__global__ __launch_bounds__(DMD_REL_THREADS) void rew_end_loss_kernel(const float* __restrict__ logits, const float* __restrict__ rew,
                                                                       const int64_t* __restrict__ end, const uint8_t* __restrict__ mask,
                                                                       float* __restrict__ losses, float* __restrict__ dlogits,
                                                                       int64_t* __restrict__ counts, int R) {
  __shared__ double lsum[2][DMD_REL_THREADS];
  __shared__ int cnt[14][DMD_REL_THREADS];  // rows 0-12: the confusion counts, row 13: masked rows
  __shared__ int n_all;
  const int tid = threadIdx.x;
  int mine = 0;
  for (int r = tid; r < R; r += DMD_REL_THREADS) mine += mask[r] != 0 ? 1 : 0;
  cnt[13][tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < DMD_REL_THREADS; ++i) n += cnt[13][i];
    n_all = n;
  }
  __syncthreads();
  const int n = n_all;
  const float nf = (float)n;
  double s_rew = 0.0, s_end = 0.0;
  int c[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) c[k] = 0;
  for (int r = tid; r < R; r += DMD_REL_THREADS) {
    float* d = dlogits + (size_t)r * 5;
    if (mask[r] == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) d[k] = 0.f;
      continue;
    }
    const float* l = logits + (size_t)r * 5;
    const float l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3], l4 = l[4];
    const float rv = rew[r];
    const int tr = rv > 0.f ? 2 : (rv < 0.f ? 0 : 1);
    const int te = end[r] != 0 ? 1 : 0;
    {  // reward head
      const float m = fmaxf(l0, fmaxf(l1, l2));
      const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
      const float s = e0 + e1 + e2;
      const float lt = tr == 0 ? l0 : (tr == 1 ? l1 : l2);
      s_rew += (double)(logf(s) - (lt - m));
      d[0] = (e0 / s - (tr == 0 ? 1.f : 0.f)) / nf;
      d[1] = (e1 / s - (tr == 1 ? 1.f : 0.f)) / nf;
      d[2] = (e2 / s - (tr == 2 ? 1.f : 0.f)) / nf;
      int pr = 0;
      float best = l0;
      if (l1 > best) {
        best = l1;
        pr = 1;
      }
      if (l2 > best) pr = 2;
      const int cell = tr * 3 + pr;
#pragma unroll
      for (int k = 0; k < 9; ++k) c[k] += cell == k ? 1 : 0;
    }
    {  // end head
      const float m = fmaxf(l3, l4);
      const float e0 = expf(l3 - m), e1 = expf(l4 - m);
      const float s = e0 + e1;
      const float lt = te == 0 ? l3 : l4;
      s_end += (double)(logf(s) - (lt - m));
      d[3] = (e0 / s - (te == 0 ? 1.f : 0.f)) / nf;
      d[4] = (e1 / s - (te == 1 ? 1.f : 0.f)) / nf;
      const int cell = te * 2 + (l4 > l3 ? 1 : 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) c[9 + k] += cell == k ? 1 : 0;
    }
  }
  lsum[0][tid] = s_rew;
  lsum[1][tid] = s_end;
#pragma unroll
  for (int k = 0; k < 13; ++k) cnt[k][tid] = c[k];
  __syncthreads();
  if (tid < 13) {
    int64_t a = 0;
    for (int i = 0; i < DMD_REL_THREADS; ++i) a += cnt[tid][i];
    counts[tid] = a;
  } else if (tid < 15) {
    double a = 0.0;
    for (int i = 0; i < DMD_REL_THREADS; ++i) a += lsum[tid - 13][i];
    losses[tid - 13] = (float)(a / (double)n);
  }
}

extern "C" int dmd_rew_end_loss(const float* logits, const float* rew, const int64_t* end, const uint8_t* mask, float* losses,
                                float* dlogits, int64_t* counts, int R, dmd_stream_t stream) {
  DMD_CHECK_ARG(logits && rew && end && mask && losses && dlogits && counts, "rew_end_loss: null");
  DMD_CHECK_ARG(R >= 1 && R <= (1 << 20), "rew_end_loss: R %d (1 ... 2^20 rows)", R);
  hipLaunchKernelGGL(rew_end_loss_kernel, dim3(1), dim3(DMD_REL_THREADS), 0, (hipStream_t)stream, logits, rew, end, mask, losses, dlogits,
                     counts, R);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- device-resident replay store: a (B, T) training batch out of the uint8 arena in one launch ---------------------------------
// (reference data/utils.py:12-41 make_segment + collate_segments_to_batch, per sample on the CPU, then an fp32 upload.)
// HBM-bound: 1 byte read and 4 written per value.  Workgroups are laid over FRAMES -- the T positions of a sample, then its
// final observation -- so what a frame is (an arena row, the final observation, or zeros) is uniform over the workgroup: the
// descriptor is read through scalar loads and no lane diverges.  A workgroup covers 256 x W levels:
//   W = 16  per_frame % 16 == 0: a lane takes FOUR 4-byte words 1 KiB apart -- every load of a wave is 256 contiguous bytes,
//           every 16-byte store of a wave 1 KiB contiguous, four loads in flight per lane.  (A lane that owns 16 CONSECUTIVE
//           levels -- one 16-byte load -- would store 16-byte pieces 64 bytes apart, a quarter of each store's segments.)
//   W = 4   one word per lane;   W = 1  one level per lane: any per_frame, any alignment
// A padded position stores zeros and loads nothing.  The five small fields have workgroups of their own in the same launch.

// (float)q / 255.0f * 2.0f - 1.0f (data/episode.py:40) with the division as q * fl(1 / 255) plus ONE residual step: three
// instructions for the ~10 of an fp32 division, in a kernel whose waves all load, then all convert, then all store.  The
// quotient is the correctly rounded one for every level 0 ... 255 (tests: all 256 levels, bit for bit against the division).
__device__ __forceinline__ float seg_dequant(uint32_t q) {
  const float qf = (float)q, rcp = 1.0f / 255.0f;
  float r = qf * rcp;
  r = __builtin_fmaf(__builtin_fmaf(-255.0f, r, qf), rcp, r);
  return r * 2.0f - 1.0f;
}

__device__ __forceinline__ f32x4 seg_dequant4(uint32_t pk) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = seg_dequant((pk >> (8 * e)) & 0xff);
  return v;
}

template <int W>
__global__ __launch_bounds__(256) void segment_gather_kernel(dmd_segment_gather_params p, int64_t units) {
  // grid (workgroups per frame, T + 2, B), no division anywhere; workgroups are dispatched along a frame, then along the segment:
  //   y <  T      frame (b, y)          y == T      the sample's final observation
  //   y == T + 1  the five small fields of the sample's T positions, one lane each -- in workgroups of their own, so that no
  //               frame wave waits for the act / rew / end / trunc loads before it issues its frame loads
  const int64_t b = blockIdx.z;
  const int64_t first = p.seg[b * 4 + 0], start = p.seg[b * 4 + 1], len = p.seg[b * 4 + 2];
  if ((int)blockIdx.y == p.T + 1) {
    if (blockIdx.x != 0) return;
    for (int t = threadIdx.x; t < p.T; t += 256) {
      const int64_t s = start + t, f = b * p.T + t;
      const bool valid = s >= 0 && s < len;
      const int64_t a = valid ? first + s : 0;
      if (p.out_act) p.out_act[f] = valid ? p.act[a] : 0;
      if (p.out_rew) p.out_rew[f] = valid ? p.rew[a] : 0.0f;
      const uint8_t e = (valid && p.out_end) ? p.end[a] : 0, tr = (valid && p.out_trunc) ? p.trunc[a] : 0;
      if (p.flag_size == 8) {
        if (p.out_end) ((int64_t*)p.out_end)[f] = e;
        if (p.out_trunc) ((int64_t*)p.out_trunc)[f] = tr;
      } else {
        if (p.out_end) ((uint8_t*)p.out_end)[f] = e;
        if (p.out_trunc) ((uint8_t*)p.out_trunc)[f] = tr;
      }
      if (p.out_mask) p.out_mask[f] = valid ? 1 : 0;
    }
    return;
  }
  const bool is_final = (int)blockIdx.y == p.T;
  const int t = is_final ? 0 : (int)blockIdx.y;
  float* dst = is_final ? p.out_final : p.out_obs;
  if (!dst) return;
  dst += (is_final ? b : b * p.T + t) * p.per_frame;
  const int64_t final_row = p.finals ? p.seg[b * 4 + 3] : -1;
  const int64_t s = start + t;
  const uint8_t* src = nullptr;  // nullptr: a frame of zeros
  if (is_final) {
    if (final_row >= 0) src = p.finals + final_row * p.per_frame;
  } else if (s >= 0 && s < len) {
    src = p.frames + (first + s) * p.per_frame;
  } else if (p.put_back_final && s == len && t >= 1 && len >= 1 && final_row >= 0 && p.end[first + len - 1] != 0) {
    src = p.finals + final_row * p.per_frame;
  }
  const int64_t chunk = blockIdx.x;  // 256 lanes x W levels
  if (W == 16) {
    const int64_t words = units * 4;  // `units` of 16 levels = 4 words each; the chunk's words: chunk * 1024 ... + 1023
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
    if (src) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
        if (w < words) pk[j] = *(const uint32_t*)(src + w * 4);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
      if (w < words) *(f32x4*)(dst + w * 4) = src ? seg_dequant4(pk[j]) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  } else {
    const int64_t u = chunk * 256 + threadIdx.x;  // this lane's unit of W levels
    if (u < units) {
      if (W == 4)
        *(f32x4*)(dst + u * 4) = src ? seg_dequant4(*(const uint32_t*)(src + u * 4)) : (f32x4){0.f, 0.f, 0.f, 0.f};
      else
        dst[u] = src ? seg_dequant(src[u]) : 0.0f;
    }
  }
}

extern "C" int dmd_segment_gather(const dmd_segment_gather_params* pp, dmd_stream_t stream) {
  DMD_CHECK_ARG(pp, "segment_gather: null parameter block");
  const dmd_segment_gather_params& p = *pp;
  DMD_CHECK_ARG(p.frames && p.act && p.rew && p.end && p.trunc && p.seg, "segment_gather: null arena array or descriptor");
  DMD_CHECK_ARG(p.B >= 0 && p.T >= 1 && p.per_frame >= 1, "segment_gather: B %d, T %d, per_frame %lld", p.B, p.T, (long long)p.per_frame);
  DMD_CHECK_ARG(p.flag_size == 1 || p.flag_size == 8, "segment_gather: end / trunc elements of %d bytes (1 or 8)", p.flag_size);
  if (p.B == 0) return 0;
  const uintptr_t u8_bases = (uintptr_t)p.frames | (uintptr_t)p.finals;
  const uintptr_t f32_bases = (uintptr_t)p.out_obs | (uintptr_t)p.out_final;
  const bool words = p.per_frame % 4 == 0 && u8_bases % 4 == 0 && f32_bases % 16 == 0;  // 4-byte loads, 16-byte stores
  const int W = !words ? 1 : (p.per_frame % 16 == 0 ? 16 : 4);
  const int64_t units = p.per_frame / W;
  const int64_t bpf = (units + 255) / 256;
  DMD_CHECK_ARG(p.B <= 65535 && p.T <= 65533 && bpf * (p.T + 2) * p.B <= 0x7fffffffLL,
                "segment_gather: B %d, T %d, %lld workgroups per frame: beyond one launch's grid", p.B, p.T, (long long)bpf);
  // one workgroup per 256 x W levels (a frame of 3 x 64 x 64: three).  Measured at B = 32, T = 20 (tools/replay_bench.py): 10.0 us
  // per launch; fewer, looping workgroups per frame are slower (two: 13.1 us, one: 12.3 us)
  const dim3 grid((unsigned)bpf, (unsigned)p.T + 2, (unsigned)p.B), block(256);
  if (W == 16)
    hipLaunchKernelGGL(segment_gather_kernel<16>, grid, block, 0, (hipStream_t)stream, p, units);
  else if (W == 4)
    hipLaunchKernelGGL(segment_gather_kernel<4>, grid, block, 0, (hipStream_t)stream, p, units);
  else
    hipLaunchKernelGGL(segment_gather_kernel<1>, grid, block, 0, (hipStream_t)stream, p, units);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- device-resident replay store: a window of env steps INTO the uint8 arena in one launch -------------------------------------
// (reference coroutines/collector.py:53-106: a host Episode concatenated step by step, the grown episode uploaded whole again.)
// HBM-bound the other way round: 4 bytes read and 1 written per value.  grid.x runs over FRAMES -- the launch's `total` frames in
// run order, then one workgroup per 256 frames for their small fields --, grid.y over a frame's chunks of 256 x W levels, so a
// workgroup's run (kind, source row, destination row) is uniform: the (R, 4) table is walked through scalar loads (R is a window's
// envs + deaths + moved episodes: tens) and no lane diverges.  W as in the gather: 16 = four words per lane 256 words apart, every
// 16-byte fp32 load of a wave 1 KiB contiguous, every 4-byte packed store 256 bytes contiguous, four loads in flight; 4 = one word
// per lane; 1 = one level per lane, any per_frame, any alignment.  A kind-2 run (an episode moving to a larger slot) copies words.
__device__ __forceinline__ uint32_t rec_levels4(f32x4 v, bool& bad) {
  uint32_t pk = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lc = dmd_level(v[e]);
    bad |= !((lc / 255.0f) * 2.0f - 1.0f == v[e]);  // quantize_u8_kernel's rule
    pk |= (uint32_t)lc << (8 * e);
  }
  return pk;
}

// the run that holds frame f of the launch: (kind, source row, destination row) of that frame; false for a frame beyond the
// runs' sum or in a run the contract excludes (n < 1 is never entered; unknown kind, rows outside the arrays)
__device__ __forceinline__ bool rec_locate(const dmd_record_window_params& p, int64_t f, int64_t& kind, int64_t& src, int64_t& dst) {
  int64_t at = 0;
  for (int r = 0; r < p.R; ++r) {
    const int64_t n = p.runs[r * 4 + 2];
    if (n < 1) continue;
    if (f < at + n) {
      kind = p.runs[r * 4 + 0];
      const int64_t s0 = p.runs[r * 4 + 1], d0 = p.runs[r * 4 + 3];
      src = s0 + (f - at);
      dst = d0 + (f - at);
      if (s0 < 0 || d0 < 0) return false;
      if (kind == 0) return s0 + n <= p.steps && d0 + n <= p.F;
      if (kind == 1) return p.final_obs && p.finals && n == 1 && s0 < p.K && d0 < p.E;
      if (kind == 2) return s0 + n <= p.F && d0 + n <= p.F;
      return false;
    }
    at += n;
  }
  return false;
}

template <int W>
__global__ __launch_bounds__(256) void record_window_kernel(dmd_record_window_params p, int64_t units) {
  int64_t kind = 0, src = 0, dst = 0;
  if ((int64_t)blockIdx.x >= p.total) {  // the small fields of 256 frames, one lane each
    if (blockIdx.y != 0) return;
    const int64_t f = ((int64_t)blockIdx.x - p.total) * 256 + threadIdx.x;
    if (f >= p.total || !rec_locate(p, f, kind, src, dst) || kind == 1) return;
    if (kind == 0) {
      p.arena_act[dst] = p.act[src];
      p.arena_rew[dst] = p.rew[src];
      if (p.flag_size == 8) {
        p.arena_end[dst] = ((const int64_t*)p.end)[src] != 0;
        p.arena_trunc[dst] = ((const int64_t*)p.trunc)[src] != 0;
      } else {
        p.arena_end[dst] = ((const uint8_t*)p.end)[src] != 0;
        p.arena_trunc[dst] = ((const uint8_t*)p.trunc)[src] != 0;
      }
    } else {
      p.arena_act[dst] = p.arena_act[src];
      p.arena_rew[dst] = p.arena_rew[src];
      p.arena_end[dst] = p.arena_end[src];
      p.arena_trunc[dst] = p.arena_trunc[src];
    }
    return;
  }
  if (!rec_locate(p, blockIdx.x, kind, src, dst)) return;
  const float* sf = kind == 0 ? p.obs + src * p.per_frame : (kind == 1 ? p.final_obs + src * p.per_frame : nullptr);
  const uint8_t* sb = p.frames + src * p.per_frame;  // (followed for kind 2 only)
  uint8_t* out = (kind == 1 ? p.finals : p.frames) + dst * p.per_frame;
  const int64_t chunk = blockIdx.y;  // 256 lanes x W levels
  bool bad = false;
  if (W == 16) {
    const int64_t words = units * 4;  // the chunk's words: chunk * 1024 ... + 1023
    if (sf) {
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
        if (w < words) v[j] = *(const f32x4*)(sf + w * 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
        if (w < words) *(uint32_t*)(out + w * 4) = rec_levels4(v[j], bad);
      }
    } else {
      uint32_t pk[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
        if (w < words) pk[j] = *(const uint32_t*)(sb + w * 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = chunk * 1024 + j * 256 + threadIdx.x;
        if (w < words) *(uint32_t*)(out + w * 4) = pk[j];
      }
    }
  } else {
    const int64_t u = chunk * 256 + threadIdx.x;  // this lane's unit of W levels
    if (u < units) {
      if (W == 4) {
        *(uint32_t*)(out + u * 4) = sf ? rec_levels4(*(const f32x4*)(sf + u * 4), bad) : *(const uint32_t*)(sb + u * 4);
      } else if (sf) {
        const float v = sf[u], lc = dmd_level(v);
        bad = !((lc / 255.0f) * 2.0f - 1.0f == v);
        out[u] = (uint8_t)lc;
      } else {
        out[u] = sb[u];
      }
    }
  }
  if (bad) *p.off_grid = 1;  // benign race: every writer stores 1
}

extern "C" int dmd_record_window(const dmd_record_window_params* pp, dmd_stream_t stream) {
  DMD_CHECK_ARG(pp, "record_window: null parameter block");
  const dmd_record_window_params& p = *pp;
  DMD_CHECK_ARG(p.R >= 0 && p.total >= 0 && p.steps >= 0 && p.K >= 0 && p.F >= 0 && p.E >= 0 && p.per_frame >= 1,
                "record_window: R %d, total %lld, steps %lld, K %lld, F %lld, E %lld, per_frame %lld", p.R, (long long)p.total,
                (long long)p.steps, (long long)p.K, (long long)p.F, (long long)p.E, (long long)p.per_frame);
  DMD_CHECK_ARG(p.flag_size == 1 || p.flag_size == 8, "record_window: end / trunc elements of %d bytes (1 or 8)", p.flag_size);
  if (p.R == 0 || p.total == 0) return 0;
  DMD_CHECK_ARG(p.obs && p.act && p.rew && p.end && p.trunc, "record_window: null source array");
  DMD_CHECK_ARG(p.frames && p.arena_act && p.arena_rew && p.arena_end && p.arena_trunc, "record_window: null arena array");
  DMD_CHECK_ARG(p.runs && p.off_grid, "record_window: null runs or off_grid");
  DMD_CHECK_ARG(p.K == 0 || (p.final_obs && p.finals), "record_window: K %lld final observations (kind 1) without final_obs or finals",
                (long long)p.K);
  const uintptr_t u8_bases = (uintptr_t)p.frames | (uintptr_t)p.finals;
  const uintptr_t f32_bases = (uintptr_t)p.obs | (uintptr_t)p.final_obs;
  const bool words = p.per_frame % 4 == 0 && u8_bases % 4 == 0 && f32_bases % 16 == 0;  // 16-byte loads, 4-byte stores
  const int W = !words ? 1 : (p.per_frame % 16 == 0 ? 16 : 4);
  const int64_t units = p.per_frame / W;
  const int64_t bpf = (units + 255) / 256;
  const int64_t gx = p.total + (p.total + 255) / 256;
  DMD_CHECK_ARG(gx <= 0x7fffffffLL && bpf <= 65535 && gx * bpf <= 0x7fffffffLL,
                "record_window: %lld frames of %lld workgroups: beyond one launch's grid", (long long)p.total, (long long)bpf);
  const dim3 grid((unsigned)gx, (unsigned)bpf), block(256);
  if (W == 16)
    hipLaunchKernelGGL(record_window_kernel<16>, grid, block, 0, (hipStream_t)stream, p, units);
  else if (W == 4)
    hipLaunchKernelGGL(record_window_kernel<4>, grid, block, 0, (hipStream_t)stream, p, units);
  else
    hipLaunchKernelGGL(record_window_kernel<1>, grid, block, 0, (hipStream_t)stream, p, units);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- open-loop world-model evaluation: one step closed on the device ------------------------------------------------------------
// The sampler's frame `pred` against what the arena recorded at that episode step, then the ring advance from the prediction
// (free running) or from the recording (teacher forced): the frame metrics in uint8 levels, the recorded reward / end of the
// transition, two validity flags, the ring's oldest slot overwritten.  One workgroup per SAMPLE -- what its frame's target is (an
// arena row, the final observation, or nothing) is uniform over the workgroup, the descriptor comes through scalar loads, and the
// four metrics are reduced inside it: lanes' partial sums over the wave (__shfl_xor butterfly), the four waves through LDS, in a
// fixed order; they are integers, so any order gives the same bits.  HBM-bound: per value 4 bytes of `pred` and 1 of the target
// in, 4 bytes of ring (and 1 of levels) out.  Lanes walk the frame as dmd_segment_gather's do: 4-byte target words, 16-byte fp32
// accesses, consecutive lanes on consecutive words (a wave's fp32 access is 1 KiB contiguous); W = 16 keeps four words 1 KiB apart
// in flight per lane, W = 4 one; W = 1 is the any-size, any-alignment path.
struct ol_sums {
  unsigned long long sq, ab, off;
  unsigned int mx;
};

// q = level(v) against the target level t; returns q
__device__ __forceinline__ uint32_t ol_level(float v, uint32_t t, ol_sums& a) {
  const int q = (int)dmd_level(v);
  const int d = q - (int)t;
  const unsigned int m = (unsigned int)(d < 0 ? -d : d);
  a.sq += m * m;
  a.ab += m;
  a.off += m != 0 ? 1u : 0u;
  a.mx = m > a.mx ? m : a.mx;
  return (uint32_t)q;
}

__device__ __forceinline__ uint32_t ol_word(const f32x4 v, uint32_t tgt, ol_sums& a) {
  uint32_t lv = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) lv |= ol_level(v[e], (tgt >> (8 * e)) & 0xff, a) << (8 * e);
  return lv;
}

__device__ __forceinline__ unsigned long long ol_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int W>
__global__ __launch_bounds__(256) void openloop_step_kernel(dmd_openloop_params p) {
  __shared__ unsigned long long red[4][4];
  const int64_t b = blockIdx.x, pf = p.per_frame;
  const int tid = threadIdx.x;
  const int64_t first = p.seg[b * 4 + 0], start = p.seg[b * 4 + 1], len = p.seg[b * 4 + 2];
  const int64_t final_row = p.finals ? p.seg[b * 4 + 3] : -1;
  const int64_t s = start + p.T + p.step;  // the predicted frame's episode step; its transition is s - 1
  const uint8_t* src = nullptr;            // nullptr: no recorded frame (invalid)
  if (s >= 0 && s < len)
    src = p.frames + (first + s) * pf;
  else if (s == len && len >= 1 && final_row >= 0 && p.end[first + len - 1] != 0)
    src = p.finals + final_row * pf;
  const bool forced = p.teacher_forced != 0 && src != nullptr;
  const float* pred = p.pred + b * pf;
  float* ring = p.ctx_obs + (b * p.T + p.head) * pf;
  uint8_t* lev = p.out_levels ? p.out_levels + b * pf : nullptr;
  ol_sums a = {0ull, 0ull, 0ull, 0u};
  if (W == 1) {
    for (int64_t u = tid; u < pf; u += 256) {
      const float v = pred[u];
      const uint32_t t = src ? src[u] : 0u;
      const uint32_t q = ol_level(v, t, a);
      ring[u] = forced ? seg_dequant(t) : v;
      if (lev) lev[u] = (uint8_t)q;
    }
  } else {
    constexpr int U = W == 16 ? 4 : 1;  // words in flight per lane
    const int64_t words = pf >> 2;
    for (int64_t w0 = 0; w0 < words; w0 += 256 * U) {
      f32x4 v[U];
      uint32_t pk[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t w = w0 + k * 256 + tid;
        pk[k] = 0u;
        if (w < words) {
          v[k] = *(const f32x4*)(pred + w * 4);
          if (src) pk[k] = *(const uint32_t*)(src + w * 4);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t w = w0 + k * 256 + tid;
        if (w < words) {
          const uint32_t q = ol_word(v[k], pk[k], a);
          *(f32x4*)(ring + w * 4) = forced ? seg_dequant4(pk[k]) : v[k];
          if (lev) *(uint32_t*)(lev + w * 4) = q;
        }
      }
    }
  }
  // every lane arrives here (no early exit above): wave butterflies, then the four waves in order
  a.sq = ol_wave_sum(a.sq);
  a.ab = ol_wave_sum(a.ab);
  a.off = ol_wave_sum(a.off);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned int o = __shfl_xor(a.mx, off, 64);
    a.mx = o > a.mx ? o : a.mx;
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a.sq;
    red[tid >> 6][1] = a.ab;
    red[tid >> 6][2] = a.mx;
    red[tid >> 6][3] = a.off;
  }
  __syncthreads();
  if (tid != 0) return;
  unsigned long long m[4] = {0ull, 0ull, 0ull, 0ull};
  if (src) {
    for (int wv = 0; wv < 4; ++wv) {
      m[0] += red[wv][0];
      m[1] += red[wv][1];
      m[2] = red[wv][2] > m[2] ? red[wv][2] : m[2];
      m[3] += red[wv][3];
    }
  }
  for (int k = 0; k < 4; ++k) p.metrics[b * 4 + k] = (int64_t)m[k];
  const int64_t j = s - 1;
  const bool tv = j >= 0 && j < len, sv = s >= 0 && s < len;
  p.out_rew[b] = tv ? p.rew[first + j] : 0.0f;
  p.out_end[b] = tv ? p.end[first + j] : (uint8_t)0;
  p.out_valid[b * 2 + 0] = src ? 1 : 0;
  p.out_valid[b * 2 + 1] = tv ? 1 : 0;
  p.ctx_act[b * p.T + p.head] = sv ? p.act[first + s] : 0;
}

extern "C" int dmd_openloop_step(const dmd_openloop_params* pp, dmd_stream_t stream) {
  DMD_CHECK_ARG(pp, "openloop_step: null parameter block");
  const dmd_openloop_params& p = *pp;
  DMD_CHECK_ARG(p.frames && p.act && p.rew && p.end && p.seg, "openloop_step: null arena array or descriptor");
  DMD_CHECK_ARG(p.pred && p.ctx_obs && p.ctx_act, "openloop_step: null prediction or context ring");
  DMD_CHECK_ARG(p.metrics && p.out_rew && p.out_end && p.out_valid, "openloop_step: null output (only out_levels is optional)");
  DMD_CHECK_ARG(p.B >= 0 && p.T >= 1 && p.per_frame >= 1 && p.per_frame <= (1ll << 40), "openloop_step: B %d, T %d, per_frame %lld", p.B, p.T,
                (long long)p.per_frame);
  DMD_CHECK_ARG(p.step >= 0 && p.head >= 0 && p.head < p.T, "openloop_step: step %d (>= 0), head %d of a ring of %d", p.step, p.head, p.T);
  DMD_CHECK_ARG(p.teacher_forced == 0 || p.teacher_forced == 1, "openloop_step: teacher_forced %d (0 or 1)", p.teacher_forced);
  if (p.B == 0) return 0;
  const uintptr_t u8_bases = (uintptr_t)p.frames | (uintptr_t)p.finals | (uintptr_t)p.out_levels;
  const uintptr_t f32_bases = (uintptr_t)p.pred | (uintptr_t)p.ctx_obs;
  const bool words = p.per_frame % 4 == 0 && u8_bases % 4 == 0 && f32_bases % 16 == 0;  // 4-byte level words, 16-byte fp32 accesses
  const dim3 grid((unsigned)p.B), block(256);
  if (words && p.per_frame % 16 == 0)
    hipLaunchKernelGGL(openloop_step_kernel<16>, grid, block, 0, (hipStream_t)stream, p);
  else if (words)
    hipLaunchKernelGGL(openloop_step_kernel<4>, grid, block, 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(openloop_step_kernel<1>, grid, block, 0, (hipStream_t)stream, p);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- open-loop evaluation: what moved, and what copying a frame would have scored ------------------------------------------------
// Launched BEFORE openloop_step_kernel of the same step, on the ring as it stands: the target y against the previous recorded
// frame r and the context's last frame a (the two "models" that copy a frame), and the prediction's level q against the level m
// of the ring's newest frame (what the model itself saw last) -- eight exact integer sums per sample, the contract at
// dmd_openloop_motion in include/diamond_hip.h.  Read-only but for `out` / `out_valid`.  One workgroup per sample and the lane
// walk of openloop_step_kernel (4-byte level words, 16-byte fp32 accesses, W = 16 / 4 / 1), per value 3 bytes of levels and 8 of
// fp32 in; r and a are not loaded where they are not valid (level 0 stands in, the sums that use it are zeroed by lane 0), and a
// sample without a target loads nothing at all.  Seven 64-bit sums: wave butterflies, then the four waves through LDS in order.
#define OM_SUMS 7
struct om_sums {
  unsigned long long e[OM_SUMS];
};

// the target of sample b at `step`, nullptr where there is none: the rule of openloop_step_kernel, restated (that kernel's and
// frame_ssim_tile_kernel's machine code stay as measured; the tests hold the three against each other on every kind of row)
__device__ __forceinline__ const uint8_t* om_target(const dmd_openloop_motion_params& p, int64_t first, int64_t s, int64_t len,
                                                    int64_t final_row, int64_t pf) {
  if (s >= 0 && s < len) return p.frames + (first + s) * pf;
  if (s == len && len >= 1 && final_row >= 0 && p.end[first + len - 1] != 0) return p.finals + final_row * pf;
  return nullptr;
}

__device__ __forceinline__ void om_level(uint32_t y, uint32_t r, uint32_t a, float pv, float mv, om_sums& s) {
  const int q = (int)dmd_level(pv), m = (int)dmd_level(mv);
  const int dr = (int)y - (int)r, da = (int)y - (int)a, dq = q - (int)y;
  const bool moved = dr != 0, pred_moved = q != m;
  s.e[0] += (unsigned int)(dr * dr);
  s.e[1] += (unsigned int)(da * da);
  s.e[2] += moved ? 1u : 0u;
  s.e[3] += pred_moved ? 1u : 0u;
  s.e[4] += moved && pred_moved ? 1u : 0u;
  s.e[5] += moved ? (unsigned int)(dq * dq) : 0u;
  s.e[6] += moved && dq == 0 ? 1u : 0u;
}

template <int W>
__global__ __launch_bounds__(256) void openloop_motion_kernel(dmd_openloop_motion_params p) {
  __shared__ unsigned long long red[4][OM_SUMS];
  const int64_t b = blockIdx.x, pf = p.per_frame;
  const int tid = threadIdx.x;
  const int64_t first = p.seg[b * 4 + 0], start = p.seg[b * 4 + 1], len = p.seg[b * 4 + 2];
  const int64_t final_row = p.finals ? p.seg[b * 4 + 3] : -1;
  const int64_t s = start + p.T + p.step, c = start + p.T - 1;  // the predicted frame's episode step; the context's last
  const uint8_t* ysrc = om_target(p, first, s, len, final_row, pf);
  const uint8_t* rsrc = ysrc && s >= 1 ? p.frames + (first + s - 1) * pf : nullptr;  // (a valid frame has s <= len)
  const uint8_t* asrc = ysrc && c >= 0 && c < len ? p.frames + (first + c) * pf : nullptr;
  const float* pred = p.pred + b * pf;
  const float* seen = p.ctx_obs + (b * p.T + (p.head + p.T - 1) % p.T) * pf;
  om_sums acc;
#pragma unroll
  for (int k = 0; k < OM_SUMS; ++k) acc.e[k] = 0ull;
  if (ysrc) {  // uniform over the workgroup
    if (W == 1) {
      for (int64_t u = tid; u < pf; u += 256)
        om_level(ysrc[u], rsrc ? rsrc[u] : 0u, asrc ? asrc[u] : 0u, pred[u], seen[u], acc);
    } else {
      constexpr int U = W == 16 ? 4 : 1;  // words in flight per lane
      const int64_t words = pf >> 2;
      for (int64_t w0 = 0; w0 < words; w0 += 256 * U) {
        f32x4 pv[U], mv[U];
        uint32_t yk[U], rk[U], ak[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t w = w0 + k * 256 + tid;
          rk[k] = ak[k] = 0u;
          if (w < words) {
            pv[k] = *(const f32x4*)(pred + w * 4);
            mv[k] = *(const f32x4*)(seen + w * 4);
            yk[k] = *(const uint32_t*)(ysrc + w * 4);
            if (rsrc) rk[k] = *(const uint32_t*)(rsrc + w * 4);
            if (asrc) ak[k] = *(const uint32_t*)(asrc + w * 4);
          }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          if (w0 + k * 256 + tid < words) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              om_level((yk[k] >> (8 * e)) & 0xff, (rk[k] >> (8 * e)) & 0xff, (ak[k] >> (8 * e)) & 0xff, pv[k][e], mv[k][e], acc);
          }
        }
      }
    }
  }
  // every lane arrives here: wave butterflies, then the four waves in order
#pragma unroll
  for (int k = 0; k < OM_SUMS; ++k) acc.e[k] = ol_wave_sum(acc.e[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < OM_SUMS; ++k) red[tid >> 6][k] = acc.e[k];
  }
  __syncthreads();
  if (tid != 0) return;
  unsigned long long m[OM_SUMS];
  for (int k = 0; k < OM_SUMS; ++k) m[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  if (!rsrc) m[0] = m[2] = m[4] = m[5] = m[6] = 0ull;
  if (!asrc) m[1] = 0ull;
  for (int k = 0; k < OM_SUMS; ++k) p.out[b * 8 + k] = (int64_t)m[k];
  p.out[b * 8 + 7] = 0;
  p.out_valid[b * 3 + 0] = ysrc ? 1 : 0;
  p.out_valid[b * 3 + 1] = rsrc ? 1 : 0;
  p.out_valid[b * 3 + 2] = asrc ? 1 : 0;
}

extern "C" int dmd_openloop_motion(const dmd_openloop_motion_params* pp, dmd_stream_t stream) {
  DMD_CHECK_ARG(pp, "openloop_motion: null parameter block");
  const dmd_openloop_motion_params& p = *pp;
  DMD_CHECK_ARG(p.frames && p.end && p.seg, "openloop_motion: null arena array or descriptor");
  DMD_CHECK_ARG(p.pred && p.ctx_obs, "openloop_motion: null prediction or context ring");
  DMD_CHECK_ARG(p.out && p.out_valid, "openloop_motion: null output");
  DMD_CHECK_ARG(p.B >= 0 && p.T >= 1 && p.per_frame >= 1 && p.per_frame <= (1ll << 40), "openloop_motion: B %d, T %d, per_frame %lld", p.B, p.T,
                (long long)p.per_frame);
  DMD_CHECK_ARG(p.step >= 0 && p.head >= 0 && p.head < p.T, "openloop_motion: step %d (>= 0), head %d of a ring of %d", p.step, p.head, p.T);
  if (p.B == 0) return 0;
  const uintptr_t u8_bases = (uintptr_t)p.frames | (uintptr_t)p.finals;
  const uintptr_t f32_bases = (uintptr_t)p.pred | (uintptr_t)p.ctx_obs;
  const bool words = p.per_frame % 4 == 0 && u8_bases % 4 == 0 && f32_bases % 16 == 0;  // 4-byte level words, 16-byte fp32 loads
  const dim3 grid((unsigned)p.B), block(256);
  if (words && p.per_frame % 16 == 0)
    hipLaunchKernelGGL(openloop_motion_kernel<16>, grid, block, 0, (hipStream_t)stream, p);
  else if (words)
    hipLaunchKernelGGL(openloop_motion_kernel<4>, grid, block, 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(openloop_motion_kernel<1>, grid, block, 0, (hipStream_t)stream, p);
  DMD_LAUNCH_CHECK();
  return 0;
}

// ---- per-frame SSIM of uint8 levels in fp64 (open-loop evaluation's structure metric) -------------------------------------------
// Wang et al. 2004, 11 x 11 window of weights win[i] * win[j], positions whose window lies inside the frame; the contract and the
// summation order are stated at dmd_frame_ssim in include/diamond_hip.h.  The window sum is SEPARABLE: a workgroup owns one
// channel's tile of SSIM_S x SSIM_S positions, stages the (SSIM_S + 10)^2 levels of both operands in LDS (as floats: exact), forms
// the five horizontal sums of its (SSIM_S + 10) x SSIM_S (row, column) pairs into LDS as doubles, and each lane then the five
// vertical sums of its own position: 2 x 11 taps per moment where the direct form has 121.  fp64 throughout, no atomics: the
// tile's two sums are reduced by a wave butterfly and then over the four waves in order, written to the workspace, and a second
// launch adds a frame's tiles in one fixed order.  x and y go through the same operations (identical frames: exactly 1.0).
// Compute-light (a 3 x 64 x 64 batch of 32: 1536 workgroups, ~75 kFLOP each); levels are read byte by byte, so any alignment.
#define SSIM_S 16
#define SSIM_IN (SSIM_S + DMD_SSIM_TAPS - 1)
// level rows 48 floats apart: rows r and r + 1, which share a 32-lane group in the horizontal pass, sit on disjoint halves of the
// 32 banks a 4-byte LDS read sees
#define SSIM_LD 48

__device__ __forceinline__ double ssim_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// operand b of sample n in arena mode, nullptr where the sample has no target: the rule of openloop_step_kernel, restated (with
// one shared device function that kernel's machine code changed, and its measurements and GPU runs are to stay valid) -- the
// tests hold the two against each other on every kind of descriptor row
__device__ __forceinline__ const uint8_t* ssim_arena_target(const dmd_ssim_params& p, int64_t n, int64_t pf) {
  const int64_t first = p.seg[n * 4 + 0], start = p.seg[n * 4 + 1], len = p.seg[n * 4 + 2];
  const int64_t final_row = p.finals ? p.seg[n * 4 + 3] : -1;
  const int64_t s = start + p.T + p.step;
  if (s >= 0 && s < len) return p.frames + (first + s) * pf;
  if (s == len && len >= 1 && final_row >= 0 && p.end[first + len - 1] != 0) return p.finals + final_row * pf;
  return nullptr;
}

__global__ __launch_bounds__(256) void frame_ssim_tile_kernel(dmd_ssim_params p, int tiles_x) {
  __shared__ float lev[2][SSIM_IN][SSIM_LD];
  __shared__ double hsum[5][SSIM_IN][SSIM_S];
  __shared__ double red[4][2];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y;
  const int64_t n = blockIdx.z;
  const int64_t plane = (int64_t)p.H * p.W, pf = plane * p.C;
  const uint8_t* b_u8 = p.b_u8;
  if (p.seg) {  // arena mode (uniform over the workgroup): a sample without a target is left to the second launch
    b_u8 = ssim_arena_target(p, n, pf);
    if (!b_u8) return;
  } else if (b_u8) {
    b_u8 += n * pf;
  }
  const int64_t base = n * pf + c * plane;
  const int y0 = (tile / tiles_x) * SSIM_S, x0 = (tile % tiles_x) * SSIM_S;
  // 1. the levels of the tile and its 10-wide apron; outside the frame: zeros (they reach only positions that do not count)
  for (int i = tid; i < SSIM_IN * SSIM_IN; i += 256) {
    const int r = i / SSIM_IN, q = i - r * SSIM_IN;
    const int y = y0 + r, x = x0 + q;
    float va = 0.0f, vb = 0.0f;
    if (y < p.H && x < p.W) {
      const int64_t at = (int64_t)y * p.W + x;
      va = p.a_u8 ? (float)p.a_u8[base + at] : dmd_level(p.a_f32[base + at]);
      vb = b_u8 ? (float)b_u8[c * plane + at] : dmd_level(p.b_f32[base + at]);
    }
    lev[0][r][q] = va;
    lev[1][r][q] = vb;
  }
  __syncthreads();
  // 2. horizontal sums, taps ascending
  for (int i = tid; i < SSIM_IN * SSIM_S; i += 256) {
    const int r = i / SSIM_S, q = i - r * SSIM_S;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int k = 0; k < DMD_SSIM_TAPS; ++k) {
      const double w = p.win[k], x = (double)lev[0][r][q + k], y = (double)lev[1][r][q + k];
      sx += w * x;
      sy += w * y;
      sxx += w * (x * x);
      syy += w * (y * y);
      sxy += w * (x * y);
    }
    hsum[0][r][q] = sx;
    hsum[1][r][q] = sy;
    hsum[2][r][q] = sxx;
    hsum[3][r][q] = syy;
    hsum[4][r][q] = sxy;
  }
  __syncthreads();
  // 3. vertical sums of this lane's position, taps ascending; then the two ratios
  const int ty = tid / SSIM_S, tx = tid - ty * SSIM_S;
  double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < DMD_SSIM_TAPS; ++k) {
    const double w = p.win[k];
#pragma unroll
    for (int j = 0; j < 5; ++j) m[j] += w * hsum[j][ty + k][tx];
  }
  double ssim = 0.0, cs = 0.0;
  if (y0 + ty < p.H - (DMD_SSIM_TAPS - 1) && x0 + tx < p.W - (DMD_SSIM_TAPS - 1)) {
    const double mx = m[0], my = m[1];
    const double vxx = m[2] - mx * mx, vyy = m[3] - my * my, vxy = m[4] - mx * my;
    cs = (2.0 * vxy + p.c2) / (vxx + vyy + p.c2);
    ssim = (2.0 * (mx * my) + p.c1) / (mx * mx + my * my + p.c1) * cs;
  }
  // 4. the tile's sums: every lane arrives here; wave butterflies, then the four waves in order
  ssim = ssim_wave_sum(ssim);
  cs = ssim_wave_sum(cs);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = ssim;
    red[tid >> 6][1] = cs;
  }
  __syncthreads();
  if (tid != 0) return;
  double t0 = 0.0, t1 = 0.0;
  for (int wv = 0; wv < 4; ++wv) {
    t0 += red[wv][0];
    t1 += red[wv][1];
  }
  double* part = p.workspace + ((n * p.C + c) * (int64_t)gridDim.x + tile) * 2;
  part[0] = t0;
  part[1] = t1;
}

// one wave per frame: lane l adds the frame's partials l, l + 64, ... in ascending order, then the butterfly
__global__ __launch_bounds__(64) void frame_ssim_mean_kernel(dmd_ssim_params p, int64_t parts) {
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x;
  const bool valid = !p.seg || ssim_arena_target(p, n, (int64_t)p.H * p.W * p.C) != nullptr;  // uniform over the wave
  double s0 = 0.0, s1 = 0.0;
  if (valid) {
    const double* part = p.workspace + n * parts * 2;
    for (int64_t i = lane; i < parts; i += 64) {
      s0 += part[i * 2 + 0];
      s1 += part[i * 2 + 1];
    }
  }
  s0 = ssim_wave_sum(s0);
  s1 = ssim_wave_sum(s1);
  if (lane != 0) return;
  const double count = (double)((int64_t)p.C * (p.H - (DMD_SSIM_TAPS - 1)) * (p.W - (DMD_SSIM_TAPS - 1)));
  const double none = __builtin_nan("");  // a sample without a target
  p.out[n * 2 + 0] = valid ? s0 / count : none;
  p.out[n * 2 + 1] = valid ? s1 / count : none;
}

static bool ssim_sizes_ok(int64_t N, int64_t C, int64_t H, int64_t W) {
  return N >= 0 && N <= 65535 && C >= 1 && C <= 65535 && H >= DMD_SSIM_TAPS && W >= DMD_SSIM_TAPS && H <= 32768 && W <= 32768;
}

static int64_t ssim_tiles(int64_t extent) { return (extent - (DMD_SSIM_TAPS - 1) + SSIM_S - 1) / SSIM_S; }

extern "C" int64_t dmd_ssim_workspace_doubles(int N, int C, int H, int W) {
  if (!ssim_sizes_ok(N, C, H, W)) return 0;
  return 2 * (int64_t)N * C * ssim_tiles(H) * ssim_tiles(W);
}

extern "C" int dmd_frame_ssim(const dmd_ssim_params* pp, dmd_stream_t stream) {
  DMD_CHECK_ARG(pp, "frame_ssim: null parameter block");
  const dmd_ssim_params& p = *pp;
  DMD_CHECK_ARG(p.H >= DMD_SSIM_TAPS && p.W >= DMD_SSIM_TAPS, "frame_ssim: frames of %d x %d, the window needs %d x %d", p.H, p.W, DMD_SSIM_TAPS,
                DMD_SSIM_TAPS);
  DMD_CHECK_ARG(ssim_sizes_ok(p.N, p.C, p.H, p.W), "frame_ssim: N %d (0 ... 65535), C %d (1 ... 65535), H %d, W %d (11 ... 32768)", p.N, p.C, p.H, p.W);
  DMD_CHECK_ARG((p.a_f32 != nullptr) != (p.a_u8 != nullptr), "frame_ssim: operand a needs exactly one of a_f32 / a_u8");
  const bool arena = p.frames || p.finals || p.end || p.seg;
  if (arena) {
    DMD_CHECK_ARG(!p.b_f32 && !p.b_u8, "frame_ssim: a direct operand b together with arena fields");
    DMD_CHECK_ARG(p.frames && p.end && p.seg, "frame_ssim: arena mode needs frames, end and seg");
  } else {
    DMD_CHECK_ARG((p.b_f32 != nullptr) != (p.b_u8 != nullptr), "frame_ssim: operand b needs exactly one of b_f32 / b_u8 (or the arena fields)");
  }
  DMD_CHECK_ARG(p.T >= 0 && p.step >= 0, "frame_ssim: T %d, step %d (both >= 0)", p.T, p.step);
  DMD_CHECK_ARG(p.out && p.workspace, "frame_ssim: null out or workspace");
  if (p.N == 0) return 0;
  const int64_t tx = ssim_tiles(p.W), ty = ssim_tiles(p.H);
  DMD_CHECK_ARG(tx * ty * p.C * p.N <= 0x7fffffffLL, "frame_ssim: %lld workgroups: beyond one launch's grid", (long long)(tx * ty * p.C * p.N));
  hipLaunchKernelGGL(frame_ssim_tile_kernel, dim3((unsigned)(tx * ty), (unsigned)p.C, (unsigned)p.N), dim3(256), 0, (hipStream_t)stream, p, (int)tx);
  DMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_ssim_mean_kernel, dim3((unsigned)p.N), dim3(64), 0, (hipStream_t)stream, p, tx * ty * p.C);
  DMD_LAUNCH_CHECK();
  return 0;
}
