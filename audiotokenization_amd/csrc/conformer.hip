// Conformer-STFT codec family (vq/codec_encoder.py:92-209, vq/codec_decoder.py:145-274, 385-509,
// vq/module.py:357-547): everything of it that is not a Linear / 1x1 conv (those run on the conv path).
//
//  stft_frames_kernel : STFT.forward (codec_encoder.py:108-122) as a basis product, real rows then imaginary rows.
//  rmsnorm_kernel     : rmsnorm / RMSNorm over channels per (b, t) (module.py:357-370), optional gain, optional SiLU.
//  dwconv_glu_kernel  : nn.GLU(dim=1) + the depthwise conv (module.py:476-480, 488-489), the gate applied on load.
//  swiglu_kernel      : silu(w1 x) * (w3 x) over the stacked w1 / w3 output (module.py:468).
//  attention_kernel   : q / k RMS norm, RoPE, softmax(q k^T / sqrt(D)) v (module.py:416-453, manual branch), flash
//                       style: keys and values pass through LDS in tiles, the softmax is online, no T x T array.
//  istft_head_kernel  : ISTFTHead after its Linear (codec_decoder.py:171-213, 261-274): exp / clip / cos / sin, irfft as
//                       a basis product, window, overlap-add, crop, division by the window-square envelope.
//
// All of it is fp32 VALU arithmetic whatever the conv precision mode is (the long sums fold 16-term fp32 partial
// sums into an fp64 total); none of these kernels uses the matrix cores (DESIGN.md section 26 says what that costs).
#include <algorithm>
#include "../../include/bigcodec.h"
#include "bc_common.h"
#include "bc_internal.h"

namespace bc {

// cos(x) with bc_sin's reduction (the published SLEEF xcosf: q = 1 + 2 rint(x / pi - 0.5) quarter periods, Cody-Waite
// by pi / 2 in four fma steps, the same odd polynomial); inputs outside the reduction range take cosf.
__device__ __forceinline__ float bc_cos(float x) {
  if (!(fabsf(x) < 39000.0f)) return cosf(x);
  const float q = 1.0f + 2.0f * rintf(x * 0.318309886183790671538f - 0.5f);
  float d = fmaf(q, -3.140625f * 0.5f, x);
  d = fmaf(q, -0.0009670257568359375f * 0.5f, d);
  d = fmaf(q, -6.2771141529083251953e-07f * 0.5f, d);
  d = fmaf(q, -1.2154201256553420762e-10f * 0.5f, d);
  const float s = d * d;
  if ((((int)q) & 2) == 0) d = -d;
  float u = 2.6083159809786593541503e-06f;
  u = fmaf(u, s, -0.0001981069071916863322258f);
  u = fmaf(u, s, 0.00833307858556509017944336f);
  u = fmaf(u, s, -0.166666597127914428710938f);
  return fmaf(s, u * d, d);
}

__device__ __forceinline__ float bc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- STFT ----------------------------------------------------------------------------------------------------------
// y[b][c][f] = sum_n basisT[n][c] * xpad[b][f * hop - pad + n], c < C2 = 2 * bins, zero outside the clip.
// One workgroup: STFT_FT frames of one clip x 256 channels; the frames' samples sit in LDS (broadcast reads).
constexpr int STFT_FT = 8;
constexpr int ACC_CHUNK = 16;  // fp32 terms per partial sum before it joins the fp64 total

__global__ void __launch_bounds__(256) stft_frames_kernel(const float* __restrict__ x, const float* __restrict__ basisT,
                                                          float* __restrict__ y, long long T, int n_fft, int hop, int pad,
                                                          int F, int C2) {
  extern __shared__ float stft_xs[];
  const int f0 = blockIdx.x * STFT_FT, b = blockIdx.z;
  const int c = blockIdx.y * 256 + threadIdx.x;
  const int span = (STFT_FT - 1) * hop + n_fft;
  const long long s0 = (long long)f0 * hop - pad;
  const float* xb = x + (long long)b * T;
  for (int e = threadIdx.x; e < span; e += 256) {
    const long long s = s0 + e;
    stft_xs[e] = (s >= 0 && s < T) ? xb[s] : 0.f;
  }
  __syncthreads();
  if (c >= C2) return;
  double acc[STFT_FT];
  float part[STFT_FT];
#pragma unroll
  for (int i = 0; i < STFT_FT; ++i) acc[i] = 0.0, part[i] = 0.f;
  for (int n0 = 0; n0 < n_fft; n0 += ACC_CHUNK) {
    const int n1 = min(n0 + ACC_CHUNK, n_fft);
    for (int n = n0; n < n1; ++n) {
      const float bv = basisT[(long long)n * C2 + c];
#pragma unroll
      for (int i = 0; i < STFT_FT; ++i) part[i] = fmaf(bv, stft_xs[i * hop + n], part[i]);
    }
#pragma unroll
    for (int i = 0; i < STFT_FT; ++i) acc[i] += (double)part[i], part[i] = 0.f;
  }
  float* yr = y + ((long long)b * C2 + c) * F;
#pragma unroll
  for (int i = 0; i < STFT_FT; ++i)
    if (f0 + i < F && BC_DOK(c < C2 && f0 + i >= 0)) yr[f0 + i] = (float)acc[i];
}

// ---- RMSNorm over channels -----------------------------------------------------------------------------------------
// One thread per (b, t): y[c] = (x[c] * rsqrt(mean_c x^2 + eps)) * w[c], then SiLU when asked; coalesced over t.
__global__ void __launch_bounds__(256) rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ y, int C, int T, float eps, int silu,
                                                      long long rows) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;  // b * T + t
  if (r >= rows) return;
  const long long b = r / T, t = r - b * T;
  const float* xr = x + b * C * T + t;
  float* yr = y + b * C * T + t;
  double ss = 0.0;
  for (int c = 0; c < C; ++c) {
    const float v = xr[(long long)c * T];
    ss += (double)(v * v);
  }
  const float mean = (float)(ss / (double)C);
  const float rs = 1.0f / sqrtf(mean + eps);
  for (int c = 0; c < C; ++c) {
    float v = xr[(long long)c * T] * rs;
    if (w) v = v * w[c];
    if (silu) v = v * bc_sigmoid(v);
    if (BC_DOK(c < C && t < T)) yr[(long long)c * T] = v;
  }
}

// ---- GLU + depthwise conv ------------------------------------------------------------------------------------------
// x is the (B, 2C, T) output of pointwise_conv1: g[c][t] = x[c][t] * sigmoid(x[C + c][t]);
// y[b][c][t] = bias[c] + sum_k w[c][k] g[c][t + k - pl], zero outside [0, T).  One workgroup: 256 outputs of a row.
constexpr int DW_TILE = 256;
constexpr int DW_MAXK = 63;

__global__ void __launch_bounds__(256) dwconv_glu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int C,
                                                         int T, int K, int pl, int ntiles) {
  __shared__ float g[DW_TILE + DW_MAXK];
  __shared__ float wk[DW_MAXK + 1];
  const int tile = blockIdx.x % ntiles;
  const long long row = blockIdx.x / ntiles;  // b * C + c
  const int c = (int)(row % C);
  const long long b = row / C;
  const float* xa = x + (b * 2 * C + c) * T;
  const float* xg = xa + (long long)C * T;
  const int t0 = tile * DW_TILE;
  for (int e = threadIdx.x; e < DW_TILE + K - 1; e += 256) {
    const int t = t0 + e - pl;
    g[e] = (t >= 0 && t < T) ? xa[t] * bc_sigmoid(xg[t]) : 0.f;
  }
  if (threadIdx.x < K) wk[threadIdx.x] = w[c * K + threadIdx.x];
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= T) return;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(wk[k], g[threadIdx.x + k], acc);
  if (bias) acc += bias[c];
  if (BC_DOK(t >= 0 && t < T)) y[row * T + t] = acc;
}

// ---- SwiGLU --------------------------------------------------------------------------------------------------------
// h is the (B, 2H, T) output of the stacked w1 / w3 conv: y[b][j][t] = silu(h[b][j][t]) * h[b][H + j][t].
__global__ void __launch_bounds__(256) swiglu_kernel(const float* __restrict__ h, float* __restrict__ y, long long HT,
                                                     long long total) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const long long b = e / HT, r = e - b * HT;
    const float a = h[b * 2 * HT + r], g = h[b * 2 * HT + HT + r];
    y[e] = (a * bc_sigmoid(a)) * g;
  }
}

// ---- attention -----------------------------------------------------------------------------------------------------
// qkv[b][s * dim + h * D + d][t] (s = 0 q, 1 k, 2 v); rope[t][i] = (cos, sin) of pair i < D / 2;
// y[b][h * D + d][t].  One workgroup: ATT_QT queries of one (b, h), one query per thread, q and the output row in
// registers; keys and values pass through LDS ATT_KT at a time (threads [0, ATT_KT) normalise and rotate a key each,
// threads [ATT_KT, 2 ATT_KT) copy a value each), every lane reads the same LDS word (broadcast).
constexpr int ATT_QT = 128;
constexpr int ATT_KT = 64;

template <int D>
__device__ __forceinline__ void norm_rope(float (&v)[D], const float* __restrict__ rope_t) {
  float ss = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) ss = fmaf(v[d], v[d], ss);
  const float rs = 1.0f / sqrtf(ss * (1.0f / D) + 1e-6f);
#pragma unroll
  for (int i = 0; i < D / 2; ++i) {
    const float a = v[2 * i] * rs, bq = v[2 * i + 1] * rs;
    const float co = rope_t[2 * i], si = rope_t[2 * i + 1];
    v[2 * i] = a * co - bq * si;
    v[2 * i + 1] = a * si + bq * co;
  }
}

template <int D>
__global__ void __launch_bounds__(ATT_QT) attention_kernel(const float* __restrict__ qkv, const float* __restrict__ rope,
                                                           float* __restrict__ y, int n_head, int T, int causal) {
  constexpr int P = D + 4;  // LDS row pitch: 16-byte rows, staging writes spread over 16 banks
  __shared__ __attribute__((aligned(16))) float ks[ATT_KT * P];
  __shared__ __attribute__((aligned(16))) float vs[ATT_KT * P];
  const int h = blockIdx.y, b = blockIdx.z;
  const int dim = n_head * D;
  const int tq = blockIdx.x * ATT_QT + threadIdx.x;
  const bool live = tq < T;
  const float* base = qkv + (long long)b * 3 * dim * T;
  const float* qp = base + (long long)(h * D) * T;
  const float* kp = base + (long long)(dim + h * D) * T;
  const float* vp = base + (long long)(2 * dim + h * D) * T;
  float q[D], acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) q[d] = live ? qp[(long long)d * T + tq] : 0.f, acc[d] = 0.f;
  if (live) norm_rope<D>(q, rope + (long long)tq * D);
  const float scale = 1.0f / sqrtf((float)D);
  float m = -INFINITY, l = 0.f;
  const int qmax = min(blockIdx.x * ATT_QT + ATT_QT - 1, T - 1);
  const int kend = causal ? qmax + 1 : T;
  for (int k0 = 0; k0 < kend; k0 += ATT_KT) {
    __syncthreads();
    {
      const int j = threadIdx.x & (ATT_KT - 1), tk = k0 + j;
      float r[D];
      if (threadIdx.x < ATT_KT) {
#pragma unroll
        for (int d = 0; d < D; ++d) r[d] = tk < T ? kp[(long long)d * T + tk] : 0.f;
        if (tk < T) norm_rope<D>(r, rope + (long long)tk * D);
#pragma unroll
        for (int d = 0; d < D; ++d) ks[j * P + d] = r[d];
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) vs[j * P + d] = tk < T ? vp[(long long)d * T + tk] : 0.f;
      }
    }
    __syncthreads();
    const int jn = min(ATT_KT, kend - k0);
    for (int j = 0; j < jn; ++j) {
      if (causal && k0 + j > tq) break;
      const floatx4* kr = reinterpret_cast<const floatx4*>(ks + j * P);
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const floatx4 kv = kr[d4];
        s0 = fmaf(q[4 * d4], kv.x, s0);
        s1 = fmaf(q[4 * d4 + 1], kv.y, s1);
        s2 = fmaf(q[4 * d4 + 2], kv.z, s2);
        s3 = fmaf(q[4 * d4 + 3], kv.w, s3);
      }
      const float s = ((s0 + s1) + (s2 + s3)) * scale;
      if (s > m) {  // a new running maximum: rescale what has been summed
        const float r = expf(m - s);  // (m = -inf: exp(-inf) = 0)
        l *= r;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] *= r;
        m = s;
      }
      const float p = expf(s - m);
      l += p;
      const floatx4* vr = reinterpret_cast<const floatx4*>(vs + j * P);
#pragma unroll
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const floatx4 vv = vr[d4];
        acc[4 * d4] = fmaf(p, vv.x, acc[4 * d4]);
        acc[4 * d4 + 1] = fmaf(p, vv.y, acc[4 * d4 + 1]);
        acc[4 * d4 + 2] = fmaf(p, vv.z, acc[4 * d4 + 2]);
        acc[4 * d4 + 3] = fmaf(p, vv.w, acc[4 * d4 + 3]);
      }
    }
  }
  if (!live) return;
  float* yp = y + ((long long)b * dim + h * D) * T;
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (BC_DOK(tq >= 0 && tq < T)) yp[(long long)d * T + tq] = acc[d] / l;
}

// ---- ISTFT head ----------------------------------------------------------------------------------------------------
// xp[b][c][f], c < n_fft + 2: rows [0, bins) log-magnitudes, rows [bins, 2 bins) phases.  S = min(exp(.), 100) *
// (cos p, sin p).  basis[c][n], c < 2 bins: the windowed inverse real DFT (backward norm; the imaginary rows of DC and
// Nyquist are zero), so frame f contributes sum_c basis[c][n] S[c][f] to sample u = f * hop + n of the overlap-add.
// y[b][j] = ola[j + pad] / env[j + pad], env the sum of window[n]^2 over the frames that overlap the sample.
// One workgroup: one hop of overlap-add samples (u in [h * hop, (h + 1) * hop)) of ISTFT_NB clips; the spectra of the
// frames that reach it sit in LDS as s[slot][c][clip].
constexpr int ISTFT_NB = 2;

__global__ void __launch_bounds__(256) istft_head_kernel(const float* __restrict__ xp, const float* __restrict__ basis,
                                                         const float* __restrict__ window, float* __restrict__ y, int B,
                                                         int F, int n_fft, int hop, int pad, int nslots,
                                                         long long Tout) {
  extern __shared__ float istft_s[];
  const int bins = n_fft / 2 + 1, C2 = 2 * bins;
  const int h = blockIdx.x, b0 = blockIdx.y * ISTFT_NB;
  for (int e = threadIdx.x; e < nslots * bins * ISTFT_NB; e += 256) {
    const int bi = e % ISTFT_NB, k = (e / ISTFT_NB) % bins, r = e / (ISTFT_NB * bins);
    const int f = h - r, b = b0 + bi;
    float re = 0.f, im = 0.f;
    if (f >= 0 && f < F && b < B) {
      const float* col = xp + (long long)b * C2 * F + f;
      const float mag = fminf(expf(col[(long long)k * F]), 100.0f);
      const float p = col[(long long)(bins + k) * F];
      re = mag * bc_cos(p);
      im = mag * bc_sin(p);
    }
    istft_s[(r * C2 + k) * ISTFT_NB + bi] = re;
    istft_s[(r * C2 + bins + k) * ISTFT_NB + bi] = im;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < hop; i += 256) {
    const long long u = (long long)h * hop + i, j = u - pad;
    if (j < 0 || j >= Tout) continue;
    double acc[ISTFT_NB];
    float env = 0.f;
#pragma unroll
    for (int bi = 0; bi < ISTFT_NB; ++bi) acc[bi] = 0.0;
    for (int r = 0; r < nslots; ++r) {
      const int f = h - r, n = i + r * hop;
      if (f < 0 || f >= F || n >= n_fft) continue;
      const float wn = window[n];
      env = fmaf(wn, wn, env);
      const float* sr = istft_s + (long long)r * C2 * ISTFT_NB;
      for (int c0 = 0; c0 < C2; c0 += ACC_CHUNK) {
        const int c1 = min(c0 + ACC_CHUNK, C2);
        float part[ISTFT_NB];
#pragma unroll
        for (int bi = 0; bi < ISTFT_NB; ++bi) part[bi] = 0.f;
        for (int c = c0; c < c1; ++c) {
          const float bv = basis[(long long)c * n_fft + n];
#pragma unroll
          for (int bi = 0; bi < ISTFT_NB; ++bi) part[bi] = fmaf(bv, sr[c * ISTFT_NB + bi], part[bi]);
        }
#pragma unroll
        for (int bi = 0; bi < ISTFT_NB; ++bi) acc[bi] += (double)part[bi];
      }
    }
#pragma unroll
    for (int bi = 0; bi < ISTFT_NB; ++bi)
      if (b0 + bi < B && BC_DOK(j >= 0 && j < Tout)) y[(long long)(b0 + bi) * Tout + j] = (float)acc[bi] / env;
  }
}

}  // namespace bc

using namespace bc;
static inline hipStream_t CS(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

int bc_stft_frames(const float* x, const float* basisT, float* y, int B, long long T, int n_fft, int hop, int win,
                   void* stream) {
  if (!x || !basisT || !y || B < 1 || T < 1 || n_fft < 2 || hop < 1 || win < hop) return BC_ERR_ARG;
  if (win != n_fft || (n_fft & 1)) return BC_ERR_UNSUPPORTED;
  const int pad = (win - hop) / 2;
  const long long Fl = (T + 2 * pad - n_fft) / hop + 1;
  if (T + 2 * pad < n_fft || Fl < 1) return BC_ERR_ARG;
  const size_t lds = (size_t)((STFT_FT - 1) * (long long)hop + n_fft) * sizeof(float);
  if (Fl > 0x7fffffffLL / hop || B > 65535 || lds > 64 * 1024) return BC_ERR_UNSUPPORTED;
  const int F = (int)Fl, C2 = n_fft + 2;
  hipLaunchKernelGGL(stft_frames_kernel, dim3((F + STFT_FT - 1) / STFT_FT, (C2 + 255) / 256, B), dim3(256), lds,
                     CS(stream), x, basisT, y, T, n_fft, hop, pad, F, C2);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int bc_rmsnorm_fwd(const float* x, const float* w, float* y, int B, int C, int T, float eps, int silu, void* stream) {
  if (!x || !y || B < 1 || C < 1 || T < 1) return BC_ERR_ARG;
  const long long rows = (long long)B * T;
  if (rows > 0x7fffffffLL * 256 || (rows + 255) / 256 > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rmsnorm_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, CS(stream), x, w, y, C, T, eps,
                     silu, rows);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int bc_dwconv_glu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int T, int K,
                      int pad_left, void* stream) {
  if (!x || !w || !y || B < 1 || C < 1 || T < 1 || K < 1 || pad_left < 0 || pad_left >= K) return BC_ERR_ARG;
  if (K > DW_MAXK) return BC_ERR_UNSUPPORTED;
  const int ntiles = (T + DW_TILE - 1) / DW_TILE;
  const long long nwg = (long long)B * C * ntiles;
  if (nwg > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dwconv_glu_kernel, dim3((unsigned)nwg), dim3(256), 0, CS(stream), x, w, bias, y, C, T, K, pad_left,
                     ntiles);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int bc_swiglu_fwd(const float* h, float* y, int B, int H, long long T, void* stream) {
  if (!h || !y || B < 1 || H < 1 || T < 1) return BC_ERR_ARG;
  const long long HT = (long long)H * T, total = HT * B;
  const long long g = std::min<long long>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)g), dim3(256), 0, CS(stream), h, y, HT, total);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int bc_attention_tiles(int* q_tile, int* kv_tile) {
  if (q_tile) *q_tile = ATT_QT;
  if (kv_tile) *kv_tile = ATT_KT;
  return BC_OK;
}

int bc_attention_fwd(const float* qkv, const float* rope, float* y, int B, int n_head, int head_dim, int T, int causal,
                     void* stream) {
  if (!qkv || !rope || !y || B < 1 || n_head < 1 || T < 1) return BC_ERR_ARG;
  if ((head_dim != 32 && head_dim != 64) || B > 65535 || n_head > 65535) return BC_ERR_UNSUPPORTED;
  const dim3 grid((T + ATT_QT - 1) / ATT_QT, n_head, B);
  if (head_dim == 32)
    hipLaunchKernelGGL(attention_kernel<32>, grid, dim3(ATT_QT), 0, CS(stream), qkv, rope, y, n_head, T, causal);
  else
    hipLaunchKernelGGL(attention_kernel<64>, grid, dim3(ATT_QT), 0, CS(stream), qkv, rope, y, n_head, T, causal);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int bc_istft_head(const float* xp, const float* basis, const float* window, float* y, int B, int F, int n_fft, int hop,
                  void* stream) {
  if (!xp || !basis || !window || !y || B < 1 || F < 1 || n_fft < 2 || hop < 1 || hop > n_fft) return BC_ERR_ARG;
  if (n_fft & 1) return BC_ERR_UNSUPPORTED;
  const int pad = (n_fft - hop) / 2, nslots = (n_fft + hop - 1) / hop;
  const long long Tout = (long long)(F - 1) * hop + n_fft - 2 * pad;
  const size_t lds = (size_t)nslots * (n_fft + 2) * ISTFT_NB * sizeof(float);
  if (lds > 64 * 1024 || (long long)F + nslots > 0x7fffffffLL / hop || B > 65535 * ISTFT_NB) return BC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(istft_head_kernel, dim3(F + nslots - 1, (B + ISTFT_NB - 1) / ISTFT_NB), dim3(256), lds, CS(stream),
                     xp, basis, window, y, B, F, n_fft, hop, pad, nslots, Tout);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

}  // extern "C"

BC_DEBUG_EXPORT(conformer)
