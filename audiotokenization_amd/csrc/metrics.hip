// Round-trip quality metrics of a batch of (reference, reconstruction) waveform pairs, computed where the
// waveforms already are (added under ABI 18).
//
//  si_snr_kernel    : scale-invariant SNR per clip (torchmetrics' ScaleInvariantSignalNoiseRatio written out, as
//                     inference_full.py:723 feeds it), three passes over the clip's own samples with fp64
//                     accumulators: the means, then alpha, then the residual energy itself (never the expanded
//                     square, which cancels to nothing at 60-80 dB).
//  logmel_l1_kernel : one resolution of criterions/mel_loss.py's multi-resolution log-mel L1 distance.  One
//                     workgroup owns MEL_TILE_FRAMES frames of one clip: the frame columns are read straight from
//                     the waveform staged in LDS (implicit im2col, reflect padding by index at the clip's OWN two
//                     ends), windowed DFT basis x frames on v_mfma_f32_16x16x4_f32 for both signals against the same
//                     basis fragments, magnitudes in registers, mel matrix x magnitudes on the same MFMA through a
//                     64-bin LDS slab, then clamp, log10, |difference| and one fp64 partial per workgroup.  No
//                     spectrogram reaches HBM.  logmel_finish_kernel sums each clip's partials in a fixed order.
//  code_hist_kernel : codebook usage counts, an LDS-privatised histogram flushed with vector atomics.
//
// Per-clip results come from per-clip work in a fixed order: a clip in a batch gets bit for bit what it gets alone,
// and samples at or beyond a clip's own length are never read (the ragged rule of DESIGN.md §15).
#include <algorithm>
#include <limits>
#include "bc_common.h"
#include "bc_internal.h"

namespace bc {

// Sum over the workgroup in a fixed tree (NT a power of two); every thread gets the result.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- SI-SNR ---------------------------------------------------------------------------------------------------
// One workgroup per clip, so the summation order is the clip's own whatever the batch.  t = ref, p = rec:
//   t' = t - mean(t), p' = p - mean(p), alpha = (sum p't' + eps) / (sum t't' + eps), s = alpha t',
//   out = 10 log10((sum s^2 + eps) / (sum (s - p')^2 + eps)),  eps = 2^-23 (float32's, as torchmetrics takes it).
constexpr int SNR_THREADS = 1024;

__global__ void __launch_bounds__(SNR_THREADS) si_snr_kernel(const float* __restrict__ ref,
                                                             const float* __restrict__ rec,
                                                             const int* __restrict__ lens, float* __restrict__ out,
                                                             long long T, long long total) {
  __shared__ double red[SNR_THREADS];
  const int b = blockIdx.x;
  long long n = lens ? (long long)lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  if (n == 0) {  // (uniform) no samples: no value
    if (threadIdx.x == 0) out[b] = std::numeric_limits<float>::quiet_NaN();
    return;
  }
  const long long base = (long long)b * T;
  const float* t = ref + base;
  const float* p = rec + base;
  const double eps = 1.1920928955078125e-07;
  double st = 0.0, sp = 0.0;
  for (long long i = threadIdx.x; i < n; i += SNR_THREADS) {
    if (!BC_DOK(base + i < total)) break;
    st += (double)t[i];
    sp += (double)p[i];
  }
  const double mt = block_sum<SNR_THREADS>(st, red) / (double)n;
  const double mp = block_sum<SNR_THREADS>(sp, red) / (double)n;
  double dot = 0.0, ett = 0.0;
  for (long long i = threadIdx.x; i < n; i += SNR_THREADS) {
    if (!BC_DOK(base + i < total)) break;
    const double tz = (double)t[i] - mt, pz = (double)p[i] - mp;
    dot += tz * pz;
    ett += tz * tz;
  }
  dot = block_sum<SNR_THREADS>(dot, red);
  ett = block_sum<SNR_THREADS>(ett, red);
  const double alpha = (dot + eps) / (ett + eps);
  double es = 0.0, en = 0.0;
  for (long long i = threadIdx.x; i < n; i += SNR_THREADS) {
    if (!BC_DOK(base + i < total)) break;
    const double s = alpha * ((double)t[i] - mt), r = s - ((double)p[i] - mp);
    es += s * s;
    en += r * r;
  }
  es = block_sum<SNR_THREADS>(es, red);
  en = block_sum<SNR_THREADS>(en, red);
  if (threadIdx.x == 0) out[b] = (float)(10.0 * log10((es + eps) / (en + eps)));
}

int si_snr_launch(const float* ref, const float* rec, const int* lens, float* out, int B, long long T, hipStream_t st) {
  if (!ref || !rec || !out || B <= 0 || T <= 0) return BC_ERR_ARG;
  if (T > (1LL << 62) / B) return BC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(si_snr_kernel, dim3(B), dim3(SNR_THREADS), 0, st, ref, rec, lens, out, T, (long long)B * T);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// ---- log-mel L1 distance, one resolution ------------------------------------------------------------------------
// Frame f of a clip of len samples is x[reflect(f hop + k - n_fft / 2)], k < n_fft (torch.stft center=True,
// pad_mode="reflect"), frames = 1 + len / hop, hop = n_fft / 4.  A tile of MEL_TILE_FRAMES frames spans
// (MEL_TILE_FRAMES + 3) hop samples, staged once per signal with four floats of padding after every hop samples:
// lane (frame n, k-group kk) of an MFMA B operand then reads the 16 bytes at n (hop + 4) + k + 4 (k / hop), which
// for the 64 lanes of one k-block are 64 distinct 16-byte groups spread over the banks.
//
// DFT GEMM: A = basis rows (re: bin, im: bins + bin), B = frames, K = n_fft in k-blocks of 16.  The order of k inside
// an MFMA is free as long as A and B agree, so lane (row, kk) takes the four CONSECUTIVE k = 16 kb + 4 kk + i as one
// 16-byte load of each operand and MFMA i of the k-block multiplies the k = 16 kb + 4 kk + i of the four kk.  Each
// wave owns a 16-bin tile per round, with re / im x ref / rec as four independent accumulators.  64 k are accumulated
// in fresh registers and added to a (hi, lo) pair with an error-free TwoSum, so the rounding of a 2048-term sum
// is that of 64-term sums (the fp32 MFMA is an fmaf chain: products are exact).
// Mel GEMM: the accumulator layout (row = 4 (lane >> 4) + reg, col = lane & 15) of a 16-bin magnitude tile is
// written to a [64 bins][ref 16 | rec 16 | pad 16] LDS slab per round (four waves' tiles); wave w then multiplies
// mel tiles w, w + 4, ... (16 mel rows each, at most MEL_MAX_MT per wave) by the slab.
constexpr int MEL_TILE_FRAMES = 16;
constexpr int MEL_THREADS = 256;
constexpr int MEL_MAG_PITCH = 48;
constexpr int MEL_MAX_MT = 5;             // mel tiles per wave: n_mels <= 4 * 5 * 16 = 320
constexpr int MEL_SPAN_HOPS = MEL_TILE_FRAMES + 3;
constexpr int MEL_MAX_LDS = 160 * 1024;

__device__ __forceinline__ void two_sum_add(floatx4& hi, floatx4& lo, const floatx4 a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float s = hi[i] + a[i];
    const float bb = s - hi[i];
    lo[i] += (hi[i] - (s - bb)) + (a[i] - bb);
    hi[i] = s;
  }
}

__global__ void __launch_bounds__(MEL_THREADS) logmel_l1_kernel(const float* __restrict__ ref,
                                                                const float* __restrict__ rec,
                                                                const int* __restrict__ lens,
                                                                const float* __restrict__ basis,
                                                                const float* __restrict__ melw,
                                                                double* __restrict__ partial, long long T, int n_fft,
                                                                int n_mels, float clamp_eps, long long total) {
  extern __shared__ __attribute__((aligned(16))) float mel_sm[];
  __shared__ double red[MEL_THREADS];
  const int hop = n_fft / 4, bins = n_fft / 2 + 1, pitch = hop + 4, span = MEL_SPAN_HOPS * pitch;
  float* xs_ref = mel_sm;
  float* xs_rec = mel_sm + span;
  float* mag = mel_sm + 2 * span;
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  long long len = lens ? (long long)lens[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const long long frames = 1 + len / hop;
  const long long f0 = (long long)tile * MEL_TILE_FRAMES;
  double* slot = partial + (long long)b * gridDim.x + tile;
  if (len < n_fft / 2 + 1) {  // (uniform) reflect padding is undefined: the clip's result is NaN, nothing is read
    if (tid == 0) *slot = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  if (f0 >= frames) {  // (uniform) a tile past the clip's last frame
    if (tid == 0) *slot = 0.0;
    return;
  }
  // the tile's samples, reflected at the clip's own ends; what only frames >= `frames` would read is zero
  const long long s0 = f0 * hop - n_fft / 2, base = (long long)b * T;
  for (int j = tid; j < MEL_SPAN_HOPS * hop; j += MEL_THREADS) {
    long long s = s0 + j;
    if (s < 0) s = -s;
    if (s >= len) s = 2 * (len - 1) - s;
    float vr = 0.f, vc = 0.f;
    if (s >= 0 && s < len && BC_DOK(base + s < total)) {
      vr = ref[base + s];
      vc = rec[base + s];
    }
    const int pos = j + 4 * (j / hop);
    xs_ref[pos] = vr;
    xs_rec[pos] = vc;
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int nbt = (bins + 15) / 16, rounds = (nbt + 3) / 4, nmt = (n_mels + 15) / 16, nkb = n_fft / 16;
  const long long basis_floats = 2LL * bins * n_fft, mel_floats = (long long)n_mels * bins;
  floatx4 macc[MEL_MAX_MT][2];
#pragma unroll
  for (int t = 0; t < MEL_MAX_MT; ++t) macc[t][0] = macc[t][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float* bref = xs_ref + n * pitch;
  const float* brec = xs_rec + n * pitch;

  for (int r = 0; r < rounds; ++r) {
    const int bt = r * 4 + wave;
    floatx4 hi[4], lo[4];  // re x ref, re x rec, im x ref, im x rec
#pragma unroll
    for (int q = 0; q < 4; ++q) hi[q] = lo[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (bt < nbt) {  // (wave-uniform)
      const int row = bt * 16 + n;
      const bool rowok = row < bins;
      const long long ore = (long long)row * n_fft + 4 * kk, oim = (long long)(bins + row) * n_fft + 4 * kk;
      for (int kb0 = 0; kb0 < nkb; kb0 += 4) {
        floatx4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
        const int kb1 = kb0 + 4 < nkb ? kb0 + 4 : nkb;
        for (int kb = kb0; kb < kb1; ++kb) {
          floatx4 are = floatx4{0.f, 0.f, 0.f, 0.f}, aim = are;
          if (rowok && BC_DOK(oim + 16 * kb + 3 < basis_floats)) {
            are = *reinterpret_cast<const floatx4*>(basis + ore + 16 * kb);
            aim = *reinterpret_cast<const floatx4*>(basis + oim + 16 * kb);
          }
          const int k = 16 * kb + 4 * kk;
          const int pos = k + 4 * (k / hop);
          const floatx4 xr = *reinterpret_cast<const floatx4*>(bref + pos);
          const floatx4 xc = *reinterpret_cast<const floatx4*>(brec + pos);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[i], xr[i], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[i], xc[i], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[i], xr[i], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[i], xc[i], acc[3], 0, 0, 0);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) two_sum_add(hi[q], lo[q], acc[q]);
      }
    }
    // magnitudes of this wave's 16 bins x 16 frames x 2 signals -> the slab (zeros for a tile past the last bin)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float rr = hi[0][i] + lo[0][i], rc = hi[1][i] + lo[1][i];
      const float ir = hi[2][i] + lo[2][i], ic = hi[3][i] + lo[3][i];
      float* m = mag + (wave * 16 + kk * 4 + i) * MEL_MAG_PITCH + n;
      m[0] = sqrtf(rr * rr + ir * ir);
      m[16] = sqrtf(rc * rc + ic * ic);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MEL_MAX_MT; ++t) {
      const int mt = wave + 4 * t;
      if (mt < nmt) {  // (wave-uniform)
        const int mrow = mt * 16 + n;
        const long long om = (long long)mrow * bins;
        for (int ks = 0; ks < 16; ++ks) {
          const int bl = ks * 4 + kk, bin = r * 64 + bl;
          float a = 0.f;
          if (mrow < n_mels && bin < bins && BC_DOK(om + bin < mel_floats)) a = melw[om + bin];
          const float xr = mag[bl * MEL_MAG_PITCH + n], xc = mag[bl * MEL_MAG_PITCH + 16 + n];
          macc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr, macc[t][0], 0, 0, 0);
          macc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xc, macc[t][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // |log10 max(mel_ref, eps) - log10 max(mel_rec, eps)| over the tile's valid (mel, frame) cells
  double sum = 0.0;
  const bool fok = f0 + n < frames;
#pragma unroll
  for (int t = 0; t < MEL_MAX_MT; ++t) {
    const int mt = wave + 4 * t;
    if (mt < nmt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mel = mt * 16 + kk * 4 + i;
        if (fok && mel < n_mels)
          sum += (double)fabsf(log10f(fmaxf(macc[t][0][i], clamp_eps)) - log10f(fmaxf(macc[t][1][i], clamp_eps)));
      }
    }
  }
  sum = block_sum<MEL_THREADS>(sum, red);
  if (tid == 0) *slot = sum;
}

// Each clip's partials in a fixed order (a tile past the clip's frames holds 0.0, which changes no sum), over
// n_mels x frames cells.
__global__ void __launch_bounds__(MEL_THREADS) logmel_finish_kernel(const double* __restrict__ partial,
                                                                    const int* __restrict__ lens,
                                                                    float* __restrict__ out, long long T, int hop,
                                                                    int n_mels, int tiles) {
  __shared__ double red[MEL_THREADS];
  const int b = blockIdx.x;
  long long len = lens ? (long long)lens[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  double s = 0.0;
  for (int i = threadIdx.x; i < tiles; i += MEL_THREADS) s += partial[(long long)b * tiles + i];
  s = block_sum<MEL_THREADS>(s, red);
  if (threadIdx.x == 0) out[b] = (float)(s / ((double)n_mels * (double)(1 + len / hop)));
}

int logmel_tile_frames() { return MEL_TILE_FRAMES; }

static long long logmel_tiles(long long T, int n_fft) {
  const long long frames = 1 + T / (n_fft / 4);
  return (frames + MEL_TILE_FRAMES - 1) / MEL_TILE_FRAMES;
}

long long logmel_workspace_doubles(int B, long long T, int n_fft) {
  if (B <= 0 || T <= 0 || n_fft < 16 || n_fft % 16) return -1;
  const long long tiles = logmel_tiles(T, n_fft);
  if (tiles > 0x7fffffffLL || tiles > (1LL << 40) / B) return -1;
  return tiles * B;
}

int logmel_l1_launch(const float* ref, const float* rec, const int* lens, const float* basis, const float* melw,
                     float* out, double* ws, int B, long long T, int n_fft, int n_mels, float clamp_eps,
                     hipStream_t st) {
  if (!ref || !rec || !basis || !melw || !out || !ws || B <= 0 || T <= 0 || n_mels <= 0) return BC_ERR_ARG;
  if (n_fft < 16 || n_fft % 16 || !(clamp_eps > 0.f)) return BC_ERR_ARG;
  if (((unsigned long long)basis & 15) != 0) return BC_ERR_ARG;  // 16-byte basis loads
  if (n_mels > 4 * MEL_MAX_MT * 16 || B > 65535) return BC_ERR_UNSUPPORTED;
  const long long nws = logmel_workspace_doubles(B, T, n_fft);
  if (nws < 0 || T > (1LL << 62) / B) return BC_ERR_UNSUPPORTED;
  const int hop = n_fft / 4, tiles = (int)(nws / B);
  const size_t lds = sizeof(float) * (2 * (size_t)MEL_SPAN_HOPS * (hop + 4) + 64 * MEL_MAG_PITCH);
  if (lds + sizeof(double) * MEL_THREADS > (size_t)MEL_MAX_LDS) return BC_ERR_UNSUPPORTED;
  if (lds > 64 * 1024) {  // (more dynamic LDS than the default limit: allowed up to the CU's 160 KiB)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(logmel_l1_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipGetLastError();
  }
  hipLaunchKernelGGL(logmel_l1_kernel, dim3(tiles, B), dim3(MEL_THREADS), lds, st, ref, rec, lens, basis, melw, ws, T,
                     n_fft, n_mels, clamp_eps, (long long)B * T);
  BC_CHECK_LAUNCH();
  hipLaunchKernelGGL(logmel_finish_kernel, dim3(B), dim3(MEL_THREADS), 0, st, ws, lens, out, T, hop, n_mels, tiles);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// ---- codebook usage ---------------------------------------------------------------------------------------------
// counts[c] += the number of codes[b][t] == c with t < lens[b] (every t when lens is null); codes outside
// [0, n_codes) are ignored (inference_full.py:589).  Each workgroup counts into its own LDS histogram and adds the
// non-zero bins to the device counter once.
constexpr int HIST_THREADS = 256;

template <typename IT>
__global__ void __launch_bounds__(HIST_THREADS) code_hist_kernel(const IT* __restrict__ codes,
                                                                 const int* __restrict__ lens,
                                                                 unsigned long long* __restrict__ counts, long long T,
                                                                 long long total, int n_codes) {
  extern __shared__ unsigned int hist_sm[];
  for (int i = threadIdx.x; i < n_codes; i += HIST_THREADS) hist_sm[i] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * HIST_THREADS + threadIdx.x; i < total;
       i += (long long)gridDim.x * HIST_THREADS) {
    const long long b = i / T;
    if (lens && i - b * T >= (long long)lens[b]) continue;
    const long long c = (long long)codes[i];
    if (c < 0 || c >= n_codes) continue;
    atomicAdd(&hist_sm[c], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_codes; i += HIST_THREADS) {
    const unsigned int v = hist_sm[i];
    if (v && BC_DOK(i >= 0 && i < n_codes)) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

int code_hist_launch(const void* codes, int code_bits, const int* lens, long long* counts, int B, long long T,
                     int n_codes, hipStream_t st) {
  if (!codes || !counts || B <= 0 || T <= 0 || n_codes <= 0 || (code_bits != 32 && code_bits != 64)) return BC_ERR_ARG;
  if ((size_t)n_codes * sizeof(unsigned int) > 64 * 1024 || T > (1LL << 38) / B) return BC_ERR_UNSUPPORTED;
  const long long total = (long long)B * T;
  // (a workgroup's LDS bins are 32-bit: with total <= 2^38 a full grid's workgroup sees at most 2^30 codes)
  const int grid = (int)std::min<long long>((total + 4 * HIST_THREADS - 1) / (4 * HIST_THREADS), 256);
  const size_t lds = (size_t)n_codes * sizeof(unsigned int);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (code_bits == 64)
    hipLaunchKernelGGL(code_hist_kernel<long long>, dim3(grid), dim3(HIST_THREADS), lds, st,
                       static_cast<const long long*>(codes), lens, cnt, T, total, n_codes);
  else
    hipLaunchKernelGGL(code_hist_kernel<int>, dim3(grid), dim3(HIST_THREADS), lds, st, static_cast<const int*>(codes),
                       lens, cnt, T, total, n_codes);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

}  // namespace bc

BC_DEBUG_EXPORT(metrics)
