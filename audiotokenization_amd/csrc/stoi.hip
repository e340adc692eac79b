// STOI (Taal et al. 2011, the non-extended measure as the pystoi package computes it) of a batch of (clean, processed)
// waveform pairs, computed where the waveforms already are (additive under ABI 18).  The definition
// this file is held to is tests/stoi_ref.py.
//
//  stoi_resample_kernel : both signals to 10 kHz, y[n] = sum_m x[m] h[q n - p m + L] (scipy's resample_poly with the
//                         Octave-style Kaiser filter the host builds), fp64 accumulation in a fixed order.  Not
//                         launched at 10 kHz.
//  stoi_energy_kernel   : the windowed energy of every 256-sample frame (hop 128) of the clean signal, 256 terms in
//                         fp64, one wave per frame.
//  stoi_mask_kernel     : one workgroup per clip: the loudest frame, the 40 dB threshold, an exclusive scan of the
//                         kept flags -> src[b][k], the original index of kept frame k, and kept[b].
//  stoi_tob_kernel      : one workgroup owns 16 STFT frames of one clip.  The silence-removed signal is never written:
//                         its samples are gathered through src from the 10 kHz samples (overlap-add of the two kept
//                         windowed frames that cover each hop) into LDS for both signals, windowed DFT basis (bins
//                         7 .. 230) x frames on v_mfma_f32_16x16x4_f32 against the same basis fragments, |X|^2 from
//                         the accumulators through an LDS slab, the 15 third-octave band sums, sqrt ->
//                         band[2][B][15][frames].  No spectrogram reaches HBM.
//  stoi_corr_kernel     : one workgroup per clip: per (30-frame segment, band) scale, clip, centre, normalise and
//                         correlate in fp64, summed in a fixed order.
//
// Per-clip results come from per-clip work in a fixed order: a clip in a batch gets bit for bit what it gets alone,
// and samples at or beyond a clip's own length are never read (the ragged rule of DESIGN.md §15).
#include <limits>
#include "bc_common.h"
#include "bc_internal.h"

namespace bc {

constexpr int STOI_FRAME = 256;
constexpr int STOI_HOP = 128;
constexpr int STOI_BANDS = 15;
constexpr int STOI_SEG = 30;
constexpr int STOI_BIN0 = 7;      // the basis holds bins 7 .. 230: 14 tiles of 16
constexpr int STOI_ROWS = 224;
constexpr int STOI_TILE = 16;     // STFT frames per workgroup
constexpr int STOI_THREADS = 256;
constexpr int STOI_PITCH = STOI_HOP + 4;
constexpr int STOI_SPAN_HOPS = STOI_TILE + 1;
constexpr int STOI_PW_PITCH = 33;
constexpr int STOI_MAX_TAPS = 4096;
constexpr int STOI_MAX_RATIO = 64;
constexpr double STOI_EPS = 2.220446049250313e-16;  // float64's epsilon, as the definition adds it
constexpr double STOI_TWO_PI = 6.283185307179586476925287;

// band i sums the bins [stoi_band_edge[i], stoi_band_edge[i + 1]) (fs 10000, n = 512: tests/stoi_ref.py BANDS)
__constant__ int stoi_band_edge[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ __forceinline__ long long stoi_len10(long long len, int up, int down) {
  return (len * up + down - 1) / down;
}
__host__ __device__ __forceinline__ long long stoi_frames(long long n10) {
  return n10 >= STOI_FRAME ? (n10 - STOI_FRAME) / STOI_HOP + 1 : 0;
}
__device__ __forceinline__ long long stoi_clip_len(const int* lens, int b, long long T) {
  const long long len = lens ? (long long)lens[b] : T;
  return len < 0 ? 0 : (len > T ? T : len);
}
// w[n] of the 256-point Hann window without its zero end points (np.hanning(258)[1:-1])
__device__ __forceinline__ double stoi_window(int n) {
  return 0.5 - 0.5 * cos(STOI_TWO_PI * (double)(n + 1) / (double)(STOI_FRAME + 1));
}

// Sum over the workgroup in a fixed tree; every thread gets the result.
__device__ __forceinline__ double stoi_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = STOI_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- resampling to 10 kHz ---------------------------------------------------------------------------------------
// Output n of a clip of len samples, n < ceil(len up / down): the taps j = down n + L - up m in [0, 2 L], m in
// [0, len).  blockIdx.z selects the signal; the filter is staged in LDS.
__global__ void __launch_bounds__(STOI_THREADS) stoi_resample_kernel(const float* __restrict__ clean,
                                                                     const float* __restrict__ proc,
                                                                     const int* __restrict__ lens,
                                                                     const float* __restrict__ filt,
                                                                     float* __restrict__ x10, long long T,
                                                                     long long T10, int up, int down, int half_len,
                                                                     long long total, long long total10) {
  extern __shared__ float stoi_filt_sm[];
  const int b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x, taps = 2 * half_len + 1;
  const long long len = stoi_clip_len(lens, b, T), n10 = stoi_len10(len, up, down);
  const long long n0 = (long long)blockIdx.x * STOI_THREADS;
  if (n0 >= n10) return;  // (uniform) a block past the clip's last output
  for (int j = tid; j < taps; j += STOI_THREADS) stoi_filt_sm[j] = filt[j];
  __syncthreads();
  const long long n = n0 + tid;
  if (n >= n10) return;
  const long long base = (long long)b * T;
  const float* x = (sig ? proc : clean) + base;
  const long long c = (long long)down * n + half_len, lo = c - 2LL * half_len;
  const long long m_lo = lo <= 0 ? 0 : (lo + up - 1) / up;
  long long m_hi = c / up;
  if (m_hi > len - 1) m_hi = len - 1;
  double acc = 0.0;
  for (long long m = m_lo; m <= m_hi; ++m) {
    const long long j = c - (long long)up * m;
    if (!BC_DOK(j >= 0 && j < taps && base + m < total)) break;
    acc += (double)x[m] * (double)stoi_filt_sm[j];
  }
  const long long dst = ((long long)sig * gridDim.y + b) * T10 + n;
  if (BC_DOK(dst < total10)) x10[dst] = (float)acc;
}

// ---- frame energies of the clean signal ---------------------------------------------------------------------------
// energy[b][f] = sum_n (w[n] x[128 f + n])^2, n < 256, in fp64: wave w of a workgroup owns frame 4 blockIdx.x + w.
__global__ void __launch_bounds__(STOI_THREADS) stoi_energy_kernel(const float* __restrict__ xc, long long pitch,
                                                                   const int* __restrict__ lens,
                                                                   double* __restrict__ energy, long long T,
                                                                   long long F, int up, int down, long long total) {
  __shared__ double red[STOI_THREADS];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long frames = stoi_frames(stoi_len10(stoi_clip_len(lens, b, T), up, down));
  const long long f = (long long)blockIdx.x * 4 + wave;
  double s = 0.0;
  if (f < frames) {  // (wave-uniform)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = lane + 64 * i;
      const long long idx = (long long)b * pitch + STOI_HOP * f + n;
      if (BC_DOK(idx < total)) {
        const double v = stoi_window(n) * (double)xc[idx];
        s += v * v;
      }
    }
  }
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) {
    if (lane < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (lane == 0 && f < frames && BC_DOK(f < F)) energy[(long long)b * F + f] = red[tid];
}

// ---- silent-frame mask --------------------------------------------------------------------------------------------
// e = 20 log10(sqrt(energy) + eps); frame f is kept when (max e - 40) - e < 0.  Thread t owns the contiguous frames
// [t chunk, (t + 1) chunk): counts, a serial exclusive scan of the 256 counts, then the kept frames' indices.
__device__ __forceinline__ double stoi_db(double energy) { return 20.0 * log10(sqrt(energy) + STOI_EPS); }

__global__ void __launch_bounds__(STOI_THREADS) stoi_mask_kernel(const double* __restrict__ energy,
                                                                 const int* __restrict__ lens, int* __restrict__ src,
                                                                 int* __restrict__ kept, long long T, long long F,
                                                                 int up, int down) {
  __shared__ double red[STOI_THREADS];
  __shared__ int cnt[STOI_THREADS + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long frames = stoi_frames(stoi_len10(stoi_clip_len(lens, b, T), up, down));
  if (frames == 0) {  // (uniform) no whole frame: nothing is kept
    if (tid == 0) kept[b] = 0;
    return;
  }
  const double* e = energy + (long long)b * F;
  double mx = -std::numeric_limits<double>::infinity();
  for (long long f = tid; f < frames; f += STOI_THREADS) mx = fmax(mx, stoi_db(e[f]));
  red[tid] = mx;
  __syncthreads();
#pragma unroll
  for (int s = STOI_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double thr = red[0] - 40.0;
  const long long chunk = (frames + STOI_THREADS - 1) / STOI_THREADS;
  const long long f0 = tid * chunk, f1 = f0 + chunk < frames ? f0 + chunk : frames;
  int c = 0;
  for (long long f = f0; f < f1; ++f) c += (thr - stoi_db(e[f]) < 0.0) ? 1 : 0;
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < STOI_THREADS; ++i) {
      const int v = cnt[i];
      cnt[i] = run;
      run += v;
    }
    cnt[STOI_THREADS] = run;
  }
  __syncthreads();
  long long k = cnt[tid];
  for (long long f = f0; f < f1; ++f) {
    if (thr - stoi_db(e[f]) < 0.0) {
      if (BC_DOK(k < F)) src[(long long)b * F + k] = (int)f;
      ++k;
    }
  }
  if (tid == 0) kept[b] = cnt[STOI_THREADS];
}

// ---- third-octave band magnitudes -----------------------------------------------------------------------------------
// STFT frame k < kept - 1 of the silence-removed signal is its samples [128 k, 128 k + 256).  Hop g of that signal
// (samples [128 g, 128 g + 128), g < kept) is the overlap-add of the second half of kept frame g - 1 (g >= 1) and the
// first half of kept frame g, each windowed: w[n + 128] x[128 src[g - 1] + 128 + n] + w[n] x[128 src[g] + n].  A tile
// of 16 frames spans 17 hops, staged once per signal with four floats of padding after every hop: lane (frame n,
// k-group kk) of an MFMA B operand then reads the 16 bytes at n (128 + 4) + k + 4 (k / 128).
//
// DFT GEMM as in logmel_l1_kernel (metrics.hip): A = basis rows (re: row, im: 224 + row; the rows are w[n] cos and
// -w[n] sin of 2 pi (7 + row) n / 512, n < 256), B = frames, K = 256 in k-blocks of 16; lane (row, kk) takes the four
// consecutive k = 16 kb + 4 kk + i as one 16-byte load of each operand.  Wave w owns bin tiles w, w + 4, ... with
// re / im x clean / processed as four accumulators; 64 k are accumulated in fresh registers and added to a (hi, lo)
// pair with an error-free TwoSum.  The accumulator layout (row = 4 (lane >> 4) + reg, col = lane & 15) of |X|^2 goes
// to a [224 bins][clean 16 | processed 16 | pad] LDS slab; 480 threads' worth of (signal, band, frame) cells then sum
// their band's bins in ascending order.
__device__ __forceinline__ void stoi_two_sum_add(floatx4& hi, floatx4& lo, const floatx4 a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float s = hi[i] + a[i];
    const float bb = s - hi[i];
    lo[i] += (hi[i] - (s - bb)) + (a[i] - bb);
    hi[i] = s;
  }
}

__global__ void __launch_bounds__(STOI_THREADS) stoi_tob_kernel(const float* __restrict__ xc,
                                                                const float* __restrict__ xp, long long pitch,
                                                                const int* __restrict__ src,
                                                                const int* __restrict__ kept,
                                                                const float* __restrict__ basis,
                                                                float* __restrict__ band, long long F, long long total,
                                                                long long band_total) {
  __shared__ __attribute__((aligned(16))) float xs[2][STOI_SPAN_HOPS * STOI_PITCH];
  __shared__ float pw[STOI_ROWS * STOI_PW_PITCH];
  __shared__ float win[STOI_FRAME];
  const int b = blockIdx.y, tid = threadIdx.x, B = gridDim.y;
  const long long K = kept[b], S = K - 1, k0 = (long long)blockIdx.x * STOI_TILE;
  if (k0 >= S) return;  // (uniform) a tile past the clip's last STFT frame
  win[tid] = (float)stoi_window(tid);
  __syncthreads();
  const int* sb = src + (long long)b * F;
  const long long base = (long long)b * pitch;
  for (int j = tid; j < STOI_SPAN_HOPS * STOI_HOP; j += STOI_THREADS) {
    const int h = j / STOI_HOP, n = j % STOI_HOP;
    const long long g = k0 + h;
    float vc = 0.f, vp = 0.f;
    if (g < K && BC_DOK(g < F)) {  // (what only frames >= S would read is zero)
      const long long i1 = base + (long long)STOI_HOP * sb[g] + n;
      if (BC_DOK(i1 >= 0 && i1 < total)) {
        vc = win[n] * xc[i1];
        vp = win[n] * xp[i1];
      }
      if (g >= 1) {
        const long long i0 = base + (long long)STOI_HOP * sb[g - 1] + STOI_HOP + n;
        if (BC_DOK(i0 >= 0 && i0 < total)) {
          vc = win[n + STOI_HOP] * xc[i0] + vc;
          vp = win[n + STOI_HOP] * xp[i0] + vp;
        }
      }
    }
    xs[0][h * STOI_PITCH + n] = vc;
    xs[1][h * STOI_PITCH + n] = vp;
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  constexpr int NBT = STOI_ROWS / 16, NKB = STOI_FRAME / 16;
  constexpr long long BASIS_FLOATS = 2LL * STOI_ROWS * STOI_FRAME;
  const float* bcl = xs[0] + n * STOI_PITCH;
  const float* bpr = xs[1] + n * STOI_PITCH;
  for (int bt = wave; bt < NBT; bt += 4) {  // (wave-uniform)
    floatx4 hi[4], lo[4];  // re x clean, re x processed, im x clean, im x processed
#pragma unroll
    for (int q = 0; q < 4; ++q) hi[q] = lo[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    const long long ore = (long long)(bt * 16 + n) * STOI_FRAME + 4 * kk;
    const long long oim = ore + (long long)STOI_ROWS * STOI_FRAME;
    for (int kb0 = 0; kb0 < NKB; kb0 += 4) {
      floatx4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = kb0; kb < kb0 + 4; ++kb) {
        floatx4 are = floatx4{0.f, 0.f, 0.f, 0.f}, aim = are;
        if (BC_DOK(oim + 16 * kb + 3 < BASIS_FLOATS)) {
          are = *reinterpret_cast<const floatx4*>(basis + ore + 16 * kb);
          aim = *reinterpret_cast<const floatx4*>(basis + oim + 16 * kb);
        }
        const int k = 16 * kb + 4 * kk;
        const int pos = k + 4 * (k / STOI_HOP);
        const floatx4 xa = *reinterpret_cast<const floatx4*>(bcl + pos);
        const floatx4 xb = *reinterpret_cast<const floatx4*>(bpr + pos);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[i], xa[i], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(are[i], xb[i], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[i], xa[i], acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(aim[i], xb[i], acc[3], 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) stoi_two_sum_add(hi[q], lo[q], acc[q]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float rc = hi[0][i] + lo[0][i], rp = hi[1][i] + lo[1][i];
      const float ic = hi[2][i] + lo[2][i], ip = hi[3][i] + lo[3][i];
      float* p = pw + (bt * 16 + kk * 4 + i) * STOI_PW_PITCH + n;
      p[0] = rc * rc + ic * ic;
      p[16] = rp * rp + ip * ip;
    }
  }
  __syncthreads();

  for (int o = tid; o < 2 * STOI_BANDS * STOI_TILE; o += STOI_THREADS) {
    const int sig = o / (STOI_BANDS * STOI_TILE), q = (o / STOI_TILE) % STOI_BANDS, fr = o % STOI_TILE;
    if (k0 + fr >= S) continue;
    float s = 0.f;
    for (int bin = stoi_band_edge[q]; bin < stoi_band_edge[q + 1]; ++bin)
      s += pw[(bin - STOI_BIN0) * STOI_PW_PITCH + sig * 16 + fr];
    const long long dst = (((long long)sig * B + b) * STOI_BANDS + q) * F + k0 + fr;
    if (BC_DOK(dst < band_total)) band[dst] = sqrtf(s);
  }
}

// ---- segments and score -------------------------------------------------------------------------------------------
// For segment j < J = S - 29 and band q, over the 30 frames j .. j + 29 of x = clean and y = processed band values:
//   y' = min(y |x| / (|y| + eps), x (1 + 10^(15 / 20))), both centred, d += <x, y'> / ((|x| + eps) (|y'| + eps));
// out = d / (15 J).  Thread t takes the (j, q) pairs t, t + 256, ... in order; the threads' sums go through a fixed tree.
__global__ void __launch_bounds__(STOI_THREADS) stoi_corr_kernel(const float* __restrict__ band,
                                                                 const int* __restrict__ lens,
                                                                 const int* __restrict__ kept, float* __restrict__ out,
                                                                 long long F, long long band_total) {
  __shared__ double red[STOI_THREADS];
  const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
  if (lens && lens[b] <= 0) {  // (uniform) no samples: no value, nothing is read
    if (tid == 0) out[b] = std::numeric_limits<float>::quiet_NaN();
    return;
  }
  const long long S = (long long)kept[b] - 1;
  if (S < STOI_SEG) {  // (uniform) fewer than 30 STFT frames: the definition's fixed answer
    if (tid == 0) out[b] = 1e-5f;
    return;
  }
  const long long J = S - STOI_SEG + 1, items = J * STOI_BANDS;
  const double clip = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20)
  double sum = 0.0;
  for (long long it = tid; it < items; it += STOI_THREADS) {
    const long long j = it / STOI_BANDS, q = it % STOI_BANDS;
    const long long ox = ((long long)b * STOI_BANDS + q) * F + j, oy = (((long long)B + b) * STOI_BANDS + q) * F + j;
    if (!BC_DOK(oy + STOI_SEG - 1 < band_total)) break;
    const float* px = band + ox;
    const float* py = band + oy;
    double sx2 = 0.0, sy2 = 0.0;
    for (int i = 0; i < STOI_SEG; ++i) {
      const double x = (double)px[i], y = (double)py[i];
      sx2 += x * x;
      sy2 += y * y;
    }
    const double c = sqrt(sx2) / (sqrt(sy2) + STOI_EPS);
    double mx = 0.0, my = 0.0;
    for (int i = 0; i < STOI_SEG; ++i) {
      const double x = (double)px[i];
      mx += x;
      my += fmin((double)py[i] * c, x * clip);
    }
    mx /= (double)STOI_SEG;
    my /= (double)STOI_SEG;
    double ex = 0.0, ey = 0.0, dot = 0.0;
    for (int i = 0; i < STOI_SEG; ++i) {
      const double x = (double)px[i];
      const double xz = x - mx, yz = fmin((double)py[i] * c, x * clip) - my;
      ex += xz * xz;
      ey += yz * yz;
      dot += xz * yz;
    }
    sum += dot / ((sqrt(ex) + STOI_EPS) * (sqrt(ey) + STOI_EPS));
  }
  sum = stoi_block_sum(sum, red);
  if (tid == 0) out[b] = (float)(sum / ((double)STOI_BANDS * (double)J));
}

// ---- host -----------------------------------------------------------------------------------------------------------
// workspace: [x10: 2 B T10 floats, when resampling] [energy: B F doubles] [src: B F ints] [band: 2 B 15 F floats],
// each part rounded up to 16 bytes; T10 = ceil(T up / down), F = the frames of T10 samples.
struct StoiLayout {
  long long T10, F, off_energy, off_src, off_band, bytes;
};

static long long stoi_gcd(long long a, long long b) { return b ? stoi_gcd(b, a % b) : a; }

// 0 ok, BC_ERR_ARG, BC_ERR_UNSUPPORTED
static int stoi_layout(int B, long long T, int up, int down, StoiLayout& w) {
  if (B <= 0 || T <= 0 || up <= 0 || down <= 0) return BC_ERR_ARG;
  if (up > STOI_MAX_RATIO || down > STOI_MAX_RATIO || stoi_gcd(up, down) != 1) return BC_ERR_UNSUPPORTED;
  if (B > 65535 || T > (1LL << 31) || T > (1LL << 36) / B) return BC_ERR_UNSUPPORTED;
  auto up16 = [](long long v) { return (v + 15) & ~15LL; };
  w.T10 = stoi_len10(T, up, down);
  w.F = stoi_frames(w.T10);
  const long long Fa = w.F > 0 ? w.F : 1;
  w.off_energy = (up == 1 && down == 1) ? 0 : up16(2LL * B * w.T10 * (long long)sizeof(float));
  w.off_src = w.off_energy + up16((long long)B * Fa * (long long)sizeof(double));
  w.off_band = w.off_src + up16((long long)B * Fa * (long long)sizeof(int));
  w.bytes = w.off_band + up16(2LL * B * STOI_BANDS * Fa * (long long)sizeof(float));
  return BC_OK;
}

long long stoi_workspace_bytes(int B, long long T, int up, int down) {
  StoiLayout w;
  return stoi_layout(B, T, up, down, w) == BC_OK ? w.bytes : -1;
}

int stoi_launch(const float* clean, const float* proc, const int* lens, const float* filt, int up, int down,
                int half_len, const float* basis, float* out, int* kept, void* ws, int B, long long T,
                hipStream_t st) {
  if (!clean || !proc || !basis || !out || !kept || !ws || B <= 0 || T <= 0 || up <= 0 || down <= 0) return BC_ERR_ARG;
  const bool resample = !(up == 1 && down == 1);
  if (resample && (!filt || half_len <= 0)) return BC_ERR_ARG;
  if (((unsigned long long)basis & 15) != 0 || ((unsigned long long)ws & 15) != 0) return BC_ERR_ARG;  // 16-byte loads
  StoiLayout w;
  const int rc = stoi_layout(B, T, up, down, w);
  if (rc != BC_OK) return rc;
  if (resample && 2LL * half_len + 1 > STOI_MAX_TAPS) return BC_ERR_UNSUPPORTED;
  char* base = static_cast<char*>(ws);
  const long long F = w.F > 0 ? w.F : 1;
  const float* xc = clean;
  const float* xp = proc;
  long long pitch = T, total = (long long)B * T;
  if (resample) {
    float* x10 = reinterpret_cast<float*>(base);
    const int taps = 2 * half_len + 1;
    hipLaunchKernelGGL(stoi_resample_kernel, dim3((unsigned)((w.T10 + STOI_THREADS - 1) / STOI_THREADS), B, 2),
                       dim3(STOI_THREADS), sizeof(float) * taps, st, clean, proc, lens, filt, x10, T, w.T10, up, down,
                       half_len, total, 2LL * B * w.T10);
    BC_CHECK_LAUNCH();
    xc = x10;
    xp = x10 + (long long)B * w.T10;
    pitch = w.T10;
    total = (long long)B * w.T10;
  }
  double* energy = reinterpret_cast<double*>(base + w.off_energy);
  int* src = reinterpret_cast<int*>(base + w.off_src);
  float* band = reinterpret_cast<float*>(base + w.off_band);
  if (w.F > 0) {
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((w.F + 3) / 4), B), dim3(STOI_THREADS), 0, st, xc, pitch,
                       lens, energy, T, F, up, down, total);
    BC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(B), dim3(STOI_THREADS), 0, st, energy, lens, src, kept, T, F, up, down);
  BC_CHECK_LAUNCH();
  if (w.F > 1) {
    hipLaunchKernelGGL(stoi_tob_kernel, dim3((unsigned)((w.F - 1 + STOI_TILE - 1) / STOI_TILE), B), dim3(STOI_THREADS),
                       0, st, xc, xp, pitch, src, kept, basis, band, F, total, 2LL * B * STOI_BANDS * F);
    BC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(stoi_corr_kernel, dim3(B), dim3(STOI_THREADS), 0, st, band, lens, kept, out, F,
                     2LL * B * STOI_BANDS * F);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

}  // namespace bc

BC_DEBUG_EXPORT(stoi)
