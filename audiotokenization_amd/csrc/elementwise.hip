// HBM-bound elementwise / resampling kernels.
//
//  snake_kernel     : SnakeBeta alone (vq/activations.py:107-118) for a standalone Activation1d /
//                     SnakeBeta module call.  Inside the encoder/decoder stacks the Snake is fused
//                     into the following conv's input staging instead (conv1d.hip).
//  aa_snake_kernel  : Activation1d with antialias=True (vq/alias_free_torch/act.py:25-32):
//                     UpSample1d (resample.py:25-33: replicate pad 5, depthwise 12-tap transposed
//                     conv stride 2, x2 gain, crop [15:-15]) -> SnakeBeta -> DownSample1d
//                     (filter.py:86-95: replicate pad (5,6), depthwise 12-tap conv stride 2), fused so
//                     the 2T intermediate never leaves LDS.
//  transpose kernels: [B][C][T] <-> [C][T][B] layouts around the ResLSTM (vq/module.py:160-166).
//  synth_clips      : counter-hash white noise generated in HBM.
//  window_kernel    : a stream's [carried columns | new columns (+ Snake) | zeros] window and its next carry, for the
//                     five bc_stream_window* entry points: dense carries (a causal or a look-ahead stream), or pool
//                     rows per entry (streaming.py StreamPool / LookaheadPool), chosen at compile time.
//  lstm_state_gather / lstm_state_scatter : a pool's carried ResLSTM state, indexed by per-entry pool rows.
//  zero_tail        : zeros from each clip's own length to the padded end of a ragged batch's rows.
#include <algorithm>
#include "bc_common.h"
#include "bc_internal.h"

namespace bc {

__global__ void snake_kernel(const float* __restrict__ x, const float* __restrict__ sa,
                             const float* __restrict__ sb, float* __restrict__ y, int C, long long T,
                             long long total) {
  // element pairs through the packed Snake (the one every conv epilogue runs); an odd tail alone
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = 2 * ((long long)blockIdx.x * blockDim.x + threadIdx.x); i < total; i += 2 * stride) {
    const int c0 = (int)((i / T) % C);
    if (i + 1 < total) {
      const int c1 = (int)(((i + 1) / T) % C);
      const f32x2 v = snake_pk((f32x2){x[i], x[i + 1]}, (f32x2){sa[c0], sa[c1]}, (f32x2){sb[c0], sb[c1]});
      y[i] = v.x;
      y[i + 1] = v.y;
    } else {
      y[i] = snake(x[i], sa[c0], sb[c0]);
    }
  }
}

// One workgroup = one (b, c) row segment of AA_TILE outputs.
constexpr int AA_TILE = 256;
constexpr int AA_TAPS = 12;

__global__ void __launch_bounds__(256) aa_snake_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ sa,
                                                       const float* __restrict__ sb,
                                                       const float* __restrict__ fup,
                                                       const float* __restrict__ fdown,
                                                       float* __restrict__ y, int C, int T,
                                                       int ntiles) {
  __shared__ float xl[AA_TILE / 2 + AA_TILE + 32];
  __shared__ float sl[2 * AA_TILE + 16];
  __shared__ float fu[AA_TAPS], fd[AA_TAPS];
  const int tile = blockIdx.x % ntiles;
  const long long row = blockIdx.x / ntiles;  // b*C + c
  const int c = (int)(row % C);
  const float* xr = x + row * T;
  float* yr = y + row * T;
  const int t0 = tile * AA_TILE;
  if (threadIdx.x < AA_TAPS) {
    fu[threadIdx.x] = fup[threadIdx.x];
    fd[threadIdx.x] = fdown[threadIdx.x];
  }
  // Down stage needs snake values at up-sample index v in [2*t0-5, 2*t0+2*AA_TILE+5].
  // Up-sample index v (after the [15:-15] crop) = u - 15 where u indexes the transposed-conv
  // output; u = 2*i + k with i indexing the replicate-padded input x_p[i] = x[clamp(i-5)].
  const int vbase = 2 * t0 - 5;
  const int nv = 2 * AA_TILE + 11;
  // input indices needed: i = (v + 15 - k)/2 for k in [0,12): i in [(vbase+4)/2, (vmax+15)/2]
  const int ibase = (vbase + 15 - 11) >> 1;  // floor, vbase+4 may be negative -> arithmetic shift
  const int ni = (nv + 12) / 2 + 2;
  for (int e = threadIdx.x; e < ni; e += 256) {
    int xi = ibase + e - 5;
    xi = xi < 0 ? 0 : (xi >= T ? T - 1 : xi);
    xl[e] = xr[xi];
  }
  __syncthreads();
  const float a = sa[c], ib = sb[c];
  for (int e = threadIdx.x; e < nv; e += 256) {
    int v = vbase + e;
    v = v < 0 ? 0 : (v >= 2 * T ? 2 * T - 1 : v);  // replicate pad of the snake output (down stage)
    const int u = v + 15;
    float acc = 0.f;
    // conv_transpose1d: out[u] = sum_{k: (u-k) even} x_p[(u-k)/2] * f[k]
#pragma unroll
    for (int k = (u & 1); k < AA_TAPS; k += 2) {
      const int i = (u - k) >> 1;
      acc = acc + xl[i - ibase] * fu[k];
    }
    const float up = 2.0f * acc;
    sl[e] = snake(up, a, ib);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < AA_TILE; e += 256) {
    const int t = t0 + e;
    if (t >= T) break;
    // out[t] = sum_k z_p[2t+k] f[k], z_p[j] = s[clamp(j-5)]  -> s index v = 2t+k-5
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < AA_TAPS; ++k) acc = acc + sl[2 * e + k] * fd[k];
    yr[t] = acc;
  }
}

// x[B][C][T] -> y[C][T][B]   (tiles of 32 t x B<=64 per channel)
__global__ void __launch_bounds__(256) btc_to_ctb_kernel(const float* __restrict__ x,
                                                         float* __restrict__ y, int B, int C,
                                                         int T) {
  __shared__ float tl[64][33];
  const int tt = blockIdx.x;  // t-tile of 32
  const int c = blockIdx.y;
  const int bt = blockIdx.z;  // b-tile of 64
  const int t0 = tt * 32, b0 = bt * 64;
  for (int e = threadIdx.x; e < 64 * 32; e += 256) {
    const int bl = e / 32, tl_ = e % 32;
    const int b = b0 + bl, t = t0 + tl_;
    tl[bl][tl_] = (b < B && t < T) ? x[((long long)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 32; e += 256) {
    const int tl_ = e / 64, bl = e % 64;
    const int b = b0 + bl, t = t0 + tl_;
    if (b < B && t < T) y[((long long)c * T + t) * B + b] = tl[bl][tl_];
  }
}

// out[B][C][T] = act(y[C][T][B] + skip[B][C][T])   (ResLSTM skip, vq/module.py:163-166; act = the
// following Activation1d's Snake when sa != nullptr, fused so the LSTM output is written once)
__global__ void __launch_bounds__(256) ctb_to_btc_add_kernel(const float* __restrict__ yin,
                                                             const float* __restrict__ skip,
                                                             const float* __restrict__ sa,
                                                             const float* __restrict__ sb,
                                                             float* __restrict__ out, int B, int C,
                                                             int T) {
  __shared__ float tl[64][33];
  const int tt = blockIdx.x, c = blockIdx.y, bt = blockIdx.z;
  const int t0 = tt * 32, b0 = bt * 64;
  for (int e = threadIdx.x; e < 64 * 32; e += 256) {
    const int tl_ = e / 64, bl = e % 64;
    const int b = b0 + bl, t = t0 + tl_;
    tl[bl][tl_] = (b < B && t < T) ? yin[((long long)c * T + t) * B + b] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 32; e += 256) {
    const int bl = e / 32, tl_ = e % 32;
    const int b = b0 + bl, t = t0 + tl_;
    if (b < B && t < T) {
      const long long i = ((long long)b * C + c) * T + t;
      const float v = tl[bl][tl_] + skip[i];
      out[i] = sa ? snake(v, sa[c], sb[c]) : v;
    }
  }
}

// nn.Tanh (codec_decoder.py:80) as a standalone module call (decoder.model run as the reference's
// nn.Sequential); inside decode() it is the last conv's epilogue (same tanhf).
__global__ void tanh_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = tanhf(x[i]);
}

// Clip i, sample n: u = (splitmix64(0xB16C0DEC ^ (i<<32) ^ n) >> 40) * 2^-24, x = u - 0.5.
__global__ void synth_clips_kernel(float* __restrict__ x, int B, long long T, long long clip0) {
  const long long total = (long long)B * T;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const unsigned long long i = (unsigned long long)(clip0 + e / T);
    const unsigned long long n = (unsigned long long)(e % T);
    const unsigned long long h = splitmix64(0xB16C0DECull ^ (i << 32) ^ n);
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    x[e] = u - 0.5f;
  }
}

static inline int grid_for(long long n, int block) {
  long long g = (n + block - 1) / block;
  if (g > 65536) g = 65536;
  if (g < 1) g = 1;
  return (int)g;
}

int snake_launch(const float* x, const float* sa, const float* sb, float* y, int B, int C,
                 long long T, hipStream_t st) {
  const long long total = (long long)B * C * T;
  if (total == 0) return BC_OK;
  hipLaunchKernelGGL(snake_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, x, sa, sb, y, C, T,
                     total);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// The streaming window (streaming.py): one kernel behind the five bc_stream_window*
// entry points.  A stage of a stream is a lazy valid conv (or a whole one-launch ResidualUnit) over
// [the columns it carried | the new columns | zeros], and it hands on the columns it has not finished with.  For each
// (b, c) row, with W window columns:
//   win[j] = j < ci ? (cr ? cr[j] : 0) : j < ci + n ? act(x[xo + j - ci]) : 0      (j < W)
//   nr[i]  = win[keep + i]   for i < co                                            (co == 0: nothing stored)
// act = SnakeBeta through snake() (bit-identical to snake_kernel's pairs and to the convs' Snake epilogue) or the
// identity.  A missing carry reads zeros (a stream's first chunk: the conv's left zero padding; snake(0) = 0, so
// zeros are the same before and after the activation).  x may be a strided view (row pitch xT, batch pitch xbs: a
// ResidualUnit run over its own window hands its last columns on without a copy); it is never dereferenced with
// n == 0 and never at or past an entry's own n (it may hold NaN there).  The zeros behind ci + n are a layer's right
// zero padding at a flush and the tail behind a short entry alike.  A carry never holds one of them: keep + co <=
// ci + n, which with keep < ci reaches back into the old carry.
// Who sets what (a Rows descriptor, passed by value, turns a row into a WinRow):
//   WinDense<true>   bc_stream_window          ci = co = P, n, xo = 0, keep = n, W = P + n   kernel arguments only:
//   WinDense<false>  bc_stream_window_la       ci = Pin, co = Pout, keep = Pin + n - Pout,   cr = ctx + row * Pin,
//                                              W = Pin + n + R                               nr = ctx_out + row * Pout
//   WinSlots<false>  bc_stream_window_slots    ci = co = P, n = keep = the chunk, W = P + n  pool rows src[b] / dst[b]
//   WinSlots<true>   bc_stream_window_slots_lens  n = keep = clamp(lens[b] * unit, 0, chunk) and lens[b]
//   WinSlotsLa       bc_stream_window_slots_la cin, n, xoff, keep, cout [b], any W           pool rows src[b] / dst[b]
// The dense rows read no per-entry array: a dependent src[b] / dst[b] load in front of this little work costs a
// quarter of the kernel, hence a template and not a run-time switch.  Pool rows: pool is
// [pool_rows][C][pitch], src[b] < 0 reads the carry as zeros (a fresh session), dst[b] < 0 stores nothing (co = 0:
// the padding entries of a graph replay); the values come from device memory, so the debug build checks them against
// the pool and a bad one is skipped.  WinSlotsLa clamps cin and cout to [0, Pmax], xoff to [0, xn] and n to [0, min(W - cin,
// xn - xoff)], so no index array can take an access out of x, win or a pool row.
// IN-PLACE HAZARD: with keep < ci, carry element i of a row is read by the thread that writes window column i and
// overwritten by the thread at column keep + i, which may sit in another workgroup, so a pool row must never be read
// and written in one launch.  The HOST guarantees it: the src and dst row sets of a launch are disjoint and dst holds
// no row twice (the pools' ping-pong rows 2s / 2s + 1 per session); the kernel cannot check it.
// 2-D grid (three 64-bit divisions per element): y walks the (b, c) rows (one 32-bit division per row),
// x the W columns of a row.  One float per lane, coalesced along the row: the three streams of a row start at
// row * W, row * pitch and a strided view's column offset (3d behind a one-launch ResidualUnit), with carries of
// 6d = 6, 18, 54 columns in steady state, so they are never 16-byte aligned together and no stage would take a vector
// path.
struct WinRow {
  const float* cr;  // the carried columns (null: zeros)
  float* nr;        // where the next carry goes (not dereferenced with co == 0)
  int ci, n, xo, keep, co;
};

// (pin / pout: the pitch of a carry row read / written; xn: the columns of x an entry may touch; tail: zeros may
// follow the new columns, W > ci + n.)  What a launcher knows is a template argument, because these kernels are bound
// by the instructions of a wave, not by bytes: Plain is bc_stream_window's pout == pin, W == pin + xn; Lens is
// bc_stream_window_slots_lens' length per entry.
template <bool Plain>
struct WinDense {
  static constexpr bool tail = !Plain;
  const float* ctx;
  float* ctx_out;
  int pin, xn, pout;
  __device__ WinRow row(int row, int, int, int) const {
    // (a null ctx_out comes with a carry out of no columns, so it is never dereferenced)
    if (Plain) {
      const long long at = (long long)row * pin;
      return {ctx ? ctx + at : nullptr, ctx_out + at, pin, xn, 0, xn, pin};
    }
    return {ctx ? ctx + (long long)row * pin : nullptr, ctx_out + (long long)row * pout, pin, xn, 0, pin + xn - pout,
            pout};
  }
};

template <bool Lens>
struct WinSlots {
  static constexpr bool tail = Lens;
  float* pool;
  const int *src, *dst, *lens;  // (lens is read with Lens only)
  int unit, pin, pout, xn, pool_rows;
  __device__ WinRow row(int, int b, int c, int C) const {
    const int s = src[b], d = dst[b];
    int L = xn;
    if (Lens) {
      const long long want = (long long)lens[b] * unit;
      L = want < 0 ? 0 : want > xn ? xn : (int)want;
    }
    return {(s >= 0 && BC_DOK(s < pool_rows)) ? pool + ((long long)s * C + c) * pin : nullptr,
            pool + ((long long)max(d, 0) * C + c) * pin, pin, L, 0, L, (d >= 0 && BC_DOK(d < pool_rows)) ? pin : 0};
  }
};

struct WinSlotsLa {
  static constexpr bool tail = true;
  float* pool;
  const int *src, *dst, *cin, *nnew, *xoff, *keep, *cout;
  int W, pin, pout, xn, pool_rows;
  __device__ WinRow row(int, int b, int c, int C) const {
    const int s = src[b], d = dst[b];
    const int ci = min(max(cin[b], 0), pin), co = min(max(cout[b], 0), pin);
    const int xo = min(max(xoff[b], 0), xn);
    const int n = min(max(nnew[b], 0), min(W - ci, xn - xo));  // (W - ci < 0: no new column, the carry fills the row)
    return {(s >= 0 && BC_DOK(s < pool_rows)) ? pool + ((long long)s * C + c) * pin : nullptr,
            pool + ((long long)max(d, 0) * C + c) * pin, ci, n, xo, keep[b],
            (d >= 0 && BC_DOK(d < pool_rows)) ? co : 0};
  }
};

template <class Rows>
__global__ void __launch_bounds__(256) window_kernel(const Rows rows_of, const float* __restrict__ x, long long xbs,
                                                     long long xT, const float* __restrict__ sa,
                                                     const float* __restrict__ sb, float* __restrict__ win, int C,
                                                     int W, int rows) {
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int b = row / C, c = row - b * C;
    const WinRow r = rows_of.row(row, b, c, C);
    const float* __restrict__ cr = r.cr;
    float* __restrict__ nr = r.nr;
    const int S = r.ci + r.n;
    const float* xr = x + (long long)b * xbs + (long long)c * xT + r.xo;
    float* wr = win + (long long)row * W;
    const float a_ = sa ? sa[c] : 0.f, b_ = sa ? sb[c] : 0.f;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < W; j += gridDim.x * blockDim.x) {
      float v = 0.f;
      if (j < r.ci) {
        if (cr && BC_DOK(j >= 0 && j < rows_of.pin && row < rows)) v = cr[j];
      } else if (!Rows::tail || j < S) {
        if (BC_DOK(j - r.ci >= 0 && r.xo + (j - r.ci) < rows_of.xn && r.xo + (j - r.ci) < xT)) {
          v = xr[(unsigned)(j - r.ci)];
          if (sa) v = snake(v, a_, b_);
        }
      }
      if (BC_DOK(j >= 0 && j < W && row < rows)) wr[j] = v;
      // keep <= j < keep + co in one compare (j < S: a carry that reaches into the zeros is a host bug the debug
      // build reports)
      if ((unsigned)j - (unsigned)r.keep < (unsigned)r.co &&
          BC_DOK(j - r.keep >= 0 && j - r.keep < rows_of.pout && j < S))
        nr[(unsigned)j - (unsigned)r.keep] = v;
    }
  }
}

// (the launchers have checked that rows and W fit an int, and W >= 1)
template <class Rows>
static int launch_window(const Rows& rows_of, const float* x, long long xbs, long long xT, const float* sa,
                         const float* sb, float* win, int C, long long W, long long rows, hipStream_t st) {
  const int gx = (int)std::min<long long>((W + 255) / 256, 1024), gy = (int)std::min<long long>(rows, 65535);
  hipLaunchKernelGGL(window_kernel<Rows>, dim3(gx, gy), dim3(256), 0, st, rows_of, x, xbs, xT, sa, sb, win, C, (int)W,
                     (int)rows);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int stream_window_launch(const float* x, long long xbs, long long xT, const float* ctx, const float* sa, const float* sb,
                         float* win, float* ctx_out, int B, int C, int n, int P, hipStream_t st) {
  if (!x || !win || B < 0 || C < 1 || n < 1 || P < 0 || xT < n || xbs < (long long)(C - 1) * xT + n) return BC_ERR_ARG;
  if ((sa == nullptr) != (sb == nullptr) || (P > 0 && !ctx_out)) return BC_ERR_ARG;
  const long long rows = (long long)B * C, W = (long long)P + n;
  if (rows == 0) return BC_OK;
  if (rows > 0x7fffffffLL || W > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  return launch_window(WinDense<true>{ctx, ctx_out, P, n, P}, x, xbs, xT, sa, sb, win, C, W, rows, st);
}

int stream_window_la_launch(const float* x, long long xbs, long long xT, const float* ctx, const float* sa,
                            const float* sb, float* win, float* ctx_out, int B, int C, int n, int Pin, int R, int Pout,
                            hipStream_t st) {
  if (!win || B < 0 || C < 1 || n < 0 || Pin < 0 || R < 0 || Pout < 0) return BC_ERR_ARG;
  if (n > 0 && (!x || xT < n || xbs < (long long)(C - 1) * xT + n)) return BC_ERR_ARG;
  if ((sa == nullptr) != (sb == nullptr) || (ctx_out == nullptr) != (Pout == 0)) return BC_ERR_ARG;
  const long long rows = (long long)B * C, S = (long long)Pin + n, W = S + R;
  if (W < 1 || Pout > S) return BC_ERR_ARG;
  if (rows > 0x7fffffffLL || W > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  if (rows == 0) return BC_OK;
  return launch_window(WinDense<false>{ctx, ctx_out, Pin, n, Pout}, x, xbs, xT, sa, sb, win, C, W, rows, st);
}

int stream_window_slots_launch(const float* x, long long xbs, long long xT, float* pool, const int* src, const int* dst,
                               const float* sa, const float* sb, float* win, int B, int C, int n, int P, int pool_rows,
                               hipStream_t st) {
  if (!x || !pool || !src || !dst || !win || B < 0 || C < 1 || n < 1 || P < 1 || pool_rows < 1) return BC_ERR_ARG;
  if (xT < n || xbs < (long long)(C - 1) * xT + n || (sa == nullptr) != (sb == nullptr)) return BC_ERR_ARG;
  const long long rows = (long long)B * C, W = (long long)P + n;
  if (rows > 0x7fffffffLL || W > 0x7fffffffLL || (long long)pool_rows * C > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  if (rows == 0) return BC_OK;
  return launch_window(WinSlots<false>{pool, src, dst, nullptr, 1, P, P, n, pool_rows}, x, xbs, xT, sa, sb, win, C, W,
                       rows, st);
}

// A chunk length per entry (StreamPool.push(..., hops=)): lens in hops, unit = this stage's columns per hop.
// lens[b] * unit == n for every b is bc_stream_window_slots bit for bit.
int stream_window_slots_lens_launch(const float* x, long long xbs, long long xT, float* pool, const int* src,
                                    const int* dst, const int* lens, int unit, const float* sa, const float* sb,
                                    float* win, int B, int C, int n, int P, int pool_rows, hipStream_t st) {
  if (!x || !pool || !src || !dst || !lens || !win || B < 0 || C < 1 || n < 1 || P < 1 || pool_rows < 1 || unit < 1)
    return BC_ERR_ARG;
  if (xT < n || xbs < (long long)(C - 1) * xT + n || (sa == nullptr) != (sb == nullptr)) return BC_ERR_ARG;
  const long long rows = (long long)B * C, W = (long long)P + n;
  if (rows > 0x7fffffffLL || W > 0x7fffffffLL || (long long)pool_rows * C > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  if (rows == 0) return BC_OK;
  return launch_window(WinSlots<true>{pool, src, dst, lens, unit, P, P, n, pool_rows}, x, xbs, xT, sa, sb, win, C, W,
                       rows, st);
}

int stream_window_slots_la_launch(const float* x, long long xbs, long long xT, int xn, float* pool, const int* src,
                                  const int* dst, const int* cin, const int* nnew, const int* xoff, const int* keep,
                                  const int* cout, const float* sa, const float* sb, float* win, int B, int C, int W,
                                  int Pmax, int pool_rows, hipStream_t st) {
  if (!pool || !src || !dst || !cin || !nnew || !xoff || !keep || !cout || !win) return BC_ERR_ARG;
  if (B < 0 || C < 1 || W < 1 || Pmax < 1 || pool_rows < 1 || xn < 0) return BC_ERR_ARG;
  if (xn > 0 && (!x || xT < xn || xbs < (long long)(C - 1) * xT + xn)) return BC_ERR_ARG;
  if ((sa == nullptr) != (sb == nullptr)) return BC_ERR_ARG;
  const long long rows = (long long)B * C;
  if (rows > 0x7fffffffLL || (long long)pool_rows * C > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  if (rows == 0) return BC_OK;
  return launch_window(WinSlotsLa{pool, src, dst, cin, nnew, xoff, keep, cout, W, Pmax, Pmax, xn, pool_rows}, x, xbs, xT,
                       sa, sb, win, C, W, rows, st);
}

// The carried ResLSTM state of a session pool: bc_reslstm_fwd_state takes dense [num_layers][H][B] (unit-major) h0 / c0
// and hands back hT / cT; the pool keeps [num_layers][H][pool_rows].  Gather: h0[lu][b] = src[b] >= 0 ?
// h_pool[lu][src[b]] : 0 (a fresh session's zero state), c likewise; scatter: h_pool[lu][dst[b]] = hT[lu][b] for
// dst[b] >= 0.  lu walks the LH = num_layers * H units; h and c in one launch.
__global__ void __launch_bounds__(256) lstm_state_gather_kernel(const float* __restrict__ h_pool,
                                                                const float* __restrict__ c_pool,
                                                                const int* __restrict__ src, float* __restrict__ h0,
                                                                float* __restrict__ c0, int LH, int B, int pool_rows) {
  const int total = LH * B;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int lu = e / B, b = e - lu * B;
    const int s = src[b];
    const bool live = s >= 0 && BC_DOK(s < pool_rows);
    const long long i = (long long)lu * pool_rows + s;
    h0[e] = live ? h_pool[i] : 0.f;
    c0[e] = live ? c_pool[i] : 0.f;
  }
}

__global__ void __launch_bounds__(256) lstm_state_scatter_kernel(float* __restrict__ h_pool, float* __restrict__ c_pool,
                                                                 const int* __restrict__ dst,
                                                                 const float* __restrict__ hT,
                                                                 const float* __restrict__ cT, int LH, int B,
                                                                 int pool_rows) {
  const int total = LH * B;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int lu = e / B, b = e - lu * B;
    const int d = dst[b];
    if (d < 0 || !BC_DOK(d < pool_rows)) continue;
    const long long i = (long long)lu * pool_rows + d;
    h_pool[i] = hT[e];
    c_pool[i] = cT[e];
  }
}

static int lstm_state_sizes(int num_layers, int H, int B, int pool_rows, long long* total) {
  if (num_layers < 1 || H < 1 || B < 0 || pool_rows < 1) return BC_ERR_ARG;
  *total = (long long)num_layers * H * B;
  if ((long long)num_layers * H > 0x7fffffffLL || *total > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  return BC_OK;
}

int lstm_state_gather_launch(const float* h_pool, const float* c_pool, const int* src, float* h0, float* c0,
                             int num_layers, int H, int B, int pool_rows, hipStream_t st) {
  long long total = 0;
  if (!h_pool || !c_pool || !src || !h0 || !c0) return BC_ERR_ARG;
  if (const int rc = lstm_state_sizes(num_layers, H, B, pool_rows, &total)) return rc;
  if (total == 0) return BC_OK;
  hipLaunchKernelGGL(lstm_state_gather_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, h_pool, c_pool, src, h0, c0,
                     num_layers * H, B, pool_rows);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int lstm_state_scatter_launch(float* h_pool, float* c_pool, const int* dst, const float* hT, const float* cT,
                              int num_layers, int H, int B, int pool_rows, hipStream_t st) {
  long long total = 0;
  if (!h_pool || !c_pool || !dst || !hT || !cT) return BC_ERR_ARG;
  if (const int rc = lstm_state_sizes(num_layers, H, B, pool_rows, &total)) return rc;
  if (total == 0) return BC_OK;
  hipLaunchKernelGGL(lstm_state_scatter_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, h_pool, c_pool, dst, hT, cT,
                     num_layers * H, B, pool_rows);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// Ragged batches (blocks.py Ragged): clips of different lengths share one zero-padded batch, and the computation stays
// the per-clip one as long as every producer's output is exactly zero from the clip's own per-layer length lens[b] to
// the padded end T (the zero padding every conv of the per-clip forward reads there).  For each row (b, c) of y (and of
// y2, the activated twin of a dual output) this stores 0.0f at t in [clamp(lens[b], 0, T), T): stores, never a
// multiplication by a mask, since the tail may hold Inf / NaN.  Only the tails are touched: grid x walks groups of four
// floats from the 16-byte boundary at or below the row's first tail element (16-byte stores for whole groups when
// vec: y and y2 16-byte aligned; single floats for the unaligned head, the end of the row and unaligned views), grid
// y the rows (one 32-bit division per row), so the cost scales with the padding, tail_max = T - min(lens) columns at
// the most, and a row with lens[b] >= T does nothing.  total = rows * T bounds the debug build's index guards.
__global__ void __launch_bounds__(256) zero_tail_kernel(float* __restrict__ y, float* __restrict__ y2,
                                                        const int* __restrict__ lens, int C, long long T, int rows,
                                                        long long total, bool vec) {
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int b = row / C;
    long long len = lens[b];
    len = len < 0 ? 0 : len;
    if (len >= T) continue;
    const long long first = (long long)row * T + len, end = (long long)row * T + T;  // the tail's elements of y
    const long long g0 = first & ~3LL;
    for (long long e = g0 + 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x); e < end;
         e += 4LL * gridDim.x * blockDim.x) {
      if (vec && e >= first && e + 4 <= end) {
        if (!BC_DOK(e >= 0 && e + 3 < total)) continue;
        *reinterpret_cast<floatx4*>(y + e) = floatx4{0.f, 0.f, 0.f, 0.f};
        if (y2) *reinterpret_cast<floatx4*>(y2 + e) = floatx4{0.f, 0.f, 0.f, 0.f};
      } else {
        const long long lo = e < first ? first : e, hi = e + 4 < end ? e + 4 : end;
        for (long long i = lo; i < hi; ++i) {
          if (!BC_DOK(i >= 0 && i < total)) break;
          y[i] = 0.f;
          if (y2) y2[i] = 0.f;
        }
      }
    }
  }
}

int zero_tail_launch(float* y, float* y2, const int* lens, int B, int C, long long T, long long tail_max, hipStream_t st) {
  if (!y || !lens || B <= 0 || C <= 0 || T <= 0) return BC_ERR_ARG;
  if (tail_max <= 0) return BC_OK;  // every clip fills the batch: nothing to zero
  const long long rows = (long long)B * C;
  if (rows > 0x7fffffffLL || T > (1LL << 62) / rows) return BC_ERR_UNSUPPORTED;
  if (tail_max > T) tail_max = T;
  const long long groups = (tail_max + 3) / 4 + 1;  // (+1: the group that straddles the tail's first element)
  const int gx = (int)std::min<long long>((groups + 255) / 256, 1024), gy = (int)std::min<long long>(rows, 65535);
  const bool vec = (((unsigned long long)y | (unsigned long long)y2) & 15) == 0;
  hipLaunchKernelGGL(zero_tail_kernel, dim3(gx, gy), dim3(256), 0, st, y, y2, lens, C, T, (int)rows, rows * T, vec);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// Activation1d with any (up_ratio, up taps, down_ratio, down taps) (act.py:8-23 constructor arguments):
// the same three stages as aa_snake_kernel, with the geometry of resample.py:10-33 / filter.py:86-95 at
// run time.  Up: replicate pad P = Ku / ru - 1, transposed conv stride ru, x ru, crop [PL, -PR) with
// PL = P ru + (Ku - ru) / 2; Snake; down: replicate pad (Kd / 2 - even, Kd / 2), conv stride rd.
// One workgroup = AA_TILE outputs of one (b, c) row; the tile's snake values s[j] (j = t rd + k - DL)
// and the x range they need sit in dynamic LDS.
__global__ void __launch_bounds__(256) aa_snake_gen_kernel(const float* __restrict__ x, const float* __restrict__ sa,
                                                           const float* __restrict__ sb, const float* __restrict__ fup,
                                                           const float* __restrict__ fdown, float* __restrict__ y,
                                                           int C, int T, int Tout, int ntiles, int ru, int ku, int rd,
                                                           int kd, int nx, int ns) {
  extern __shared__ float aa_sm[];
  float* fu = aa_sm;
  float* fd = fu + ku;
  float* xl = fd + kd;
  float* sl = xl + nx;
  const int tile = blockIdx.x % ntiles;
  const long long row = blockIdx.x / ntiles;  // b*C + c
  const int c = (int)(row % C);
  const float* xr = x + row * T;
  float* yr = y + row * (long long)Tout;
  const int t0 = tile * AA_TILE;
  const long long L = (long long)T * ru;            // up-sampled length
  const int up_pad = ku / ru - 1;
  const int up_pl = up_pad * ru + (ku - ru) / 2;    // crop offset into the transposed-conv output
  const int dn_pl = kd / 2 - (kd % 2 == 0 ? 1 : 0);
  for (int e = threadIdx.x; e < ku; e += 256) fu[e] = fup[e];
  for (int e = threadIdx.x; e < kd; e += 256) fd[e] = fdown[e];
  // s index range of the tile: j = t rd + k - dn_pl, clamped to [0, L) (replicate pad of the Snake output)
  const long long j0 = (long long)t0 * rd - dn_pl;
  const long long v0 = j0 < 0 ? 0 : (j0 >= L ? L - 1 : j0);
  // transposed-conv input indices i = (v + up_pl - k) / ru over the clamped v range
  const long long ibase = (v0 + up_pl - (ku - 1)) / ru - 1;
  for (int e = threadIdx.x; e < nx; e += 256) {
    long long xi = ibase + e - up_pad;  // padded index -> x index, replicate
    xi = xi < 0 ? 0 : (xi >= T ? T - 1 : xi);
    xl[e] = xr[xi];
  }
  __syncthreads();
  const float a = sa[c], ib = sb[c];
  const long long np = (long long)T + 2 * up_pad;  // padded input length
  for (int e = threadIdx.x; e < ns; e += 256) {
    long long v = j0 + e;
    v = v < 0 ? 0 : (v >= L ? L - 1 : v);
    const long long u = v + up_pl;
    float acc = 0.f;
    for (int k = (int)(u % ru); k < ku; k += ru) {  // out[u] = sum_{k: (u - k) % ru == 0} x_p[(u - k) / ru] f[k]
      const long long i = (u - k) / ru;
      if (i >= np) continue;
      if (i < 0) break;
      acc = acc + xl[i - ibase] * fu[k];
    }
    sl[e] = snake((float)ru * acc, a, ib);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < AA_TILE; e += 256) {
    const int t = t0 + e;
    if (t >= Tout) break;
    float acc = 0.f;
    for (int k = 0; k < kd; ++k) acc = acc + sl[e * rd + k] * fd[k];
    yr[t] = acc;
  }
}

// output length of the general activation (the down stage's conv over the padded up-sampled signal)
long long aa_snake_out_len(int T, int ru, int rd, int kd) {
  const long long L = (long long)T * ru;
  const int pl = kd / 2 - (kd % 2 == 0 ? 1 : 0), pr = kd / 2;
  const long long n = L + pl + pr - kd;
  return n < 0 ? 0 : n / rd + 1;
}

int aa_snake_gen_launch(const float* x, const float* sa, const float* sb, const float* fu, const float* fd, float* y,
                        int B, int C, int T, int ru, int ku, int rd, int kd, hipStream_t st) {
  if (ru < 1 || rd < 1 || ku < ru || kd < 1 || ku > 256 || kd > 256 || ru > 16 || rd > 16) return BC_ERR_UNSUPPORTED;
  const long long Tout = aa_snake_out_len(T, ru, rd, kd);
  if ((long long)B * C * T == 0 || Tout == 0) return BC_OK;
  if (Tout > 0x7fffffffLL) return BC_ERR_UNSUPPORTED;
  const int ntiles = (int)((Tout + AA_TILE - 1) / AA_TILE);
  const long long nwg = (long long)B * C * ntiles;
  if (nwg > 0x7fffffffLL) return BC_ERR_ARG;
  const int ns = (AA_TILE - 1) * rd + kd;
  const int nx = (ns + ku) / ru + 4;
  const size_t lds = (size_t)(ku + kd + nx + ns) * sizeof(float);
  if (lds > 64 * 1024) return BC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(aa_snake_gen_kernel, dim3((unsigned)nwg), dim3(256), lds, st, x, sa, sb, fu, fd, y, C, T,
                     (int)Tout, ntiles, ru, ku, rd, kd, nx, ns);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int aa_snake_launch(const float* x, const float* sa, const float* sb, const float* fu,
                    const float* fd, float* y, int B, int C, int T, hipStream_t st) {
  if ((long long)B * C * T == 0) return BC_OK;
  const int ntiles = (T + AA_TILE - 1) / AA_TILE;
  const long long nwg = (long long)B * C * ntiles;
  if (nwg > 0x7fffffffLL) return BC_ERR_ARG;
  hipLaunchKernelGGL(aa_snake_kernel, dim3((unsigned)nwg), dim3(256), 0, st, x, sa, sb, fu, fd, y, C,
                     T, ntiles);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int btc_to_ctb_launch(const float* x, float* y, int B, int C, int T, hipStream_t st) {
  if ((long long)B * C * T == 0) return BC_OK;
  dim3 grid((T + 31) / 32, C, (B + 63) / 64);
  hipLaunchKernelGGL(btc_to_ctb_kernel, grid, dim3(256), 0, st, x, y, B, C, T);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int ctb_to_btc_add_launch(const float* y, const float* skip, const float* sa, const float* sb,
                          float* out, int B, int C, int T, hipStream_t st) {
  if ((long long)B * C * T == 0) return BC_OK;
  dim3 grid((T + 31) / 32, C, (B + 63) / 64);
  hipLaunchKernelGGL(ctb_to_btc_add_kernel, grid, dim3(256), 0, st, y, skip, sa, sb, out, B, C, T);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// [C][T][B] -> [C][T][B] with time reversed (the backward direction of a bidirectional LSTM runs the
// forward recurrence over the reversed sequence); B floats per (c, t) row, 16-byte moves when B % 4 == 0.
__global__ void time_reverse_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int T, int B) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  if (B % 4 == 0) {
    const int q = B / 4;
    const long long n = rows * q;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
      const long long row = e / q, c = row / T;
      const int t = (int)(row - c * T), j = (int)(e - row * q);
      reinterpret_cast<float4*>(y)[(c * T + (T - 1 - t)) * q + j] = reinterpret_cast<const float4*>(x)[e];
    }
    return;
  }
  const long long n = rows * B;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const long long row = e / B, c = row / T;
    const int t = (int)(row - c * T), b = (int)(e - row * B);
    y[(c * T + (T - 1 - t)) * B + b] = x[e];
  }
}

int time_reverse_launch(const float* x, float* y, int C, int T, int B, hipStream_t st) {
  const long long rows = (long long)C * T, n = rows * (B % 4 == 0 ? B / 4 : B);
  if (n == 0) return BC_OK;
  hipLaunchKernelGGL(time_reverse_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, rows, T, B);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int tanh_launch(const float* x, float* y, long long n, hipStream_t st) {
  if (n == 0) return BC_OK;
  hipLaunchKernelGGL(tanh_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, n);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

int synth_clips_launch(float* x, int B, long long T, long long clip0, hipStream_t st) {
  const long long total = (long long)B * T;
  if (total == 0) return BC_OK;
  hipLaunchKernelGGL(synth_clips_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, x, B, T,
                     clip0);
  BC_CHECK_LAUNCH();
  return BC_OK;
}

// ConvTranspose1d interleave (bc_convT1d_fwd_ws): output t of row (b, co) is phase r = (t + p) mod s, position
// q = (t + p) div s of that phase, i.e. element q - q_lo[r] of the phase's contiguous row (b, co) in the workspace.
// One thread per 4 consecutive outputs (16-byte stores where the row allows).
__global__ void __launch_bounds__(256) convT_interleave_kernel(const float* __restrict__ ph, const float* __restrict__ ph2,
                                                               float* __restrict__ y, float* __restrict__ y2, int Tout,
                                                               int Q4, long long plane, ConvTInterleave il, bool vec) {
  const long long row = blockIdx.y;  // b * Cout + co
  const int t0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (t0 >= Tout) return;
  float v[4], v2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = t0 + k;
    if (t >= Tout) break;
    const int u = t + il.p;
    const int r = u % il.s, q = u / il.s;
    const long long src = r * plane + row * Q4 + (q - il.q_lo[r]);
    v[k] = ph[src];
    if (ph2) v2[k] = ph2[src];
  }
  float* yr = y + row * Tout;
  float* y2r = y2 ? y2 + row * Tout : nullptr;
  if (vec && t0 + 3 < Tout) {  // vec: Tout % 4 == 0 and y / y2 16-byte aligned (callers may pass views)
    *reinterpret_cast<floatx4*>(yr + t0) = floatx4{v[0], v[1], v[2], v[3]};
    if (y2r) *reinterpret_cast<floatx4*>(y2r + t0) = floatx4{v2[0], v2[1], v2[2], v2[3]};
  } else {
    for (int k = 0; k < 4 && t0 + k < Tout; ++k) {
      yr[t0 + k] = v[k];
      if (y2r) y2r[t0 + k] = v2[k];
    }
  }
}

int convT_interleave_launch(const float* ph, const float* ph2, float* y, float* y2, int B, int Cout, int Tout, int Q4,
                            const ConvTInterleave& il, hipStream_t st) {
  const long long rows = (long long)B * Cout;
  if (rows <= 0 || Tout <= 0) return BC_OK;
  if (rows > 65535 * 1024LL) return BC_ERR_UNSUPPORTED;
  const int gx = (Tout + 1023) / 1024;
  const bool vec = (Tout & 3) == 0 && (((unsigned long long)y | (unsigned long long)y2) & 15) == 0;
  // grid.y is limited to 65535: fold the rows into chunks
  for (long long r0 = 0; r0 < rows; r0 += 65535) {
    const int ny = (int)(rows - r0 < 65535 ? rows - r0 : 65535);
    hipLaunchKernelGGL(convT_interleave_kernel, dim3(gx, ny), dim3(256), 0, st, ph + r0 * Q4, ph2 ? ph2 + r0 * Q4 : nullptr,
                       y + r0 * Tout, y2 ? y2 + r0 * Tout : nullptr, Tout, Q4, (long long)rows * Q4, il, vec);
    BC_CHECK_LAUNCH();
  }
  return BC_OK;
}

}  // namespace bc

BC_DEBUG_EXPORT(elementwise)
