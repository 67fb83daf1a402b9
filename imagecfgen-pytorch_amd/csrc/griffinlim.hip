// Griffin-Lim phase reconstruction (include/ali_hip.h: ali_gl_init / ali_gl_ola / ali_gl_phase / ali_gl_check): the
// torchaudio.transforms.GriffinLim the reference builds next to every Spectrogram (image_scms/audio_mnist.py:62-64,
// whalecalls.py:56-59, esrf_acoustic.py:40-43) and calls as spectrogram_to_audio(img_to_spect(G(...)).exp()).
//
// One iteration is   X --[inverse DFT GEMM]--> fr --ali_gl_ola--> frames --[forward DFT GEMM]--> Y --ali_gl_phase--> X
// with both DFT products on the fp32-MFMA GEMM (ali_conv_fwd, 1x1) and the three HBM-bound steps here:
//   ali_gl_init   [B][F][T] source -> magnitudes [B*T][F] and the first GEMM operand [B*T][2F] (re | im of angles*mag),
//                 transposed through a 32x32 LDS tile; the random initial phases come from the counter RNG.
//   ali_gl_ola    overlap-add of the inverse frames in gather form (fixed order, no atomics), times the reciprocal
//                 window envelope, written either as the NEXT transform's frames (centre=True, reflect padding folded
//                 into the index map: the waveform itself is never stored) or as the final waveform.
//   ali_gl_phase  a = Y - m*tprev, X = a / (|a| + 1e-16) * mag, float4 in and out.
#include <math.h>
#include "ali_common.h"

namespace ali {

constexpr int kGlBlock = 256;

// ---- ali_gl_init ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGlBlock)
gl_init_kernel(const float* __restrict__ src, int F, int T, int mode, const float* __restrict__ mean,
               const float* __restrict__ stdv, float clip_k, float inv_power, const float* __restrict__ a0_re,
               const float* __restrict__ a0_im, int rand_init, uint64_t seed, const long long* __restrict__ dev_counter,
               uint64_t offset, float* __restrict__ mag, float* __restrict__ X) {
  __shared__ float tile[3][32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const uint64_t key = phase_key(rng_base_key(seed, dev_counter));
  for (int r = ty; r < 32; r += 8) {                        // rows = frequencies, columns = frames (contiguous in src)
    const int f = f0 + r, t = t0 + tx;
    float m = 0.f, re = 0.f, im = 0.f;
    if (f < F && t < T) {
      const long long e = ((long long)b * F + f) * T + t;
      const float v = src[e];
      if (mode == ALI_GL_SRC_IMAGE) m = expf((v * clip_k * (stdv[t] + 1e-6f) + mean[t]) * inv_power);
      else if (mode == ALI_GL_SRC_LOG) m = expf(v * inv_power);
      else m = inv_power == 0.5f ? sqrtf(v) : (inv_power == 1.f ? v : powf(v, inv_power));
      if (a0_re) {
        re = a0_re[e];
        im = a0_im[e];
      } else if (rand_init) {                               // both parts from one hash: disjoint 24-bit fields, exact in fp32
        const uint64_t h = hash_at(key, offset + (uint64_t)e);
        re = (float)hi24(h) * kInv24;
        im = (float)lo24(h) * kInv24;
      } else {
        re = 1.f;
      }
    }
    tile[0][r][tx] = m;
    tile[1][r][tx] = re * m;
    tile[2][r][tx] = im * m;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {                        // rows = frames, columns = frequencies (contiguous in mag, X)
    const int t = t0 + r, f = f0 + tx;
    if (t < T && f < F) {
      const long long row = (long long)b * T + t;
      mag[row * F + f] = tile[0][tx][r];
      X[row * 2 * F + f] = tile[1][tx][r];
      X[row * 2 * F + F + f] = tile[2][tx][r];
    }
  }
}

// ---- ali_gl_phase --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGlBlock)
gl_phase_kernel(const float* __restrict__ Y, const float* __restrict__ tprev, const float* __restrict__ mag, float m,
                long long nvec, int F4, float* __restrict__ X) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += step) {
    const long long row = v / F4;
    const int f = (int)(v - row * F4) * 4;
    const long long ore = row * (8LL * F4) + f, oim = ore + 4LL * F4;
    f32x4 re = *reinterpret_cast<const f32x4*>(Y + ore), im = *reinterpret_cast<const f32x4*>(Y + oim);
    if (tprev) {
      re -= m * *reinterpret_cast<const f32x4*>(tprev + ore);
      im -= m * *reinterpret_cast<const f32x4*>(tprev + oim);
    }
    const f32x4 g = *reinterpret_cast<const f32x4*>(mag + row * (4LL * F4) + f);
    f32x4 xr, xi;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = 1.f / (hypotf(re[c], im[c]) + 1e-16f);   // a == 0: s = 1e16, a*s = 0 exactly; never NaN
      xr[c] = re[c] * s * g[c];
      xi[c] = im[c] * s * g[c];
    }
    *reinterpret_cast<f32x4*>(X + ore) = xr;
    *reinterpret_cast<f32x4*>(X + oim) = xi;
  }
}

// ---- ali_gl_ola ----------------------------------------------------------------------------------------------------
// Coordinates: p indexes the un-cut overlap-add signal (frame t covers p = t*hop + left + j, j < win), i = p - start
// the kept signal [0, L) with start = n_fft/2.  The next transform's frame t, tap j reads the reflect-padded kept
// signal at u = t*hop + left + j -- the SAME coordinate as p -- so frames[t][j] = y[start + reflect(u - start)].
struct OlaGeom {
  int T, win, hop, left, start;
  int L;          // re-frame: length of the kept signal (reflect bounds); final: samples of it that exist (<= length)
  int R;          // frames (re-frame) or hop-sized chunks (final) a block owns
  int rows_cap;   // LDS rows reserved for staged inverse frames
};
struct OlaRange {
  int i_lo, i_hi;   // kept-signal samples the block needs (inclusive; empty when i_hi < i_lo)
  int t_lo, t_hi;   // inverse frames that reach them
};
__host__ __device__ inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__host__ __device__ inline int ceil_div(int a, int b) { return floor_div(a + b - 1, b); }
__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }

template <bool FINAL>
__host__ __device__ inline OlaRange ola_range(const OlaGeom& g, int blk) {
  OlaRange r;
  if (FINAL) {
    r.i_lo = blk * g.R * g.hop;
    r.i_hi = imin(r.i_lo + g.R * g.hop, g.L) - 1;
  } else {
    const int t0 = blk * g.R, t1 = imin(t0 + g.R, g.T) - 1;
    const int ilo = t0 * g.hop + g.left - g.start, ihi = t1 * g.hop + g.left + g.win - 1 - g.start;
    int lo = 0x7fffffff, hi = -1;
    if (imax(ilo, 0) <= imin(ihi, g.L - 1)) { lo = imax(ilo, 0); hi = imin(ihi, g.L - 1); }
    if (ilo < 0) {                                   // i in [ilo, min(ihi, -1)] reads -i
      lo = imin(lo, -imin(ihi, -1));
      hi = imax(hi, -ilo);
    }
    if (ihi >= g.L) {                                // i in [max(ilo, L), ihi] reads 2(L-1) - i
      lo = imin(lo, 2 * (g.L - 1) - ihi);
      hi = imax(hi, 2 * (g.L - 1) - imax(ilo, g.L));
    }
    r.i_lo = imax(lo, 0);
    r.i_hi = imin(hi, g.L - 1);
  }
  if (r.i_hi < r.i_lo) { r.t_lo = 0; r.t_hi = -1; return r; }
  r.t_lo = imax(0, ceil_div(g.start + r.i_lo - g.left - g.win + 1, g.hop));
  r.t_hi = imin(g.T - 1, floor_div(g.start + r.i_hi - g.left, g.hop));
  return r;
}

template <bool FINAL>
__global__ void __launch_bounds__(kGlBlock)
gl_ola_kernel(const float* __restrict__ fr, const float* __restrict__ renv, int n_renv, OlaGeom g, float* __restrict__ out,
              long long out_len, long long* __restrict__ advance) {
  extern __shared__ __align__(16) float lds[];
  float* rows = lds;                                 // [rows_cap][win] staged inverse frames
  float* ybuf = lds + g.rows_cap * g.win;            // the block's stretch of y
  const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const OlaRange r = ola_range<FINAL>(g, blk);
  const int nrows = imin(r.t_hi - r.t_lo + 1, g.rows_cap), ny = r.i_hi - r.i_lo + 1;
  if (nrows > 0) {                                   // consecutive frames of one clip are one contiguous stretch
    const f32x4* s4 = reinterpret_cast<const f32x4*>(fr + ((long long)b * g.T + r.t_lo) * g.win);
    f32x4* d4 = reinterpret_cast<f32x4*>(rows);
    for (int v = tid; v < nrows * (g.win / 4); v += kGlBlock) d4[v] = s4[v];
  }
  __syncthreads();
  for (int k = tid; k < ny; k += kGlBlock) {
    const int p = g.start + r.i_lo + k;
    const int ta = imax(r.t_lo, ceil_div(p - g.left - g.win + 1, g.hop));
    const int tb = imin(r.t_lo + nrows - 1, floor_div(p - g.left, g.hop));
    float acc = 0.f;
    for (int t = ta; t <= tb; ++t) acc += rows[(t - r.t_lo) * g.win + (p - t * g.hop - g.left)];   // ascending t
    ybuf[k] = acc * (p < n_renv ? renv[p] : 0.f);
  }
  __syncthreads();
  if (FINAL) {
    const long long i0 = (long long)blk * g.R * g.hop;
    const long long i1 = i0 + (long long)g.R * g.hop < out_len ? i0 + (long long)g.R * g.hop : out_len;
    for (long long i = i0 + tid; i < i1; i += kGlBlock) {
      const long long k = i - r.i_lo;
      out[(long long)b * out_len + i] = (k >= 0 && k < ny) ? ybuf[k] : 0.f;     // behind the signal's end: zero padding
    }
    if (advance && blk == 0 && b == 0 && tid == 0) advance[0] += 1;             // this call's phases are drawn: next key
  } else {
    const int t0 = blk * g.R, nfr = imin(t0 + g.R, g.T) - t0, wv = g.win / 4;
    for (int v = tid; v < nfr * wv; v += kGlBlock) {
      const int t = t0 + v / wv, j = (v % wv) * 4;
      const int ia = t * g.hop + g.left + j - g.start;
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = ia + c;
        const int k = (i < 0 ? -i : (i >= g.L ? 2 * (g.L - 1) - i : i)) - r.i_lo;
        o[c] = (unsigned)k < (unsigned)ny ? ybuf[k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(out + ((long long)b * g.T + t) * g.win + j) = o;
    }
  }
}

// LDS floats of a launch with R frames per block: the widest row and sample stretch any block needs
template <bool FINAL>
static size_t ola_lds_floats(OlaGeom& g, int nblk) {
  int rows = 1, ny = 1;
  for (int blk = 0; blk < nblk; ++blk) {
    const OlaRange r = ola_range<FINAL>(g, blk);
    rows = imax(rows, r.t_hi - r.t_lo + 1);
    ny = imax(ny, r.i_hi - r.i_lo + 1);
  }
  g.rows_cap = rows;
  return (size_t)rows * g.win + (size_t)((ny + 3) & ~3);
}

static bool gl_geom_ok(int n_fft, int win, int hop, int T) {
  return n_fft >= 2 && win >= 1 && win <= n_fft && hop >= 1 && hop <= win && T >= 1 &&
         (long long)n_fft + (long long)hop * (T - 1) < (1LL << 30);
}

}  // namespace ali

using namespace ali;

extern "C" int32_t ali_gl_check(int32_t n_fft, int32_t win, int32_t hop, int32_t T, int64_t length) {
  if (!gl_geom_ok(n_fft, win, hop, T)) {
    set_error("ali_gl_check: need 0 < hop_length <= win_length <= n_fft (got n_fft %d, win %d, hop %d, T %d)", n_fft, win, hop, T);
    return ALI_ERR_BAD_ARG;
  }
  const int left = (n_fft - win) / 2, start = n_fft / 2;
  const long long N = (long long)n_fft + (long long)hop * (T - 1);
  long long end = length > 0 ? start + length : N - start;
  if (end > N) end = N;
  const double kTwoPi = 6.283185307179586476925286766559;
  for (long long p = start; p < end; ++p) {
    double env = 0.0;
    const int ta = imax(0, ceil_div((int)p - left - win + 1, hop)), tb = imin(T - 1, floor_div((int)p - left, hop));
    for (int t = ta; t <= tb; ++t) {
      const double w = 0.5 - 0.5 * cos(kTwoPi * (double)(p - (long long)t * hop - left) / (double)win);
      env += w * w;
    }
    if (!(env > 1e-11)) return 0;
  }
  return 1;
}

extern "C" int ali_gl_init(const float* src, int32_t B, int32_t F, int32_t T, int32_t mode, const float* mean,
                           const float* stdv, float stds_kept, float power, const float* a0_re, const float* a0_im,
                           int32_t rand_init, uint64_t seed, const int64_t* dev_counter, uint64_t offset, float* mag,
                           float* X, ali_stream_t stream) {
  if (!src || !mag || !X || B <= 0 || F <= 0 || T <= 0 || B > 65535 || !(power > 0.f) || mode < ALI_GL_SRC_IMAGE ||
      mode > ALI_GL_SRC_SPEC || (mode == ALI_GL_SRC_IMAGE && (!mean || !stdv)) || (!a0_re != !a0_im)) {
    set_error("ali_gl_init: bad argument");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(gl_init_kernel, dim3((T + 31) / 32, (F + 31) / 32, B), dim3(kGlBlock), 0, ST(stream), src, F, T, mode,
                     mean, stdv, stds_kept, 1.f / power, a0_re, a0_im, rand_init, seed,
                     reinterpret_cast<const long long*>(dev_counter), offset, mag, X);
  return check_launch("gl_init_kernel");
}

extern "C" int ali_gl_phase(const float* Y, const float* tprev, const float* mag, float m, int64_t rows, int32_t F,
                            float* X, ali_stream_t stream) {
  if (!Y || !mag || !X || rows <= 0 || F <= 0 || (F & 3) || !(m >= 0.f && m < 1.f) ||
      ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(tprev) | reinterpret_cast<uintptr_t>(mag) |
        reinterpret_cast<uintptr_t>(X)) & 15)) {
    set_error("ali_gl_phase: bad argument (F %% 4 == 0, 16-byte aligned buffers, 0 <= m < 1)");
    return ALI_ERR_BAD_ARG;
  }
  const long long nvec = (long long)rows * (F / 4);
  long long grid = (nvec + kGlBlock - 1) / kGlBlock;
  if (grid > 8 * kNumCU) grid = 8 * kNumCU;
  hipLaunchKernelGGL(gl_phase_kernel, dim3((unsigned)grid), dim3(kGlBlock), 0, ST(stream), Y, m > 0.f ? tprev : nullptr,
                     mag, m, nvec, F / 4, X);
  return check_launch("gl_phase_kernel");
}

extern "C" int ali_gl_ola(const float* fr, const float* renv, int32_t n_renv, int32_t B, int32_t T, int32_t n_fft,
                          int32_t win, int32_t hop, int64_t length, int32_t final_wave, float* out,
                          int32_t frames_per_block, int64_t* advance, ali_stream_t stream) {
  if (!fr || !renv || !out || n_renv <= 0 || B <= 0 || B > 65535 || !gl_geom_ok(n_fft, win, hop, T) || (win & 3) ||
      length <= n_fft / 2 || length >= (1LL << 30) || frames_per_block < 0 ||
      ((reinterpret_cast<uintptr_t>(fr) | reinterpret_cast<uintptr_t>(out)) & 15)) {
    set_error("ali_gl_ola: bad argument (win %% 4 == 0, hop <= win <= n_fft, length > n_fft/2, 16-byte aligned buffers)");
    return ALI_ERR_BAD_ARG;
  }
  OlaGeom g;
  g.T = T; g.win = win; g.hop = hop; g.left = (n_fft - win) / 2; g.start = n_fft / 2;
  const long long avail = (long long)n_fft + (long long)hop * (T - 1) - g.start;    // samples of y behind `start`
  if (!final_wave && 1 + (length + 2 * g.start - n_fft) / hop != T) {
    set_error("ali_gl_ola: a signal of %lld samples has %lld frames, not %d", (long long)length,
              (long long)(1 + (length + 2 * g.start - n_fft) / hop), T);
    return ALI_ERR_BAD_ARG;
  }
  g.L = (int)(final_wave ? (length < avail ? length : avail) : length);
  const long long units = final_wave ? (length + hop - 1) / hop : T;      // what the blocks of one clip share out
  size_t floats = 0;
  int nblk = 0;
  for (int R = frames_per_block ? frames_per_block : 32; R >= 1; R >>= 1) {
    g.R = R;
    nblk = (int)((units + R - 1) / R);
    floats = final_wave ? ola_lds_floats<true>(g, nblk) : ola_lds_floats<false>(g, nblk);
    if (frames_per_block || floats * sizeof(float) <= (48u << 10)) break;
  }
  if (floats * sizeof(float) > (64u << 10)) {
    set_error("ali_gl_ola: %zu bytes of LDS for %d frames per block", floats * sizeof(float), g.R);
    return ALI_ERR_BAD_ARG;
  }
  if (final_wave)
    hipLaunchKernelGGL(gl_ola_kernel<true>, dim3(nblk, B), dim3(kGlBlock), floats * sizeof(float), ST(stream), fr, renv,
                       n_renv, g, out, (long long)length, reinterpret_cast<long long*>(advance));
  else
    hipLaunchKernelGGL(gl_ola_kernel<false>, dim3(nblk, B), dim3(kGlBlock), floats * sizeof(float), ST(stream), fr, renv,
                       n_renv, g, out, (long long)length, nullptr);
  return check_launch("gl_ola_kernel");
}
