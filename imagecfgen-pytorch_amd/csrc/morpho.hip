// The morphomnist family (include/ali_hip.h: ali_morpho_binarise, ali_morpho_edt, ali_morpho_thin, ali_morpho_measure):
// thickness, stroke length, area, intensity and slant of a batch of images, measured the way morphomnist/morpho.py
// (the statement, numpy / scipy in fp64) measures one image -- up-sample, binarise, exact Euclidean distance map,
// ordered thinning, sums over the skeleton -- without a host step in between.
//
// One workgroup owns one image in every kernel, so nothing crosses a block: no arrival counters, no atomics.
//   binarise  T = X AWt goes to the workspace ([H][W s] floats, s times smaller than the up-sampled image); the
//             up-sampled image itself is formed twice, 8 rows x 256 columns at a time, as 255 * AH T with explicit fmaf
//             (both passes give the same bits), and never stored: pass 1 reduces min, max and six fp64 moment sums,
//             pass 2 thresholds, packs 32 pixels to a word by wave ballot and counts.  The product is taken of the
//             image less its minimum (the plate goes back on the sums in fp64), so that an image in -1 .. 1 and the
//             same image in 0 .. 255 go through the same arithmetic.  A constant input is all foreground by definition.
//   edt       a thread per column finds the distance g to the nearest background pixel of the column (down, then up),
//             as uint16 in the workspace; then a thread per pixel takes min_j' (j - j')^2 + g(i, j')^2 over |j - j'| < g:
//             a candidate farther along the row than the column distance cannot win.  Integers throughout: exact.
//   thin      the statement visits the foreground in ascending key order and sets each pixel to keep[its current 3 x 3
//             neighbourhood].  A visit reads only the eight neighbours, so a pixel may be visited as soon as every
//             neighbour with a smaller key has been: by induction over the key order every pixel then sees exactly the
//             neighbourhood the sequential walk shows it.  The kernel runs rounds: (A) every undecided pixel whose
//             smaller-key neighbours are all decided is marked ready, barrier, (B) the ready pixels decide, barrier.
//             Two adjacent pixels are never ready in the same round (the larger of the two waits for the smaller), so
//             a ready pixel's neighbourhood does not change during (B).  Two bitmaps live in LDS, the current image
//             and the decided pixels (which takes the place of the initial image once the keys have been compared):
//             2 * 4 * H s * ceil(W s / 32) bytes, 64 KB at 512 x 512 and 49 KB at 448 x 448; the per-pixel
//             "which neighbours are smaller" byte is computed once, from d2, the initial neighbourhoods and the hash,
//             and kept in the workspace (each byte is written and read by one thread).  The undecided pixel with the
//             smallest key is always ready, so <= (foreground count) rounds suffice; the loop is capped there, and
//             also left when a round decides nothing: status 2.
//   measure   skeleton pixels, straight and diagonal neighbour pairs, the fp64 sum of sqrt(d2); on the input image
//             min, max, the median of the pixels >= the middle by radix selection on the ordered bit patterns (32
//             counting passes per order statistic: exact, and linear in the pixel count), and fp64 moments.
// The perturbation half (ali_morpho_reshape, ali_morpho_shear_reduce, ali_morpho_set_intensity; the statement is
// morphomnist/perturb.py) continues from the bitmap and the thickness these leave on the device:
//   reshape   SetThickness: the radius from the measured and the target thickness, then dilation / erosion by the
//             footprint's half widths through a per-row distance map (uint16 in the workspace, the bitmap in LDS).
//   shear_reduce  SetSlant as an exact fp64 shift per row, then downscale: T = warped RWt and 255 RH T in fp64, rounded
//             once, quantised with a guard of 1/128 grey level.
//   set_intensity  the median of the bright pixels by `measure`'s selection, q * (target / median) clipped to 0 .. 255.
// The local perturbations (ali_morpho_locate, ali_morpho_local; the statement is morphomnist/skeleton.py and the second
// half of morphomnist/perturb.py) are described in front of their kernels below, as are the bounding parallelogram
// (ali_morpho_bounds) and SetWidth (ali_morpho_width, ali_morpho_affine_reduce).
// Every sum runs in a fixed order (ali_reduce.h): the same inputs give the same bits on every run.
#include "ali_reduce.h"

namespace ali {

constexpr int kMoMaxSide = 512;                                      // H * scale and W * scale
constexpr int kMoBlock = 256;
constexpr int kMoWaves = kMoBlock / 64;
constexpr int kMoRows = 8;                                           // rows of the up-sampled image a thread forms at once
constexpr int kThinBlock = 1024;
constexpr int kThinWords = (kMoMaxSide * (kMoMaxSide / 32) + kThinBlock - 1) / kThinBlock;   // bitmap words per thread
constexpr uint32_t kNoBg = 0xFFFFu;                                  // column distance: no background in the column

struct KeepTable { uint32_t w[16]; };

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
template <int WAVES>
__device__ __forceinline__ int block_isum(int v, int* s) { return waves_sum<WAVES>(wave_isum(v), s); }

// bits x-1, x, x+1 of row y of a bitmap (bits 0..2); outside the image: 0
__device__ __forceinline__ uint32_t row3(const uint32_t* bm, int Hh, int wpr, int y, int x) {
  if (y < 0 || y >= Hh) return 0u;
  const uint32_t* r = bm + y * wpr;
  const int w = x >> 5, b = x & 31;
  uint64_t v = (uint64_t)r[w] << 1;
  if (b == 0 && w > 0) v |= r[w - 1] >> 31;
  if (b == 31 && w + 1 < wpr) v |= (uint64_t)(r[w + 1] & 1u) << 33;
  return (uint32_t)(v >> b) & 7u;
}
// the 3 x 3 neighbourhood of (y, x): bit 3 * r + c, centre at bit 4
__device__ __forceinline__ uint32_t nbhd(const uint32_t* bm, int Hh, int wpr, int y, int x) {
  return row3(bm, Hh, wpr, y - 1, x) | (row3(bm, Hh, wpr, y, x) << 3) | (row3(bm, Hh, wpr, y + 1, x) << 6);
}
// the bits of the last word of a row that lie inside the image
__device__ __forceinline__ uint32_t tail_mask(int w, int wpr, int Wh) {
  return ((w % wpr) == wpr - 1 && (Wh & 31)) ? (1u << (Wh & 31)) - 1u : 0xFFFFFFFFu;
}

// ------------------------------------------------------------------------------------------------------- binarise
template <bool EXPAND>
__global__ void __launch_bounds__(kMoBlock)
morpho_binarise_kernel(const float* __restrict__ x, long long ld, int H, int W, int s, const float* __restrict__ AH,
                       const float* __restrict__ AW, float threshold, float* __restrict__ T, uint32_t* __restrict__ bin,
                       int wpr, int* __restrict__ fg, double* __restrict__ hstats) {
  __shared__ float s_f[kMoWaves];
  __shared__ double s_d[kMoWaves];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Hh = H * s, Wh = W * s;
  const float* X = x + (long long)b * ld;
  float* Tb = T + (long long)b * H * Wh;
  // The input's minimum comes off before the product and goes back on, in fp64, when the sums are written (the
  // operator's rows sum to 1: a plate stays a plate).  The background of an image in -1 .. 1 is then formed as 0, not as
  // -255 through operators rounded to fp32 -- the same arithmetic as for the same image in 0 .. 255.  A constant input
  // is all foreground: its up-sampled image is constant too, and what rounding leaves of it is not thresholded.
  float xmn = INFINITY, xmx = -INFINITY;
  for (int e = tid; e < H * W; e += kMoBlock) {
    xmn = fminf(xmn, X[e]);
    xmx = fmaxf(xmx, X[e]);
  }
  xmx = block_max<kMoWaves>(xmx, s_f);
  xmn = -block_max<kMoWaves>(-xmn, s_f);
  const bool flat = xmn == xmx;
  if (EXPAND) {
    for (int e = tid; e < H * Wh; e += kMoBlock) {
      const int r = e / Wh, j = e % Wh;
      float acc = 0.f;
      for (int c = 0; c < W; ++c) acc = fmaf(X[r * W + c] - xmn, AW[j * W + c], acc);
      Tb[e] = acc;
    }
    __syncthreads();                                                 // (the block reads what the block wrote)
  }
  // rows i0 .. i0 + 7 of column j of the up-sampled image
  auto tile = [&](int i0, int j, float (&v)[kMoRows]) {
    if (!EXPAND) {
#pragma unroll
      for (int k = 0; k < kMoRows; ++k) v[k] = i0 + k < Hh ? X[(i0 + k) * W + j] : 0.f;
      return;
    }
    float acc[kMoRows];
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) acc[k] = 0.f;
    for (int r = 0; r < H; ++r) {
      const float t = Tb[r * Wh + j];
#pragma unroll
      for (int k = 0; k < kMoRows; ++k) {
        const int i = i0 + k < Hh ? i0 + k : Hh - 1;                 // (uniform in the block)
        acc[k] = fmaf(AH[i * H + r], t, acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) v[k] = 255.f * acc[k];
  };

  float mn = INFINITY, mx = -INFINITY;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < Hh; i0 += kMoRows)
    for (int j = tid; j < Wh; j += kMoBlock) {
      float v[kMoRows];
      tile(i0, j, v);
#pragma unroll
      for (int k = 0; k < kMoRows; ++k) {
        if (i0 + k >= Hh) break;
        mn = fminf(mn, v[k]);
        mx = fmaxf(mx, v[k]);
        const double d = (double)v[k], xx = (double)j, yy = (double)(i0 + k);
        m[0] += d; m[1] += xx * d; m[2] += yy * d; m[3] += xx * xx * d; m[4] += xx * yy * d; m[5] += yy * yy * d;
      }
    }
  mx = block_max<kMoWaves>(mx, s_f);
  mn = -block_max<kMoWaves>(-mn, s_f);
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = block_sum<kMoWaves>(m[q], s_d);
  if (tid == 0) {
    double* hs = hstats + (long long)b * 8;
    const double plate = EXPAND ? 255.0 * (double)xmn : 0.0, Hn = (double)Hh, Wn = (double)Wh;
    const double sx = Wn * (Wn - 1.0) / 2.0, sy = Hn * (Hn - 1.0) / 2.0;
    const double sxx = (Wn - 1.0) * Wn * (2.0 * Wn - 1.0) / 6.0, syy = (Hn - 1.0) * Hn * (2.0 * Hn - 1.0) / 6.0;
    const double grid[6] = {Hn * Wn, Hn * sx, Wn * sy, Hn * sxx, sx * sy, Wn * syy};   // the sums of a plate of 1
    hs[0] = (double)mn + plate; hs[1] = (double)mx + plate;
#pragma unroll
    for (int q = 0; q < 6; ++q) hs[2 + q] = m[q] + plate * grid[q];
  }
  const float thr = mn + (mx - mn) * threshold;
  uint32_t* out = bin + (long long)b * Hh * wpr;
  int count = 0;                                                     // per wave: every lane holds the wave's count
  for (int i0 = 0; i0 < Hh; i0 += kMoRows)
    for (int j0 = 0; j0 < Wh; j0 += kMoBlock) {                      // (uniform trip count: every lane reaches the ballot)
      const int j = j0 + tid;
      float v[kMoRows];
      if (j < Wh) tile(i0, j, v);
      const int w0 = (j0 + (tid & ~63)) >> 5;
#pragma unroll
      for (int k = 0; k < kMoRows; ++k) {
        if (i0 + k >= Hh) break;
        const unsigned long long bits = __ballot(j < Wh && (flat || v[k] >= thr));
        count += __popcll(bits);
        uint32_t* row = out + (i0 + k) * wpr;
        if ((tid & 63) == 0 && w0 < wpr) row[w0] = (uint32_t)bits;
        if ((tid & 63) == 32 && w0 + 1 < wpr) row[w0 + 1] = (uint32_t)(bits >> 32);
      }
    }
  count = waves_sum<kMoWaves>(count, s_i);
  if (tid == 0) fg[b] = count;
}

// ------------------------------------------------------------------------------------------------------------ edt
__global__ void __launch_bounds__(kMoBlock)
morpho_edt_kernel(const uint32_t* __restrict__ bin, int Hh, int Wh, int wpr, uint16_t* __restrict__ G,
                  int* __restrict__ d2, int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* bm = bin + (long long)b * Hh * wpr;
  uint16_t* g = G + (long long)b * Hh * Wh;
  int* out = d2 + (long long)b * Hh * Wh;
  int any_bg = 0;
  for (int j = tid; j < Wh; j += kMoBlock) {
    int last = -1;
    for (int i = 0; i < Hh; ++i) {
      if (!((bm[i * wpr + (j >> 5)] >> (j & 31)) & 1u)) last = i;
      g[i * Wh + j] = (uint16_t)(last < 0 ? kNoBg : (uint32_t)(i - last));
    }
    any_bg |= last >= 0;
    last = -1;
    for (int i = Hh - 1; i >= 0; --i) {
      if (!((bm[i * wpr + (j >> 5)] >> (j & 31)) & 1u)) last = i;
      const uint32_t up = last < 0 ? kNoBg : (uint32_t)(last - i);
      if (up < g[i * Wh + j]) g[i * Wh + j] = (uint16_t)up;
    }
  }
  const int has_bg = __syncthreads_or(any_bg);                       // (and the column distances are the block's to read)
  if (tid == 0) status[b] = has_bg ? 0 : 1;
  if (!has_bg) return;                                               // no background anywhere: d2 stays undefined
  for (int e = tid; e < Hh * Wh; e += kMoBlock) {
    const int i = e / Wh, j = e % Wh;
    const uint32_t gc = g[e];
    int best = 0;
    if (gc != 0) {
      const bool open = gc == kNoBg;                                 // no background in this column: the whole row
      best = open ? 0x7FFFFFFF : (int)(gc * gc);
      const int reach = open ? Wh : (int)gc - 1;
      const uint16_t* row = g + i * Wh;
      for (int dj = 1; dj <= reach && dj * dj < best; ++dj) {
        if (j - dj >= 0) {
          const uint32_t q = row[j - dj];
          if (q != kNoBg) best = min(best, (int)(q * q) + dj * dj);
        }
        if (j + dj < Wh) {
          const uint32_t q = row[j + dj];
          if (q != kNoBg) best = min(best, (int)(q * q) + dj * dj);
        }
      }
    }
    out[e] = best;
  }
}

// ----------------------------------------------------------------------------------------------------------- thin
__global__ void __launch_bounds__(kThinBlock)
morpho_thin_kernel(const uint32_t* __restrict__ bin, const int* __restrict__ d2, int Hh, int Wh, int wpr, uint64_t seed,
                   KeepTable keep, uint8_t* __restrict__ less_ws, const int* __restrict__ fg,
                   uint32_t* __restrict__ skel, int* __restrict__ status) {
  extern __shared__ uint32_t s_bm[];
  __shared__ uint32_t s_keep[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nw = Hh * wpr;                                           // <= kThinWords * kThinBlock
  uint32_t* init = s_bm;                                             // the input, until the keys are compared; then
  uint32_t* dec = s_bm;                                              // decided, or not foreground: ~init to begin with
  uint32_t* cur = s_bm + nw;
  const uint32_t* bm = bin + (long long)b * nw;
  const int* D = d2 + (long long)b * Hh * Wh;
  uint8_t* L = less_ws + (long long)b * Hh * Wh;
  const int st = status[b];
  if (tid < 16) s_keep[tid] = keep.w[tid];
  for (int w = tid; w < nw; w += kThinBlock) {
    const uint32_t v = st == 0 ? bm[w] & tail_mask(w, wpr, Wh) : 0u; // (an image without background has no skeleton)
    init[w] = v;
    cur[w] = v;
  }
  __syncthreads();
  // which neighbours come before a pixel: the key (d2, corner, tiebreak, linear index), compared lazily
  const uint64_t key = thin_key(rng_base_key(seed, nullptr));
  for (int w = tid; w < nw; w += kThinBlock) {
    uint32_t u = init[w];
    const int y = w / wpr, x0 = (w % wpr) * 32;
    while (u) {
      const int bit = __ffs(u) - 1;
      u &= u - 1;
      const int x = x0 + bit, lin = y * Wh + x;
      const uint32_t nb = nbhd(init, Hh, wpr, y, x);
      const int d = D[lin], c = 9 - __popc(nb);
      uint32_t less = 0;
#pragma unroll
      for (int n = 0; n < 9; ++n) {
        if (n == 4 || !((nb >> n) & 1u)) continue;
        const int qy = y + n / 3 - 1, qx = x + n % 3 - 1, ql = qy * Wh + qx;
        const int qd = D[ql];
        bool lt;
        if (qd != d) {
          lt = qd < d;
        } else {
          const int qc = 9 - __popc(nbhd(init, Hh, wpr, qy, qx));
          if (qc != c) {
            lt = qc < c;
          } else {
            const uint32_t qt = hi24(hash_at(key, (uint64_t)ql)), pt = hi24(hash_at(key, (uint64_t)lin));
            lt = qt != pt ? qt < pt : ql < lin;
          }
        }
        if (lt) less |= 1u << (n < 4 ? n : n - 1);
      }
      L[lin] = (uint8_t)less;
    }
  }
  __syncthreads();                                                   // (every neighbourhood of `init` has been read)
  for (int w = tid; w < nw; w += kThinBlock) dec[w] = ~init[w];
  __syncthreads();
  const int cap = fg[b];
  int stuck = 0, left = 0;
  for (int round = 0; round < cap; ++round) {
    uint32_t ready[kThinWords];
#pragma unroll
    for (int k = 0; k < kThinWords; ++k) {
      const int w = tid + k * kThinBlock;
      ready[k] = 0u;
      if (w >= nw) continue;
      uint32_t u = ~dec[w];
      const int y = w / wpr, x0 = (w % wpr) * 32;
      while (u) {
        const int bit = __ffs(u) - 1;
        u &= u - 1;
        const uint32_t dn = nbhd(dec, Hh, wpr, y, x0 + bit);
        const uint32_t have = (dn & 15u) | ((dn >> 5) << 4);
        if (!((uint32_t)L[y * Wh + x0 + bit] & ~have)) ready[k] |= 1u << bit;
      }
    }
    __syncthreads();                                                 // (A) read `dec`; (B) writes it
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kThinWords; ++k) {
      const int w = tid + k * kThinBlock;
      if (w >= nw) continue;
      uint32_t r = ready[k], clear = 0u;
      const int y = w / wpr, x0 = (w % wpr) * 32;
      while (r) {
        const int bit = __ffs(r) - 1;
        r &= r - 1;
        const uint32_t idx = nbhd(cur, Hh, wpr, y, x0 + bit);
        if (!((s_keep[idx >> 5] >> (idx & 31)) & 1u)) clear |= 1u << bit;
      }
      if (ready[k]) {
        cur[w] &= ~clear;                                            // (this thread is the only writer of word w)
        dec[w] |= ready[k];
        mine |= 2;
      }
      if (~dec[w]) mine |= 1;
    }
    left = __syncthreads_or(mine & 1);                               // (a predicate: any thread, not a bitwise or)
    const int moved = __syncthreads_or(mine & 2);
    if (!left) break;
    if (!moved) { stuck = 1; break; }                                // (cannot happen: the smallest key is always ready)
  }
  for (int w = tid; w < nw; w += kThinBlock) skel[(long long)b * nw + w] = cur[w];
  if (tid == 0 && (stuck || left)) status[b] = 2;
}

// -------------------------------------------------------------------------------------------------------- measure
// floats as unsigned integers in the same order
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float from_ordered_bits(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k);
}

// the k-th smallest (from 0) of the pixels >= thr: one counting pass per bit, from the top
__device__ float select_kth(const float* X, int N, double thr, int k, int* s_i) {
  uint32_t prefix = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t above = bit == 31 ? 0u : ~((2u << bit) - 1u);
    int cnt = 0;
    for (int e = threadIdx.x; e < N; e += kMoBlock) {
      const float v = X[e];
      const uint32_t kb = ordered_bits(v);
      cnt += (double)v >= thr && (kb & above) == prefix && !((kb >> bit) & 1u);
    }
    cnt = block_isum<kMoWaves>(cnt, s_i);
    if (k >= cnt) {
      k -= cnt;
      prefix |= 1u << bit;
    }
  }
  return from_ordered_bits(prefix);
}

__global__ void __launch_bounds__(kMoBlock)
morpho_measure_kernel(const float* __restrict__ x, long long ld, int H, int W, int s, const uint32_t* __restrict__ skel,
                      const int* __restrict__ d2, int wpr, const int* __restrict__ fg, const double* __restrict__ hstats,
                      const int* __restrict__ status, int* __restrict__ counts, float* __restrict__ values,
                      float* __restrict__ slant) {
  __shared__ float s_f[kMoWaves];
  __shared__ double s_d[kMoWaves];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Hh = H * s, Wh = W * s, nw = Hh * wpr;
  const uint32_t* sk = skel + (long long)b * nw;
  const int* D = d2 + (long long)b * Hh * Wh;
  const int st = status[b];
  int n_sk = 0, n_st = 0, n_dg = 0;
  double sum_d = 0.0;
  for (int w = tid; w < nw; w += kMoBlock) {
    uint32_t u = sk[w] & tail_mask(w, wpr, Wh);
    const int y = w / wpr, x0 = (w % wpr) * 32;
    while (u) {
      const int bit = __ffs(u) - 1;
      u &= u - 1;
      const int xx = x0 + bit;
      const uint32_t here = row3(sk, Hh, wpr, y, xx), below = row3(sk, Hh, wpr, y + 1, xx);
      n_sk += 1;
      n_st += (int)((here >> 2) & 1u) + (int)((below >> 1) & 1u);    // right, below
      n_dg += (int)(below & 1u) + (int)((below >> 2) & 1u);          // below-left, below-right
      sum_d += sqrt((double)D[y * Wh + xx]);
    }
  }
  n_sk = block_isum<kMoWaves>(n_sk, s_i);
  n_st = block_isum<kMoWaves>(n_st, s_i);
  n_dg = block_isum<kMoWaves>(n_dg, s_i);
  sum_d = block_sum<kMoWaves>(sum_d, s_d);

  // the input image: min, max, moments
  const float* X = x + (long long)b * ld;
  const int N = H * W;
  float mn = INFINITY, mx = -INFINITY;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int e = tid; e < N; e += kMoBlock) {
    const float v = X[e];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    const double d = (double)v, xx = (double)(e % W), yy = (double)(e / W);
    m[0] += d; m[1] += xx * d; m[2] += yy * d; m[3] += xx * xx * d; m[4] += xx * yy * d; m[5] += yy * yy * d;
  }
  mx = block_max<kMoWaves>(mx, s_f);
  mn = -block_max<kMoWaves>(-mn, s_f);
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = block_sum<kMoWaves>(m[q], s_d);
  const double thr = (double)mn + ((double)mx - (double)mn) * 0.5;
  int n_sel = 0;
  for (int e = tid; e < N; e += kMoBlock) n_sel += (double)X[e] >= thr;
  n_sel = block_isum<kMoWaves>(n_sel, s_i);
  const float nan = __int_as_float(0x7fc00000);
  float intensity = nan;                                             // (NaN pixels: nothing is >= the middle)
  if (n_sel > 0) {                                                   // (uniform)
    const float hi = select_kth(X, N, thr, n_sel / 2, s_i);
    intensity = hi;
    if (!(n_sel & 1)) {
      const float lo = select_kth(X, N, thr, n_sel / 2 - 1, s_i);
      intensity = (float)(((double)lo + (double)hi) * 0.5);
    }
  }
  if (tid != 0) return;
  // -u11 / u02 of an Hn x Wn image less its minimum, from the raw sums q = (1, x, y, xx, xy, yy) of the image: the
  // sums of a constant plate are closed forms, exact in fp64
  auto shear = [](const double* q, double lo, double Hn, double Wn) {
    const double sx = Wn * (Wn - 1.0) / 2.0, sy = Hn * (Hn - 1.0) / 2.0;
    const double syy = (Hn - 1.0) * Hn * (2.0 * Hn - 1.0) / 6.0;
    const double m00 = q[0] - lo * Hn * Wn;
    const double m10 = (q[1] - lo * Hn * sx) / m00, m01 = (q[2] - lo * Wn * sy) / m00;
    const double u11 = (q[4] - lo * sx * sy) / m00 - m10 * m01, u02 = (q[5] - lo * Wn * syy) / m00 - m01 * m01;
    return -u11 / u02;
  };
  const bool ok = st == 0;
  const double ds = (double)s;
  int* c = counts + (long long)b * 4;
  c[0] = fg[b]; c[1] = n_sk; c[2] = n_st; c[3] = n_dg;
  float* v = values + (long long)b * 5;
  v[0] = ok ? (float)((double)fg[b] / (ds * ds)) : nan;
  v[1] = ok ? (float)(((double)n_st + sqrt(2.0) * (double)n_dg) / ds) : nan;
  v[2] = ok && n_sk > 0 ? (float)(2.0 * (sum_d / (double)n_sk) / ds) : nan;
  v[3] = intensity;
  v[4] = (float)shear(m, (double)mn, (double)H, (double)W);
  const double* hs = hstats + (long long)b * 8;
  slant[b] = (float)atan(shear(hs + 2, hs[0], (double)Hh, (double)Wh));
}

// -------------------------------------------------------------------------------------------------------- reshape
constexpr int kMoMaxRadius = 64;
constexpr int kMoStuck = 4;                                          // status: nothing left to work with
constexpr int kMoTooFar = 3;                                         // status: radius > max_radius

__device__ __forceinline__ long long wave_lsum(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// SetThickness on the bitmaps: flat dilation (erosion: of the complement, complemented) by the footprint of the radius
// the kernel forms itself from the measured and the target thickness.  A footprint is its half widths (every row one
// centred run), so out(y, x) = any_dy hd(y + dy, x) <= half[dy], hd the distance along the row to the nearest set
// pixel: uint16 in the workspace (the bitmap is in LDS, the 2-byte map of 448 x 448 would not fit), one coalesced read
// per (pixel, dy) whatever the half width is, where OR-ing shifted rows costs 2 half + 1 word shifts.  Distances are
// looked for two words to either side: a pixel in the third word is 65 or more away, above every half width (<= 64).
__global__ void __launch_bounds__(kMoBlock)
morpho_reshape_kernel(const uint32_t* __restrict__ bin, const float* __restrict__ thickness, long long thick_ld,
                      const float* __restrict__ target, const int* __restrict__ status_in,
                      const int16_t* __restrict__ half, int max_radius, int Hh, int Wh, int wpr, int scale,
                      uint16_t* __restrict__ HD, uint32_t* __restrict__ out, int* __restrict__ radius,
                      long long* __restrict__ sums, int* __restrict__ status_out) {
  __shared__ uint32_t s_bm[kMoMaxSide * (kMoMaxSide / 32)];
  __shared__ int s_half[2 * kMoMaxRadius + 1];
  __shared__ long long s_l[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x, nw = Hh * wpr;
  const uint32_t* bm = bin + (long long)b * nw;
  uint32_t* ob = out + (long long)b * nw;
  uint16_t* hd = HD + (long long)b * Hh * Wh;
  const float thick = thickness[(long long)b * thick_ld];
  const double delta = (double)(target ? target[b] : thick) - (double)thick;
  int st = status_in[b], r = 0;
  if (st == 0) {
    if (delta != delta) {
      st = kMoStuck;                                                 // NaN thickness: no skeleton
    } else {
      r = (int)fmin((double)scale * fabs(delta) / 2.0, 1073741824.0);
      if (r > max_radius) st = kMoTooFar;
    }
  }
  const bool erode = delta < 0.0;
  if (st != 0) {                                                     // (uniform)
    for (int w = tid; w < nw; w += kMoBlock) ob[w] = 0u;
    if (tid == 0) {
      radius[b] = st == kMoTooFar ? (erode ? -r : r) : 0;
      status_out[b] = st;
      for (int q = 0; q < 6; ++q) sums[(long long)b * 6 + q] = 0;
    }
    return;
  }
  for (int w = tid; w < nw; w += kMoBlock) s_bm[w] = (erode ? ~bm[w] : bm[w]) & tail_mask(w, wpr, Wh);
  const int16_t* hrow = half + (long long)r * (2 * max_radius + 1);
  for (int k = tid; k <= 2 * r; k += kMoBlock) s_half[k] = hrow[k];
  __syncthreads();
  for (int e = tid; e < Hh * Wh; e += kMoBlock) {
    const int y = e / Wh, x = e % Wh, w = x >> 5, bit = x & 31;
    const uint32_t* row = s_bm + y * wpr;
    uint32_t d = kNoBg;
    uint32_t v = row[w] & (0xFFFFFFFFu >> (31 - bit));               // the bits at or left of x
    if (v) {
      d = (uint32_t)(bit - (31 - __clz(v)));
    } else {
      for (int k = 1; k <= 2 && w - k >= 0; ++k)
        if ((v = row[w - k]) != 0u) {
          d = (uint32_t)(x - ((w - k) * 32 + 31 - __clz(v)));
          break;
        }
    }
    v = row[w] & (0xFFFFFFFFu << bit);                               // at or right of x
    if (v) {
      d = min(d, (uint32_t)(__ffs(v) - 1 - bit));
    } else {
      for (int k = 1; k <= 2 && w + k < wpr; ++k)
        if ((v = row[w + k]) != 0u) {
          d = min(d, (uint32_t)((w + k) * 32 + __ffs(v) - 1 - x));
          break;
        }
    }
    hd[e] = (uint16_t)d;
  }
  __syncthreads();                                                   // (the block reads what the block wrote)
  long long m[6] = {0, 0, 0, 0, 0, 0};
  for (int y = 0; y < Hh; ++y) {
    const int lo = max(-r, -y), hi = min(r, Hh - 1 - y);
    for (int j0 = 0; j0 < Wh; j0 += kMoBlock) {                      // (uniform trip count: every lane reaches the ballot)
      const int j = j0 + tid;
      bool hit = false;
      if (j < Wh)
        for (int dy = lo; dy <= hi && !hit; ++dy) hit = (int)hd[(y + dy) * Wh + j] <= s_half[dy + r];
      const bool set = j < Wh && (hit != erode);
      const unsigned long long bits = __ballot(set);
      const int w0 = (j0 + (tid & ~63)) >> 5;
      if ((tid & 63) == 0 && w0 < wpr) ob[y * wpr + w0] = (uint32_t)bits;
      if ((tid & 63) == 32 && w0 + 1 < wpr) ob[y * wpr + w0 + 1] = (uint32_t)(bits >> 32);
      if (set) {
        const long long xx = j, yy = y;
        m[0] += 1; m[1] += xx; m[2] += yy; m[3] += xx * xx; m[4] += xx * yy; m[5] += yy * yy;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = waves_sum<kMoWaves>(wave_lsum(m[q]), s_l);
  if (m[0] == 0 || m[0] * m[5] == m[2] * m[2]) {                     // nothing left, or one row (u02 == 0): uniform
    for (int w = tid; w < nw; w += kMoBlock) ob[w] = 0u;             // (behind the barriers of the sums)
#pragma unroll
    for (int q = 0; q < 6; ++q) m[q] = 0;
    st = kMoStuck;
  }
  if (tid == 0) {
    radius[b] = erode ? -r : r;
    status_out[b] = st;
    for (int q = 0; q < 6; ++q) sums[(long long)b * 6 + q] = m[q];
  }
}

// --------------------------------------------------------------------------------------------------- shear, reduce
// u11 / u02 and the centroid row of a bitmap from its integer sums, and a row's shift, in fp64 with every operation
// rounded on its own (no contraction): the bits numpy forms
__device__ void shear_of_sums(const long long* q, double* shear, double* cy) {
#pragma clang fp contract(off)
  const double n = (double)q[0], sx = (double)q[1], sy = (double)q[2], sxy = (double)q[4], syy = (double)q[5];
  const double m10 = sx / n, m01 = sy / n;
  const double a = sxy / n, bb = m10 * m01, c = syy / n, d = m01 * m01;
  const double u11 = a - bb, u02 = c - d;
  *shear = u11 / u02;
  *cy = m01;
}
__device__ int row_shift(double delta, double cy, int y, int Wh) {
#pragma clang fp contract(off)
  const double dy = (double)y - cy;
  const double t = delta * dy;
  const double f = floor(0.5 - t);
  return (int)fmin(fmax(f, -(double)Wh), (double)Wh);
}

// downscale of the warped bitmap s_w (LDS, pad bits 0) of one image by the whole block: T = warped RWt into Tb (a sum
// over the set pixels of a row, ascending), raw = 255 * RH T rounded to fp32 once, Q = floor(clip(raw, 0, 255) + 2^-7).
// Shared by ali_morpho_shear_reduce and ali_morpho_affine_reduce.  Returns whether this thread wrote a Q above 0.
__device__ __forceinline__ bool reduce_warped(const uint32_t* s_w, int H, int W, int s, int wpr,
                                              const double* __restrict__ RH, const double* __restrict__ RW,
                                              double* __restrict__ Tb, float* __restrict__ Q, float* __restrict__ raw) {
  const int tid = threadIdx.x, Hh = H * s, Wh = W * s, N = H * W;
  bool any = false;
  if (s > 1) {
    for (int e = tid; e < Hh * W; e += kMoBlock) {
      const int y = e / W, c = e % W;
      const double* rw = RW + (long long)c * Wh;
      double acc = 0.0;
      for (int w = 0; w < wpr; ++w) {
        uint32_t u = s_w[y * wpr + w];
        while (u) {
          const int bit = __ffs(u) - 1;
          u &= u - 1;
          acc += rw[32 * w + bit];
        }
      }
      Tb[e] = acc;
    }
    __syncthreads();                                                 // (the block reads what the block wrote)
  }
  for (int e = tid; e < N; e += kMoBlock) {
    const int i = e / W, c = e % W;
    double acc;
    if (s > 1) {
      acc = 0.0;
      const double* rh = RH + (long long)i * Hh;
      for (int y = 0; y < Hh; ++y) acc = fma(rh[y], Tb[y * W + c], acc);
    } else {
      acc = (double)((s_w[i * wpr + (c >> 5)] >> (c & 31)) & 1u);
    }
    const float v = (float)(255.0 * acc);
    if (raw) raw[e] = v;
    const float q = floorf(fminf(fmaxf(v, 0.f), 255.f) + 0.0078125f);
    Q[e] = q;
    any = any || q > 0.f;
  }
  return any;
}

// SetSlant and downscale: the bitmap sheared row by row (nearest neighbour, 0 outside) into LDS, T = warped RWt into
// the workspace (a sum over the set pixels of a row, ascending), raw = 255 * RH T rounded to fp32 once, q =
// floor(clip(raw, 0, 255) + 2^-7) in fp32.  Operators, T and both sums are fp64: the rows of the reduce operator have
// lobes of both signs, and where they cancel an operator rounded to fp32 alone leaves an error of thousands of ulps
// of the pixel -- as large as the fp32 statement's whole error, which is the yardstick the tests hold this kernel to.
__global__ void __launch_bounds__(kMoBlock)
morpho_shear_reduce_kernel(const uint32_t* __restrict__ bin, const long long* __restrict__ sums,
                           const double* __restrict__ target_shear, const int* __restrict__ status, int H, int W, int s,
                           int wpr, const double* __restrict__ RH, const double* __restrict__ RW, double* __restrict__ T,
                           float* __restrict__ qout, float* __restrict__ raw, int* __restrict__ shifts,
                           double* __restrict__ shear_out) {
  __shared__ uint32_t s_w[kMoMaxSide * (kMoMaxSide / 32)];
  __shared__ int s_shift[kMoMaxSide];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Hh = H * s, Wh = W * s, nw = Hh * wpr, N = H * W;
  float* Q = qout + (long long)b * N;
  if (status[b] != 0) {                                              // (uniform)
    for (int e = tid; e < N; e += kMoBlock) {
      Q[e] = 0.f;
      if (raw) raw[(long long)b * N + e] = 0.f;
    }
    if (shifts)
      for (int y = tid; y < Hh; y += kMoBlock) shifts[(long long)b * Hh + y] = 0;
    if (tid == 0) shear_out[b] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  double shear, cy;
  shear_of_sums(sums + (long long)b * 6, &shear, &cy);
  const double delta = target_shear ? __dsub_rn(target_shear[b], shear) : 0.0;
  if (tid == 0) shear_out[b] = shear;
  for (int y = tid; y < Hh; y += kMoBlock) {
    const int sh = row_shift(delta, cy, y, Wh);
    s_shift[y] = sh;
    if (shifts) shifts[(long long)b * Hh + y] = sh;
  }
  __syncthreads();
  const uint32_t* bm = bin + (long long)b * nw;
  for (int e = tid; e < nw; e += kMoBlock) {
    const int y = e / wpr, w = e % wpr;
    const int p = 32 * w + s_shift[y];                               // the source column of bit 0
    const int k = p >> 5, off = p & 31;                              // (floor: p may be negative)
    const uint32_t* row = bm + y * wpr;
    const uint64_t lo = k >= 0 && k < wpr ? row[k] & tail_mask(k, wpr, Wh) : 0u;
    const uint64_t hi = k + 1 >= 0 && k + 1 < wpr ? row[k + 1] & tail_mask(k + 1, wpr, Wh) : 0u;
    s_w[e] = (uint32_t)(((hi << 32) | lo) >> off) & tail_mask(w, wpr, Wh);
  }
  __syncthreads();
  reduce_warped(s_w, H, W, s, wpr, RH, RW, T + (long long)b * Hh * W, Q, raw ? raw + (long long)b * N : nullptr);
}

// ------------------------------------------------------------------------------------------------------ intensity
// SetIntensity on the quantised image: the median of the pixels in the upper half of its range (the selection of
// `measure`), factor = target / median and the product in fp32, clipped to 0 .. 255.  An image that is 0 everywhere
// gets status 4; an image with a status is written as 0.
__global__ void __launch_bounds__(kMoBlock)
morpho_set_intensity_kernel(const float* __restrict__ q, const float* __restrict__ target,
                            const int* __restrict__ status_in, int N, float* __restrict__ out,
                            float* __restrict__ median, int* __restrict__ status_out) {
  __shared__ float s_f[kMoWaves];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* X = q + (long long)b * N;
  float* O = out + (long long)b * N;
  float mn = INFINITY, mx = -INFINITY;
  for (int e = tid; e < N; e += kMoBlock) {
    mn = fminf(mn, X[e]);
    mx = fmaxf(mx, X[e]);
  }
  mx = block_max<kMoWaves>(mx, s_f);
  mn = -block_max<kMoWaves>(-mn, s_f);
  int st = status_in[b];
  if (st == 0 && !(mx > 0.f)) st = kMoStuck;
  const float nan = __int_as_float(0x7fc00000);
  if (st != 0) {                                                     // (uniform)
    for (int e = tid; e < N; e += kMoBlock) O[e] = 0.f;
    if (tid == 0) {
      median[b] = nan;
      status_out[b] = st;
    }
    return;
  }
  const double thr = (double)mn + ((double)mx - (double)mn) * 0.5;
  int n_sel = 0;
  for (int e = tid; e < N; e += kMoBlock) n_sel += (double)X[e] >= thr;
  n_sel = block_isum<kMoWaves>(n_sel, s_i);                          // (>= 1: the maximum is selected)
  float med = select_kth(X, N, thr, n_sel / 2, s_i);
  if (!(n_sel & 1)) {
    const float lo = select_kth(X, N, thr, n_sel / 2 - 1, s_i);
    med = (float)(((double)lo + (double)med) * 0.5);
  }
  if (target) {
    const float mult = target[b] / med;
    for (int e = tid; e < N; e += kMoBlock) O[e] = fminf(fmaxf(X[e] * mult, 0.f), 255.f);
  } else {
    for (int e = tid; e < N; e += kMoBlock) O[e] = X[e];
  }
  if (tid == 0) {
    median[b] = med;
    status_out[b] = 0;
  }
}

// ---------------------------------------------------------------------------------------------- locate and local
// The Morpho-MNIST local perturbations (ali_morpho_locate, ali_morpho_local; the statement is morphomnist/skeleton.py
// and the second half of morphomnist/perturb.py): plain, thinning, thickening, swelling and fracture of the bitmaps,
// from the distance map and the skeleton the measurement kernels left on the device.
//   locate    two bitmaps in LDS, the skeleton the seeds are read from and the one the disks around them are cleared in
//             (integer atomicAnd on LDS words: the result does not depend on the order).  Tips are found on the
//             skeleton, forks on what the first erase left.  Candidates are counted per row; draw k is the
//             ((hi24 * n) >> 24)-th set pixel in row-major order.  For a fracture the block then takes the six integer
//             sums of the skeleton in the window around each centre, and thread 0 forms direction and end points in
//             fp64 with every operation rounded on its own.
//   local     the new bitmap is built in LDS by kind -- copy, d2 > r^2, !(d2c > r^2), the gather of the radial warp, or
//             the bitmap less a disk around every pixel of every line -- then written with its six moment sums (what
//             ali_morpho_shear_reduce takes for the low-resolution image).
constexpr int kMoDraws = 8;                                          // MAX_DRAWS of ali_hip/rng.py
constexpr int kMoStampMax = 1024;                                    // a disk radius above the diagonal of any image
constexpr double kMoRadiusLimit = 32768.0;                           // RADIUS_LIMIT of morphomnist/perturb.py
enum { kMoPlain = 0, kMoThin = 1, kMoThick = 2, kMoSwell = 3, kMoFracture = 4 };

struct LocalParams {
  double thin_amount, thick_amount, swell_exponent, swell_radius;
  int frac_r, n_frac;
};

// floor(sqrt(v)), 0 <= v <= 2^21
__device__ __forceinline__ int isqrt_floor(int v) {
  int s = (int)sqrtf((float)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}
// clear, in row y of an LDS bitmap, the pixels within r of (cy, cx); the centre may lie outside the image
__device__ __forceinline__ void stamp_row(uint32_t* bm, int Hh, int Wh, int wpr, int cy, int cx, int r, int y) {
  const int dy = y - cy;
  if (y < 0 || y >= Hh || dy > r || dy < -r) return;
  const int half = isqrt_floor(r * r - dy * dy);
  const int x_lo = max(cx - half, 0), x_hi = min(cx + half, Wh - 1);
  if (x_lo > x_hi) return;
  for (int w = x_lo >> 5; w <= (x_hi >> 5); ++w) {
    const int a = max(x_lo - 32 * w, 0), b = min(x_hi - 32 * w, 31);
    const uint32_t mask = (0xFFFFFFFFu >> (31 - b)) & (0xFFFFFFFFu << a);
    atomicAnd(&bm[y * wpr + w], ~mask);
  }
}
// erase(from = the bitmap the seeds are read in, into): the disks of radius r around the pixels of `from` with exactly
// `want` neighbours
__device__ void erase_around(const uint32_t* from, uint32_t* into, int Hh, int Wh, int wpr, int want, int r) {
  const int nw = Hh * wpr;
  for (int w = threadIdx.x; w < nw; w += kMoBlock) {
    uint32_t u = from[w];
    const int y = w / wpr, x0 = (w % wpr) * 32;
    while (u) {
      const int bit = __ffs(u) - 1;
      u &= u - 1;
      if (__popc(nbhd(from, Hh, wpr, y, x0 + bit) & ~16u) != want) continue;
      for (int yy = max(y - r, 0); yy <= min(y + r, Hh - 1); ++yy) stamp_row(into, Hh, Wh, wpr, y, x0 + bit, r, yy);
    }
  }
}

// (cos, sin) of the major axis from the six integer sums, fp64, nothing fused: skeleton.direction
__device__ void local_direction(const long long* q, double* c, double* s) {
#pragma clang fp contract(off)
  const long long n = q[0], sx = q[1], sy = q[2], sxx = q[3], sxy = q[4], syy = q[5];
  const long long A = n * sxx - sx * sx, C = n * syy - sy * sy, Bc = n * sxy - sx * sy;
  const double a = (double)(A - C), b = (double)(2 * Bc);
  const double aa = a * a, bb = b * b;
  const double h = __dsqrt_rn(aa + bb);
  if (h == 0.0) {
    *c = 1.0;
    *s = 0.0;
    return;
  }
  const double c2 = a / h;
  const double up = (1.0 + c2) / 2.0, dn = (1.0 - c2) / 2.0;
  *c = __dsqrt_rn(up);
  *s = copysign(__dsqrt_rn(dn), b);
}
// the ends of the cut through (i, j): perturb.fracture_endpoints
__device__ void local_endpoints(double c, double s, int d2, int i, int j, int scale, int* out) {
#pragma clang fp contract(off)
  const double ext = 0.5 * (double)scale;
  const double L = __dsqrt_rn((double)d2) + ext;
  const double nr = L * c, ls = L * s;
  const double nc = -ls, fi = (double)i, fj = (double)j;
  const double r0 = fi + nr, c0 = fj + nc, r1 = fi - nr, c1 = fj - nc;
  out[0] = (int)r0; out[1] = (int)c0; out[2] = (int)r1; out[3] = (int)c1;
}

__global__ void __launch_bounds__(kMoBlock)
morpho_locate_kernel(const uint32_t* __restrict__ skel, const int* __restrict__ d2, const int* __restrict__ status,
                     const int* __restrict__ kind, int Hh, int Wh, int wpr, int scale, int r_tips, int r_forks, int num,
                     uint64_t seed, const long long* __restrict__ dev_counter, uint64_t offset,
                     int* __restrict__ n_cand, int* __restrict__ fallback, int* __restrict__ centres,
                     int* __restrict__ endpoints) {
  extern __shared__ uint32_t s_two[];
  __shared__ int s_rows[kMoMaxSide];
  __shared__ int s_i[kMoWaves];
  __shared__ long long s_l[kMoWaves];
  __shared__ int s_c[kMoDraws][2];
  const int b = blockIdx.x, tid = threadIdx.x, nw = Hh * wpr;
  uint32_t* from = s_two;                                            // the skeleton the seeds are read in
  uint32_t* cand = s_two + nw;                                       // the candidates
  const uint32_t* sk = skel + (long long)b * nw;
  int* ce = centres + (long long)b * kMoDraws * 2;
  int* en = endpoints + (long long)b * kMoDraws * 4;
  if (tid < kMoDraws * 2) ce[tid] = -1;
  if (tid < kMoDraws * 4) en[tid] = 0;
  const int kd = kind[b];
  if (status[b] != 0 || (kd != kMoSwell && kd != kMoFracture)) {     // (uniform)
    if (tid == 0) {
      n_cand[b] = 0;
      fallback[b] = 0;
    }
    return;
  }
  const int n_draw = kd == kMoSwell ? 1 : num;
  const int rt = kd == kMoFracture ? r_tips : -1, rf = kd == kMoFracture ? r_forks : -1;
  for (int w = tid; w < nw; w += kMoBlock) from[w] = cand[w] = sk[w] & tail_mask(w, wpr, Wh);
  __syncthreads();
  if (rt >= 0) {
    erase_around(from, cand, Hh, Wh, wpr, 1, rt);
    __syncthreads();
  }
  if (rf >= 0) {
    if (rt >= 0) {
      for (int w = tid; w < nw; w += kMoBlock) from[w] = cand[w];
      __syncthreads();
    }
    erase_around(from, cand, Hh, Wh, wpr, 3, rf);
    __syncthreads();
  }
  auto count = [&]() {
    int n = 0;
    for (int y = tid; y < Hh; y += kMoBlock) {
      int c = 0;
      for (int w = 0; w < wpr; ++w) c += __popc(cand[y * wpr + w]);
      s_rows[y] = c;
      n += c;
    }
    return block_isum<kMoWaves>(n, s_i);                             // (its barriers publish s_rows)
  };
  int n = count(), fb = 0;
  if (n == 0 && (rt >= 0 || rf >= 0)) {                              // overpruned: the whole skeleton (uniform)
    for (int w = tid; w < nw; w += kMoBlock) cand[w] = sk[w] & tail_mask(w, wpr, Wh);
    __syncthreads();
    n = count();
    fb = n > 0;
  }
  if (tid == 0) {
    n_cand[b] = n;
    fallback[b] = fb;
  }
  if (n == 0) return;                                                // (uniform)
  if (tid < n_draw) {
    const uint64_t key = locate_key(rng_base_key(seed, dev_counter));
    const uint64_t e = (offset + (uint64_t)b) * (uint64_t)kMoDraws + (uint64_t)tid;
    int idx = (int)(((uint64_t)hi24(hash_at(key, e)) * (uint64_t)n) >> 24);   // < n
    int y = 0;
    while (y < Hh - 1 && idx >= s_rows[y]) idx -= s_rows[y++];
    int w = 0;
    while (w < wpr - 1 && idx >= __popc(cand[y * wpr + w])) idx -= __popc(cand[y * wpr + w++]);
    uint32_t u = cand[y * wpr + w];
    for (int i = 0; i < idx; ++i) u &= u - 1;
    const int x = 32 * w + __ffs(u) - 1;
    s_c[tid][0] = y;
    s_c[tid][1] = x;
    ce[2 * tid] = y;
    ce[2 * tid + 1] = x;
  }
  if (kd != kMoFracture) return;                                     // (uniform)
  __syncthreads();
  const int* D = d2 + (long long)b * Hh * Wh;
  const int r = 2 * scale;                                           // the reference's _ANGLE_WINDOW
  for (int k = 0; k < n_draw; ++k) {
    const int ci = s_c[k][0], cj = s_c[k][1];
    const int y_lo = max(ci - r, 0), y_hi = min(ci + r, Hh - 1), x_lo = max(cj - r, 0), x_hi = min(cj + r, Wh - 1);
    const int w_lo = x_lo >> 5, n_w = (x_hi >> 5) - w_lo + 1;
    long long m[6] = {0, 0, 0, 0, 0, 0};
    for (int e = tid; e < (y_hi - y_lo + 1) * n_w; e += kMoBlock) {
      const int y = y_lo + e / n_w, w = w_lo + e % n_w;
      const int a = max(x_lo - 32 * w, 0), z = min(x_hi - 32 * w, 31);
      uint32_t u = sk[y * wpr + w] & tail_mask(w, wpr, Wh) & (0xFFFFFFFFu >> (31 - z)) & (0xFFFFFFFFu << a);
      const long long yy = y - (ci - r);
      while (u) {
        const int bit = __ffs(u) - 1;
        u &= u - 1;
        const long long xx = 32 * w + bit - (cj - r);
        m[0] += 1; m[1] += xx; m[2] += yy; m[3] += xx * xx; m[4] += xx * yy; m[5] += yy * yy;
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) m[q] = waves_sum<kMoWaves>(wave_lsum(m[q]), s_l);
    if (tid == 0) {
      double c, s;
      local_direction(m, &c, &s);
      local_endpoints(c, s, D[ci * Wh + cj], ci, cj, scale, en + 4 * k);
    }
  }
}

// the source pixel of the radial warp for output pixel (y, x): perturb.swell
__device__ bool swell_source(const uint32_t* bm, int Hh, int Wh, int wpr, int cy, int cx, double RR, double ex, int y,
                             int x) {
#pragma clang fp contract(off)
  const int idx = x - cx, idy = y - cy;
  const double dx = (double)idx, dy = (double)idy, dd = (double)(idx * idx + idy * idy);
  double w = 1.0;
  if (!(dd > RR)) {
    const double q = dd / RR;
    w = ex == 1.0 ? q : pow(q, ex);
  }
  const double wy = w * dy, wx = w * dx;
  const double ty = (double)cy + wy, tx = (double)cx + wx;
  const double fy = ty + 0.5, fx = tx + 0.5;
  const double sy = floor(fy), sx = floor(fx);
  if (!(sy >= 0.0 && sy < (double)Hh && sx >= 0.0 && sx < (double)Wh)) return false;
  const int iy = (int)sy, ix = (int)sx;
  return (bm[iy * wpr + (ix >> 5)] >> (ix & 31)) & 1u;
}
__device__ int disk_radius(double amount, int scale, double thick) {
#pragma clang fp contract(off)
  const double as = amount * (double)scale;
  const double at = as * thick;
  return (int)fmin(at / 2.0, kMoRadiusLimit);
}
__device__ double swelling_radius(double radius, int scale, double thick) {
#pragma clang fp contract(off)
  const double rs = radius * __dsqrt_rn(thick);
  const double h = rs / 2.0;
  return h * (double)scale;
}

__global__ void __launch_bounds__(kMoBlock)
morpho_local_kernel(const uint32_t* __restrict__ bin, const int* __restrict__ d2, const int* __restrict__ d2c,
                    const float* __restrict__ thickness, long long thick_ld, const int* __restrict__ status_in,
                    const int* __restrict__ kind, const int* __restrict__ n_cand, const int* __restrict__ centres,
                    const int* __restrict__ endpoints, LocalParams p, int Hh, int Wh, int wpr, int scale,
                    uint32_t* __restrict__ out, int* __restrict__ radius, long long* __restrict__ sums,
                    int* __restrict__ status_out) {
  __shared__ uint32_t s_o[kMoMaxSide * (kMoMaxSide / 32)];
  __shared__ long long s_l[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x, nw = Hh * wpr;
  const uint32_t* bm = bin + (long long)b * nw;
  uint32_t* ob = out + (long long)b * nw;
  const int kd = kind[b];
  const double thick = (double)thickness[(long long)b * thick_ld];
  const bool nan = thick != thick;
  int st = status_in[b], r = 0;
  double RR = 0.0;
  if (st == 0) {
    if (kd == kMoThin || kd == kMoThick) {
      if (nan || (kd == kMoThick && !d2c)) st = kMoStuck;
      else r = disk_radius(kd == kMoThin ? p.thin_amount : p.thick_amount, scale, thick);
    } else if (kd == kMoSwell) {
      if (nan || n_cand[b] == 0) {
        st = kMoStuck;
      } else {
        const double R = swelling_radius(p.swell_radius, scale, thick);
        RR = __dmul_rn(R, R);
        r = (int)fmin(R, kMoRadiusLimit);
      }
    } else if (kd == kMoFracture) {
      if (n_cand[b] == 0) st = kMoStuck;
      else r = p.frac_r;
    } else if (kd != kMoPlain) {
      st = kMoStuck;                                                 // not a kind
    }
  }
  if (st != 0) {                                                     // (uniform)
    for (int w = tid; w < nw; w += kMoBlock) ob[w] = 0u;
    if (tid == 0) {
      radius[b] = 0;
      status_out[b] = st;
      for (int q = 0; q < 6; ++q) sums[(long long)b * 6 + q] = 0;
    }
    return;
  }
  if (kd == kMoPlain || kd == kMoFracture) {
    for (int w = tid; w < nw; w += kMoBlock) s_o[w] = bm[w] & tail_mask(w, wpr, Wh);
    if (kd == kMoFracture) {
      __syncthreads();
      const int* en = endpoints + (long long)b * kMoDraws * 4;
      const int rows = 2 * r + 1;
      for (int k = 0; k < p.n_frac; ++k) {
        const int r0 = en[4 * k], c0 = en[4 * k + 1], dr = en[4 * k + 2] - r0, dc = en[4 * k + 3] - c0;
        const int ar = abs(dr), ac = abs(dc), m = max(ar, ac);
        const int sr = (dr > 0) - (dr < 0), sc = (dc > 0) - (dc < 0);
        for (int e = tid; e < (m + 1) * rows; e += kMoBlock) {
          const int t = e / rows, dy = e % rows - r;
          int py = r0, px = c0;
          if (m > 0) {
            if (ar > ac) {
              py = r0 + sr * t;
              px = c0 + sc * ((2 * t * ac + m) / (2 * m));
            } else {
              py = r0 + sr * ((2 * t * ar + m) / (2 * m));
              px = c0 + sc * t;
            }
          }
          stamp_row(s_o, Hh, Wh, wpr, py, px, r, py + dy);
        }
      }
    }
  } else {
    const int* D = (kd == kMoThick ? d2c : d2) + (long long)b * Hh * Wh;
    const int rr = r * r;                                            // (r <= 2^15)
    const int cy = centres[(long long)b * kMoDraws * 2], cx = centres[(long long)b * kMoDraws * 2 + 1];
    for (int y = 0; y < Hh; ++y)
      for (int j0 = 0; j0 < Wh; j0 += kMoBlock) {                    // (uniform trip count: every lane reaches the ballot)
        const int j = j0 + tid;
        bool set = false;
        if (j < Wh) {
          if (kd == kMoThin) set = D[y * Wh + j] > rr;
          else if (kd == kMoThick) set = !(D[y * Wh + j] > rr);
          else set = swell_source(bm, Hh, Wh, wpr, cy, cx, RR, p.swell_exponent, y, j);
        }
        const unsigned long long bits = __ballot(set);
        const int w0 = (j0 + (tid & ~63)) >> 5;
        if ((tid & 63) == 0 && w0 < wpr) s_o[y * wpr + w0] = (uint32_t)bits;
        if ((tid & 63) == 32 && w0 + 1 < wpr) s_o[y * wpr + w0 + 1] = (uint32_t)(bits >> 32);
      }
  }
  __syncthreads();
  long long m[6] = {0, 0, 0, 0, 0, 0};
  for (int w = tid; w < nw; w += kMoBlock) {
    uint32_t u = s_o[w];
    ob[w] = u;
    const long long yy = w / wpr;
    const int x0 = (w % wpr) * 32;
    while (u) {
      const int bit = __ffs(u) - 1;
      u &= u - 1;
      const long long xx = x0 + bit;
      m[0] += 1; m[1] += xx; m[2] += yy; m[3] += xx * xx; m[4] += xx * yy; m[5] += yy * yy;
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = waves_sum<kMoWaves>(wave_lsum(m[q]), s_l);
  if (tid == 0) {
    radius[b] = r;
    status_out[b] = m[0] == 0 ? kMoStuck : 0;                        // (an empty bitmap is written as it is: zeros)
    for (int q = 0; q < 6; ++q) sums[(long long)b * 6 + q] = m[q];
  }
}

// --------------------------------------------------------------------------------------------------------- bounds
// The bounding parallelogram of morphomnist/morpho.py (bounds_of) on hires = expand(X - min X), formed as
// morpho_binarise_kernel forms it and never stored.  Pass 1 reduces the fp64 moments behind the shear u11 / u02 and the
// centroid row; pass 2 forms every row again (the same instructions: the same bits), takes its fp64 prefix P_y in LDS,
// and the thread that owns bin t adds P_y[k(y, t)] in ascending y, k(y, t) = #{x : x + .5 < t + shear (y - middle)}
// counted with the statement's own comparison.  The vertical cdf is the running sum of the rows' totals.  Then the
// four crossings of quantile_loc.  T = (X - min) AWt stays in LDS up to kBdLdsT floats (28 x 448: 50 KB), else in the
// workspace.
constexpr int kBdLdsT = 28 * 448;

// rows i0 .. i0 + kMoRows - 1 of column j of hires.  MODE 0: scale 1 (hires = X - min); 1, 2: 255 * AH T with explicit
// fmaf in ascending r, as morpho_binarise_kernel's tile
template <int MODE>
__device__ __forceinline__ void bounds_tile(const float* X, float xmn, int H, int W, int Hh, int Wh, const float* T,
                                            const float* __restrict__ AH, int i0, int j, float (&v)[kMoRows]) {
  if (MODE == 0) {
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) v[k] = i0 + k < Hh ? X[(i0 + k) * W + j] - xmn : 0.f;
    return;
  }
  float acc[kMoRows];
#pragma unroll
  for (int k = 0; k < kMoRows; ++k) acc[k] = 0.f;
  for (int r = 0; r < H; ++r) {
    const float t = T[r * Wh + j];
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) {
      const int i = i0 + k < Hh ? i0 + k : Hh - 1;                   // (uniform in the block)
      acc[k] = fmaf(AH[i * H + r], t, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kMoRows; ++k) v[k] = 255.f * acc[k];
}

// shear = u11 / u02 and middle = m01 from the sums q = (m00, x, y, xy, yy), each operation rounded on its own as
// ImageMoments forms them
__device__ void bounds_moments(const double* q, double* shear, double* middle) {
#pragma clang fp contract(off)
  const double m00 = q[0];
  const double m10 = q[1] / m00, m01 = q[2] / m00;
  const double u11 = q[3] / m00 - m10 * m01;
  const double u02 = q[4] / m00 - m01 * m01;
  *shear = u11 / u02;
  *middle = m01;
}

// #{x in 0 .. Wh - 1 : x + .5 < t + shear * (y - middle)}, the comparison evaluated as the statement writes it
__device__ int bounds_count(int t, int y, double shear, double middle, int Wh) {
#pragma clang fp contract(off)
  const double dy = (double)y - middle;
  const double sd = shear * dy;
  const double c = (double)t + sd;
  if (!(0.5 < c)) return 0;                                          // (NaN: no x)
  int k = (int)fmin(fmax(ceil(c - 0.5), 0.0), (double)Wh);          // an estimate, then the comparison itself decides
  while (k > 0 && !((double)(k - 1) + 0.5 < c)) --k;
  while (k < Wh && (double)k + 0.5 < c) ++k;
  return k;
}

// np.interp's interpolation on interval j of the cdf c
__device__ double bounds_interp(const double* c, int j, double f) {
#pragma clang fp contract(off)
  if (f == c[j]) return (double)j;
  const double slope = ((double)(j + 1) - (double)j) / (c[j + 1] - c[j]);
  const double d = f - c[j];
  const double p = slope * d;
  return p + (double)j;
}

__device__ __forceinline__ int block_imax(int v, int* s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s[0];
#pragma unroll
  for (int w = 1; w < kMoWaves; ++w) t = max(t, s[w]);
  __syncthreads();
  return t;
}

// quantile_loc(c[0 .. n - 1], f, left / right) by the whole block
__device__ double bounds_locate(const double* c, int n, double f, bool right, int* s_i) {
  constexpr int kNone = -(1 << 30);
  int best = kNone;                                                  // right: the last j; left: -(the first j)
  for (int j = threadIdx.x; j + 1 < n; j += kMoBlock)
    if (c[j] <= f && f < c[j + 1]) best = max(best, right ? j : -j);
  best = block_imax(best, s_i);
  if (!(f >= c[0])) return 0.0;
  if (f >= c[n - 1]) return (double)(n - 1);
  if (best == kNone) return __longlong_as_double(0x7ff8000000000000LL);   // (a finite cdf always crosses here)
  return bounds_interp(c, right ? best : -best, f);
}

template <int MODE>
__global__ void __launch_bounds__(kMoBlock)
morpho_bounds_kernel(const float* __restrict__ x, long long ld, int H, int W, int s, const float* __restrict__ AH,
                     const float* __restrict__ AW, double frac, float* __restrict__ Tws, double* __restrict__ bounds,
                     double* __restrict__ hcdf, double* __restrict__ vcdf) {
  __shared__ double s_big[kBdLdsT / 2];                              // T (MODE 1); after pass 2: hcdf
  __shared__ double s_P[kMoMaxSide + 1];                             // the prefix of the current row
  __shared__ double s_seg[2 * kMoWaves];                             // its 64-column segment totals
  __shared__ double s_vc[kMoMaxSide];                                // the mass above each row, then vcdf
  __shared__ float s_f[kMoWaves];
  __shared__ double s_d[kMoWaves];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Hh = H * s, Wh = W * s;
  const float* X = x + (long long)b * ld;
  float* T = MODE == 0 ? nullptr : MODE == 1 ? reinterpret_cast<float*>(s_big) : Tws + (long long)b * H * Wh;
  float xmn = INFINITY;
  for (int e = tid; e < H * W; e += kMoBlock) xmn = fminf(xmn, X[e]);
  xmn = -block_max<kMoWaves>(-xmn, s_f);
  if (MODE != 0) {
    for (int e = tid; e < H * Wh; e += kMoBlock) {
      const int r = e / Wh, j = e % Wh;
      float acc = 0.f;
      for (int c = 0; c < W; ++c) acc = fmaf(X[r * W + c] - xmn, AW[j * W + c], acc);
      T[e] = acc;
    }
    __syncthreads();                                                 // (the block reads what the block wrote)
  }
  // pass 1: m00, sum x h, sum y h, sum x y h, sum y^2 h
  double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < Hh; i0 += kMoRows)
    for (int j = tid; j < Wh; j += kMoBlock) {
      float v[kMoRows];
      bounds_tile<MODE>(X, xmn, H, W, Hh, Wh, T, AH, i0, j, v);
#pragma unroll
      for (int k = 0; k < kMoRows; ++k) {
        if (i0 + k >= Hh) break;
        const double d = (double)v[k], xx = (double)j, yy = (double)(i0 + k);
        m[0] += d; m[1] += xx * d; m[2] += yy * d; m[3] += xx * yy * d; m[4] += yy * yy * d;
      }
    }
#pragma unroll
  for (int q = 0; q < 5; ++q) m[q] = block_sum<kMoWaves>(m[q], s_d);
  double shear, middle;
  bounds_moments(m, &shear, &middle);
  // pass 2: the rows again, their prefixes, the bins
  const int j0 = tid, j1 = tid + kMoBlock;
  double hacc[2] = {0.0, 0.0}, above = 0.0;                          // (above: thread 0's running row total)
  if (tid == 0) s_P[0] = 0.0;
  for (int i0 = 0; i0 < Hh; i0 += kMoRows) {
    float v0[kMoRows], v1[kMoRows];
    if (j0 < Wh) bounds_tile<MODE>(X, xmn, H, W, Hh, Wh, T, AH, i0, j0, v0);
    if (j1 < Wh) bounds_tile<MODE>(X, xmn, H, W, Hh, Wh, T, AH, i0, j1, v1);
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) {
      const int y = i0 + k;
      if (y >= Hh) break;                                            // (uniform)
      double a = j0 < Wh ? (double)v0[k] : 0.0, c = j1 < Wh ? (double)v1[k] : 0.0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {                             // inclusive scans along the wave, in a fixed order
        const double pa = __shfl_up(a, d, 64), pc = __shfl_up(c, d, 64);
        if (lane >= d) { a = pa + a; c = pc + c; }
      }
      if (lane == 63) { s_seg[wave] = a; s_seg[kMoWaves + wave] = c; }
      __syncthreads();
      double run = 0.0, off0 = 0.0, off1 = 0.0;                      // the segments in column order
#pragma unroll
      for (int q = 0; q < 2 * kMoWaves; ++q) {
        if (q == wave) off0 = run;
        if (q == kMoWaves + wave) off1 = run;
        run = run + s_seg[q];
      }
      if (j0 < Wh) s_P[j0 + 1] = off0 + a;
      if (j1 < Wh) s_P[j1 + 1] = off1 + c;
      if (tid == 0) {
        s_vc[y] = above;
        above = above + run;
      }
      __syncthreads();
      if (j0 < Wh) hacc[0] += s_P[bounds_count(j0, y, shear, middle, Wh)];
      if (j1 < Wh) hacc[1] += s_P[bounds_count(j1, y, shear, middle, Wh)];
    }
  }
  // (every read of T and s_P lies before the last barrier above)
  double* s_hc = s_big;
  if (j0 < Wh) s_hc[j0] = hacc[0] / m[0];
  if (j1 < Wh) s_hc[j1] = hacc[1] / m[0];
  __syncthreads();                                                   // (s_vc is thread 0's until here)
  for (int t = tid; t < Hh; t += kMoBlock) s_vc[t] = s_vc[t] / m[0];
  __syncthreads();
  if (hcdf)
    for (int t = tid; t < Wh; t += kMoBlock) hcdf[(long long)b * Wh + t] = s_hc[t];
  if (vcdf)
    for (int t = tid; t < Hh; t += kMoBlock) vcdf[(long long)b * Hh + t] = s_vc[t];
  const double half = frac / 2.0, upper = 1.0 - half;
  const double left = bounds_locate(s_hc, Wh, half, false, s_i);
  const double right = bounds_locate(s_hc, Wh, upper, true, s_i);
  const double top = bounds_locate(s_vc, Hh, half, false, s_i);
  const double bottom = bounds_locate(s_vc, Hh, upper, true, s_i);
  if (tid == 0) {
    const bool ok = m[0] > 0.0 && isfinite(shear);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* o = bounds + (long long)b * 6;
    o[0] = ok ? left : nan; o[1] = ok ? right : nan; o[2] = ok ? top : nan; o[3] = ok ? bottom : nan;
    o[4] = shear; o[5] = middle;
  }
}

// ---------------------------------------------------------------------------------------------------------- width
// SetWidth (morphomnist/perturb.py: width_stage, width_columns, affine_stage).  morpho_width_kernel measures: the
// bitmap's integer moment sums, shear / cx / cy from them as shear_of_sums forms them, then pass 2 of
// morpho_bounds_kernel under THESE moments -- the rows of hires by bounds_tile, their fp64 prefixes in LDS, the bins by
// bounds_count -- with the grey mass m00 taken as the running total of the rows (every thread adds the same segment
// totals in the same order: the same bits in every thread), the horizontal cdf alone and its two crossings.  T lives
// where morpho_bounds_kernel keeps it (LDS up to kBdLdsT floats).  morpho_affine_reduce_kernel warps: a thread per
// output pixel forms the source column in fp64 in the statement's order, reads that bit of the row and the wave packs
// 64 of them by ballot into LDS; then reduce_warped.
constexpr int kMoBadTarget = 5;                                      // status: the target width is NaN, infinite or <= 0

// k = shear * (1 - factor): the off-diagonal entry of SetWidth's matrix
__device__ double width_offdiag(double shear, double factor) {
#pragma clang fp contract(off)
  const double g = 1.0 - factor;
  return shear * g;
}
// u(x) = cx + a * (x - cx) and v(y) = k * (y - cy): the two halves of a source column
__device__ double width_along(double a, double cx, int x) {
#pragma clang fp contract(off)
  const double dx = (double)x - cx;
  const double p = a * dx;
  return cx + p;
}
__device__ double width_across(double k, double cy, int y) {
#pragma clang fp contract(off)
  const double dy = (double)y - cy;
  return k * dy;
}
// floor((u + v) + 0.5) held to -1 .. Wh (a NaN: -1)
__device__ int width_column(double u, double v, int Wh) {
#pragma clang fp contract(off)
  const double w = u + v;
  const double z = w + 0.5;
  const double f = floor(z);
  if (!(f == f)) return -1;
  return (int)fmin(fmax(f, -1.0), (double)Wh);
}

template <int MODE>
__global__ void __launch_bounds__(kMoBlock)
morpho_width_kernel(const float* __restrict__ x, long long ld, int H, int W, int s, const float* __restrict__ AH,
                    const float* __restrict__ AW, const uint32_t* __restrict__ bin, int wpr, const int* __restrict__ fg,
                    double frac, const double* __restrict__ target, float* __restrict__ Tws,
                    long long* __restrict__ sums, double* __restrict__ wb, int* __restrict__ status,
                    double* __restrict__ hcdf) {
  __shared__ double s_big[kBdLdsT / 2];                              // T (MODE 1); after pass 2: hcdf
  __shared__ double s_P[kMoMaxSide + 1];                             // the prefix of the current row
  __shared__ double s_seg[2 * kMoWaves];                             // its 64-column segment totals
  __shared__ float s_f[kMoWaves];
  __shared__ long long s_l[kMoWaves];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Hh = H * s, Wh = W * s, nw = Hh * wpr;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  // leave with a status: sums 0, wb NaN, hcdf 0 (st is uniform in the block wherever this is called)
  auto leave = [&](int st) {
    if (hcdf)
      for (int t = tid; t < Wh; t += kMoBlock) hcdf[(long long)b * Wh + t] = 0.0;
    if (tid < 6) {
      sums[(long long)b * 6 + tid] = 0;
      wb[(long long)b * 6 + tid] = nan;
    }
    if (tid == 0) status[b] = st;
  };
  const double tgt = target[b];
  if (fg[b] == Hh * Wh) return leave(1);
  if (!(tgt > 0.0) || isinf(tgt)) return leave(kMoBadTarget);
  // the bitmap's six sums
  const uint32_t* bm = bin + (long long)b * nw;
  long long m[6] = {0, 0, 0, 0, 0, 0};
  for (int e = tid; e < nw; e += kMoBlock) {
    const long long yy = e / wpr;
    const int x0 = 32 * (e % wpr);
    uint32_t u = bm[e] & tail_mask(e, wpr, Wh);
    while (u) {
      const long long xx = x0 + __ffs(u) - 1;
      u &= u - 1;
      m[0] += 1; m[1] += xx; m[2] += yy; m[3] += xx * xx; m[4] += xx * yy; m[5] += yy * yy;
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) m[q] = waves_sum<kMoWaves>(wave_lsum(m[q]), s_l);
  if (m[0] == 0 || m[0] * m[5] == m[2] * m[2]) return leave(kMoStuck);   // empty, or one row (u02 == 0)
  double shear, middle;
  shear_of_sums(m, &shear, &middle);
  const double cx = __ddiv_rn((double)m[1], (double)m[0]);
  // T = (X - min) AWt
  const float* X = x + (long long)b * ld;
  float* T = MODE == 0 ? nullptr : MODE == 1 ? reinterpret_cast<float*>(s_big) : Tws + (long long)b * H * Wh;
  float xmn = INFINITY;
  for (int e = tid; e < H * W; e += kMoBlock) xmn = fminf(xmn, X[e]);
  xmn = -block_max<kMoWaves>(-xmn, s_f);
  if (MODE != 0) {
    for (int e = tid; e < H * Wh; e += kMoBlock) {
      const int r = e / Wh, j = e % Wh;
      float acc = 0.f;
      for (int c = 0; c < W; ++c) acc = fmaf(X[r * W + c] - xmn, AW[j * W + c], acc);
      T[e] = acc;
    }
    __syncthreads();                                                 // (the block reads what the block wrote)
  }
  // the rows, their prefixes, the bins (morpho_bounds_kernel's pass 2)
  const int j0 = tid, j1 = tid + kMoBlock;
  double hacc[2] = {0.0, 0.0}, m00 = 0.0;
  if (tid == 0) s_P[0] = 0.0;
  for (int i0 = 0; i0 < Hh; i0 += kMoRows) {
    float v0[kMoRows], v1[kMoRows];
    if (j0 < Wh) bounds_tile<MODE>(X, xmn, H, W, Hh, Wh, T, AH, i0, j0, v0);
    if (j1 < Wh) bounds_tile<MODE>(X, xmn, H, W, Hh, Wh, T, AH, i0, j1, v1);
#pragma unroll
    for (int k = 0; k < kMoRows; ++k) {
      const int y = i0 + k;
      if (y >= Hh) break;                                            // (uniform)
      double a = j0 < Wh ? (double)v0[k] : 0.0, c = j1 < Wh ? (double)v1[k] : 0.0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {                             // inclusive scans along the wave, in a fixed order
        const double pa = __shfl_up(a, d, 64), pc = __shfl_up(c, d, 64);
        if (lane >= d) { a = pa + a; c = pc + c; }
      }
      if (lane == 63) { s_seg[wave] = a; s_seg[kMoWaves + wave] = c; }
      __syncthreads();
      double run = 0.0, off0 = 0.0, off1 = 0.0;                      // the segments in column order
#pragma unroll
      for (int q = 0; q < 2 * kMoWaves; ++q) {
        if (q == wave) off0 = run;
        if (q == kMoWaves + wave) off1 = run;
        run = run + s_seg[q];
      }
      if (j0 < Wh) s_P[j0 + 1] = off0 + a;
      if (j1 < Wh) s_P[j1 + 1] = off1 + c;
      m00 = m00 + run;
      __syncthreads();
      if (j0 < Wh) hacc[0] += s_P[bounds_count(j0, y, shear, middle, Wh)];
      if (j1 < Wh) hacc[1] += s_P[bounds_count(j1, y, shear, middle, Wh)];
    }
  }
  __syncthreads();                                                   // (the last reads of T and s_P lie before here)
  double* s_hc = s_big;
  if (j0 < Wh) s_hc[j0] = hacc[0] / m00;
  if (j1 < Wh) s_hc[j1] = hacc[1] / m00;
  __syncthreads();
  const double half = frac / 2.0, upper = 1.0 - half;
  const double left = bounds_locate(s_hc, Wh, half, false, s_i);
  const double right = bounds_locate(s_hc, Wh, upper, true, s_i);
  const bool ok = m00 > 0.0 && isfinite(shear);
  const double width = ok ? __ddiv_rn(__dsub_rn(right, left), (double)s) : nan;
  if (!(isfinite(width) && width > 0.0)) return leave(kMoStuck);      // (uniform: every thread holds the same values)
  if (hcdf)
    for (int t = tid; t < Wh; t += kMoBlock) hcdf[(long long)b * Wh + t] = s_hc[t];
  if (tid == 0) {
    double* o = wb + (long long)b * 6;
    o[0] = left; o[1] = right; o[2] = shear; o[3] = cx; o[4] = middle; o[5] = __ddiv_rn(width, tgt);
    for (int q = 0; q < 6; ++q) sums[(long long)b * 6 + q] = m[q];
    status[b] = 0;
  }
}

__global__ void __launch_bounds__(kMoBlock)
morpho_affine_reduce_kernel(const uint32_t* __restrict__ bin, const long long* __restrict__ sums,
                            const double* __restrict__ wb, const int* __restrict__ status, int H, int W, int s, int wpr,
                            const double* __restrict__ RH, const double* __restrict__ RW, double* __restrict__ T,
                            float* __restrict__ qout, float* __restrict__ raw, uint32_t* __restrict__ warped,
                            int* __restrict__ status_out) {
  __shared__ uint32_t s_w[kMoMaxSide * (kMoMaxSide / 32)];
  __shared__ int s_i[kMoWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Hh = H * s, Wh = W * s, nw = Hh * wpr, N = H * W;
  float* Q = qout + (long long)b * N;
  const int st = status[b];
  if (st != 0) {                                                     // (uniform)
    for (int e = tid; e < N; e += kMoBlock) {
      Q[e] = 0.f;
      if (raw) raw[(long long)b * N + e] = 0.f;
    }
    if (warped)
      for (int e = tid; e < nw; e += kMoBlock) warped[(long long)b * nw + e] = 0u;
    if (tid == 0) status_out[b] = st;
    return;
  }
  double shear, cy;
  shear_of_sums(sums + (long long)b * 6, &shear, &cy);
  const double cx = __ddiv_rn((double)sums[(long long)b * 6 + 1], (double)sums[(long long)b * 6]);
  const double factor = wb[(long long)b * 6 + 5];
  const double k = width_offdiag(shear, factor);
  const uint32_t* bm = bin + (long long)b * nw;
  // a thread owns columns tid and tid + kMoBlock (Wh <= 2 * kMoBlock); 64 pixels of a row make two words by ballot
  double u[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) u[h] = width_along(factor, cx, tid + h * kMoBlock);
  for (int y = 0; y < Hh; ++y) {
    const double v = width_across(k, cy, y);
    const uint32_t* row = bm + y * wpr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = tid + h * kMoBlock;
      if (h * kMoBlock >= Wh) break;                                 // (uniform: every lane reaches the ballot)
      bool set = false;
      if (j < Wh) {
        const int c = width_column(u[h], v, Wh);
        if (c >= 0 && c < Wh) set = (row[c >> 5] >> (c & 31)) & 1u;
      }
      const unsigned long long bits = __ballot(set);
      const int w0 = (h * kMoBlock + (tid & ~63)) >> 5;
      if ((tid & 63) == 0 && w0 < wpr) s_w[y * wpr + w0] = (uint32_t)bits;
      if ((tid & 63) == 32 && w0 + 1 < wpr) s_w[y * wpr + w0 + 1] = (uint32_t)(bits >> 32);
    }
  }
  __syncthreads();
  if (warped)
    for (int e = tid; e < nw; e += kMoBlock) warped[(long long)b * nw + e] = s_w[e];
  const bool any = reduce_warped(s_w, H, W, s, wpr, RH, RW, T + (long long)b * Hh * W, Q,
                                 raw ? raw + (long long)b * N : nullptr);
  const int lit = block_imax(any ? 1 : 0, s_i);
  if (tid == 0) status_out[b] = lit ? 0 : kMoStuck;                  // (Q is 0 everywhere already)
}

// the side limits every entry point shares
static int morpho_check_dims(const char* who, int32_t B, int32_t Hh, int32_t Wh) {
  if (B < 1 || Hh < 1 || Wh < 1 || Hh > kMoMaxSide || Wh > kMoMaxSide) {
    set_error("%s: B = %d < 1 or an up-sampled image of %d x %d outside [1, %d] x [1, %d]", who, (int)B, (int)Hh,
              (int)Wh, kMoMaxSide, kMoMaxSide);
    return ALI_ERR_BAD_ARG;
  }
  return ALI_OK;
}
// n * scale, or one past the limit when it is larger (no overflow)
static int32_t hires_side(int32_t n, int32_t scale) {
  const int64_t v = (int64_t)n * scale;
  return (int32_t)(v > kMoMaxSide ? kMoMaxSide + 1 : v);
}
static int morpho_scratch(const char* who, void* ws, size_t ws_bytes, size_t need, void** at) {
  if (need && (!ws || ws_payload_bytes(ws_bytes) < need)) {
    set_error("%s: workspace too small (%zu bytes behind the reserved head needed)", who, need);
    return ALI_ERR_WORKSPACE;
  }
  *at = ws_payload(ws);
  return ALI_OK;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_morpho_binarise(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale,
                                   const float* AH, const float* AW, float threshold, uint32_t* bin, int32_t* fg,
                                   double* hstats, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!x || !bin || !fg || !hstats || (scale > 1 && (!AH || !AW))) {
    set_error("ali_morpho_binarise: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1 || ld < (int64_t)H * W) {
    set_error("ali_morpho_binarise: H = %d, W = %d or scale = %d < 1, or ld = %lld < H * W", (int)H, (int)W, (int)scale,
              (long long)ld);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_binarise", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  const int Wh = W * scale, wpr = (Wh + 31) / 32;
  void* T = nullptr;
  rc = morpho_scratch("ali_morpho_binarise", ws, ws_bytes, scale > 1 ? sizeof(float) * (size_t)B * H * Wh : 0, &T);
  if (rc != ALI_OK) return rc;
  if (scale > 1)
    hipLaunchKernelGGL(morpho_binarise_kernel<true>, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld,
                       (int)H, (int)W, (int)scale, AH, AW, threshold, static_cast<float*>(T), bin, wpr,
                       reinterpret_cast<int*>(fg), hstats);
  else
    hipLaunchKernelGGL(morpho_binarise_kernel<false>, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld,
                       (int)H, (int)W, 1, AH, AW, threshold, static_cast<float*>(T), bin, wpr,
                       reinterpret_cast<int*>(fg), hstats);
  return check_launch("morpho_binarise_kernel");
}

extern "C" int ali_morpho_edt(const uint32_t* bin, int32_t B, int32_t Hh, int32_t Wh, int32_t* d2, int32_t* status,
                              void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!bin || !d2 || !status) {
    set_error("ali_morpho_edt: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_edt", B, Hh, Wh);
  if (rc != ALI_OK) return rc;
  void* G = nullptr;
  rc = morpho_scratch("ali_morpho_edt", ws, ws_bytes, sizeof(uint16_t) * (size_t)B * Hh * Wh, &G);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(morpho_edt_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), bin, (int)Hh, (int)Wh,
                     (Wh + 31) / 32, static_cast<uint16_t*>(G), reinterpret_cast<int*>(d2),
                     reinterpret_cast<int*>(status));
  return check_launch("morpho_edt_kernel");
}

extern "C" int ali_morpho_thin(const uint32_t* bin, const int32_t* d2, const int32_t* fg, int32_t B, int32_t Hh,
                               int32_t Wh, uint64_t seed, const uint32_t* keep16, uint32_t* skel, int32_t* status,
                               void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!bin || !d2 || !fg || !keep16 || !skel || !status) {
    set_error("ali_morpho_thin: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_thin", B, Hh, Wh);
  if (rc != ALI_OK) return rc;
  void* L = nullptr;
  rc = morpho_scratch("ali_morpho_thin", ws, ws_bytes, (size_t)B * Hh * Wh, &L);
  if (rc != ALI_OK) return rc;
  KeepTable keep;
  for (int i = 0; i < 16; ++i) keep.w[i] = keep16[i];
  const int wpr = (Wh + 31) / 32;
  const size_t lds = 2 * sizeof(uint32_t) * (size_t)Hh * wpr;        // <= 64 KB of the CU's 160
  if (lds + 64 > 64 * 1024) {                                        // (512 x 512 alone: above a workgroup's default limit)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(morpho_thin_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             2 * (int)sizeof(uint32_t) * kMoMaxSide * (kMoMaxSide / 32));
    if (e != hipSuccess) {
      set_error("ali_morpho_thin: cannot raise the kernel's LDS limit: %s", hipGetErrorString(e));
      return ALI_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(morpho_thin_kernel, dim3((unsigned)B), dim3(kThinBlock), lds, ST(stream), bin,
                     reinterpret_cast<const int*>(d2), (int)Hh, (int)Wh, wpr, seed, keep, static_cast<uint8_t*>(L),
                     reinterpret_cast<const int*>(fg), skel, reinterpret_cast<int*>(status));
  return check_launch("morpho_thin_kernel");
}

extern "C" int ali_morpho_measure(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale,
                                  const uint32_t* skel, const int32_t* d2, const int32_t* fg, const double* hstats,
                                  const int32_t* status, int32_t* counts, float* values, float* slant_hires,
                                  ali_stream_t stream) {
  if (!x || !skel || !d2 || !fg || !hstats || !status || !counts || !values || !slant_hires) {
    set_error("ali_morpho_measure: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1 || ld < (int64_t)H * W) {
    set_error("ali_morpho_measure: H = %d, W = %d or scale = %d < 1, or ld = %lld < H * W", (int)H, (int)W, (int)scale,
              (long long)ld);
    return ALI_ERR_BAD_ARG;
  }
  const int rc = morpho_check_dims("ali_morpho_measure", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(morpho_measure_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld, (int)H,
                     (int)W, (int)scale, skel, reinterpret_cast<const int*>(d2), (W * scale + 31) / 32,
                     reinterpret_cast<const int*>(fg), hstats, reinterpret_cast<const int*>(status),
                     reinterpret_cast<int*>(counts), values, slant_hires);
  return check_launch("morpho_measure_kernel");
}

extern "C" int ali_morpho_reshape(const uint32_t* bin, const float* thickness, int64_t thickness_ld, const float* target,
                                  const int32_t* status_in, const int16_t* half, int32_t max_radius, int32_t B,
                                  int32_t Hh, int32_t Wh, int32_t scale, uint32_t* out, int32_t* radius, int64_t* sums,
                                  int32_t* status_out, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!bin || !thickness || !status_in || !half || !out || !radius || !sums || !status_out) {
    set_error("ali_morpho_reshape: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (max_radius < 0 || max_radius > kMoMaxRadius || scale < 1 || thickness_ld < 1) {
    set_error("ali_morpho_reshape: max_radius = %d outside [0, %d], scale = %d < 1 or thickness_ld = %lld < 1",
              (int)max_radius, kMoMaxRadius, (int)scale, (long long)thickness_ld);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_reshape", B, Hh, Wh);
  if (rc != ALI_OK) return rc;
  void* HD = nullptr;
  rc = morpho_scratch("ali_morpho_reshape", ws, ws_bytes, sizeof(uint16_t) * (size_t)B * Hh * Wh, &HD);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(morpho_reshape_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), bin, thickness,
                     (long long)thickness_ld, target, reinterpret_cast<const int*>(status_in), half, (int)max_radius,
                     (int)Hh, (int)Wh, (Wh + 31) / 32, (int)scale, static_cast<uint16_t*>(HD), out,
                     reinterpret_cast<int*>(radius), reinterpret_cast<long long*>(sums),
                     reinterpret_cast<int*>(status_out));
  return check_launch("morpho_reshape_kernel");
}

extern "C" int ali_morpho_shear_reduce(const uint32_t* bin, const int64_t* sums, const double* target_shear,
                                       const int32_t* status, int32_t B, int32_t H, int32_t W, int32_t scale,
                                       const double* RH, const double* RW, float* q, float* raw, int32_t* shifts,
                                       double* shear, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!bin || !sums || !status || !q || !shear || (scale > 1 && (!RH || !RW))) {
    set_error("ali_morpho_shear_reduce: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1) {
    set_error("ali_morpho_shear_reduce: H = %d, W = %d or scale = %d < 1", (int)H, (int)W, (int)scale);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_shear_reduce", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  void* T = nullptr;
  rc = morpho_scratch("ali_morpho_shear_reduce", ws, ws_bytes,
                      scale > 1 ? sizeof(double) * (size_t)B * H * scale * W : 0, &T);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(morpho_shear_reduce_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), bin,
                     reinterpret_cast<const long long*>(sums), target_shear, reinterpret_cast<const int*>(status),
                     (int)H, (int)W, (int)scale, (W * scale + 31) / 32, RH, RW, static_cast<double*>(T), q, raw,
                     reinterpret_cast<int*>(shifts), shear);
  return check_launch("morpho_shear_reduce_kernel");
}

extern "C" int ali_morpho_set_intensity(const float* q, const float* target, const int32_t* status_in, int32_t B,
                                        int32_t N, float* out, float* median, int32_t* status_out,
                                        ali_stream_t stream) {
  if (!q || !status_in || !out || !median || !status_out) {
    set_error("ali_morpho_set_intensity: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (B < 1 || N < 1 || N > kMoMaxSide * kMoMaxSide) {
    set_error("ali_morpho_set_intensity: B = %d < 1 or N = %d outside [1, %d]", (int)B, (int)N,
              kMoMaxSide * kMoMaxSide);
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(morpho_set_intensity_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), q, target,
                     reinterpret_cast<const int*>(status_in), (int)N, out, median, reinterpret_cast<int*>(status_out));
  return check_launch("morpho_set_intensity_kernel");
}

extern "C" int ali_morpho_locate(const uint32_t* skel, const int32_t* d2, const int32_t* status, const int32_t* kind,
                                 int32_t B, int32_t Hh, int32_t Wh, int32_t scale, int32_t r_tips, int32_t r_forks,
                                 int32_t num, uint64_t seed, const int64_t* dev_counter, uint64_t offset,
                                 int32_t* n_candidates, int32_t* fallback, int32_t* centres, int32_t* endpoints,
                                 ali_stream_t stream) {
  if (!skel || !d2 || !status || !kind || !n_candidates || !fallback || !centres || !endpoints) {
    set_error("ali_morpho_locate: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (scale < 1 || scale > kMoMaxSide || num < 1 || num > kMoDraws) {
    set_error("ali_morpho_locate: scale = %d outside [1, %d] or num = %d outside [1, %d]", (int)scale, kMoMaxSide,
              (int)num, kMoDraws);
    return ALI_ERR_BAD_ARG;
  }
  const int rc = morpho_check_dims("ali_morpho_locate", B, Hh, Wh);
  if (rc != ALI_OK) return rc;
  const int wpr = (Wh + 31) / 32;
  const size_t lds = 2 * sizeof(uint32_t) * (size_t)Hh * wpr;        // <= 64 KB of the CU's 160
  if (lds + 4096 > 64 * 1024) {                                      // (with the static arrays above the default limit)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(morpho_locate_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             2 * (int)sizeof(uint32_t) * kMoMaxSide * (kMoMaxSide / 32));
    if (e != hipSuccess) {
      set_error("ali_morpho_locate: cannot raise the kernel's LDS limit: %s", hipGetErrorString(e));
      return ALI_ERR_LAUNCH;
    }
  }
  // a disk of radius kMoStampMax already covers every image: larger radii erase the same pixels
  const int rt = r_tips < 0 ? -1 : (r_tips > kMoStampMax ? kMoStampMax : (int)r_tips);
  const int rf = r_forks < 0 ? -1 : (r_forks > kMoStampMax ? kMoStampMax : (int)r_forks);
  hipLaunchKernelGGL(morpho_locate_kernel, dim3((unsigned)B), dim3(kMoBlock), lds, ST(stream), skel,
                     reinterpret_cast<const int*>(d2), reinterpret_cast<const int*>(status),
                     reinterpret_cast<const int*>(kind), (int)Hh, (int)Wh, wpr, (int)scale, rt, rf, (int)num, seed,
                     reinterpret_cast<const long long*>(dev_counter), offset, reinterpret_cast<int*>(n_candidates),
                     reinterpret_cast<int*>(fallback), reinterpret_cast<int*>(centres),
                     reinterpret_cast<int*>(endpoints));
  return check_launch("morpho_locate_kernel");
}

extern "C" int ali_morpho_local(const uint32_t* bin, const int32_t* d2, const int32_t* d2c, const float* thickness,
                                int64_t thickness_ld, const int32_t* status_in, const int32_t* kind,
                                const int32_t* n_candidates, const int32_t* centres, const int32_t* endpoints,
                                double thin_amount, double thick_amount, double swell_strength, double swell_radius,
                                int32_t frac_radius, int32_t num_frac, int32_t B, int32_t Hh, int32_t Wh, int32_t scale,
                                uint32_t* out, int32_t* radius, int64_t* sums, int32_t* status_out,
                                ali_stream_t stream) {
  if (!bin || !d2 || !thickness || !status_in || !kind || !n_candidates || !centres || !endpoints || !out || !radius ||
      !sums || !status_out) {
    set_error("ali_morpho_local: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (!(thin_amount >= 0.0) || !(thick_amount >= 0.0) || !(swell_strength >= 1.0) || !(swell_radius >= 0.0) ||
      frac_radius < 0 || frac_radius > kMoStampMax || num_frac < 1 || num_frac > kMoDraws || scale < 1 ||
      scale > kMoMaxSide || thickness_ld < 1) {
    set_error("ali_morpho_local: an amount or the swelling radius < 0, swell_strength < 1, frac_radius = %d outside "
              "[0, %d], num_frac = %d outside [1, %d], scale = %d outside [1, %d] or thickness_ld = %lld < 1",
              (int)frac_radius, kMoStampMax, (int)num_frac, kMoDraws, (int)scale, kMoMaxSide, (long long)thickness_ld);
    return ALI_ERR_BAD_ARG;
  }
  const int rc = morpho_check_dims("ali_morpho_local", B, Hh, Wh);
  if (rc != ALI_OK) return rc;
  LocalParams p;
  p.thin_amount = thin_amount;
  p.thick_amount = thick_amount;
  p.swell_exponent = (swell_strength - 1.0) / 2.0;
  p.swell_radius = swell_radius;
  p.frac_r = (int)frac_radius;
  p.n_frac = (int)num_frac;
  hipLaunchKernelGGL(morpho_local_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), bin,
                     reinterpret_cast<const int*>(d2), reinterpret_cast<const int*>(d2c), thickness,
                     (long long)thickness_ld, reinterpret_cast<const int*>(status_in),
                     reinterpret_cast<const int*>(kind), reinterpret_cast<const int*>(n_candidates),
                     reinterpret_cast<const int*>(centres), reinterpret_cast<const int*>(endpoints), p, (int)Hh, (int)Wh,
                     (Wh + 31) / 32, (int)scale, out, reinterpret_cast<int*>(radius), reinterpret_cast<long long*>(sums),
                     reinterpret_cast<int*>(status_out));
  return check_launch("morpho_local_kernel");
}

extern "C" int ali_morpho_bounds(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale,
                                 const float* AH, const float* AW, double bound_frac, double* bounds, double* hcdf,
                                 double* vcdf, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!x || !bounds || (scale > 1 && (!AH || !AW))) {
    set_error("ali_morpho_bounds: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1 || ld < (int64_t)H * W || !(bound_frac > 0.0 && bound_frac < 1.0)) {
    set_error("ali_morpho_bounds: H = %d, W = %d or scale = %d < 1, ld = %lld < H * W, or bound_frac = %g outside "
              "(0, 1)", (int)H, (int)W, (int)scale, (long long)ld, bound_frac);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_bounds", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  const int Wh = W * scale;
  const int mode = scale == 1 ? 0 : (H * Wh <= kBdLdsT ? 1 : 2);
  void* T = nullptr;
  rc = morpho_scratch("ali_morpho_bounds", ws, ws_bytes, mode == 2 ? sizeof(float) * (size_t)B * H * Wh : 0, &T);
  if (rc != ALI_OK) return rc;
  if (mode == 0)
    hipLaunchKernelGGL(morpho_bounds_kernel<0>, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld,
                       (int)H, (int)W, 1, AH, AW, bound_frac, static_cast<float*>(T), bounds, hcdf, vcdf);
  else if (mode == 1)
    hipLaunchKernelGGL(morpho_bounds_kernel<1>, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld,
                       (int)H, (int)W, (int)scale, AH, AW, bound_frac, static_cast<float*>(T), bounds, hcdf, vcdf);
  else
    hipLaunchKernelGGL(morpho_bounds_kernel<2>, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld,
                       (int)H, (int)W, (int)scale, AH, AW, bound_frac, static_cast<float*>(T), bounds, hcdf, vcdf);
  return check_launch("morpho_bounds_kernel");
}

extern "C" int ali_morpho_width(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale,
                                const float* AH, const float* AW, const uint32_t* bin, const int32_t* fg,
                                double bound_frac, const double* target, int64_t* sums, double* wb, int32_t* status,
                                double* hcdf, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!x || !bin || !fg || !target || !sums || !wb || !status || (scale > 1 && (!AH || !AW))) {
    set_error("ali_morpho_width: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1 || ld < (int64_t)H * W || !(bound_frac > 0.0 && bound_frac < 1.0)) {
    set_error("ali_morpho_width: H = %d, W = %d or scale = %d < 1, ld = %lld < H * W, or bound_frac = %g outside (0, 1)",
              (int)H, (int)W, (int)scale, (long long)ld, bound_frac);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_width", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  const int Wh = W * scale, wpr = (Wh + 31) / 32;
  const int mode = scale == 1 ? 0 : (H * Wh <= kBdLdsT ? 1 : 2);
  void* T = nullptr;
  rc = morpho_scratch("ali_morpho_width", ws, ws_bytes, mode == 2 ? sizeof(float) * (size_t)B * H * Wh : 0, &T);
  if (rc != ALI_OK) return rc;
  auto launch = [&](auto kernel, int s) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), x, (long long)ld, (int)H, (int)W, s, AH,
                       AW, bin, wpr, reinterpret_cast<const int*>(fg), bound_frac, target, static_cast<float*>(T),
                       reinterpret_cast<long long*>(sums), wb, reinterpret_cast<int*>(status), hcdf);
  };
  if (mode == 0)
    launch(morpho_width_kernel<0>, 1);
  else if (mode == 1)
    launch(morpho_width_kernel<1>, (int)scale);
  else
    launch(morpho_width_kernel<2>, (int)scale);
  return check_launch("morpho_width_kernel");
}

extern "C" int ali_morpho_affine_reduce(const uint32_t* bin, const int64_t* sums, const double* wb,
                                        const int32_t* status, int32_t B, int32_t H, int32_t W, int32_t scale,
                                        const double* RH, const double* RW, float* q, float* raw, uint32_t* warped,
                                        int32_t* status_out, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!bin || !sums || !wb || !status || !q || !status_out || (scale > 1 && (!RH || !RW))) {
    set_error("ali_morpho_affine_reduce: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (H < 1 || W < 1 || scale < 1) {
    set_error("ali_morpho_affine_reduce: H = %d, W = %d or scale = %d < 1", (int)H, (int)W, (int)scale);
    return ALI_ERR_BAD_ARG;
  }
  int rc = morpho_check_dims("ali_morpho_affine_reduce", B, hires_side(H, scale), hires_side(W, scale));
  if (rc != ALI_OK) return rc;
  void* T = nullptr;
  rc = morpho_scratch("ali_morpho_affine_reduce", ws, ws_bytes,
                      scale > 1 ? sizeof(double) * (size_t)B * H * scale * W : 0, &T);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(morpho_affine_reduce_kernel, dim3((unsigned)B), dim3(kMoBlock), 0, ST(stream), bin,
                     reinterpret_cast<const long long*>(sums), wb, reinterpret_cast<const int*>(status), (int)H, (int)W,
                     (int)scale, (W * scale + 31) / 32, RH, RW, static_cast<double*>(T), q, raw, warped,
                     reinterpret_cast<int*>(status_out));
  return check_launch("morpho_affine_reduce_kernel");
}
