// SSIM (structural similarity) of image pairs and its gradient (include/ali_hip.h: ali_ssim_fwd / ali_ssim_bwd): the
// reconstruction loss of the encoder fine-tuning scripts with --metric ssim (finetune_mnist_bigan.py:75-76).
//
// Both kernels are the same machine: a 32x32 output tile per 256-thread block, the input tile plus its win-1 halo
// staged in LDS, the separable filter as a horizontal pass LDS -> LDS and a vertical pass LDS -> registers, four
// outputs per thread in each pass so a staged value feeds four accumulators.
//   forward : inputs X, Y; channels x, y, x*x, y*y, x*y; epilogue = the SSIM map S, its per-tile sum and (optionally)
//             the coefficient maps A = dS/dF(Y), Bq = dS/dF(Y*Y), Cq = dS/dF(X*Y).
//   backward: inputs A, Bq, Cq zero-extended by win-1 on every side (the transposed filter is the valid filter of the
//             zero-extended map with the taps reversed); epilogue dY = w * (Ft(A) + 2*Y*Ft(Bq) + X*Ft(Cq)).
// Sums have a fixed order (shuffle tree, then four wave sums, then the tiles of a plane in index order): no atomics.
#include "ali_common.h"

namespace ali {

constexpr int kSsimTile = 32;                 // output tile edge; 256 threads = 32 columns x 8 groups of 4 rows
constexpr int kSsimHS = kSsimTile + 1;        // row stride of the horizontal-pass results (odd: the pass writes down columns)
constexpr int kSsimMaxWin = ALI_SSIM_MAX_WIN;

struct SsimLds {
  int IH, IWp, tile, hsz;                     // staged rows (= columns), padded row stride, floats per tile / per channel
  __host__ __device__ SsimLds(int win) {
    IH = kSsimTile + win - 1;
    IWp = IH | 1;                             // odd stride: the horizontal pass reads down columns without bank conflicts
    tile = IH * IWp;
    hsz = IH * kSsimHS;
  }
  // taps (32), nin staged tiles, nch horizontal-pass results, `red` floats of reduction scratch
  __host__ __device__ int floats(int nin, int nch, int red) const { return 32 + nin * tile + nch * hsz + red; }
};

// dst[r][c] = src[r0 + r][c0 + c] where that lies inside the rows x cols plane, else 0
__device__ __forceinline__ void ssim_load_tile(float* dst, const float* __restrict__ src, int r0, int c0, int rows,
                                               int cols, int IH, int IWp) {
  for (int i = threadIdx.x; i < IH * IH; i += 256) {
    const int r = i / IH, c = i - r * IH;
    const int gr = r0 + r, gc = c0 + c;
    dst[r * IWp + c] = (gr >= 0 && gr < rows && gc >= 0 && gc < cols) ? src[(long long)gr * cols + gc] : 0.f;
  }
}

// Horizontal pass over every staged row: h[ch][r][c] = sum_k g[k] * v_ch[r][c + k], c < 32.
// MOMENTS: the five channels x, y, x*x, y*y, x*y of the two tiles in0, in1; otherwise the three tiles themselves.
template <int WIN, bool MOMENTS>
__device__ __forceinline__ void ssim_hpass(const float* in0, const float* in1, const float* in2, float* h,
                                           const float* sg, int win, const SsimLds& L) {
  constexpr int NCH = MOMENTS ? 5 : 3;
  for (int it = threadIdx.x; it < L.IH * (kSsimTile / 4); it += 256) {
    const int r = it % L.IH, cg = it / L.IH;
    const int base = r * L.IWp + cg * 4;
    float acc[4][NCH];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) acc[o][ch] = 0.f;
#pragma unroll
    for (int j = 0; j < (WIN ? WIN : kSsimMaxWin) + 3; ++j) {
      if (!WIN && j >= win + 3) break;
      float v[NCH];
      if constexpr (MOMENTS) {
        const float x = in0[base + j], y = in1[base + j];
        v[0] = x; v[1] = y; v[2] = x * x; v[3] = y * y; v[4] = x * y;
      } else {
        v[0] = in0[base + j]; v[1] = in1[base + j]; v[2] = in2[base + j];
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = j - o;
        if (k >= 0 && k < win) {
          const float g = sg[k];
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) acc[o][ch] = fmaf(g, v[ch], acc[o][ch]);
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int o = 0; o < 4; ++o) h[ch * L.hsz + r * kSsimHS + cg * 4 + o] = acc[o][ch];
  }
}

// Vertical pass: acc[o][ch] = sum_k g[k] * h[ch][rg*4 + o + k][c] for the thread's column c and rows rg*4 .. rg*4+3.
template <int WIN, int NCH>
__device__ __forceinline__ void ssim_vpass(const float* h, const float* sg, int win, const SsimLds& L, int c, int rg,
                                           float (&acc)[4][NCH]) {
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[o][ch] = 0.f;
#pragma unroll
  for (int j = 0; j < (WIN ? WIN : kSsimMaxWin) + 3; ++j) {
    if (!WIN && j >= win + 3) break;
    float v[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) v[ch] = h[ch * L.hsz + (rg * 4 + j) * kSsimHS + c];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int k = j - o;
      if (k >= 0 && k < win) {
        const float g = sg[k];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[o][ch] = fmaf(g, v[ch], acc[o][ch]);
      }
    }
  }
}

// part[plane * tiles + tile] = (sum of S over the tile's map positions) * inv_n; maps (optional) [planes][Hm][Wm].
template <int WIN>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       int H, int W, const float* __restrict__ taps, int win_rt,
                                                       float C1, float C2, float inv_n, int tiles_x, int tiles,
                                                       float* __restrict__ part, float* __restrict__ mA,
                                                       float* __restrict__ mB, float* __restrict__ mC) {
  extern __shared__ __align__(16) float lds[];
  const int win = WIN ? WIN : win_rt;
  const SsimLds L(win);
  float* sg = lds;
  float* sx = lds + 32;
  float* sy = sx + L.tile;
  float* h = sy + L.tile;
  float* red = h + 5 * L.hsz;
  const int tid = threadIdx.x;
  const long long plane = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)(plane * tiles);
  const int r0 = (tile / tiles_x) * kSsimTile, c0 = (tile % tiles_x) * kSsimTile;
  const int Hm = H - win + 1, Wm = W - win + 1;
  const long long poff = plane * H * W;
  if (tid < win) sg[tid] = taps[tid];
  ssim_load_tile(sx, X + poff, r0, c0, H, W, L.IH, L.IWp);
  ssim_load_tile(sy, Y + poff, r0, c0, H, W, L.IH, L.IWp);
  __syncthreads();
  ssim_hpass<WIN, true>(sx, sy, nullptr, h, sg, win, L);
  __syncthreads();
  const int c = tid & 31, rg = tid >> 5;
  float acc[4][5];
  ssim_vpass<WIN, 5>(h, sg, win, L, c, rg, acc);
  float sum = 0.f;
  const long long moff = plane * Hm * Wm;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int i = r0 + rg * 4 + o, j = c0 + c;
    if (i < Hm && j < Wm) {
      const float m1 = acc[o][0], m2 = acc[o][1];
      const float s1 = acc[o][2] - m1 * m1, s2 = acc[o][3] - m2 * m2, s12 = acc[o][4] - m1 * m2;
      const float Ld = m1 * m1 + m2 * m2 + C1, Cd = s1 + s2 + C2;
      const float lum = (2.f * m1 * m2 + C1) / Ld, cs = (2.f * s12 + C2) / Cd;
      const float S = lum * cs;
      sum += S;
      if (mA) {
        const float Bq = -S / Cd, Cq = 2.f * lum / Cd;
        const long long q = moff + (long long)i * Wm + j;
        mA[q] = 2.f * cs * (m1 - lum * m2) / Ld - m1 * Cq - 2.f * m2 * Bq;
        mB[q] = Bq;
        mC[q] = Cq;
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) * inv_n;
}

__global__ void ssim_fold_kernel(const float* __restrict__ part, long long planes, int tiles, float* __restrict__ out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= planes) return;
  float s = 0.f;
  for (int t = 0; t < tiles; ++t) s += part[p * tiles + t];
  out[p] = s;
}

// dY[plane][i][j] = gpc[plane] * inv_n * (Ft(A) + 2*Y*Ft(Bq) + X*Ft(Cq))[i][j]; the taps are staged reversed.
template <int WIN>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       const float* __restrict__ mA, const float* __restrict__ mB,
                                                       const float* __restrict__ mC, const float* __restrict__ gpc,
                                                       int H, int W, const float* __restrict__ taps, int win_rt,
                                                       float inv_n, int tiles_x, int tiles, float* __restrict__ dY) {
  extern __shared__ __align__(16) float lds[];
  const int win = WIN ? WIN : win_rt;
  const SsimLds L(win);
  float* sg = lds;
  float* s0 = lds + 32;
  float* s1 = s0 + L.tile;
  float* s2 = s1 + L.tile;
  float* h = s2 + L.tile;
  const int tid = threadIdx.x;
  const long long plane = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)(plane * tiles);
  const int r0 = (tile / tiles_x) * kSsimTile, c0 = (tile % tiles_x) * kSsimTile;
  const int Hm = H - win + 1, Wm = W - win + 1;
  const long long moff = plane * Hm * Wm;
  if (tid < win) sg[tid] = taps[win - 1 - tid];
  ssim_load_tile(s0, mA + moff, r0 - (win - 1), c0 - (win - 1), Hm, Wm, L.IH, L.IWp);
  ssim_load_tile(s1, mB + moff, r0 - (win - 1), c0 - (win - 1), Hm, Wm, L.IH, L.IWp);
  ssim_load_tile(s2, mC + moff, r0 - (win - 1), c0 - (win - 1), Hm, Wm, L.IH, L.IWp);
  __syncthreads();
  ssim_hpass<WIN, false>(s0, s1, s2, h, sg, win, L);
  __syncthreads();
  const int c = tid & 31, rg = tid >> 5;
  float acc[4][3];
  ssim_vpass<WIN, 3>(h, sg, win, L, c, rg, acc);
  const float w = gpc[plane] * inv_n;
  const long long poff = plane * H * W;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int i = r0 + rg * 4 + o, j = c0 + c;
    if (i < H && j < W) {
      const long long p = poff + (long long)i * W + j;
      dY[p] = w * (acc[o][0] + 2.f * Y[p] * acc[o][1] + X[p] * acc[o][2]);
    }
  }
}

static bool ssim_shape_ok(const char* what, int64_t planes, int H, int W, int win, long long* tiles_out, int* tiles_x,
                          int out_h, int out_w) {
  if (planes <= 0 || win < 1 || win > kSsimMaxWin || (win & 1) == 0 || H < win || W < win) {
    set_error("%s: bad shape (planes=%lld H=%d W=%d win=%d; win odd, <= %d, <= H, W)", what, (long long)planes, H, W,
              win, kSsimMaxWin);
    return false;
  }
  *tiles_x = (out_w + kSsimTile - 1) / kSsimTile;
  *tiles_out = (long long)*tiles_x * ((out_h + kSsimTile - 1) / kSsimTile);
  if (*tiles_out * planes >= (1LL << 31)) { set_error("%s: too many tiles", what); return false; }
  return true;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_ssim_fwd(const float* X, const float* Y, int64_t planes, int32_t H, int32_t W, const float* win,
                            int32_t win_size, float C1, float C2, float* ssim_pc, float* mA, float* mB, float* mC,
                            void* ws, size_t ws_bytes, ali_stream_t stream) {
  ws = ws_payload(ws);
  ws_bytes = ws_payload_bytes(ws_bytes);
  if (!X || !Y || !win || !ssim_pc || (mA && (!mB || !mC))) { set_error("ali_ssim_fwd: bad argument"); return ALI_ERR_BAD_ARG; }
  long long tiles;
  int tiles_x;
  if (!ssim_shape_ok("ali_ssim_fwd", planes, H, W, win_size, &tiles, &tiles_x, H - win_size + 1, W - win_size + 1))
    return ALI_ERR_BAD_ARG;
  float* part = ssim_pc;
  if (tiles > 1) {
    if (!ws || ws_bytes < (size_t)(planes * tiles) * sizeof(float)) { set_error("ali_ssim_fwd: workspace too small"); return ALI_ERR_WORKSPACE; }
    part = reinterpret_cast<float*>(ws);
  }
  const float inv_n = 1.f / ((float)(H - win_size + 1) * (float)(W - win_size + 1));
  const size_t lds = (size_t)SsimLds(win_size).floats(2, 5, 4) * sizeof(float);
  const dim3 grid((unsigned)(planes * tiles));
  if (win_size == 11)
    hipLaunchKernelGGL(ssim_fwd_kernel<11>, grid, dim3(256), lds, ST(stream), X, Y, H, W, win, win_size, C1, C2, inv_n,
                       tiles_x, (int)tiles, part, mA, mB, mC);
  else
    hipLaunchKernelGGL(ssim_fwd_kernel<0>, grid, dim3(256), lds, ST(stream), X, Y, H, W, win, win_size, C1, C2, inv_n,
                       tiles_x, (int)tiles, part, mA, mB, mC);
  int rc = check_launch("ssim_fwd_kernel");
  if (rc || tiles == 1) return rc;
  hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, ST(stream), part,
                     (long long)planes, (int)tiles, ssim_pc);
  return check_launch("ssim_fold_kernel");
}

extern "C" int ali_ssim_bwd(const float* X, const float* Y, const float* mA, const float* mB, const float* mC,
                            const float* gpc, int64_t planes, int32_t H, int32_t W, const float* win, int32_t win_size,
                            float* dY, ali_stream_t stream) {
  if (!X || !Y || !mA || !mB || !mC || !gpc || !win || !dY) { set_error("ali_ssim_bwd: bad argument"); return ALI_ERR_BAD_ARG; }
  long long tiles;
  int tiles_x;
  if (!ssim_shape_ok("ali_ssim_bwd", planes, H, W, win_size, &tiles, &tiles_x, H, W)) return ALI_ERR_BAD_ARG;
  const float inv_n = 1.f / ((float)(H - win_size + 1) * (float)(W - win_size + 1));
  const size_t lds = (size_t)SsimLds(win_size).floats(3, 3, 0) * sizeof(float);
  const dim3 grid((unsigned)(planes * tiles));
  if (win_size == 11)
    hipLaunchKernelGGL(ssim_bwd_kernel<11>, grid, dim3(256), lds, ST(stream), X, Y, mA, mB, mC, gpc, H, W, win,
                       win_size, inv_n, tiles_x, (int)tiles, dY);
  else
    hipLaunchKernelGGL(ssim_bwd_kernel<0>, grid, dim3(256), lds, ST(stream), X, Y, mA, mB, mC, gpc, H, W, win,
                       win_size, inv_n, tiles_x, (int)tiles, dY);
  return check_launch("ssim_bwd_kernel");
}
