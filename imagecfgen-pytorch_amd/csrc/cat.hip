// The attribute SCM of AudioMNIST on the device (attribute_scms/audio_mnist.py; include/ali_hip.h: ali_cat_plan,
// ali_cat_nll, ali_cat_map): country_of_origin -> native_speaker, (country_of_origin, native_speaker) -> accent, two
// ReLU MLPs whose heads are categorical logits.
//
//   cat_nll_kernel    a block walks row tiles of 32: both MLPs forward, the two log-softmaxes, and -- GRAD -- the data
//                     gradients back to every trained layer's pre-activation; inputs and pre-activation gradients of the
//                     trained layers are parked in the workspace in fp64
//   cat_wgrad_kernel  one block per 16 x 16 tile of a trained weight (the bias rides as input column K, which reads 1):
//                     dW = dZ^T X over all rows, 16 waves striding the rows, folded wave 0 .. 15
//   cat_map_kernel    logits / ancestral draw / draw-until-it-differs / abduction / counterfactual of row tiles
//
// Every matrix product runs on v_mfma_f64_16x16x4_f64: weights and contexts are fp32 in memory and exact in fp64, the
// activations stay fp64 from layer to layer (LDS, workspace), and a result is rounded to fp32 once, where it leaves
// (lp, out3, gtheta, logits_out).  Operand lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register r of
// lane l is D[(l >> 4) + 4 r][l & 15] (the f64 form's own map, not the f32 forms').
//
// Sums over rows have fixed orders: out3 per thread over its tiles, lanes, waves, blocks ascending in the block that
// arrives last (ali_reduce.h); a weight gradient per wave over its k-steps (rows 4 s .. 4 s + 3, s = wave, wave + 16,
// ...; inside the MFMA), then waves ascending.  No float atomics.
#include "ali_reduce.h"
#include "ali_gumbel.h"

namespace ali {

constexpr int kCatThreads = 256, kCatWaves = kCatThreads / 64;
constexpr int kCatMT = 2, kCatRows = 16 * kCatMT;     // M-tiles and rows of a row tile
constexpr int kCatMaxBlocks = 256;
constexpr int kCatH = 128, kCatT = 64;                // widths: native_speaker's hidden layers | towers, accent's hidden
constexpr int kCatLd = kCatH + 4;                     // LDS row stride of an activation tile, in doubles
constexpr int kCatZLd = 64;                           // LDS row stride of a logit tile
constexpr int kCatWThreads = 1024, kCatWWaves = kCatWThreads / 64;
constexpr int kCatMaxC = 64;
constexpr int kCatKU = 8;                              // k-steps whose operand loads are in flight together
using f64x4 = __attribute__((ext_vector_type(4))) double;

// offsets (in floats) into theta and into the tower buffer; include/ali_hip.h states both layouts
struct CatLayout {
  int w1, b1, w2, b2, w3, b3, w4, b4, v1, c1, v2, c2, total;
  int tower[2], towers_total;
};
__host__ __device__ inline CatLayout cat_layout(int Cc, int Cn, int Ca) {
  CatLayout L;
  int o = 0;
  L.w1 = o; o += kCatH * Cc;     L.b1 = o; o += kCatH;
  L.w2 = o; o += kCatH * kCatH;  L.b2 = o; o += kCatH;
  L.w3 = o; o += kCatH * kCatH;  L.b3 = o; o += kCatH;
  L.w4 = o; o += Cn * kCatH;     L.b4 = o; o += Cn;
  L.v1 = o; o += kCatT * kCatH;  L.c1 = o; o += kCatT;
  L.v2 = o; o += Ca * kCatT;     L.c2 = o; o += Ca;
  L.total = o;
  L.tower[0] = 0;
  L.tower[1] = kCatT * Cc + kCatT + 3 * (kCatT * kCatT + kCatT);
  L.towers_total = L.tower[1] + kCatT * Cn + kCatT + 3 * (kCatT * kCatT + kCatT);
  return L;
}

// the parked fp64 arrays of a gradient launch, as offsets in doubles behind the block partials
struct CatPark {
  long long h1, h2, h3, f, hd, dz1, dz2, dz3, dz4, dzd1, dzd2, total;
};
__host__ __device__ inline CatPark cat_park(long long N, int Cn, int Ca) {
  CatPark P;
  long long o = 0;
  P.h1 = o; o += N * kCatH;  P.h2 = o; o += N * kCatH;  P.h3 = o; o += N * kCatH;
  P.f = o; o += N * kCatH;   P.hd = o; o += N * kCatT;
  P.dz1 = o; o += N * kCatH; P.dz2 = o; o += N * kCatH; P.dz3 = o; o += N * kCatH;
  P.dz4 = o; o += N * Cn;    P.dzd1 = o; o += N * kCatT; P.dzd2 = o; o += N * Ca;
  P.total = o;
  return P;
}
constexpr size_t kCatPartBytes = (size_t)2 * kCatMaxBlocks * sizeof(double);

struct CatNet {
  const float* theta;
  const float* towers;
  int Cc, Cn, Ca;
  CatLayout L;
};

// rows of a strided fp32 table, optionally gathered: row n reads source row index[n]
struct CatRows {
  const float* p;
  long long ld;
  const long long* index;
  long long src_rows;
  __device__ __forceinline__ long long src(long long n, bool& ok) const {
    const long long s = index ? index[n] : n;
    ok = s >= 0 && s < src_rows;
    return ok ? s : 0;
  }
};

// ------------------------------------------------------------------------------------------------------- the tile
// Y[r][j] = act(sum_{c < Cdim} X[r][c] * M(c, j) + bias[j]) for the 32 rows of a tile, j < J, with M(c, j) =
// W[c * sc + j * sj]: a Linear's forward is (sc, sj) = (1, K) over its [O][K] weight, its data gradient (K, 1).
// X, Y: LDS tiles.  gate (global, row stride ldg, the tile's first row): rows of Y pass only where gate > 0 -- the
// ReLU's gradient, read from the parked post-activation, which is > 0 exactly where the pre-activation is.
// park (global, row stride J, the tile's first row): the valid rows of Y are stored there too.
__device__ __forceinline__ void dense_tile(const double* X, int ldx, int Cdim, const float* __restrict__ W, int sc, int sj,
                                           const float* __restrict__ bias, int J, double* Y, int ldy, bool relu,
                                           const double* gate, int ldg, double* park, int rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  for (int jt = wave; jt * 16 < J; jt += kCatWaves) {
    const int j = jt * 16 + lr;
    const bool jok = j < J;
    f64x4 acc[kCatMT];
#pragma unroll
    for (int mt = 0; mt < kCatMT; ++mt) acc[mt] = f64x4{0.0, 0.0, 0.0, 0.0};
    // kCatKU k-steps at a time, their operand loads issued together (the weights come from L2)
    for (int c0 = 0; c0 < Cdim; c0 += 4 * kCatKU) {
      double b[kCatKU], a[kCatKU][kCatMT];
#pragma unroll
      for (int u = 0; u < kCatKU; ++u) {
        const int c = c0 + 4 * u + lk;
        const bool cok = c < Cdim;
        b[u] = (jok && cok) ? (double)W[(long long)c * sc + (long long)j * sj] : 0.0;
#pragma unroll
        for (int mt = 0; mt < kCatMT; ++mt) a[u][mt] = cok ? X[(mt * 16 + lr) * ldx + c] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kCatKU; ++u) {
#pragma unroll
        for (int mt = 0; mt < kCatMT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][mt], b[u], acc[mt], 0, 0, 0);
      }
    }
    const double bj = (bias && jok) ? (double)bias[j] : 0.0;
#pragma unroll
    for (int mt = 0; mt < kCatMT; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + lk + 4 * r;
        double v = acc[mt][r] + bj;
        if (relu) v = v > 0.0 ? v : 0.0;
        if (gate && jok && !(row < rows && gate[(long long)row * ldg + j] > 0.0)) v = 0.0;
        if (jok) {
          Y[row * ldy + j] = v;
          if (park && row < rows) park[(long long)row * J + j] = v;
        }
      }
    }
  }
  __syncthreads();
}

// the tile's rows of a table into LDS as doubles; rows past the end (and rows whose index is out of range) are zero
__device__ __forceinline__ void stage_rows(double* X, const CatRows& R, int C, long long row0, int rows) {
  for (int i = threadIdx.x; i < kCatRows * C; i += kCatThreads) {
    const int r = i / C, c = i - r * C;
    double v = 0.0;
    if (r < rows) {
      bool ok;
      const long long s = R.src(row0 + r, ok);
      if (ok) v = (double)R.p[s * R.ld + c];
    }
    X[r * kCatLd + c] = v;
  }
  __syncthreads();
}

// one-hot rows of the tile's classes (a class outside [0, C) gives a zero row)
__device__ __forceinline__ void stage_onehot(double* X, const int* cls, int C) {
  for (int i = threadIdx.x; i < kCatRows * C; i += kCatThreads) {
    const int r = i / C, c = i - r * C;
    X[r * kCatLd + c] = cls[r] == c ? 1.0 : 0.0;
  }
  __syncthreads();
}

// the LDS of a block: three activation tiles (ping, pong, the tower features) and the logit tile
struct CatLds {
  double *A, *B, *F, *z;
};
constexpr int kCatActDoubles = 3 * kCatRows * kCatLd + kCatRows * kCatZLd;
constexpr size_t kCatLdsBytes = (size_t)kCatActDoubles * sizeof(double);
__device__ __forceinline__ CatLds cat_lds(double* s) {
  return CatLds{s, s + kCatRows * kCatLd, s + 2 * kCatRows * kCatLd, s + 3 * kCatRows * kCatLd};
}

// native_speaker's logits of the tile into S.z; stage(X) puts the country rows into X.  hpark: the tile's rows of the
// parked h1, h2, h3 (or NULLs).
template <class StageC>
__device__ __forceinline__ void native_fwd(const CatNet& P, const CatLds& S, StageC stage, double* h1, double* h2,
                                           double* h3, int rows) {
  const float* t = P.theta;
  stage(S.A);
  dense_tile(S.A, kCatLd, P.Cc, t + P.L.w1, 1, P.Cc, t + P.L.b1, kCatH, S.B, kCatLd, true, nullptr, 0, h1, rows);
  dense_tile(S.B, kCatLd, kCatH, t + P.L.w2, 1, kCatH, t + P.L.b2, kCatH, S.A, kCatLd, true, nullptr, 0, h2, rows);
  dense_tile(S.A, kCatLd, kCatH, t + P.L.w3, 1, kCatH, t + P.L.b3, kCatH, S.B, kCatLd, true, nullptr, 0, h3, rows);
  dense_tile(S.B, kCatLd, kCatH, t + P.L.w4, 1, kCatH, t + P.L.b4, P.Cn, S.z, kCatZLd, false, nullptr, 0, nullptr, rows);
}

// one frozen tower: Linear(C, 64) ReLU, two Linear(64, 64) ReLU, Linear(64, 64), into columns col0 .. col0 + 63 of F
template <class Stage>
__device__ __forceinline__ void tower_fwd(const float* w, int C, const CatLds& S, Stage stage, int col0, int rows) {
  stage(S.A);
  const float* b = w + kCatT * C;
  dense_tile(S.A, kCatLd, C, w, 1, C, b, kCatT, S.B, kCatLd, true, nullptr, 0, nullptr, rows);
  w = b + kCatT; b = w + kCatT * kCatT;
  dense_tile(S.B, kCatLd, kCatT, w, 1, kCatT, b, kCatT, S.A, kCatLd, true, nullptr, 0, nullptr, rows);
  w = b + kCatT; b = w + kCatT * kCatT;
  dense_tile(S.A, kCatLd, kCatT, w, 1, kCatT, b, kCatT, S.B, kCatLd, true, nullptr, 0, nullptr, rows);
  w = b + kCatT; b = w + kCatT * kCatT;
  dense_tile(S.B, kCatLd, kCatT, w, 1, kCatT, b, kCatT, S.F + col0, kCatLd, false, nullptr, 0, nullptr, rows);
}

// accent's logits of the tile into S.z; fpark, hdpark: the tile's rows of the parked tower features and hidden layer
template <class StageC, class StageN>
__device__ __forceinline__ void accent_fwd(const CatNet& P, const CatLds& S, StageC stage_c, StageN stage_n, double* fpark,
                                           double* hdpark, int rows) {
  tower_fwd(P.towers + P.L.tower[0], P.Cc, S, stage_c, 0, rows);
  tower_fwd(P.towers + P.L.tower[1], P.Cn, S, stage_n, kCatT, rows);
  if (fpark) {
    for (int i = threadIdx.x; i < rows * kCatH; i += kCatThreads) {
      const int r = i / kCatH, c = i - r * kCatH;
      fpark[(long long)r * kCatH + c] = S.F[r * kCatLd + c];
    }
  }
  const float* t = P.theta;
  dense_tile(S.F, kCatLd, kCatH, t + P.L.v1, 1, kCatH, t + P.L.c1, kCatT, S.A, kCatLd, true, nullptr, 0, hdpark, rows);
  dense_tile(S.A, kCatLd, kCatT, t + P.L.v2, 1, kCatT, t + P.L.c2, P.Ca, S.z, kCatZLd, false, nullptr, 0, nullptr, rows);
}

// ---------------------------------------------------------------------------------------------------- ali_cat_nll
struct CatNllArgs {
  CatNet net;
  CatRows country, native, accent;
  long long N;
  const float* wgt;
  float gscale;
  float* lp;
  float* out3;
  unsigned long long* part;
  int* ctr;
  double* park;      // behind the partials; NULL without gradient
};

// One row's log-probability from its logits z (fp64, LDS); GRAD: z becomes w * d lp / d z.  The class is the first
// maximum of the target row.
template <bool GRAD>
__device__ __forceinline__ double nll_row(double* z, int C, const CatRows& T, long long n, double w) {
  bool ok;
  const float* tg = T.p + T.src(n, ok) * T.ld;
  int y = 0;
  float best = tg[0];
  for (int c = 1; c < C; ++c)
    if (tg[c] > best) { best = tg[c]; y = c; }
  double m = z[0];
  for (int c = 1; c < C; ++c) m = fmax(m, z[c]);
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += exp(z[c] - m);
  const double lse = m + log(s);
  const double lp = ok ? z[y] - lse : (double)NAN;
  if (GRAD)
    for (int c = 0; c < C; ++c) z[c] = w * ((c == y ? 1.0 : 0.0) - exp(z[c] - lse));
  return lp;
}

template <bool GRAD>
__global__ void __launch_bounds__(kCatThreads) cat_nll_kernel(const CatNllArgs a) {
  __shared__ double s_act[kCatActDoubles];
  __shared__ double s_w[kCatWaves];
  __shared__ int s_last;
  const CatLds S = cat_lds(s_act);
  const CatNet& P = a.net;
  const long long N = a.N;
  const long long tiles = (N + kCatRows - 1) / kCatRows;
  const CatPark K = cat_park(N, P.Cn, P.Ca);
  const int tr = threadIdx.x;                 // the row of the tile threads 0 .. 31 own in the softmax phases
  double sum_n = 0.0, sum_a = 0.0;

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long row0 = tile * kCatRows;
    const int rows = (int)(N - row0 < kCatRows ? N - row0 : kCatRows);
    auto stage_c = [&](double* X) { stage_rows(X, a.country, P.Cc, row0, rows); };
    auto stage_n = [&](double* X) { stage_rows(X, a.native, P.Cn, row0, rows); };
    double* pk = a.park;
    auto at = [&](long long off, int ld) { return (GRAD && pk) ? pk + off + row0 * ld : nullptr; };

    // ---- native_speaker
    native_fwd(P, S, stage_c, at(K.h1, kCatH), at(K.h2, kCatH), at(K.h3, kCatH), rows);
    if (tr < kCatRows) {
      double* z = S.z + tr * kCatZLd;
      if (tr < rows) {
        const long long n = row0 + tr;
        const double w = (double)a.gscale * (a.wgt ? (double)a.wgt[n * 2] : 1.0 / (double)N);
        const double lp = nll_row<GRAD>(z, P.Cn, a.native, n, w);
        if (a.lp) a.lp[n * 2] = (float)lp;
        sum_n += lp;
        if (GRAD)
          for (int c = 0; c < P.Cn; ++c) pk[K.dz4 + n * P.Cn + c] = z[c];
      } else if (GRAD) {
        for (int c = 0; c < P.Cn; ++c) z[c] = 0.0;
      }
    }
    __syncthreads();
    if (GRAD) {
      const float* t = P.theta;
      dense_tile(S.z, kCatZLd, P.Cn, t + P.L.w4, kCatH, 1, nullptr, kCatH, S.A, kCatLd, false, at(K.h3, kCatH), kCatH,
                 at(K.dz3, kCatH), rows);
      dense_tile(S.A, kCatLd, kCatH, t + P.L.w3, kCatH, 1, nullptr, kCatH, S.B, kCatLd, false, at(K.h2, kCatH), kCatH,
                 at(K.dz2, kCatH), rows);
      dense_tile(S.B, kCatLd, kCatH, t + P.L.w2, kCatH, 1, nullptr, kCatH, S.A, kCatLd, false, at(K.h1, kCatH), kCatH,
                 at(K.dz1, kCatH), rows);
    }

    // ---- accent
    accent_fwd(P, S, stage_c, stage_n, at(K.f, kCatH), at(K.hd, kCatT), rows);
    if (tr < kCatRows) {
      double* z = S.z + tr * kCatZLd;
      if (tr < rows) {
        const long long n = row0 + tr;
        const double w = (double)a.gscale * (a.wgt ? (double)a.wgt[n * 2 + 1] : 1.0 / (double)N);
        const double lp = nll_row<GRAD>(z, P.Ca, a.accent, n, w);
        if (a.lp) a.lp[n * 2 + 1] = (float)lp;
        sum_a += lp;
        if (GRAD)
          for (int c = 0; c < P.Ca; ++c) pk[K.dzd2 + n * P.Ca + c] = z[c];
      } else if (GRAD) {
        for (int c = 0; c < P.Ca; ++c) z[c] = 0.0;
      }
    }
    __syncthreads();
    if (GRAD)
      dense_tile(S.z, kCatZLd, P.Ca, P.theta + P.L.v2, kCatT, 1, nullptr, kCatT, S.A, kCatLd, false, at(K.hd, kCatT),
                 kCatT, at(K.dzd1, kCatT), rows);
  }

  if (!a.out3) return;
  sum_n = block_sum<kCatWaves>(sum_n, s_w);
  sum_a = block_sum<kCatWaves>(sum_a, s_w);
  if (threadIdx.x == 0) {
    partial_store(&a.part[2 * blockIdx.x], sum_n);
    partial_store(&a.part[2 * blockIdx.x + 1], sum_a);
  }
  if (!arrive_last(a.ctr, (int)gridDim.x, &s_last) || threadIdx.x != 0) return;
  double fn = 0.0, fa = 0.0;
  for (int b = 0; b < (int)gridDim.x; ++b) {           // blocks ascending, whichever block this is
    fn += partial_load(&a.part[2 * b]);
    fa += partial_load(&a.part[2 * b + 1]);
  }
  const double inv = 1.0 / (double)N;
  a.out3[0] = (float)(-(fn + fa) * inv);
  a.out3[1] = (float)(fn * inv);
  a.out3[2] = (float)(fa * inv);
}

// --------------------------------------------------------------------------------------------------- the weight gradients
struct CatWJob {
  const double* dz;      // [N][O] parked pre-activation gradients
  const double* xd;      // [N][K] parked inputs, or NULL: the country rows
  int O, K, woff, boff, tile0, ktiles;
};
struct CatWArgs {
  CatWJob job[6];
  CatRows country;
  long long N;
  float* gtheta;
};

__global__ void __launch_bounds__(kCatWThreads) cat_wgrad_kernel(const CatWArgs a) {
  __shared__ double s_red[kCatWWaves][4][64];
  int ji = 0;
#pragma unroll
  for (int q = 1; q < 6; ++q)
    if ((int)blockIdx.x >= a.job[q].tile0) ji = q;
  const CatWJob& J = a.job[ji];
  const int local = (int)blockIdx.x - J.tile0;
  const int ot = local / J.ktiles, kt = local - ot * J.ktiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int o = ot * 16 + lr, k = kt * 16 + lr;
  const long long N = a.N, steps = (N + 3) / 4;
  f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
  // kCatKU k-steps at a time, their operand loads issued together; the order of the sum is the order of the steps
  for (long long s0 = wave; s0 < steps; s0 += kCatWWaves * kCatKU) {
    double av[kCatKU], bv[kCatKU];
#pragma unroll
    for (int u = 0; u < kCatKU; ++u) {
      const long long n = (s0 + (long long)u * kCatWWaves) * 4 + lk;
      const bool nok = n < N;
      av[u] = (nok && o < J.O) ? J.dz[n * J.O + o] : 0.0;
      bv[u] = 0.0;
      if (nok) {
        if (k < J.K) {
          if (J.xd) {
            bv[u] = J.xd[n * J.K + k];
          } else {
            bool ok;
            const long long src = a.country.src(n, ok);
            bv[u] = ok ? (double)a.country.p[src * a.country.ld + k] : 0.0;
          }
        } else if (k == J.K) {
          bv[u] = 1.0;                              // the bias: input column K
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kCatKU; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_red[wave][r][lane] = acc[r];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kCatWWaves; ++w) v += s_red[w][r][lane];
    const int oo = ot * 16 + lk + 4 * r;
    if (oo < J.O) {
      if (k < J.K) a.gtheta[J.woff + oo * J.K + k] = (float)v;
      else if (k == J.K) a.gtheta[J.boff + oo] = (float)v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- ali_cat_map
struct CatMapKArgs {
  CatNet net;
  AliCatMapArgs m;
  int mode;
  long long N;
  uint64_t seed, offset;
  const long long* dev_counter;
};

// the first maximum of z[c] + e[c]: fp64 sums of stored fp32 values (z holds logits already rounded to fp32)
__device__ __forceinline__ int argmax_sum(const double* z, const float* e, int C) {
  int k = 0;
  double best = z[0] + (double)e[0];
  for (int c = 1; c < C; ++c) {
    const double v = z[c] + (double)e[c];
    if (v > best) { best = v; k = c; }
  }
  return k;
}

// One row of one node after its logits: rounds them to fp32 in place (what every decision reads), stores them, and
// returns the class the node takes in this mode.  stage 1 is the prediction pass of ALI_CAT_CF.  z, e (the draws) and
// nz (the row's noise, kept from stage 0 to stage 1) are LDS rows.
__device__ __forceinline__ int map_row(const CatMapKArgs& a, uint64_t key, int stage, int node, double* z, float* e,
                                       float* nz, long long n) {
  const int Cn = a.net.Cn, Ca = a.net.Ca, Ct = Cn + Ca;
  const int C = node ? Ca : Cn, nb = node ? Cn : 0;
  const long long N = a.N;
  const AliCatMapArgs& m = a.m;
  for (int c = 0; c < C; ++c) {
    const float zf = (float)z[c];
    z[c] = (double)zf;
    if (m.logits_out) m.logits_out[((long long)stage * N + n) * Ct + nb + c] = zf;
  }
  if (stage == 1) return ((m.cf_mask >> node) & 1) ? (int)m.v[node][n] : argmax_sum(z, nz, C);
  if (a.mode == ALI_CAT_LOGITS) return m.y[node] ? (int)m.y[node][n] : -1;
  // where this node's ordinary draws lie in the stream: behind the tries of a DIFFER call
  const uint64_t tries = a.mode == ALI_CAT_DIFFER ? (uint64_t)ALI_CAT_TRIES * (uint64_t)N * (uint64_t)(m.node ? Ca : Cn) : 0ull;
  const uint64_t base = a.offset + tries + (uint64_t)n * (uint64_t)Ct + (uint64_t)nb;
  if (a.mode == ALI_CAT_DIFFER && node == m.node) {
    const int forb = (int)m.v[node][n];
    int kept = 0;
    bool found = false;
    for (int t = 0; t < ALI_CAT_TRIES; ++t) {
      const uint64_t tb = a.offset + ((uint64_t)t * (uint64_t)N + (uint64_t)n) * (uint64_t)C;
      for (int c = 0; c < C; ++c) {
        e[c] = gumbel_at(key, tb + (uint64_t)c);
        if (m.g_out) m.g_out[((long long)t * N + n) * C + c] = e[c];
      }
      if (!found) {
        kept = argmax_sum(z, e, C);
        found = kept != forb;
      }
      if (found && !m.g_out) break;              // (with g_out every try is drawn and stored)
    }
    m.status[n] = found ? 0 : 1;
    return kept;
  }
  if (a.mode == ALI_CAT_SAMPLE || a.mode == ALI_CAT_DIFFER) {
    if (m.y[node]) return (int)m.y[node][n];
    for (int c = 0; c < C; ++c) {
      e[c] = gumbel_at(key, base + (uint64_t)c);
      if (m.g_out && a.mode == ALI_CAT_SAMPLE) m.g_out[n * Ct + nb + c] = e[c];
    }
    return argmax_sum(z, e, C);
  }
  // ALI_CAT_ABDUCT, ALI_CAT_CF: the posterior noise of the observed class (ali_gumbel_posterior's formulas)
  const long long yn = m.y[node][n];
  const bool ok = yn >= 0 && yn < C;
  const int yc = ok ? (int)yn : 0;
  double zmax = z[0];
  for (int c = 1; c < C; ++c) zmax = fmax(zmax, z[c]);
  double esum = 0.0;
  for (int c = 0; c < C; ++c) {
    esum += exp(z[c] - zmax);
    e[c] = gumbel_at(key, base + (uint64_t)c);
    if (m.g_out) m.g_out[n * Ct + nb + c] = e[c];
  }
  const double lse = zmax + log(esum);
  const double gy = (double)e[yc], zy = z[yc];
  const double ey = exp(-gy - zy);
  for (int c = 0; c < C; ++c) {
    double v = gumbel_posterior_at(c == yc, (double)e[c], z[c], gy, zy, ey, lse);
    if (!ok) v = NAN;
    nz[c] = (float)v;
    if (m.noise_out) m.noise_out[n * Ct + nb + c] = nz[c];
  }
  return ok ? yc : -1;
}

__global__ void __launch_bounds__(kCatThreads) cat_map_kernel(const CatMapKArgs a) {
  __shared__ double s_act[kCatActDoubles];
  __shared__ float s_nz[2][kCatRows][kCatMaxC];
  __shared__ float s_e[kCatRows][kCatMaxC];
  __shared__ int s_cls[kCatRows];
  const CatLds S = cat_lds(s_act);
  const CatNet& P = a.net;
  const AliCatMapArgs& m = a.m;
  const long long N = a.N;
  const long long tiles = (N + kCatRows - 1) / kCatRows;
  const uint64_t key = gumbel_key(rng_base_key(a.seed, a.dev_counter));
  const int tr = threadIdx.x;
  const CatRows obs_c{m.country, m.country_ld, nullptr, N};
  const CatRows cf_c{m.country_cf ? m.country_cf : m.country, m.country_cf ? m.country_cf_ld : m.country_ld, nullptr, N};
  const CatRows nat_rows{m.native_rows, m.native_ld, nullptr, N};
  const int stages = a.mode == ALI_CAT_CF ? 2 : 1;
  const bool writes = a.mode != ALI_CAT_LOGITS && a.mode != ALI_CAT_ABDUCT;

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long row0 = tile * kCatRows;
    const int rows = (int)(N - row0 < kCatRows ? N - row0 : kCatRows);
    for (int stage = 0; stage < stages; ++stage) {
      const CatRows& ctry = stage ? cf_c : obs_c;
      auto stage_c = [&](double* X) { stage_rows(X, ctry, P.Cc, row0, rows); };
      native_fwd(P, S, stage_c, nullptr, nullptr, nullptr, rows);
      if (tr < kCatRows) {
        int k = -1;
        if (tr < rows) {
          k = map_row(a, key, stage, 0, S.z + tr * kCatZLd, s_e[tr], s_nz[0][tr], row0 + tr);
          if (m.out[0] && writes && stage == stages - 1) m.out[0][row0 + tr] = k;
        }
        s_cls[tr] = k;
      }
      __syncthreads();
      const bool dense_native = a.mode == ALI_CAT_LOGITS && m.native_rows;
      auto stage_n = [&](double* X) {
        if (dense_native) stage_rows(X, nat_rows, P.Cn, row0, rows);
        else stage_onehot(X, s_cls, P.Cn);
      };
      accent_fwd(P, S, stage_c, stage_n, nullptr, nullptr, rows);
      if (tr < rows) {
        const int k = map_row(a, key, stage, 1, S.z + tr * kCatZLd, s_e[tr], s_nz[1][tr], row0 + tr);
        if (m.out[1] && writes && stage == stages - 1) m.out[1][row0 + tr] = k;
      }
      __syncthreads();
    }
  }
}

}  // namespace ali

using namespace ali;

static bool cat_dims_ok(const char* who, int64_t N, int Cc, int Cn, int Ca) {
  if (Cc < 1 || Cc > kCatMaxC || Cn < 1 || Cn > kCatMaxC || Ca < 1 || Ca > kCatMaxC) {
    set_error("%s: class counts (%d, %d, %d) outside [1, %d]", who, Cc, Cn, Ca, kCatMaxC);
    return false;
  }
  if (N < 1 || N >= (1LL << 24)) { set_error("%s: N = %lld outside [1, 2^24)", who, (long long)N); return false; }
  return true;
}

// the six trained layers as weight-gradient jobs; returns the number of blocks
static int cat_wjobs(CatWJob* job, const CatLayout& L, const CatPark& K, double* pk, int Cc, int Cn, int Ca) {
  const struct { long long dz, x; int O, Kd, w, b; } lay[6] = {
      {K.dz1, -1, kCatH, Cc, L.w1, L.b1},     {K.dz2, K.h1, kCatH, kCatH, L.w2, L.b2}, {K.dz3, K.h2, kCatH, kCatH, L.w3, L.b3},
      {K.dz4, K.h3, Cn, kCatH, L.w4, L.b4},   {K.dzd1, K.f, kCatT, kCatH, L.v1, L.c1}, {K.dzd2, K.hd, Ca, kCatT, L.v2, L.c2}};
  int tile = 0;
  for (int q = 0; q < 6; ++q) {
    job[q].dz = pk ? pk + lay[q].dz : nullptr;
    job[q].xd = (pk && lay[q].x >= 0) ? pk + lay[q].x : nullptr;
    job[q].O = lay[q].O;
    job[q].K = lay[q].Kd;
    job[q].woff = lay[q].w;
    job[q].boff = lay[q].b;
    job[q].tile0 = tile;
    job[q].ktiles = (lay[q].Kd + 1 + 15) / 16;
    tile += ((lay[q].O + 15) / 16) * job[q].ktiles;
  }
  return tile;
}

extern "C" int ali_cat_plan(int64_t N, int32_t Cc, int32_t Cn, int32_t Ca, int32_t entry, AliCatPlan* plan) {
  if (!plan) { set_error("ali_cat_plan: plan must not be NULL"); return ALI_ERR_BAD_ARG; }
  if (!cat_dims_ok("ali_cat_plan", N, Cc, Cn, Ca)) return ALI_ERR_BAD_ARG;
  if (entry != ALI_CAT_ENTRY_NLL && entry != ALI_CAT_ENTRY_GRAD && entry != ALI_CAT_ENTRY_MAP) {
    set_error("ali_cat_plan: entry %d is none of ALI_CAT_ENTRY_NLL / GRAD / MAP", (int)entry);
    return ALI_ERR_BAD_ARG;
  }
  const int64_t tiles = (N + kCatRows - 1) / kCatRows;
  plan->tile_rows = kCatRows;
  plan->tiles = (int32_t)tiles;
  plan->grid = (int32_t)(tiles < kCatMaxBlocks ? tiles : kCatMaxBlocks);
  plan->threads = kCatThreads;
  plan->tiles_per_block = (int32_t)((tiles + plan->grid - 1) / plan->grid);
  plan->grid2 = plan->threads2 = 0;
  plan->lds_bytes = (int32_t)kCatLdsBytes;
  plan->ws_bytes = 0;
  if (entry != ALI_CAT_ENTRY_MAP) plan->ws_bytes = kWsReserved + kCatPartBytes;
  if (entry == ALI_CAT_ENTRY_GRAD) {
    CatWJob job[6];
    plan->grid2 = cat_wjobs(job, cat_layout(Cc, Cn, Ca), cat_park(N, Cn, Ca), nullptr, Cc, Cn, Ca);
    plan->threads2 = kCatWThreads;
    plan->ws_bytes += (uint64_t)cat_park(N, Cn, Ca).total * sizeof(double);
  }
  return ALI_OK;
}

extern "C" int ali_cat_nll(const float* theta, const float* towers, int32_t Cc, int32_t Cn, int32_t Ca,
                           const float* country, int64_t sc, const float* native, int64_t sn, const float* accent,
                           int64_t sa, const int64_t* index, int64_t src_rows, int64_t N, const float* wgt, float gscale,
                           float* lp, float* out3, float* gtheta, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!theta || !towers || !country || !native || !accent) {
    set_error("ali_cat_nll: theta, towers, country, native and accent must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  if (!lp && !out3 && !gtheta) { set_error("ali_cat_nll: nothing to compute (lp, out3 and gtheta are all NULL)"); return ALI_ERR_BAD_ARG; }
  AliCatPlan pl;
  const int rc = ali_cat_plan(N, Cc, Cn, Ca, gtheta ? ALI_CAT_ENTRY_GRAD : ALI_CAT_ENTRY_NLL, &pl);
  if (rc != ALI_OK) return rc;
  if (!index) src_rows = N;
  if (src_rows < 1 || src_rows >= (1LL << 24) || sc < Cc || sn < Cn || sa < Ca || sc > (1 << 16) || sn > (1 << 16) || sa > (1 << 16)) {
    set_error("ali_cat_nll: src_rows = %lld outside [1, 2^24), or a row stride below its width or above 2^16", (long long)src_rows);
    return ALI_ERR_BAD_ARG;
  }
  if (!ws || ws_bytes < pl.ws_bytes) {
    set_error("ali_cat_nll: workspace too small (%llu bytes needed, ali_cat_plan)", (unsigned long long)pl.ws_bytes);
    return ALI_ERR_WORKSPACE;
  }
  CatNllArgs a;
  a.net = CatNet{theta, towers, Cc, Cn, Ca, cat_layout(Cc, Cn, Ca)};
  const long long* ix = reinterpret_cast<const long long*>(index);
  a.country = CatRows{country, sc, ix, src_rows};
  a.native = CatRows{native, sn, ix, src_rows};
  a.accent = CatRows{accent, sa, ix, src_rows};
  a.N = N;
  a.wgt = wgt;
  a.gscale = gscale;
  a.lp = lp;
  a.out3 = out3;
  a.part = reinterpret_cast<unsigned long long*>(ws_payload(ws));
  a.ctr = reinterpret_cast<int*>(ws) + kFoldCtr;
  a.park = gtheta ? reinterpret_cast<double*>(static_cast<char*>(ws_payload(ws)) + kCatPartBytes) : nullptr;
  if (gtheta) {
    hipLaunchKernelGGL(cat_nll_kernel<true>, dim3(pl.grid), dim3(kCatThreads), 0, ST(stream), a);
    int rl = check_launch("cat_nll_kernel");
    if (rl != ALI_OK) return rl;
    CatWArgs w;
    cat_wjobs(w.job, a.net.L, cat_park(N, Cn, Ca), a.park, Cc, Cn, Ca);
    w.country = a.country;
    w.N = N;
    w.gtheta = gtheta;
    hipLaunchKernelGGL(cat_wgrad_kernel, dim3(pl.grid2), dim3(kCatWThreads), 0, ST(stream), w);
    return check_launch("cat_wgrad_kernel");
  }
  hipLaunchKernelGGL(cat_nll_kernel<false>, dim3(pl.grid), dim3(kCatThreads), 0, ST(stream), a);
  return check_launch("cat_nll_kernel");
}

extern "C" int ali_cat_map(int32_t mode, const float* theta, const float* towers, int32_t Cc, int32_t Cn, int32_t Ca,
                           int64_t N, const AliCatMapArgs* m, uint64_t seed, const int64_t* dev_counter, uint64_t offset,
                           ali_stream_t stream) {
  if (!theta || !towers || !m || !m->country) {
    set_error("ali_cat_map: theta, towers, the arguments and their country rows must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  AliCatPlan pl;
  const int rc = ali_cat_plan(N, Cc, Cn, Ca, ALI_CAT_ENTRY_MAP, &pl);
  if (rc != ALI_OK) return rc;
  if (mode < ALI_CAT_LOGITS || mode > ALI_CAT_CF) { set_error("ali_cat_map: mode %d is none of ALI_CAT_LOGITS .. ALI_CAT_CF", (int)mode); return ALI_ERR_BAD_ARG; }
  if (m->country_ld < Cc || m->country_ld > (1 << 16) || (m->country_cf && (m->country_cf_ld < Cc || m->country_cf_ld > (1 << 16))) ||
      (m->native_rows && (m->native_ld < Cn || m->native_ld > (1 << 16)))) {
    set_error("ali_cat_map: a row stride below its width or above 2^16");
    return ALI_ERR_BAD_ARG;
  }
  const char* bad = nullptr;
  switch (mode) {
    case ALI_CAT_LOGITS:
      if (!m->logits_out || (!m->native_rows && !m->y[0])) bad = "ALI_CAT_LOGITS needs logits_out and native_rows or y[0]";
      break;
    case ALI_CAT_SAMPLE:
      if ((!m->y[0] && !m->out[0]) || (!m->y[1] && !m->out[1])) bad = "ALI_CAT_SAMPLE needs out[node] for every node it draws";
      break;
    case ALI_CAT_DIFFER:
      if (m->node < 0 || m->node > 1 || !m->v[m->node] || !m->out[m->node] || !m->status || m->y[m->node])
        bad = "ALI_CAT_DIFFER needs node in {0, 1}, its forbidden classes v[node], out[node] and status, and no held y[node]";
      else if (!m->y[1 - m->node] && !m->out[1 - m->node]) bad = "ALI_CAT_DIFFER needs out[] for the other node when it is drawn";
      break;
    case ALI_CAT_ABDUCT:
      if (!m->y[0] || !m->y[1] || !m->noise_out) bad = "ALI_CAT_ABDUCT needs both observed classes and noise_out";
      break;
    default:
      if (!m->y[0] || !m->y[1] || !m->out[0] || !m->out[1]) bad = "ALI_CAT_CF needs both observed classes and both outputs";
      else if ((m->cf_mask & ~3) || ((m->cf_mask & 1) && !m->v[0]) || ((m->cf_mask & 2) && !m->v[1]))
        bad = "ALI_CAT_CF: cf_mask outside [0, 3], or a node intervened on without v[node]";
  }
  if (bad) { set_error("ali_cat_map: %s", bad); return ALI_ERR_BAD_ARG; }
  CatMapKArgs a;
  a.net = CatNet{theta, towers, Cc, Cn, Ca, cat_layout(Cc, Cn, Ca)};
  a.m = *m;
  a.mode = mode;
  a.N = N;
  a.seed = seed;
  a.offset = offset;
  a.dev_counter = reinterpret_cast<const long long*>(dev_counter);
  hipLaunchKernelGGL(cat_map_kernel, dim3(pl.grid), dim3(kCatThreads), 0, ST(stream), a);
  return check_launch("cat_map_kernel");
}

extern "C" int32_t ali_cat_theta_size(int32_t Cc, int32_t Cn, int32_t Ca, int32_t towers) {
  if (Cc < 1 || Cc > kCatMaxC || Cn < 1 || Cn > kCatMaxC || Ca < 1 || Ca > kCatMaxC) return 0;
  const CatLayout L = cat_layout(Cc, Cn, Ca);
  return towers ? L.towers_total : L.total;
}
