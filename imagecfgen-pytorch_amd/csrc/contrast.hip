// The contrastive family (include/ali_hip.h: ali_ct_attack, ali_ct_book, ali_ct_cem_update, ali_ct_ce_update,
// ali_ct_pp_attack, ali_ct_pp_update): what sits around the classifier's conv chain when the pertinent-negative and
// pertinent-positive searches of the contrastive explanation method (Dhurandhar et al. 2018) and the counterfactual
// search of Wachter et al. 2017 run B rows as B independent searches.
// The chain carries all the arithmetic that matters; these six are bound by the launch (a row is a 28 x 28 image, a
// logit row ten numbers), so the row arithmetic is fp64 -- every fp32 result is the rounding of an fp64 evaluation --
// and every sum runs in a fixed order (ali_reduce.h).  No float atomics, no host reads, no allocation: the same inputs
// give the same bits.  Everything that decides what a launch does -- the iteration of the round, the round, the row's
// c -- is read from device memory, so ONE recorded graph serves every iteration of every round.
//
// One replay at iteration counter k = it[b] (0 <= k <= K):
//   ali_ct_(pp_)attack  logits of the iterate v_k (evaluation) and of the gradient point (seed of the data gradient)
//   ali_ct_book         v_k into the best-so-far (k >= 1); at k == K the row's c / c_lo / c_hi move
//   ali_ct_*_update     k <  K: the step to v_(k+1), its distances, it[b] = k + 1
//                       k == K: the round is over: v (y, the moments) start again from x0 (pp: from the background),
//                       it[b] = 0, rnd[b] += 1
// ali_ct_book runs before the update, so both see the same k.
//
// NaN (what falls out, untested): comparisons with NaN are false, so a NaN logit never becomes the arg-max, a NaN
// distance never becomes the best and a NaN gradient norm is not clipped; what is computed from a NaN is NaN.
#include "ali_reduce.h"

#include <initializer_list>

namespace ali {

constexpr int kCtBlock = 256;
constexpr int kCtWaves = kCtBlock / 64;

// ---------------------------------------------------------------------------------------------------- ali_ct_attack
// One thread per search row b (the eg_seed argument: C is ten, a wave per row would idle 54 lanes).  Strict > in
// ascending column order keeps the first maximum, as ali_softmax_xent does.
__device__ __forceinline__ int ct_argmax(const float* __restrict__ z, int C) {
  float zmax = -INFINITY;
  int zi = 0;                                                        // (a row of -inf / NaN only: column 0)
  for (int j = 0; j < C; ++j) {
    const float zv = z[j];
    if (zv > zmax) { zmax = zv; zi = j; }
  }
  return zi;
}

// the first largest column other than t (t in [0, C), C >= 2)
__device__ __forceinline__ int ct_other(const float* __restrict__ z, int C, int t) {
  float omax = -INFINITY;
  int oi = t == 0 ? 1 : 0;
  for (int j = 0; j < C; ++j) {
    const float zv = z[j];
    if (j != t && zv > omax) { omax = zv; oi = j; }
  }
  return oi;
}

__device__ __forceinline__ int ct_clamp_label(int tg, int C) {
  return tg < 0 ? 0 : (tg >= C ? C - 1 : tg);                        // (a label outside [0, C) reads no other row)
}

__global__ void __launch_bounds__(kCtBlock)
ct_attack_kernel(const float* __restrict__ logit, int C, int B, int eval_off, int grad_off,
                 const int* __restrict__ t0, const float* __restrict__ c, double kappa, float* __restrict__ seed,
                 int seed_ld, float* __restrict__ A, int* __restrict__ pred, int* __restrict__ succ) {
  const int b = blockIdx.x * kCtBlock + threadIdx.x;
  if (b >= B) return;
  const int zi = ct_argmax(logit + (long long)(eval_off + b) * C, C);
  pred[b] = zi;
  if (!t0) return;
  const int tg = t0[b];
  succ[b] = zi != tg ? 1 : 0;
  const int t = ct_clamp_label(tg, C);
  const float* zg = logit + (long long)(grad_off + b) * C;
  const int oi = ct_other(zg, C, t);
  const double margin = ((double)zg[t] - (double)zg[oi]) + kappa;
  const bool active = margin > 0.0;
  A[b] = active ? (float)margin : 0.f;
  const float cv = c[b];
  float* sr = seed + (long long)b * seed_ld;
  for (int j = 0; j < seed_ld; ++j) sr[j] = !active ? 0.f : (j == t ? cv : (j == oi ? -cv : 0.f));
}

// --------------------------------------------------------------------------------------------- ali_ct_pp_attack
// The pertinent-positive hinge: the sense turned round.  A success keeps t0; A = max(0, other - own +
// kappa) and its seed c (e_other - e_t0).  t0 is required.
__global__ void __launch_bounds__(kCtBlock)
ct_pp_attack_kernel(const float* __restrict__ logit, int C, int B, int eval_off, int grad_off,
                    const int* __restrict__ t0, const float* __restrict__ c, double kappa, float* __restrict__ seed,
                    int seed_ld, float* __restrict__ A, int* __restrict__ pred, int* __restrict__ succ) {
  const int b = blockIdx.x * kCtBlock + threadIdx.x;
  if (b >= B) return;
  const int zi = ct_argmax(logit + (long long)(eval_off + b) * C, C);
  pred[b] = zi;
  const int tg = t0[b];
  succ[b] = zi == tg ? 1 : 0;
  const int t = ct_clamp_label(tg, C);
  const float* zg = logit + (long long)(grad_off + b) * C;
  const int oi = ct_other(zg, C, t);
  const double margin = ((double)zg[oi] - (double)zg[t]) + kappa;
  const bool active = margin > 0.0;
  A[b] = active ? (float)margin : 0.f;
  const float cv = c[b];
  float* sr = seed + (long long)b * seed_ld;
  for (int j = 0; j < seed_ld; ++j) sr[j] = !active ? 0.f : (j == oi ? cv : (j == t ? -cv : 0.f));
}

// ------------------------------------------------------------------------------------------------------ ali_ct_book
// One block per row.  Every thread reads the decision's inputs before the barrier; thread 0 writes them after it.
__global__ void __launch_bounds__(kCtBlock)
ct_book_kernel(const float* __restrict__ v, const float* __restrict__ dist, const int* __restrict__ succ,
               const int* __restrict__ pred, const int* __restrict__ it, int K, long long N, int vec4,
               float* __restrict__ best,
               float* __restrict__ best_dist, int* __restrict__ best_label, int* __restrict__ found,
               int* __restrict__ round_succ, float* __restrict__ c, float* __restrict__ c_lo, float* __restrict__ c_hi,
               int* __restrict__ copied) {
  const long long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int k = it[b];
  const bool hit = k >= 1 && succ[b] != 0;                           // (k == 0: v is x0, no iterate of the round)
  const float d = dist[b];
  const bool better = hit && d < best_dist[b];
  __syncthreads();
  if (better) {
    const float* vr = v + b * N;
    float* br = best + b * N;
    if (vec4) {
      const f32x4* v4 = reinterpret_cast<const f32x4*>(vr);
      f32x4* b4 = reinterpret_cast<f32x4*>(br);
      for (long long i = tid; i < (N >> 2); i += kCtBlock) b4[i] = v4[i];
    } else {
      for (long long i = tid; i < N; i += kCtBlock) br[i] = vr[i];
    }
  }
  if (tid != 0) return;
  copied[b] = better ? 1 : 0;
  if (better) {
    best_dist[b] = d;
    best_label[b] = pred[b];
    found[b] = 1;
  }
  const int rs = (round_succ[b] != 0 || hit) ? 1 : 0;
  if (k < K) {
    round_succ[b] = rs;
    return;
  }
  // the round is over: the binary search on c
  const double cv = (double)c[b], lo = (double)c_lo[b], hi = (double)c_hi[b];
  if (rs) {
    const double h2 = fmin(hi, cv);
    c_hi[b] = (float)h2;
    c[b] = (float)((lo + h2) / 2.0);
  } else {
    const double l2 = fmax(lo, cv);
    c_lo[b] = (float)l2;
    c[b] = hi < 1e9 ? (float)((l2 + hi) / 2.0) : (float)(cv * 10.0);
  }
  round_succ[b] = 0;
}

// -------------------------------------------------------------------------------------------------- the two updates
// One block per row, a row loop inside.  it[b] decides the branch for the whole block and thread 0 rewrites it on
// both branches, so every thread reads it and the block meets at a barrier before any branch is taken (as in
// ct_book_kernel).  Thread t takes the elements (or the groups of four) t, t + 256, ... in
// ascending order; its partial sums go through block_sum (lanes, then waves 0..3).  V = 4: the row's offset b * N is
// a multiple of four floats, so x0 / v / y / the moments move as 16-byte accesses; the classifier's input gradient is
// read one float per pixel either way (plane 0 of an NHWC tensor: elements gs floats apart).
template <int V>
struct Vec;
template <>
struct Vec<1> {
  float e[1];
  __device__ __forceinline__ void load(const float* p) { e[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = e[0]; }
};
template <>
struct Vec<4> {
  float e[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    e[0] = q[0]; e[1] = q[1]; e[2] = q[2]; e[3] = q[3];
  }
  __device__ __forceinline__ void store(float* p) const {
    f32x4 q;
    q[0] = e[0]; q[1] = e[1]; q[2] = e[2]; q[3] = e[3];
    *reinterpret_cast<f32x4*>(p) = q;
  }
};

// FISTA step of the pertinent-negative search
template <int V>
__global__ void __launch_bounds__(kCtBlock)
ct_cem_update_kernel(const float* __restrict__ gx, int gs, float* __restrict__ v, float* __restrict__ y,
                     const float* __restrict__ x0, const float* __restrict__ lo, const float* __restrict__ hi,
                     int* __restrict__ it, int* __restrict__ rnd, int K, double lr, double beta, double clip,
                     long long N, float* __restrict__ l1, float* __restrict__ l2, float* __restrict__ dist,
                     float* __restrict__ gnorm) {
  __shared__ double s_red[kCtWaves];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int k = it[b];
  __syncthreads();                                                   // every wave has read it[b] before thread 0 moves it
  float* vr = v + b * N;
  float* yr = y + b * N;
  const float* xr = x0 + b * N;
  const float* gr = gx + b * N * gs;
  if (k >= K) {                                                      // the round is over: start again from x0
    for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
      Vec<V> xv;
      xv.load(xr + i);
      xv.store(vr + i);
      xv.store(yr + i);
    }
    if (tid == 0) {
      it[b] = 0;
      rnd[b] += 1;
      l1[b] = 0.f; l2[b] = 0.f; dist[b] = 0.f;
    }
    return;
  }
  double ss = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> xv, yv;
    xv.load(xr + i);
    yv.load(yr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double g = (double)gr[(i + j) * gs] + 2.0 * ((double)yv.e[j] - (double)xv.e[j]);
      ss += g * g;
    }
  }
  ss = block_sum<kCtWaves>(ss, s_red);
  const double norm = sqrt(ss);
  const double scale = norm > clip ? clip / norm : 1.0;
  const double step = lr * sqrt(1.0 - (double)k / (double)K);
  const double mom = (double)k / (double)(k + 3);
  const double lob = (double)lo[b], hib = (double)hi[b];
  double a1 = 0.0, a2 = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> xv, yv, vv;
    xv.load(xr + i);
    yv.load(yr + i);
    vv.load(vr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double x = (double)xv.e[j], yo = (double)yv.e[j];
      const double g = ((double)gr[(i + j) * gs] + 2.0 * (yo - x)) * scale;
      const double u = yo - step * g;
      const double d = u - x;
      double w = x;                                                  // shrink around x0, inside [lo, hi]
      if (d > beta) w = fmin(u - beta, hib);
      else if (d < -beta) w = fmax(u + beta, lob);
      const bool up = w > x;                                         // only additions
      const double vn = up ? w : x;
      const float vf = up ? (float)w : xv.e[j];
      const double yn = vn + mom * (vn - (double)vv.e[j]);
      yv.e[j] = yn > x ? (float)yn : xv.e[j];
      vv.e[j] = vf;
      const double df = (double)vf - x;                              // the distances of the iterate as stored
      a1 += fabs(df);
      a2 += df * df;
    }
    vv.store(vr + i);
    yv.store(yr + i);
  }
  a1 = block_sum<kCtWaves>(a1, s_red);
  a2 = block_sum<kCtWaves>(a2, s_red);
  if (tid == 0) {
    l1[b] = (float)a1;
    l2[b] = (float)a2;
    dist[b] = (float)(a2 + beta * a1);
    gnorm[b] = (float)norm;
    it[b] = k + 1;
  }
}

// FISTA step of the pertinent-positive search ("Pertinent positives"): ct_cem_update_kernel's shape with
// the shrink centred on the background b and the box [min(b, x0_i), max(b, x0_i)] per pixel.  b, x0_i and the box ends
// are fp32 values, so a pixel clamped to an end or shrunk to b stores that float itself.
template <int V>
__global__ void __launch_bounds__(kCtBlock)
ct_pp_update_kernel(const float* __restrict__ gx, int gs, float* __restrict__ v, float* __restrict__ y,
                    const float* __restrict__ x0, float bg, int* __restrict__ it, int* __restrict__ rnd, int K,
                    double lr, double beta, double clip, long long N, float* __restrict__ l1, float* __restrict__ l2,
                    float* __restrict__ dist, float* __restrict__ gnorm) {
  __shared__ double s_red[kCtWaves];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int k = it[b];
  __syncthreads();                                                   // every wave has read it[b] before thread 0 moves it
  float* vr = v + b * N;
  float* yr = y + b * N;
  const float* xr = x0 + b * N;
  const float* gr = gx + b * N * gs;
  if (k >= K) {                                                      // the round is over: start again from b
    Vec<V> bv;
#pragma unroll
    for (int j = 0; j < V; ++j) bv.e[j] = bg;
    for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
      bv.store(vr + i);
      bv.store(yr + i);
    }
    if (tid == 0) {
      it[b] = 0;
      rnd[b] += 1;
      l1[b] = 0.f; l2[b] = 0.f; dist[b] = 0.f;
    }
    return;
  }
  const double bd = (double)bg;
  double ss = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> yv;
    yv.load(yr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double g = (double)gr[(i + j) * gs] + 2.0 * ((double)yv.e[j] - bd);
      ss += g * g;
    }
  }
  ss = block_sum<kCtWaves>(ss, s_red);
  const double norm = sqrt(ss);
  const double scale = norm > clip ? clip / norm : 1.0;
  const double step = lr * sqrt(1.0 - (double)k / (double)K);
  const double mom = (double)k / (double)(k + 3);
  double a1 = 0.0, a2 = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> xv, yv, vv;
    xv.load(xr + i);
    yv.load(yr + i);
    vv.load(vr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double x = (double)xv.e[j], yo = (double)yv.e[j];
      const double lo = fmin(bd, x), hi = fmax(bd, x);
      const double g = ((double)gr[(i + j) * gs] + 2.0 * (yo - bd)) * scale;
      const double u = yo - step * g;
      const double d = u - bd;
      double w = bd;                                                 // shrink around b
      if (d > beta) w = u - beta;
      else if (d < -beta) w = u + beta;
      const double vn = w < lo ? lo : (w > hi ? hi : w);            // into the box
      const double ym = vn + mom * (vn - (double)vv.e[j]);
      const double yn = ym < lo ? lo : (ym > hi ? hi : ym);
      const float vf = (float)vn;
      yv.e[j] = (float)yn;
      vv.e[j] = vf;
      const double df = (double)vf - bd;                             // the distances of the iterate as stored
      a1 += fabs(df);
      a2 += df * df;
    }
    vv.store(vr + i);
    yv.store(yr + i);
  }
  a1 = block_sum<kCtWaves>(a1, s_red);
  a2 = block_sum<kCtWaves>(a2, s_red);
  if (tid == 0) {
    l1[b] = (float)a1;
    l2[b] = (float)a2;
    dist[b] = (float)(a2 + beta * a1);
    gnorm[b] = (float)norm;
    it[b] = k + 1;
  }
}

// Adam step of the counterfactual search
template <int V>
__global__ void __launch_bounds__(kCtBlock)
ct_ce_update_kernel(const float* __restrict__ gx, int gs, float* __restrict__ v, const float* __restrict__ x0,
                    const float* __restrict__ lo, const float* __restrict__ hi, float* __restrict__ m,
                    float* __restrict__ v2, int* __restrict__ it, int* __restrict__ rnd, int K, double lr, double gamma,
                    double clip, double beta1, double beta2, double eps, long long N, float* __restrict__ l1,
                    float* __restrict__ gnorm) {
  __shared__ double s_red[kCtWaves];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int k = it[b];
  __syncthreads();                                                   // every wave has read it[b] before thread 0 moves it
  float* vr = v + b * N;
  float* mr = m + b * N;
  float* sr = v2 + b * N;
  const float* xr = x0 + b * N;
  const float* gr = gx + b * N * gs;
  if (k >= K) {                                                      // the round is over: x0 and a fresh optimiser
    Vec<V> zero;
#pragma unroll
    for (int j = 0; j < V; ++j) zero.e[j] = 0.f;
    for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
      Vec<V> xv;
      xv.load(xr + i);
      xv.store(vr + i);
      zero.store(mr + i);
      zero.store(sr + i);
    }
    if (tid == 0) {
      it[b] = 0;
      rnd[b] += 1;
      l1[b] = 0.f;
    }
    return;
  }
  double ss = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> xv, vv;
    xv.load(xr + i);
    vv.load(vr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double df = (double)vv.e[j] - (double)xv.e[j];
      const double g = (double)gr[(i + j) * gs] + gamma * (df > 0.0 ? 1.0 : (df < 0.0 ? -1.0 : 0.0));
      ss += g * g;
    }
  }
  ss = block_sum<kCtWaves>(ss, s_red);
  const double norm = sqrt(ss);
  const double scale = norm > clip ? clip / norm : 1.0;
  const double t = (double)(k + 1);
  const double step = lr / (1.0 - pow(beta1, t));
  const double bias2 = sqrt(1.0 - pow(beta2, t));
  const double lob = (double)lo[b], hib = (double)hi[b];
  double a1 = 0.0;
  for (long long i = (long long)tid * V; i < N; i += kCtBlock * V) {
    Vec<V> xv, vv, mv, sv;
    xv.load(xr + i);
    vv.load(vr + i);
    mv.load(mr + i);
    sv.load(sr + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double x = (double)xv.e[j], vo = (double)vv.e[j];
      const double df = vo - x;
      const double g = ((double)gr[(i + j) * gs] + gamma * (df > 0.0 ? 1.0 : (df < 0.0 ? -1.0 : 0.0))) * scale;
      const double mn = beta1 * (double)mv.e[j] + (1.0 - beta1) * g;
      const double sn = beta2 * (double)sv.e[j] + (1.0 - beta2) * g * g;
      const double vn = vo - step * mn / (sqrt(sn) / bias2 + eps);
      const float vf = vn < lob ? lo[b] : (vn > hib ? hi[b] : (float)vn);
      mv.e[j] = (float)mn;
      sv.e[j] = (float)sn;
      vv.e[j] = vf;
      a1 += fabs((double)vf - x);
    }
    vv.store(vr + i);
    mv.store(mr + i);
    sv.store(sr + i);
  }
  a1 = block_sum<kCtWaves>(a1, s_red);
  if (tid == 0) {
    l1[b] = (float)a1;
    gnorm[b] = (float)norm;
    it[b] = k + 1;
  }
}

// rows of four floats at 16-byte offsets: N a multiple of four and every row buffer 16-byte aligned
static bool ct_vec4(long long N, std::initializer_list<const void*> ptrs) {
  if (N & 3) return false;
  for (const void* p : ptrs)
    if (!aligned16(p)) return false;
  return true;
}

static int ct_rows(const char* who, int32_t B, int64_t N, int32_t gx_stride, int32_t K) {
  if (B < 1 || N < 1 || N >= (1LL << 31) || gx_stride < 1 || gx_stride > 64 || K < 1) {
    set_error("%s: B = %d, N = %lld outside [1, 2^31), gx_stride = %d outside [1, 64] or K = %d", who, (int)B,
              (long long)N, (int)gx_stride, (int)K);
    return ALI_ERR_BAD_ARG;
  }
  return ALI_OK;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_ct_attack(const float* logit, int32_t R, int32_t C, int32_t B, int32_t eval_off, int32_t grad_off,
                             const int32_t* t0, const float* c, double kappa, float* seed, int32_t seed_ld, float* A,
                             int32_t* pred, int32_t* succ, ali_stream_t stream) {
  if (B < 1 || C < 2 || C > 1024 || eval_off < 0 || grad_off < 0 || (long long)eval_off + B > R ||
      (long long)grad_off + B > R || (long long)R * C >= (1LL << 31)) {
    set_error("ali_ct_attack: B = %d, C = %d outside [2, 1024], or the rows [%d, %d + B) / [%d, %d + B) leave the %d "
              "logit rows", (int)B, (int)C, (int)eval_off, (int)eval_off, (int)grad_off, (int)grad_off, (int)R);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !pred) {
    set_error("ali_ct_attack: logit and pred must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  if (t0 && (!c || !seed || !A || !succ || seed_ld < C || (long long)B * seed_ld >= (1LL << 31))) {
    set_error("ali_ct_attack: with t0, c / seed / A / succ must not be NULL and seed_ld = %d at least C = %d",
              (int)seed_ld, (int)C);
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(ct_attack_kernel, dim3((unsigned)((B + kCtBlock - 1) / kCtBlock)), dim3(kCtBlock), 0, ST(stream),
                     logit, (int)C, (int)B, (int)eval_off, (int)grad_off, reinterpret_cast<const int*>(t0), c, kappa,
                     seed, (int)seed_ld, A, reinterpret_cast<int*>(pred), reinterpret_cast<int*>(succ));
  return check_launch("ct_attack_kernel");
}

extern "C" int ali_ct_pp_attack(const float* logit, int32_t R, int32_t C, int32_t B, int32_t eval_off,
                                int32_t grad_off, const int32_t* t0, const float* c, double kappa, float* seed,
                                int32_t seed_ld, float* A, int32_t* pred, int32_t* succ, ali_stream_t stream) {
  if (B < 1 || C < 2 || C > 1024 || eval_off < 0 || grad_off < 0 || (long long)eval_off + B > R ||
      (long long)grad_off + B > R || (long long)R * C >= (1LL << 31)) {
    set_error("ali_ct_pp_attack: B = %d, C = %d outside [2, 1024], or the rows [%d, %d + B) / [%d, %d + B) leave the "
              "%d logit rows", (int)B, (int)C, (int)eval_off, (int)eval_off, (int)grad_off, (int)grad_off, (int)R);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !pred || !t0 || !c || !seed || !A || !succ || seed_ld < C || (long long)B * seed_ld >= (1LL << 31)) {
    set_error("ali_ct_pp_attack: no pointer may be NULL and seed_ld = %d must be at least C = %d", (int)seed_ld, (int)C);
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(ct_pp_attack_kernel, dim3((unsigned)((B + kCtBlock - 1) / kCtBlock)), dim3(kCtBlock), 0,
                     ST(stream), logit, (int)C, (int)B, (int)eval_off, (int)grad_off,
                     reinterpret_cast<const int*>(t0), c, kappa, seed, (int)seed_ld, A, reinterpret_cast<int*>(pred),
                     reinterpret_cast<int*>(succ));
  return check_launch("ct_pp_attack_kernel");
}

extern "C" int ali_ct_book(const float* v, const float* dist, const int32_t* succ, const int32_t* pred,
                           const int32_t* it, int32_t K, int32_t B, int64_t N, float* best, float* best_dist,
                           int32_t* best_label, int32_t* found, int32_t* round_succ, float* c, float* c_lo, float* c_hi,
                           int32_t* copied, ali_stream_t stream) {
  const int rc = ct_rows("ali_ct_book", B, N, 1, K);
  if (rc != ALI_OK) return rc;
  if (!v || !dist || !succ || !pred || !it || !best || !best_dist || !best_label || !found || !round_succ || !c ||
      !c_lo || !c_hi || !copied) {
    set_error("ali_ct_book: no argument may be NULL");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(ct_book_kernel, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), v, dist,
                     reinterpret_cast<const int*>(succ), reinterpret_cast<const int*>(pred),
                     reinterpret_cast<const int*>(it), (int)K, (long long)N, ct_vec4(N, {v, best}) ? 1 : 0, best,
                     best_dist,
                     reinterpret_cast<int*>(best_label), reinterpret_cast<int*>(found),
                     reinterpret_cast<int*>(round_succ), c, c_lo, c_hi, reinterpret_cast<int*>(copied));
  return check_launch("ct_book_kernel");
}

extern "C" int ali_ct_cem_update(const float* gx, int32_t gx_stride, float* v, float* y, const float* x0,
                                 const float* lo, const float* hi, int32_t* it, int32_t* rnd, int32_t K, double lr,
                                 double beta, double clip, int32_t B, int64_t N, float* l1, float* l2, float* dist,
                                 float* gnorm, ali_stream_t stream) {
  const int rc = ct_rows("ali_ct_cem_update", B, N, gx_stride, K);
  if (rc != ALI_OK) return rc;
  if (!gx || !v || !y || !x0 || !lo || !hi || !it || !rnd || !l1 || !l2 || !dist || !gnorm) {
    set_error("ali_ct_cem_update: no argument may be NULL");
    return ALI_ERR_BAD_ARG;
  }
  int* itp = reinterpret_cast<int*>(it);
  int* rp = reinterpret_cast<int*>(rnd);
  if (ct_vec4(N, {v, y, x0}))
    hipLaunchKernelGGL(ct_cem_update_kernel<4>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       y, x0, lo, hi, itp, rp, (int)K, lr, beta, clip, (long long)N, l1, l2, dist, gnorm);
  else
    hipLaunchKernelGGL(ct_cem_update_kernel<1>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       y, x0, lo, hi, itp, rp, (int)K, lr, beta, clip, (long long)N, l1, l2, dist, gnorm);
  return check_launch("ct_cem_update_kernel");
}

extern "C" int ali_ct_pp_update(const float* gx, int32_t gx_stride, float* v, float* y, const float* x0,
                                float background, int32_t* it, int32_t* rnd, int32_t K, double lr, double beta,
                                double clip, int32_t B, int64_t N, float* l1, float* l2, float* dist, float* gnorm,
                                ali_stream_t stream) {
  const int rc = ct_rows("ali_ct_pp_update", B, N, gx_stride, K);
  if (rc != ALI_OK) return rc;
  if (!gx || !v || !y || !x0 || !it || !rnd || !l1 || !l2 || !dist || !gnorm) {
    set_error("ali_ct_pp_update: no argument may be NULL");
    return ALI_ERR_BAD_ARG;
  }
  int* itp = reinterpret_cast<int*>(it);
  int* rp = reinterpret_cast<int*>(rnd);
  if (ct_vec4(N, {v, y, x0}))
    hipLaunchKernelGGL(ct_pp_update_kernel<4>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       y, x0, background, itp, rp, (int)K, lr, beta, clip, (long long)N, l1, l2, dist, gnorm);
  else
    hipLaunchKernelGGL(ct_pp_update_kernel<1>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       y, x0, background, itp, rp, (int)K, lr, beta, clip, (long long)N, l1, l2, dist, gnorm);
  return check_launch("ct_pp_update_kernel");
}

extern "C" int ali_ct_ce_update(const float* gx, int32_t gx_stride, float* v, const float* x0, const float* lo,
                                const float* hi, float* m, float* v2, int32_t* it, int32_t* rnd, int32_t K, double lr,
                                double gamma, double clip, double beta1, double beta2, double eps, int32_t B, int64_t N,
                                float* l1, float* gnorm, ali_stream_t stream) {
  const int rc = ct_rows("ali_ct_ce_update", B, N, gx_stride, K);
  if (rc != ALI_OK) return rc;
  if (!gx || !v || !x0 || !lo || !hi || !m || !v2 || !it || !rnd || !l1 || !gnorm) {
    set_error("ali_ct_ce_update: no argument may be NULL");
    return ALI_ERR_BAD_ARG;
  }
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) {
    set_error("ali_ct_ce_update: beta1 = %g and beta2 = %g must lie in [0, 1)", beta1, beta2);
    return ALI_ERR_BAD_ARG;
  }
  int* itp = reinterpret_cast<int*>(it);
  int* rp = reinterpret_cast<int*>(rnd);
  if (ct_vec4(N, {v, x0, m, v2}))
    hipLaunchKernelGGL(ct_ce_update_kernel<4>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       x0, lo, hi, m, v2, itp, rp, (int)K, lr, gamma, clip, beta1, beta2, eps, (long long)N, l1, gnorm);
  else
    hipLaunchKernelGGL(ct_ce_update_kernel<1>, dim3((unsigned)B), dim3(kCtBlock), 0, ST(stream), gx, (int)gx_stride, v,
                       x0, lo, hi, m, v2, itp, rp, (int)K, lr, gamma, clip, beta1, beta2, eps, (long long)N, l1, gnorm);
  return check_launch("ct_ce_update_kernel");
}
