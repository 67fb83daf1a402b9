// The attribute SCM of MorphoMNIST on the device (attribute_scms/mnist.py; include/ali_hip.h: ali_flow_stats,
// ali_flow_nll, ali_flow_map) and the Gumbel-max posterior of the conditional categoricals (ali_gumbel_posterior).
//
//   ali_flow_stats        mean and unbiased variance of log thickness, and the momentum update of the moving buffers
//   ali_flow_nll          the three log-densities of a batch, their means, and the gradient of all 75 parameters
//   ali_flow_map          sampling / abduction per column, or abduction-action-prediction of whole rows
//   ali_gumbel_posterior  posterior Gumbel noise of observed classes, one wave per row
//
// Every one of them is bound by launch latency at the sizes the callers have (N = 10 000 rows of three floats), so a row
// is evaluated in fp64 -- every fp32 result is the rounding of an fp64 evaluation of the statement in
// attribute_scms/_flows.py -- and nothing is vectorised.  The parameters are processed once per block into LDS
// (FlowParams: softmax / cumsum / softplus / sigmoid of the 31 raw spline parameters, the BatchNorm constants).
//
// ali_flow_nll's gradient: a thread adds its rows' terms to 103 private fp64 accumulators -- 3 log-density sums, gamma,
// beta, the 42 MLP parameters, and per spline bin the 7 processed quantities (x_k, x_k+1, y_k, y_k+1, d_k, d_k+1,
// lambda_k) the row's bin depends on.  The accumulators are indexed statically (a row adds to the 7 of its bin through
// predicated adds over the unrolled bin loop), so they live in registers.  The 7 derivatives of a row come from
// evaluating the inverse spline on dual numbers (D7: a value and 7 tangents).  Lanes, waves (in order) and blocks
// (ascending, by the block that arrives last; ali_reduce.h) are folded per accumulator; only wave 0 stores a block's
// partials, so thread 0's drain before the arrival covers all of them.  The last block then applies the Jacobians of
// cumsum, softmax, softplus and sigmoid once and writes gtheta.
#include "ali_reduce.h"
#include "ali_gumbel.h"

#include <float.h>

namespace ali {

constexpr int kFlowThreads = 256;
constexpr int kFlowWaves = kFlowThreads / 64;
constexpr int kFlowMaxBlocks = 64;
constexpr int kBins = 8;
constexpr int kHid = 10;
// theta
constexpr int kGamma = 0, kBeta = 1, kW1 = 2, kB1 = 12, kW2m = 22, kW2s = 32, kB2 = 42, kUw = 44, kUh = 52, kUd = 60, kUl = 67;
static_assert(kUl + kBins == ALI_FLOW_THETA, "theta layout");
// accumulators of ali_flow_nll
constexpr int kAccLp = 0, kAccGamma = 3, kAccBeta = 4, kAccW1 = 5, kAccB1 = 15, kAccW2m = 25, kAccW2s = 35, kAccB2 = 45,
              kAccSpline = 47, kAccAll = kAccSpline + 7 * kBins;
static_assert(kAccAll == 103, "accumulator layout (include/ali_hip.h states the workspace size with it)");

constexpr double kBnEps = 1e-5;
constexpr double kHalfLog2Pi = 0.91893853320467274178;
constexpr double kBound = 3.0;
constexpr double kPMin = (double)FLT_MIN, kPMax = 1.0 - (double)FLT_EPSILON;

struct FlowParams {
  double g, log_g, beta;
  int gamma_on;
  double w1[kHid], b1[kHid], w2m[kHid], w2s[kHid], b2m, b2s;
  double xk[kBins + 1], yk[kBins + 1], d[kBins + 1], lam[kBins];
  double smw[kBins], smh[kBins], sgd[kBins - 1], sgl[kBins];   // softmax / sigmoid values the fold's Jacobians need
  double imin, irng, smin, srng, log_irng, log_srng;
  double m, rs, half_log_v;                                      // the density direction's statistics
  double fm, fsd;                                                // the sampling direction's: mean, sqrt(var + eps)
};

#define FLOW_FN __host__ __device__ __forceinline__
FLOW_FN double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }
FLOW_FN double softplus_d(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

__host__ __device__ inline void knots_from(const float* u, double* knot, double* sm) {
  double mx = -INFINITY, sum = 0.0, e[kBins];
  for (int k = 0; k < kBins; ++k) mx = fmax(mx, (double)u[k]);
  for (int k = 0; k < kBins; ++k) { e[k] = exp((double)u[k] - mx); sum += e[k]; }
  double cum = 0.0;
  knot[0] = -kBound;
  for (int k = 0; k < kBins; ++k) {
    sm[k] = e[k] / sum;
    cum += 1e-3 + (1.0 - 1e-3 * kBins) * sm[k];
    knot[k + 1] = -kBound + 2.0 * kBound * cum;
  }
  knot[kBins] = kBound;
}

// thread 0 of a block; the others wait at the barrier behind it
__host__ __device__ inline void load_params(FlowParams& P, const float* theta, const float* cst, const float* stats_inv,
                            const float* stats_fwd) {
  const double gamma = (double)theta[kGamma];
  P.gamma_on = gamma > 0.0;
  P.g = fmax(gamma, 0.0) + 1e-6;
  P.log_g = log(P.g);
  P.beta = (double)theta[kBeta];
  for (int j = 0; j < kHid; ++j) {
    P.w1[j] = (double)theta[kW1 + j];
    P.b1[j] = (double)theta[kB1 + j];
    P.w2m[j] = (double)theta[kW2m + j];
    P.w2s[j] = (double)theta[kW2s + j];
  }
  P.b2m = (double)theta[kB2];
  P.b2s = (double)theta[kB2 + 1];
  knots_from(theta + kUw, P.xk, P.smw);
  knots_from(theta + kUh, P.yk, P.smh);
  P.d[0] = P.d[kBins] = 1.0;
  for (int k = 0; k < kBins - 1; ++k) {
    P.sgd[k] = sigmoid_d((double)theta[kUd + k]);
    P.d[k + 1] = 1e-3 + softplus_d((double)theta[kUd + k]);
  }
  for (int k = 0; k < kBins; ++k) {
    P.sgl[k] = sigmoid_d((double)theta[kUl + k]);
    P.lam[k] = 0.95 * P.sgl[k] + 0.025;
  }
  P.imin = (double)cst[0];
  P.irng = (double)cst[1];
  P.smin = (double)cst[2];
  P.srng = (double)cst[3];
  P.log_irng = log(P.irng);
  P.log_srng = log(P.srng);
  const double v = (double)stats_inv[1] + kBnEps;
  P.m = (double)stats_inv[0];
  P.rs = 1.0 / sqrt(v);
  P.half_log_v = 0.5 * log(v);
  P.fm = (double)stats_fwd[0];
  P.fsd = sqrt((double)stats_fwd[1] + kBnEps);
}

// ------------------------------------------------------------------------------------------------- dual numbers
struct D7 { double v; double d[7]; };
FLOW_FN D7 seed7(double v, int i) {
  D7 r;
  r.v = v;
#pragma unroll
  for (int j = 0; j < 7; ++j) r.d[j] = j == i ? 1.0 : 0.0;
  return r;
}
#define D7_EACH for (int j = 0; j < 7; ++j)
FLOW_FN D7 operator+(D7 a, D7 b) { _Pragma("unroll") D7_EACH a.d[j] += b.d[j]; a.v += b.v; return a; }
FLOW_FN D7 operator-(D7 a, D7 b) { _Pragma("unroll") D7_EACH a.d[j] -= b.d[j]; a.v -= b.v; return a; }
FLOW_FN D7 operator*(D7 a, D7 b) {
  D7 r;
  _Pragma("unroll") D7_EACH r.d[j] = a.d[j] * b.v + a.v * b.d[j];
  r.v = a.v * b.v;
  return r;
}
FLOW_FN D7 operator/(D7 a, D7 b) {
  D7 r;
  const double ib = 1.0 / b.v;
  r.v = a.v * ib;
  _Pragma("unroll") D7_EACH r.d[j] = (a.d[j] - r.v * b.d[j]) * ib;
  return r;
}
FLOW_FN D7 operator+(D7 a, double b) { a.v += b; return a; }
FLOW_FN D7 operator-(D7 a, double b) { a.v -= b; return a; }
FLOW_FN D7 operator-(double a, D7 b) { _Pragma("unroll") D7_EACH b.d[j] = -b.d[j]; b.v = a - b.v; return b; }
FLOW_FN D7 operator*(D7 a, double b) { _Pragma("unroll") D7_EACH a.d[j] *= b; a.v *= b; return a; }
FLOW_FN D7 fsqrt(D7 a) {
  D7 r;
  r.v = sqrt(a.v);
  const double h = 0.5 / r.v;
  _Pragma("unroll") D7_EACH r.d[j] = a.d[j] * h;
  return r;
}
FLOW_FN D7 flog(D7 a) {
  D7 r;
  r.v = log(a.v);
  const double i = 1.0 / a.v;
  _Pragma("unroll") D7_EACH r.d[j] = a.d[j] * i;
  return r;
}
FLOW_FN double fsqrt(double a) { return sqrt(a); }
FLOW_FN double flog(double a) { return log(a); }
FLOW_FN double value(double a) { return a; }
FLOW_FN double value(const D7& a) { return a.v; }

// the bin of v among knots k[0] = -3 < k[1] < ... < k[8] = 3: the number of inner knots at or below v
FLOW_FN int bin_of(const double* knot, double v) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < kBins; ++j) k += v >= knot[j] ? 1 : 0;
  return k;
}

// Rational-linear spline, bin (x0, x1, y0, y1, d0, d1, la): u = the preimage of q, ld = log(du / dq).  T = double or D7.
template <typename T>
FLOW_FN void spline_inverse(T x0, T x1, T y0, T y1, T d0, T d1, T la, double q, T& u, T& ld) {
  const T w = x1 - x0;
  const T wb = fsqrt(d0 / d1);                                    // (wa = 1)
  const T om = 1.0 - la;
  const T wc = (la * d0 + om * wb * d1) * w / (y1 - y0);
  const T yc = (om * y0 + la * wb * y1) / (om + la * wb);
  T num, den, top;
  if (q <= value(yc)) {
    num = la * (y0 - q);
    den = (wc - 1.0) * q + y0 - wc * yc;
    top = wc * la * (yc - y0);
  } else {
    num = (wc - la * wb) * q + la * wb * y1 - wc * yc;
    den = (wc - wb) * q + wb * y1 - wc * yc;
    top = wb * wc * om * (y1 - yc);
  }
  u = num / den * w + x0;
  ld = flog(top * w / (den * den));
}

FLOW_FN double spline_forward(const FlowParams& P, double x) {
  if (!(x >= -kBound && x <= kBound)) return x;
  const int k = bin_of(P.xk, x);
  const double x0 = P.xk[k], x1 = P.xk[k + 1], y0 = P.yk[k], y1 = P.yk[k + 1], d0 = P.d[k], d1 = P.d[k + 1], la = P.lam[k];
  const double w = x1 - x0, wb = sqrt(d0 / d1), om = 1.0 - la;
  const double wc = (la * d0 + om * wb * d1) * w / (y1 - y0);
  const double yc = (om * y0 + la * wb * y1) / (om + la * wb);
  const double th = (x - x0) / w;
  if (th <= la) return (y0 * (la - th) + wc * yc * th) / ((la - th) + wc * th);
  return (wc * yc * (1.0 - th) + wb * y1 * (th - la)) / (wc * (1.0 - th) + wb * (th - la));
}

FLOW_FN double spline_inverse_value(const FlowParams& P, double q) {
  if (!(q >= -kBound && q <= kBound)) return q;
  const int k = bin_of(P.yk, q);
  double u, ld;
  spline_inverse<double>(P.xk[k], P.xk[k + 1], P.yk[k], P.yk[k + 1], P.d[k], P.d[k + 1], P.lam[k], q, u, ld);
  return u;
}

// the intensity's conditioner at thickness t: hidden units, mean, clamped log-scale
FLOW_FN void mlp(const FlowParams& P, double t, double* h, double& mean, double& ls) {
  mean = P.b2m;
  double a = P.b2s;
#pragma unroll
  for (int j = 0; j < kHid; ++j) {
    h[j] = fmax(P.w1[j] * t + P.b1[j], 0.0);
    mean += P.w2m[j] * h[j];
    a += P.w2s[j] * h[j];
  }
  ls = fmin(fmax(a, -5.0), 3.0);
}

FLOW_FN double logit_of(const FlowParams& P, double i) {
  const double p = fmin(fmax((i - P.imin) / P.irng, kPMin), kPMax);
  return log(p) - log1p(-p);
}

// ---------------------------------------------------------------------------------------------------- ali_flow_stats
__global__ void __launch_bounds__(kFlowThreads)
flow_stats_kernel(const float* __restrict__ t, long long stride, long long N, float* __restrict__ out2,
                  float* __restrict__ moving, float momentum, unsigned long long* part, int* ctr) {
  __shared__ double s_w[kFlowWaves];
  __shared__ int s_last;
  double s1 = 0.0, s2 = 0.0;
  for (long long n = (long long)blockIdx.x * kFlowThreads + threadIdx.x; n < N; n += (long long)gridDim.x * kFlowThreads) {
    const double x = log((double)t[n * stride]);
    s1 += x;
    s2 += x * x;
  }
  s1 = block_sum<kFlowWaves>(s1, s_w);
  s2 = block_sum<kFlowWaves>(s2, s_w);
  if (threadIdx.x == 0) {
    partial_store(&part[2 * blockIdx.x], s1);
    partial_store(&part[2 * blockIdx.x + 1], s2);
  }
  if (!arrive_last(ctr, (int)gridDim.x, &s_last) || threadIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < (int)gridDim.x; ++i) {           // block order, whichever block this is
    a += partial_load(&part[2 * i]);
    b += partial_load(&part[2 * i + 1]);
  }
  const double mean = a / (double)N;
  const double var = N > 1 ? (b - a * mean) / (double)(N - 1) : (double)NAN;   // (one row: torch's NaN)
  out2[0] = (float)mean;
  out2[1] = (float)var;
  if (moving) {
    const double mo = (double)momentum;
    moving[0] = (float)((1.0 - mo) * (double)moving[0] + mo * mean);
    moving[1] = (float)((1.0 - mo) * (double)moving[1] + mo * var);
  }
}

// ------------------------------------------------------------------------------------------------------ ali_flow_nll
// One row: its three log-densities into lp3 and the sums, and -- GRAD -- its weighted gradient terms (weights wt, wi,
// wsl of the three densities) into the accumulators.  Every index into acc is a constant after unrolling.
template <bool GRAD, int NV>
FLOW_FN void nll_row(const FlowParams& P, double t, double iv, double sv, double wt, double wi, double wsl, double* lp3,
                     double (&acc)[NV]) {
  // thickness
  const double x1 = log(t);
  const double xs = (x1 - P.m) * P.rs;
  const double ut = xs * P.g + P.beta;
  const double lpt = -0.5 * ut * ut - kHalfLog2Pi - x1 + P.log_g - P.half_log_v;
  // intensity
  double h[kHid], mean, ls;
  mlp(P, t, h, mean, ls);
  const double w = logit_of(P, iv);
  const double els = exp(-ls);
  const double ui = (w - mean) * els;
  const double lpi = -0.5 * ui * ui - kHalfLog2Pi - ls + fabs(w) + 2.0 * log1p(exp(-fabs(w))) - P.log_irng;
  // slant
  const double q = (sv - P.smin) / P.srng;
  const bool inside = q >= -kBound && q <= kBound;
  const int k = inside ? bin_of(P.yk, q) : 0;
  double us = q, lds = 0.0, gs[7];
  if (GRAD) {
    D7 u7, ld7;
    spline_inverse<D7>(seed7(P.xk[k], 0), seed7(P.xk[k + 1], 1), seed7(P.yk[k], 2), seed7(P.yk[k + 1], 3),
                       seed7(P.d[k], 4), seed7(P.d[k + 1], 5), seed7(P.lam[k], 6), q, u7, ld7);
    if (inside) { us = u7.v; lds = ld7.v; }
#pragma unroll
    for (int j = 0; j < 7; ++j) gs[j] = inside ? ld7.d[j] - u7.v * u7.d[j] : 0.0;
  } else if (inside) {
    spline_inverse<double>(P.xk[k], P.xk[k + 1], P.yk[k], P.yk[k + 1], P.d[k], P.d[k + 1], P.lam[k], q, us, lds);
  }
  const double lps = -0.5 * us * us - kHalfLog2Pi + lds - P.log_srng;
  lp3[0] = lpt;
  lp3[1] = lpi;
  lp3[2] = lps;
  acc[kAccLp] += lpt;
  acc[kAccLp + 1] += lpi;
  acc[kAccLp + 2] += lps;
  if constexpr (GRAD) {
    if (P.gamma_on) acc[kAccGamma] += wt * (1.0 / P.g - ut * xs);
    acc[kAccBeta] += wt * -ut;
    const double gm = wi * ui * els, gl = wi * (ui * ui - 1.0);      // d lp_i / d mean, / d log_scale (straight through)
    acc[kAccB2] += gm;
    acc[kAccB2 + 1] += gl;
#pragma unroll
    for (int j = 0; j < kHid; ++j) {
      acc[kAccW2m + j] += gm * h[j];
      acc[kAccW2s + j] += gl * h[j];
      const double gh = h[j] > 0.0 ? gm * P.w2m[j] + gl * P.w2s[j] : 0.0;
      acc[kAccB1 + j] += gh;
      acc[kAccW1 + j] += gh * t;
    }
#pragma unroll
    for (int b = 0; b < kBins; ++b) {
#pragma unroll
      for (int j = 0; j < 7; ++j) acc[kAccSpline + 7 * b + j] += b == k ? wsl * gs[j] : 0.0;
    }
  }
}

// The folded sums -> out4 and gtheta: the processed spline quantities go through the Jacobians of cumsum, softmax,
// softplus and sigmoid down to the 31 raw parameters here, once.
template <bool GRAD>
FLOW_FN void nll_finish(const FlowParams& P, const double* fold, long long N, float* out4, float* gtheta) {
  if (out4) {
    const double inv = 1.0 / (double)N;
    out4[0] = (float)(-(fold[0] + fold[1] + fold[2]) * inv);
    out4[1] = (float)(fold[0] * inv);
    out4[2] = (float)(fold[1] * inv);
    out4[3] = (float)(fold[2] * inv);
  }
  if (!GRAD) return;
  gtheta[kGamma] = (float)fold[kAccGamma];
  gtheta[kBeta] = (float)fold[kAccBeta];
  for (int j = 0; j < 4 * kHid + 2; ++j) gtheta[kW1 + j] = (float)fold[kAccW1 + j];   // (the same order in both)
  // knots 0 .. 8 (the end knots and the end derivatives are constants), lambdas
  double gx[kBins + 1] = {}, gy[kBins + 1] = {}, gd[kBins + 1] = {};
  for (int b = 0; b < kBins; ++b) {
    const double* G = &fold[kAccSpline + 7 * b];
    gx[b] += G[0]; gx[b + 1] += G[1];
    gy[b] += G[2]; gy[b + 1] += G[3];
    gd[b] += G[4]; gd[b + 1] += G[5];
    const double sg = P.sgl[b];
    gtheta[kUl + b] = (float)(G[6] * 0.95 * sg * (1.0 - sg));
  }
  for (int j = 0; j < kBins - 1; ++j) gtheta[kUd + j] = (float)(gd[j + 1] * P.sgd[j]);
  for (int side = 0; side < 2; ++side) {
    const double* gk = side ? gy : gx;
    const double* sm = side ? P.smh : P.smw;
    // knot j (1 .. 7) = -3 + 6 * (w_0 + .. + w_j-1): d / d w_i = 6 * the sum over the knots behind bin i
    double gw[kBins], tail = 0.0, dot = 0.0;
    for (int i = kBins - 1; i >= 0; --i) {
      gw[i] = 2.0 * kBound * tail;
      if (i >= 1) tail += gk[i];
    }
    for (int i = 0; i < kBins; ++i) dot += gw[i] * sm[i];
    for (int i = 0; i < kBins; ++i)
      gtheta[(side ? kUh : kUw) + i] = (float)((1.0 - 1e-3 * kBins) * sm[i] * (gw[i] - dot));
  }
}

template <bool GRAD>
__global__ void __launch_bounds__(kFlowThreads)
flow_nll_kernel(const float* __restrict__ tc, long long st, const float* __restrict__ ic, long long si,
                const float* __restrict__ sc, long long ss, long long N, const float* __restrict__ theta,
                const float* __restrict__ cst, const float* __restrict__ stats, const float* __restrict__ wgt,
                float gscale, float* __restrict__ lp, float* __restrict__ out4, float* __restrict__ gtheta,
                unsigned long long* part, int* ctr) {
  constexpr int NV = GRAD ? kAccAll : 3;
  __shared__ FlowParams P;
  __shared__ double s_part[kFlowWaves * NV];
  __shared__ double s_fold[NV];
  __shared__ int s_last;
  if (threadIdx.x == 0) load_params(P, theta, cst, stats, stats);
  __syncthreads();
  double acc[NV];
#pragma unroll
  for (int a = 0; a < NV; ++a) acc[a] = 0.0;
  const double wconst = (double)gscale / (double)N;

  for (long long n = (long long)blockIdx.x * kFlowThreads + threadIdx.x; n < N; n += (long long)gridDim.x * kFlowThreads) {
    double w3[3] = {wconst, wconst, wconst}, lp3[3];
    if (GRAD && wgt) {
      w3[0] = (double)wgt[n * 3];
      w3[1] = (double)wgt[n * 3 + 1];
      w3[2] = (double)wgt[n * 3 + 2];
    }
    nll_row<GRAD, NV>(P, (double)tc[n * st], (double)ic[n * si], (double)sc[n * ss], w3[0], w3[1], w3[2], lp3, acc);
    if (lp) {
      lp[n * 3] = (float)lp3[0];
      lp[n * 3 + 1] = (float)lp3[1];
      lp[n * 3 + 2] = (float)lp3[2];
    }
  }

  // lanes, then waves in order; wave 0 alone stores the block's partials (thread 0's drain covers its wave)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NV; ++a) {
    const double r = wave_sum(acc[a]);
    if (lane == 0) s_part[wave * NV + a] = r;
  }
  __syncthreads();
  if (wave == 0) {
    for (int a = lane; a < NV; a += 64) {
      double r = 0.0;
#pragma unroll
      for (int wv = 0; wv < kFlowWaves; ++wv) r += s_part[wv * NV + a];
      partial_store(&part[(long long)blockIdx.x * NV + a], r);
    }
  }
  if (!arrive_last(ctr, (int)gridDim.x, &s_last)) return;
  for (int a = threadIdx.x; a < NV; a += kFlowThreads) {
    double r = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b) r += partial_load(&part[(long long)b * NV + a]);   // blocks ascending
    s_fold[a] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) nll_finish<GRAD>(P, s_fold, N, out4, gtheta);
}

// ------------------------------------------------------------------------------------------------------ ali_flow_map
FLOW_FN double thick_inverse(const FlowParams& P, double t) { return (log(t) - P.m) * P.rs * P.g + P.beta; }
FLOW_FN double thick_forward(const FlowParams& P, double u) { return exp((u - P.beta) / P.g * P.fsd + P.fm); }
FLOW_FN double inten_inverse(const FlowParams& P, double i, double t) {
  double h[kHid], mean, ls;
  mlp(P, t, h, mean, ls);
  return (logit_of(P, i) - mean) * exp(-ls);
}
FLOW_FN double inten_forward(const FlowParams& P, double u, double t) {
  double h[kHid], mean, ls;
  mlp(P, t, h, mean, ls);
  const double p = fmin(fmax(sigmoid_d(exp(ls) * u + mean), kPMin), kPMax);
  return p * P.irng + P.imin;
}
FLOW_FN double slant_inverse(const FlowParams& P, double s) { return spline_inverse_value(P, (s - P.smin) / P.srng); }
FLOW_FN double slant_forward(const FlowParams& P, double u) { return spline_forward(P, u) * P.srng + P.smin; }

__global__ void __launch_bounds__(kFlowThreads)
flow_map_kernel(const float* in, const float* __restrict__ val, float* out, float* __restrict__ noise_out, long long N,
                int mode_t, int mode_i, int mode_s, int cf, int cf_mask, const float* __restrict__ theta,
                const float* __restrict__ cst, const float* __restrict__ stats_inv, const float* __restrict__ stats_fwd) {
  __shared__ FlowParams P;
  if (threadIdx.x == 0) load_params(P, theta, cst, stats_inv, stats_fwd);
  __syncthreads();
  for (long long n = (long long)blockIdx.x * kFlowThreads + threadIdx.x; n < N; n += (long long)gridDim.x * kFlowThreads) {
    const double a0 = (double)in[n * 3], a1 = (double)in[n * 3 + 1], a2 = (double)in[n * 3 + 2];
    double o0, o1, o2;
    if (cf) {
      const double ut = thick_inverse(P, a0), ui = inten_inverse(P, a1, a0), us = slant_inverse(P, a2);
      if (noise_out) {
        noise_out[n * 3] = (float)ut;
        noise_out[n * 3 + 1] = (float)ui;
        noise_out[n * 3 + 2] = (float)us;
      }
      o0 = (cf_mask & 1) ? (double)val[n * 3] : thick_forward(P, ut);
      o1 = (cf_mask & 2) ? (double)val[n * 3 + 1] : inten_forward(P, ui, o0);
      o2 = (cf_mask & 4) ? (double)val[n * 3 + 2] : slant_forward(P, us);
    } else {
      o0 = mode_t == ALI_FLOW_FORWARD ? thick_forward(P, a0) : mode_t == ALI_FLOW_INVERSE ? thick_inverse(P, a0) : a0;
      const double ctx = mode_t == ALI_FLOW_FORWARD ? o0 : a0;
      o1 = mode_i == ALI_FLOW_FORWARD ? inten_forward(P, a1, ctx) : mode_i == ALI_FLOW_INVERSE ? inten_inverse(P, a1, ctx) : a1;
      o2 = mode_s == ALI_FLOW_FORWARD ? slant_forward(P, a2) : mode_s == ALI_FLOW_INVERSE ? slant_inverse(P, a2) : a2;
    }
    out[n * 3] = (float)o0;
    out[n * 3 + 1] = (float)o1;
    out[n * 3 + 2] = (float)o2;
  }
}

// ---------------------------------------------------------------------------------------------- ali_gumbel_posterior
constexpr int kGumbelWaves = 4;   // (the draw and the posterior's formula: ali_gumbel.h)

__global__ void __launch_bounds__(kGumbelWaves * 64)
gumbel_posterior_kernel(const float* __restrict__ logits, const long long* __restrict__ y, const float* __restrict__ g_in,
                        uint64_t seed, const long long* __restrict__ dev_counter, uint64_t offset, int N, int C,
                        float* __restrict__ noise, float* __restrict__ g_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t key = gumbel_key(rng_base_key(seed, dev_counter));
  for (long long n = (long long)blockIdx.x * kGumbelWaves + wave; n < N; n += (long long)gridDim.x * kGumbelWaves) {
    const float* z = logits + n * C;
    const long long yn = y[n];
    const bool ok = yn >= 0 && yn < C;
    const long long yc = ok ? yn : 0;
    float zmax = -INFINITY;
    for (int j = lane; j < C; j += 64) zmax = fmaxf(zmax, z[j]);
    zmax = wave_max(zmax);
    double esum = 0.0;
    for (int j = lane; j < C; j += 64) esum += exp((double)z[j] - (double)zmax);
    const double lse = (double)zmax + log(wave_sum(esum));
    const float gyf = g_in ? g_in[n * C + yc] : gumbel_at(key, offset + (uint64_t)(n * C + yc));
    const double gy = (double)gyf, zy = (double)z[yc];
    const double ey = exp(-gy - zy);
    for (int j = lane; j < C; j += 64) {
      const float gf = g_in ? g_in[n * C + j] : gumbel_at(key, offset + (uint64_t)(n * C + j));
      const double zj = (double)z[j];
      double v = gumbel_posterior_at(j == yc, (double)gf, zj, gy, zy, ey, lse);
      if (!ok) v = NAN;
      noise[n * C + j] = (float)v;
      if (g_out) g_out[n * C + j] = gf;
    }
  }
}

}  // namespace ali

using namespace ali;

static int flow_grid(long long N, int cap) {
  long long b = (N + kFlowThreads - 1) / kFlowThreads;
  return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ali_flow_stats(const float* t, int64_t stride, int64_t N, float* out2, float* moving, float momentum,
                              void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!t || !out2) { set_error("ali_flow_stats: t and out2 must not be NULL"); return ALI_ERR_BAD_ARG; }
  if (N < 1 || stride < 1 || N >= (1LL << 40) / stride) {
    set_error("ali_flow_stats: N = %lld or stride = %lld out of range", (long long)N, (long long)stride);
    return ALI_ERR_BAD_ARG;
  }
  if (moving && N < 2) {
    set_error("ali_flow_stats: the moving update needs N >= 2 rows (the unbiased variance of one row is undefined)");
    return ALI_ERR_BAD_ARG;
  }
  const int blocks = flow_grid(N, kFlowMaxBlocks);
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_flow_stats", ws, ws_bytes, (size_t)2 * blocks, &part, &ctr);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(flow_stats_kernel, dim3(blocks), dim3(kFlowThreads), 0, ST(stream), t, (long long)stride,
                     (long long)N, out2, moving, momentum, part, ctr);
  return check_launch("flow_stats_kernel");
}

extern "C" int ali_flow_nll(const float* t, int64_t st, const float* i, int64_t si, const float* s, int64_t ss, int64_t N,
                            const float* theta, const float* cst, const float* stats, const float* wgt, float gscale,
                            float* lp, float* out4, float* gtheta, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!t || !i || !s || !theta || !cst || !stats) {
    set_error("ali_flow_nll: t, i, s, theta, cst and stats must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  if (!lp && !out4 && !gtheta) { set_error("ali_flow_nll: nothing to compute (lp, out4 and gtheta are all NULL)"); return ALI_ERR_BAD_ARG; }
  const int64_t smax = st > si ? (st > ss ? st : ss) : (si > ss ? si : ss);
  if (N < 1 || st < 1 || si < 1 || ss < 1 || N >= (1LL << 40) / smax) {
    set_error("ali_flow_nll: N = %lld or a stride out of range", (long long)N);
    return ALI_ERR_BAD_ARG;
  }
  const int blocks = flow_grid(N, kFlowMaxBlocks);
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_flow_nll", ws, ws_bytes, (size_t)(gtheta ? kAccAll : 3) * blocks, &part, &ctr);
  if (rc != ALI_OK) return rc;
  if (gtheta)
    hipLaunchKernelGGL(flow_nll_kernel<true>, dim3(blocks), dim3(kFlowThreads), 0, ST(stream), t, (long long)st, i,
                       (long long)si, s, (long long)ss, (long long)N, theta, cst, stats, wgt, gscale, lp, out4, gtheta,
                       part, ctr);
  else
    hipLaunchKernelGGL(flow_nll_kernel<false>, dim3(blocks), dim3(kFlowThreads), 0, ST(stream), t, (long long)st, i,
                       (long long)si, s, (long long)ss, (long long)N, theta, cst, stats, wgt, gscale, lp, out4, gtheta,
                       part, ctr);
  return check_launch("flow_nll_kernel");
}

extern "C" int ali_flow_map(const float* in, const float* val, float* out, float* noise_out, int64_t N, int32_t mode_t,
                            int32_t mode_i, int32_t mode_s, int32_t cf, int32_t cf_mask, const float* theta,
                            const float* cst, const float* stats_inv, const float* stats_fwd, ali_stream_t stream) {
  if (!in || !out || !theta || !cst || !stats_inv || !stats_fwd) {
    set_error("ali_flow_map: in, out, theta, cst and both stats must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  if (N < 1 || N >= (1LL << 38)) { set_error("ali_flow_map: N = %lld outside [1, 2^38)", (long long)N); return ALI_ERR_BAD_ARG; }
  const int modes[3] = {mode_t, mode_i, mode_s};
  for (int m : modes)
    if (m != ALI_FLOW_SKIP && m != ALI_FLOW_FORWARD && m != ALI_FLOW_INVERSE) {
      set_error("ali_flow_map: mode %d is none of ALI_FLOW_SKIP / FORWARD / INVERSE", m);
      return ALI_ERR_BAD_ARG;
    }
  if (cf && ((cf_mask & ~7) || (cf_mask && !val))) {
    set_error("ali_flow_map: cf_mask = %d outside [0, 7], or columns intervened on without val", (int)cf_mask);
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(flow_map_kernel, dim3(flow_grid(N, 1024)), dim3(kFlowThreads), 0, ST(stream), in, val, out,
                     noise_out, (long long)N, (int)mode_t, (int)mode_i, (int)mode_s, (int)cf, (int)cf_mask, theta, cst,
                     stats_inv, stats_fwd);
  return check_launch("flow_map_kernel");
}

extern "C" int ali_gumbel_posterior(const float* logits, const int64_t* y, const float* g, uint64_t seed,
                                    const int64_t* dev_counter, uint64_t offset, int32_t N, int32_t C, float* noise,
                                    float* g_out, ali_stream_t stream) {
  if (!logits || !y || !noise) { set_error("ali_gumbel_posterior: logits, y and noise must not be NULL"); return ALI_ERR_BAD_ARG; }
  if (C < 1 || C > 4096) { set_error("ali_gumbel_posterior: C = %d outside [1, 4096]", (int)C); return ALI_ERR_BAD_ARG; }
  if (N < 1 || (long long)N * C >= (1LL << 31)) {
    set_error("ali_gumbel_posterior: N = %d outside [1, 2^31 / C)", (int)N);
    return ALI_ERR_BAD_ARG;
  }
  int blocks = (N + kGumbelWaves - 1) / kGumbelWaves;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(gumbel_posterior_kernel, dim3(blocks), dim3(kGumbelWaves * 64), 0, ST(stream), logits,
                     reinterpret_cast<const long long*>(y), g, seed, reinterpret_cast<const long long*>(dev_counter),
                     offset, (int)N, (int)C, noise, g_out);
  return check_launch("gumbel_posterior_kernel");
}
