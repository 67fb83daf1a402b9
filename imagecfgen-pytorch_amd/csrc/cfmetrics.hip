// What sits between the conv stacks of the cf_metrics family (include/ali_hip.h: ali_mse, ali_cf_recon,
// ali_oracle_scores) -- the autoencoder's loss of train_morphomnist_ae.py:102 and the table cells of
// morphomnist_cf_metrics.py:104-118,192-231 and mnist_oracle_scores.py:19-28,181-234 for B rows at once.
//
// All three are bytes-moved kernels: every input element is read once, every output written once, no reuse.
//   ali_mse            4 waves per block, 16-byte loads where the pointers allow, blocks grid-strided over the elements;
//                      fp64 partial per thread (ascending elements) -> block_sum -> the block that arrives last adds the
//                      block partials in block order (ali_reduce.h).  HBM bound at large n, launch bound at 784 * 64.
//   ali_cf_recon       one 64-lane wave per row (784 elements: 12.25 per lane), 4 rows per block; the four sums of a
//                      row end in one wave, so no sum crosses a block and no workspace is needed.
//   ali_oracle_scores  one wave per (row, oracle) pair, lanes strided over the C logits; fp64 row arithmetic like
//                      ali_softmax_xent (C = 10: launch bound).
// Every sum runs in a fixed order without float atomics: the same inputs give the same bits on every run.
#include "ali_reduce.h"

#include <limits.h>

namespace ali {

constexpr int kCfmWaves = 4;
constexpr int kMseMaxBlocks = 1024;
constexpr int kRowMaxBlocks = 4096;

// ------------------------------------------------------------------------------------------------------------ mse
__device__ __forceinline__ double mse_one(float yv, float xv, double gs, int tanh_out, float* g) {
  const double d = (double)yv - (double)xv;
  if (g) *g = (float)(tanh_out ? gs * d * (1.0 - (double)yv * (double)yv) : gs * d);
  return d * d;
}

template <bool VEC>
__global__ void __launch_bounds__(kCfmWaves * 64)
mse_kernel(const float* __restrict__ y, const float* __restrict__ x, long long n, double gs, int tanh_out,
           float* __restrict__ loss, float* __restrict__ grad, unsigned long long* part, int* ctr) {
  __shared__ double s_sum[kCfmWaves];
  __shared__ int s_last;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nthr = (long long)gridDim.x * blockDim.x;
  double acc = 0.0;
  if (VEC) {
    const long long n4 = n >> 2;
    for (long long i = tid; i < n4; i += nthr) {
      const float4 yv = reinterpret_cast<const float4*>(y)[i];
      const float4 xv = reinterpret_cast<const float4*>(x)[i];
      float4 g;
      acc += mse_one(yv.x, xv.x, gs, tanh_out, grad ? &g.x : nullptr);
      acc += mse_one(yv.y, xv.y, gs, tanh_out, grad ? &g.y : nullptr);
      acc += mse_one(yv.z, xv.z, gs, tanh_out, grad ? &g.z : nullptr);
      acc += mse_one(yv.w, xv.w, gs, tanh_out, grad ? &g.w : nullptr);
      if (grad) reinterpret_cast<float4*>(grad)[i] = g;
    }
    const long long i = (n4 << 2) + tid;              // the up to three elements behind the last full vector
    if (i < n) acc += mse_one(y[i], x[i], gs, tanh_out, grad ? grad + i : nullptr);
  } else {
    for (long long i = tid; i < n; i += nthr) acc += mse_one(y[i], x[i], gs, tanh_out, grad ? grad + i : nullptr);
  }
  const double b = block_sum<kCfmWaves>(acc, s_sum);
  if (threadIdx.x == 0) partial_store(&part[blockIdx.x], b);
  if (!arrive_last(ctr, (int)gridDim.x, &s_last) || threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < (int)gridDim.x; ++i) total += partial_load(&part[i]);     // block order, whichever block this is
  loss[0] = (float)(total / (double)n);
}

// ------------------------------------------------------------------------------------------------------- cf_recon
__global__ void __launch_bounds__(kCfmWaves * 64)
cf_recon_kernel(const float* __restrict__ x, const float* __restrict__ recon, long long ld_row, long long ld_plane,
                const int* __restrict__ orig, const int* __restrict__ target, int A, int B, int N, int vec,
                float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = (long long)blockIdx.x * kCfmWaves + wave; b < B; b += (long long)gridDim.x * kCfmWaves) {
    const int o = orig[b], t = target[b];
    const bool o_ok = o >= 0 && o < A - 1, t_ok = t >= 0 && t < A - 1;       // (the row is the wave's: uniform branches)
    const float* xr = x + b * N;
    const float* ra = recon + (long long)(A - 1) * ld_plane + b * ld_row;
    const float* ro = o_ok ? recon + (long long)o * ld_plane + b * ld_row : ra;      // a label out of range indexes
    const float* rt = t_ok ? recon + (long long)t * ld_plane + b * ld_row : ra;      // nothing: its sums become NaN
    double l1 = 0.0, so = 0.0, st = 0.0, sa = 0.0;
    auto one = [&](float xv, float ov, float tv, float av) {
      const double xd = (double)xv, td = (double)tv;
      const double d0 = xd - (double)ov, d1 = xd - td, d2 = td - (double)av;
      l1 += fabs(xd);
      so += d0 * d0;
      st += d1 * d1;
      sa += d2 * d2;
    };
    if (vec) {
      for (int j = lane; j < (N >> 2); j += 64) {
        const float4 xv = reinterpret_cast<const float4*>(xr)[j], ov = reinterpret_cast<const float4*>(ro)[j];
        const float4 tv = reinterpret_cast<const float4*>(rt)[j], av = reinterpret_cast<const float4*>(ra)[j];
        one(xv.x, ov.x, tv.x, av.x);
        one(xv.y, ov.y, tv.y, av.y);
        one(xv.z, ov.z, tv.z, av.z);
        one(xv.w, ov.w, tv.w, av.w);
      }
    } else {
      for (int j = lane; j < N; j += 64) one(xr[j], ro[j], rt[j], ra[j]);
    }
    l1 = wave_sum(l1);
    so = wave_sum(so);
    st = wave_sum(st);
    sa = wave_sum(sa);
    if (lane == 0) {
      const float nan = __int_as_float(0x7fc00000);
      float4 r;
      r.x = (float)l1;
      r.y = o_ok ? (float)so : nan;
      r.z = t_ok ? (float)st : nan;
      r.w = t_ok ? (float)sa : nan;
      reinterpret_cast<float4*>(out)[b] = r;
    }
  }
}

// -------------------------------------------------------------------------------------------------- oracle_scores
__global__ void __launch_bounds__(kCfmWaves * 64)
oracle_scores_kernel(const int* __restrict__ pred, const float* __restrict__ ox, const float* __restrict__ ocf,
                     long long ld_j, int J, int B, int C, int* __restrict__ os, float* __restrict__ lvs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long pairs = (long long)B * J;
  for (long long r = (long long)blockIdx.x * kCfmWaves + wave; r < pairs; r += (long long)gridDim.x * kCfmWaves) {
    const int j = (int)(r / B), b = (int)(r % B);
    const float* zp = ox + j * ld_j + (long long)b * C;
    const float* zq = ocf + j * ld_j + (long long)b * C;
    float pmax = -INFINITY, qmax = -INFINITY;
    int qi = lane < C ? lane : INT_MAX;
    for (int c = lane; c < C; c += 64) {             // ascending c per lane: a strict > keeps the lane's first maximum
      const float pv = zp[c], qv = zq[c];
      pmax = fmaxf(pmax, pv);
      if (qv > qmax) { qmax = qv; qi = c; }
    }
    pmax = wave_max(pmax);
    wave_argmax(qmax, qi);
    double psum = 0.0, qsum = 0.0;
    for (int c = lane; c < C; c += 64) {
      psum += exp((double)zp[c] - (double)pmax);
      qsum += exp((double)zq[c] - (double)qmax);
    }
    psum = wave_sum(psum);
    qsum = wave_sum(qsum);
    double kp = 0.0, kq = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double p = exp((double)zp[c] - (double)pmax) / psum;
      const double q = exp((double)zq[c] - (double)qmax) / qsum;
      const double m = 0.5 * (p + q);
      const double lm = log(m + 1e-6);
      kp += p * (log(p + 1e-6) - lm);
      kq += q * (log(q + 1e-6) - lm);
    }
    kp = wave_sum(kp);
    kq = wave_sum(kq);
    if (lane == 0) {
      os[(long long)b * J + j] = pred[b] == qi ? 1 : 0;
      lvs[(long long)b * J + j] = (float)(0.5 * (kp + kq));
    }
  }
}

}  // namespace ali

using namespace ali;

extern "C" int ali_mse(const float* y, const float* x, int64_t n, float gscale, int32_t tanh_out, float* loss,
                       float* grad, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!y || !x || !loss || n < 1) {
    set_error("ali_mse: y, x and loss must not be NULL and n >= 1");
    return ALI_ERR_BAD_ARG;
  }
  const int threads = kCfmWaves * 64;
  const bool vec = aligned16(y) && aligned16(x) && (!grad || aligned16(grad)) && n >= 4;
  const long long work = vec ? (n + 3) / 4 : n;          // (>= 3 threads whenever a tail exists: n >= 4 gives one block)
  long long blocks = (work + threads - 1) / threads;
  if (blocks > kMseMaxBlocks) blocks = kMseMaxBlocks;
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_mse", ws, ws_bytes, (size_t)blocks, &part, &ctr);
  if (rc != ALI_OK) return rc;
  const double gs = 2.0 * (double)gscale / (double)n;
  if (vec)
    hipLaunchKernelGGL(mse_kernel<true>, dim3((unsigned)blocks), dim3(threads), 0, ST(stream), y, x, (long long)n, gs,
                       (int)tanh_out, loss, grad, part, ctr);
  else
    hipLaunchKernelGGL(mse_kernel<false>, dim3((unsigned)blocks), dim3(threads), 0, ST(stream), y, x, (long long)n, gs,
                       (int)tanh_out, loss, grad, part, ctr);
  return check_launch("mse_kernel");
}

extern "C" int ali_cf_recon(const float* x, const float* recon, int64_t ld_row, int64_t ld_plane, const int32_t* orig,
                            const int32_t* target, int32_t A, int32_t B, int32_t N, float* out, ali_stream_t stream) {
  if (!x || !recon || !orig || !target || !out || A < 2 || B < 1 || N < 1 || ld_row < N || ld_plane < 0) {
    set_error("ali_cf_recon: NULL argument, A < 2, B < 1, N < 1, ld_row < N or ld_plane < 0");
    return ALI_ERR_BAD_ARG;
  }
  if (!aligned16(out)) {
    set_error("ali_cf_recon: out must be 16-byte aligned");
    return ALI_ERR_BAD_ARG;
  }
  const int vec = (N % 4 == 0) && (ld_row % 4 == 0) && (ld_plane % 4 == 0) && aligned16(x) && aligned16(recon);
  int blocks = (B + kCfmWaves - 1) / kCfmWaves;
  if (blocks > kRowMaxBlocks) blocks = kRowMaxBlocks;
  hipLaunchKernelGGL(cf_recon_kernel, dim3(blocks), dim3(kCfmWaves * 64), 0, ST(stream), x, recon, (long long)ld_row,
                     (long long)ld_plane, reinterpret_cast<const int*>(orig), reinterpret_cast<const int*>(target),
                     (int)A, (int)B, (int)N, vec, out);
  return check_launch("cf_recon_kernel");
}

extern "C" int ali_oracle_scores(const int32_t* pred, const float* ox, const float* ocf, int64_t ld_j, int32_t J,
                                 int32_t B, int32_t C, int32_t* os, float* lvs, ali_stream_t stream) {
  if (!pred || !ox || !ocf || !os || !lvs || J < 1 || B < 1 || C < 1 || (long long)B * C >= (1LL << 31) ||
      (J > 1 && ld_j < (long long)B * C)) {
    set_error("ali_oracle_scores: NULL argument, J < 1, B < 1, C < 1, B * C >= 2^31 or ld_j < B * C");
    return ALI_ERR_BAD_ARG;
  }
  long long blocks = ((long long)B * J + kCfmWaves - 1) / kCfmWaves;
  if (blocks > kRowMaxBlocks) blocks = kRowMaxBlocks;
  hipLaunchKernelGGL(oracle_scores_kernel, dim3((unsigned)blocks), dim3(kCfmWaves * 64), 0, ST(stream),
                     reinterpret_cast<const int*>(pred), ox, ocf, (long long)ld_j, (int)J, (int)B, (int)C,
                     reinterpret_cast<int*>(os), lvs);
  return check_launch("oracle_scores_kernel");
}
