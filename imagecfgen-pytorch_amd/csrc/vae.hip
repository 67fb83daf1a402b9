// What sits between the conv stacks of the DeepSCM conditional VAE (deepscm_vae/mnist.py:121-133 and its audio / whale
// copies), three launches (include/ali_hip.h: ali_vae_latent_fwd, ali_vae_loglik, ali_vae_latent_bwd):
//
//   latent forward   z[s,b,:] = mean[b] + eps[s,b] * exp(k * log_var[b]) written into columns 0..L of the decoder's input
//                    rows [S*B][ld], the conditioning columns behind them ([onehot_j @ table_j | cont | 0], the row of
//                    ali_g_input) in the same launch, and sum_b dkl_b, dkl_b = 0.5 sum_l (e^lv + mean^2 - 1 - lv).
//                    eps is given or drawn here from the latent stream of ali_normal_fill (ali_rng.h: normal_at).
//   log-likelihood   mean_b (1/S) sum_s log N(x_b; xhat_sb, e^log_var I), the loss -(lp - kl_weight * mean_b dkl) and
//                    gxhat = gscale * (xhat - x) * e^-log_var / (S*B).
//   latent backward  the [B][2L]-style head gradient from the decoder input gradient's columns 0..L, and the sum over s of
//                    its conditioning columns (the rows ali_g_input_table_grad takes).
//
// One 256-thread block per row, threads strided over the columns; the S decoder passes are S*B rows of one pass.  Row
// arithmetic is fp64 (exp included): the kernels are launch- or HBM-bound at every size the callers have, and each fp32
// result is then the rounding of an fp64 evaluation.  Reductions and the hand-off between blocks: ali_reduce.h.  Here:
// the block that arrives last folds the partials with all its threads (vae_fold).
#include "ali_reduce.h"

namespace ali {

constexpr int kVaeBlock = 256;
constexpr int kVaeWaves = kVaeBlock / 64;
constexpr int kVaeMaxBlocks = 1024;
constexpr int kVaeMaxEmb = 8;

struct VaeCond {
  const void* oh[kVaeMaxEmb];
  const float* tab[kVaeMaxEmb];
  int ncls[kVaeMaxEmb];
  int is_int[kVaeMaxEmb];
  const float* cont;
  int n_emb, n_cont;
};

// partials 0..n-1 added in a fixed order: thread t takes t, t + 256, ... ascending, then the block sum
__device__ __forceinline__ double vae_fold(const unsigned long long* part, int n, double* red) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += kVaeBlock) v += partial_load(part + i);
  return block_sum<kVaeWaves>(v, red);
}

__device__ __forceinline__ float vae_attr(const void* p, int is_int, long long i) {
  return is_int ? (float)reinterpret_cast<const int*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

__global__ void __launch_bounds__(kVaeBlock)
vae_latent_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ lv, int head_ld,
                      const float* __restrict__ eps_in, float* __restrict__ eps_out, uint64_t seed,
                      const long long* __restrict__ dev_counter, uint64_t offset, int S, int B, int L, float k,
                      VaeCond c, int write_cond, int ld, float* __restrict__ out, float* __restrict__ kl_out,
                      unsigned long long* part, int* ctr) {
  __shared__ double red[kVaeWaves];
  __shared__ int s_last;
  const long long row = blockIdx.x;
  const int b = (int)(row % B);
  const bool kl_row = kl_out != nullptr && row < B;             // the s = 0 rows own the KL terms
  const float* m = mean + (long long)b * head_ld;
  const float* v = lv + (long long)b * head_ld;
  float* o = out + row * ld;
  uint64_t key = 0;
  if (!eps_in) key = latent_key(rng_base_key(seed, dev_counter));
  double acc = 0.0;
  for (int l = threadIdx.x; l < L; l += kVaeBlock) {
    const double mv = (double)m[l], vv = (double)v[l];
    const float e = eps_in ? eps_in[row * L + l] : normal_at(key, offset + (uint64_t)(row * L + l));
    if (eps_out) eps_out[row * L + l] = e;
    o[l] = (float)(mv + (double)e * exp((double)k * vv));
    if (kl_row) acc += exp(vv) + mv * mv - 1.0 - vv;
  }
  if (write_cond) {
    const int c0 = L + 256 * c.n_emb;
    for (int col = L + threadIdx.x; col < ld; col += kVaeBlock) {
      float val = 0.f;
      if (col < c0) {
        const int j = (col - L) >> 8, kk = (col - L) & 255;
        for (int n = 0; n < c.ncls[j]; ++n) {
          const float w = vae_attr(c.oh[j], c.is_int[j], (long long)b * c.ncls[j] + n);
          if (w != 0.f) val += w * c.tab[j][n * 256 + kk];
        }
      } else if (col < c0 + c.n_cont) {
        val = c.cont[(long long)b * c.n_cont + (col - c0)];
      }
      o[col] = val;
    }
  }
  if (!kl_row) return;                                          // (block-uniform)
  const double dkl = 0.5 * block_sum<kVaeWaves>(acc, red);
  if (threadIdx.x == 0) partial_store(part + b, dkl);
  if (!arrive_last(ctr, B, &s_last)) return;
  const double total = vae_fold(part, B, red);
  if (threadIdx.x == 0) kl_out[0] = (float)total;
}

template <bool kVec>
__global__ void __launch_bounds__(kVaeBlock)
vae_loglik_kernel(const float* __restrict__ x, const float* __restrict__ xhat, int B, int S, int P, float log_var,
                  const float* __restrict__ kl_sum, float kl_weight, float gscale, float* __restrict__ out3,
                  float* __restrict__ gxhat, unsigned long long* part, int* ctr) {
  __shared__ double red[kVaeWaves];
  __shared__ int s_last;
  const long long R = (long long)S * B;
  const double inv = exp(-(double)log_var);
  const double gs = (double)gscale * inv / (double)R;
  double acc = 0.0;
  for (long long row = blockIdx.x; row < R; row += gridDim.x) {
    const float* xr = x + (row % B) * P;
    const float* hr = xhat + row * P;
    float* gr = gxhat ? gxhat + row * P : nullptr;
    if (kVec) {                                                  // P % 4 == 0 and 16-byte aligned bases
      for (int p = threadIdx.x * 4; p < P; p += kVaeBlock * 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xr + p);
        const f32x4 h = *reinterpret_cast<const f32x4*>(hr + p);
        double d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { d[i] = (double)h[i] - (double)a[i]; acc += d[i] * d[i]; }
        if (gr) *reinterpret_cast<f32x4*>(gr + p) = f32x4{(float)(gs * d[0]), (float)(gs * d[1]), (float)(gs * d[2]),
                                                          (float)(gs * d[3])};
      }
    } else {
      for (int p = threadIdx.x; p < P; p += kVaeBlock) {
        const double d = (double)hr[p] - (double)xr[p];
        acc += d * d;
        if (gr) gr[p] = (float)(gs * d);
      }
    }
  }
  const double sq = block_sum<kVaeWaves>(acc, red);
  if (threadIdx.x == 0) partial_store(part + blockIdx.x, sq);
  if (!arrive_last(ctr, (int)gridDim.x, &s_last)) return;
  const double total = vae_fold(part, (int)gridDim.x, red);
  if (threadIdx.x != 0) return;
  const double lp = -0.5 * inv * total / (double)R - 0.5 * (double)P * (double)log_var
                    - 0.5 * (double)P * 1.8378770664093454835606594728112;     // log(2 pi)
  const double klm = kl_sum ? (double)kl_sum[0] / (double)B : 0.0;
  out3[0] = (float)lp;
  out3[1] = (float)-(lp - (double)kl_weight * klm);
  out3[2] = (float)klm;
}

__global__ void __launch_bounds__(kVaeBlock)
vae_latent_bwd_kernel(const float* __restrict__ gin, int ld, const float* __restrict__ eps, const float* __restrict__ mean,
                      const float* __restrict__ lv, int head_ld, int S, int B, int L, float k, float kl_weight,
                      const float* __restrict__ kl_scale, float* __restrict__ gmean, float* __restrict__ glv, int gld,
                      int ncond, float* __restrict__ gcond) {
  const int b = blockIdx.x;
  const int col = blockIdx.y * kVaeBlock + threadIdx.x;
  if (col >= L + ncond) return;
  if (col >= L) {                                                // a conditioning column: its sum over the S draws
    double g = 0.0;
    for (int s = 0; s < S; ++s) g += (double)gin[((long long)s * B + b) * ld + col];
    gcond[(long long)b * ncond + (col - L)] = (float)g;
    return;
  }
  double gm = 0.0, gl = 0.0;
  for (int s = 0; s < S; ++s) {                                  // draws in order
    const long long row = (long long)s * B + b;
    const double gz = (double)gin[row * ld + col];
    gm += gz;
    gl += gz * (double)eps[row * L + col];
  }
  const double mv = (double)mean[(long long)b * head_ld + col], vv = (double)lv[(long long)b * head_ld + col];
  const double kw = (double)kl_weight * (kl_scale ? (double)kl_scale[0] : 1.0) / (double)B;
  gmean[(long long)b * gld + col] = (float)(gm + kw * mv);
  glv[(long long)b * gld + col] = (float)(gl * (double)k * exp((double)k * vv) + kw * 0.5 * (exp(vv) - 1.0));
}

}  // namespace ali

using namespace ali;

extern "C" int ali_vae_latent_fwd(const float* mean, const float* log_var, int32_t head_ld, const float* eps,
                                  float* eps_out, uint64_t seed, const int64_t* dev_counter, uint64_t offset, int32_t S,
                                  int32_t B, int32_t L, float k, const void* const* onehot, const int32_t* n_classes,
                                  const int32_t* onehot_is_int, const float* const* tables, int32_t n_emb,
                                  const float* cont, int32_t n_cont, int32_t write_cond, int32_t ld, float* out,
                                  float* kl_out, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!mean || !log_var || !out || S < 1 || B < 1 || L < 1 || head_ld < L || ld < L || (long long)S * B >= (1LL << 31)) {
    set_error("ali_vae_latent_fwd: bad argument");
    return ALI_ERR_BAD_ARG;
  }
  VaeCond c = {};
  if (write_cond) {
    if (n_emb < 0 || n_emb > kVaeMaxEmb || n_cont < 0 || (n_cont > 0 && !cont) ||
        (long long)L + 256LL * n_emb + n_cont > ld || (n_emb > 0 && (!onehot || !n_classes || !onehot_is_int || !tables))) {
      set_error("ali_vae_latent_fwd: bad conditioning (at most %d tables, L + 256 * n_emb + n_cont <= ld)", kVaeMaxEmb);
      return ALI_ERR_BAD_ARG;
    }
    for (int j = 0; j < n_emb; ++j) {
      if (!onehot[j] || !tables[j] || n_classes[j] < 1) {
        set_error("ali_vae_latent_fwd: bad conditioning table %d", j);
        return ALI_ERR_BAD_ARG;
      }
      c.oh[j] = onehot[j]; c.tab[j] = tables[j]; c.ncls[j] = n_classes[j]; c.is_int[j] = onehot_is_int[j];
    }
    c.cont = cont; c.n_emb = n_emb; c.n_cont = n_cont;
  }
  unsigned long long* part = nullptr;                             // (without kl_out nothing is folded)
  int* ctr = nullptr;
  if (kl_out) {
    const int rc = fold_workspace("ali_vae_latent_fwd", ws, ws_bytes, (size_t)B, &part, &ctr);
    if (rc != ALI_OK) return rc;
  }
  hipLaunchKernelGGL(vae_latent_fwd_kernel, dim3((unsigned)((long long)S * B)), dim3(kVaeBlock), 0, ST(stream), mean,
                     log_var, (int)head_ld, eps, eps_out, seed, reinterpret_cast<const long long*>(dev_counter), offset,
                     (int)S, (int)B, (int)L, k, c, (int)(write_cond != 0), (int)ld, out, kl_out, part, ctr);
  return check_launch("vae_latent_fwd_kernel");
}

extern "C" int ali_vae_loglik(const float* x, const float* xhat, int32_t B, int32_t S, int32_t P, float log_var,
                              const float* kl_sum, float kl_weight, float gscale, float* out3, float* gxhat, void* ws,
                              size_t ws_bytes, ali_stream_t stream) {
  if (!x || !xhat || !out3 || B < 1 || S < 1 || P < 1 || (long long)S * B >= (1LL << 31)) {
    set_error("ali_vae_loglik: bad argument");
    return ALI_ERR_BAD_ARG;
  }
  const long long R = (long long)S * B;
  const int blocks = (int)(R < kVaeMaxBlocks ? R : kVaeMaxBlocks);
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_vae_loglik", ws, ws_bytes, (size_t)blocks, &part, &ctr);
  if (rc != ALI_OK) return rc;
  const bool vec = P % 4 == 0 && aligned16(x) && aligned16(xhat) && (!gxhat || aligned16(gxhat));
  if (vec)
    hipLaunchKernelGGL(vae_loglik_kernel<true>, dim3(blocks), dim3(kVaeBlock), 0, ST(stream), x, xhat, (int)B, (int)S,
                       (int)P, log_var, kl_sum, kl_weight, gscale, out3, gxhat, part, ctr);
  else
    hipLaunchKernelGGL(vae_loglik_kernel<false>, dim3(blocks), dim3(kVaeBlock), 0, ST(stream), x, xhat, (int)B, (int)S,
                       (int)P, log_var, kl_sum, kl_weight, gscale, out3, gxhat, part, ctr);
  return check_launch("vae_loglik_kernel");
}

extern "C" int ali_vae_latent_bwd(const float* gin, int32_t ld, const float* eps, const float* mean, const float* log_var,
                                  int32_t head_ld, int32_t S, int32_t B, int32_t L, float k, float kl_weight,
                                  const float* kl_scale, float* gmean, float* glog_var, int32_t gld, int32_t ncond,
                                  float* gcond, ali_stream_t stream) {
  if (!gin || !eps || !mean || !log_var || !gmean || !glog_var || S < 1 || B < 1 || L < 1 || head_ld < L || gld < L ||
      ncond < 0 || (ncond > 0 && !gcond) || (long long)L + ncond > ld || (long long)S * B >= (1LL << 31)) {
    set_error("ali_vae_latent_bwd: bad argument");
    return ALI_ERR_BAD_ARG;
  }
  const int ny = (L + ncond + kVaeBlock - 1) / kVaeBlock;
  if (ny > 65535) {
    set_error("ali_vae_latent_bwd: L + ncond = %d too wide", (int)(L + ncond));
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(vae_latent_bwd_kernel, dim3((unsigned)B, (unsigned)ny), dim3(kVaeBlock), 0, (hipStream_t)stream, gin,
                     (int)ld, eps, mean, log_var, (int)head_ld, (int)S, (int)B, (int)L, k, kl_weight, kl_scale, gmean,
                     glog_var, (int)gld, (int)ncond, gcond);
  return check_launch("vae_latent_bwd_kernel");
}
