// What sits between the conv stacks of a WGAN-GP critic step (gans/audio_mnist.py: wgan_loss_it, compute_gradient_penalty;
// include/ali_hip.h: ali_gp_mix, ali_gp_penalty, ali_wgan_critic).
//
//   ali_gp_mix       xhat = eps * x_real + (1 - eps) * x_fake, eps per image: given, or drawn from the counter RNG
//   ali_gp_penalty   per-image 2-norm of the critic's input gradient, the penalty mean_b (n_b - 1)^2, and the tangent
//                    v_b = lambda * (2 / B) * (1 - 1 / n_b) * g0_b that the second (forward) pass pushes through the critic
//   ali_wgan_critic  mean(d_fake) - mean(d_real), the two means, and the constant logit gradients
//
// At the sizes the callers have (B = 64 images of 128 x 128 floats: 4 MB per operand) all three are bound by launch and
// memory latency, not by bandwidth: one block per image (penalty) or a few per image (mix), 16-byte accesses where the
// row length and the pointers allow them, everything else one element at a time.
// Reductions are fp64 in a fixed order (ali_reduce.h, the hand-off between blocks included): elements thread-strided,
// lanes, waves in order, images in order by thread 0 of the block that arrives last.  wgan_critic_kernel is one block
// with an LDS tree of its own.  The scalars are written by one thread with ordinary vector stores.
#include "ali_reduce.h"

namespace ali {

constexpr int kGpThreads = 1024;
constexpr int kGpWaves = kGpThreads / 64;
constexpr int kMixThreads = 256;

struct GpPart { unsigned long long pen_bits; unsigned long long norm_bits; };

// uniform in [0, 1): the top 24 bits of the hash of image g under the stream's key (ali_rng.h: gp_key)
__device__ __forceinline__ float gp_uniform(uint64_t key, uint64_t g) { return (float)hi24(hash_at(key, g)) * kInv24; }

// The products and the sum are rounded one by one -- contraction into a fused multiply-add is switched off for this
// function -- so the result is torch's fp32 statement eps * x_real + (1 - eps) * x_fake bit for bit.
__device__ __forceinline__ float gp_mix1(float e, float om, float xr, float xf) {
#pragma clang fp contract(off)
  const float a = e * xr;
  const float b = om * xf;
  return a + b;
}

__global__ void __launch_bounds__(kMixThreads)
gp_mix_kernel(const float* __restrict__ x_real, const float* __restrict__ x_fake, const float* __restrict__ eps_in,
              uint64_t seed, const long long* __restrict__ dev_counter, uint64_t offset, int B, long long P,
              float* __restrict__ xhat, float* __restrict__ eps_out, int vec) {
  const int b = blockIdx.y;
  float e;
  if (eps_in) {
    e = eps_in[b];
  } else {
    e = gp_uniform(gp_key(rng_base_key(seed, dev_counter)), offset + (uint64_t)b);
  }
  if (eps_out && blockIdx.x == 0 && threadIdx.x == 0) eps_out[b] = e;
  const float om = 1.f - e;
  const long long base = (long long)b * P;
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {                                   // P % 4 == 0 and 16-byte aligned bases: every row starts on a boundary
    const f32x4* r4 = reinterpret_cast<const f32x4*>(x_real + base);
    const f32x4* f4 = reinterpret_cast<const f32x4*>(x_fake + base);
    f32x4* o4 = reinterpret_cast<f32x4*>(xhat + base);
    for (long long i = t0; i < (P >> 2); i += step) {
      const f32x4 r = r4[i], f = f4[i];
      o4[i] = f32x4{gp_mix1(e, om, r.x, f.x), gp_mix1(e, om, r.y, f.y), gp_mix1(e, om, r.z, f.z),
                    gp_mix1(e, om, r.w, f.w)};
    }
  } else {
    for (long long i = t0; i < P; i += step) xhat[base + i] = gp_mix1(e, om, x_real[base + i], x_fake[base + i]);
  }
}

// One block per image.  g0 and v may be the same buffer: an element is read and written by the same thread, and the
// norm pass is complete (block barrier) before the first store.
__global__ void __launch_bounds__(kGpThreads)
gp_penalty_kernel(const float* g0, int B, long long P, float lambda, float* __restrict__ out2, float* v, GpPart* part,
                  int* ctr, int vec) {
  __shared__ double s_w[kGpWaves];
  __shared__ int s_last;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* g = g0 + (long long)b * P;
  float* o = v ? v + (long long)b * P : nullptr;
  double ss = 0.0;
  if (vec) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    for (long long i = t; i < (P >> 2); i += kGpThreads) {
      const f32x4 a = g4[i];
      ss += (double)a.x * a.x;
      ss += (double)a.y * a.y;
      ss += (double)a.z * a.z;
      ss += (double)a.w * a.w;
    }
  } else {
    for (long long i = t; i < P; i += kGpThreads) { const float a = g[i]; ss += (double)a * a; }
  }
  const double n = sqrt(block_sum<kGpWaves>(ss, s_w));       // (its barriers: the norm pass is complete)
  if (o) {
    // d/dg (n - 1)^2 / B = (2 / B) (n - 1) g / n; at n == 0 the subgradient 0, as torch's norm backward
    const float sc = n > 0.0 ? (float)((double)lambda * (2.0 / (double)B) * (1.0 - 1.0 / n)) : 0.f;
    if (vec) {
      const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
      f32x4* o4 = reinterpret_cast<f32x4*>(o);
      for (long long i = t; i < (P >> 2); i += kGpThreads) {
        const f32x4 a = g4[i];
        o4[i] = f32x4{sc * a.x, sc * a.y, sc * a.z, sc * a.w};
      }
    } else {
      for (long long i = t; i < P; i += kGpThreads) o[i] = sc * g[i];
    }
  }
  if (t == 0) {
    partial_store(&part[b].pen_bits, (n - 1.0) * (n - 1.0));
    partial_store(&part[b].norm_bits, n);
  }
  if (!arrive_last(ctr, (int)gridDim.x, &s_last) || t != 0) return;
  double pen = 0.0, nrm = 0.0;
  for (int i = 0; i < B; ++i) {                    // image order, whichever block this is
    pen += partial_load(&part[i].pen_bits);
    nrm += partial_load(&part[i].norm_bits);
  }
  out2[0] = (float)(pen / (double)B);
  out2[1] = (float)(nrm / (double)B);
}

// single block (B: a batch of logits)
__global__ void __launch_bounds__(kMixThreads)
wgan_critic_kernel(const float* __restrict__ d_fake, const float* __restrict__ d_real, int B, float gscale,
                   float* __restrict__ out3, float* __restrict__ g_fake, float* __restrict__ g_real) {
  __shared__ double r1[kMixThreads], r2[kMixThreads];
  const int t = threadIdx.x;
  double sf = 0.0, sr = 0.0;
  const float gf = gscale / (float)B;
  for (int i = t; i < B; i += kMixThreads) {
    if (d_fake) sf += (double)d_fake[i];
    if (d_real) sr += (double)d_real[i];
    if (g_fake) g_fake[i] = gf;
    if (g_real) g_real[i] = -gf;
  }
  r1[t] = sf;
  r2[t] = sr;
  __syncthreads();
  for (int off = kMixThreads / 2; off > 0; off >>= 1) {
    if (t < off) { r1[t] += r1[t + off]; r2[t] += r2[t + off]; }
    __syncthreads();
  }
  if (t == 0) {
    const double mf = r1[0] / (double)B, mr = r2[0] / (double)B;
    out3[0] = (float)(mf - mr);
    out3[1] = (float)mf;
    out3[2] = (float)mr;
  }
}

}  // namespace ali

using namespace ali;

extern "C" int ali_gp_mix(const float* x_real, const float* x_fake, const float* eps, uint64_t seed,
                          const int64_t* dev_counter, uint64_t offset, int32_t B, int64_t P, float* xhat,
                          float* eps_out, ali_stream_t stream) {
  if (!x_real || !x_fake || !xhat) { set_error("ali_gp_mix: x_real, x_fake and xhat must not be NULL"); return ALI_ERR_BAD_ARG; }
  if (B < 1 || B > 65535 || P < 1 || (long long)B * P >= (1LL << 40)) {
    set_error("ali_gp_mix: B = %d outside [1, 65535] or P = %lld outside [1, 2^40 / B)", (int)B, (long long)P);
    return ALI_ERR_BAD_ARG;
  }
  const int vec = (P % 4) == 0 && aligned16(x_real) && aligned16(x_fake) && aligned16(xhat);
  const long long work = vec ? P / 4 : P;
  long long bx = (work + kMixThreads - 1) / kMixThreads;
  if (bx > 64) bx = 64;                        // (grid-strided beyond)
  hipLaunchKernelGGL(gp_mix_kernel, dim3((unsigned)bx, (unsigned)B), dim3(kMixThreads), 0, (hipStream_t)stream, x_real,
                     x_fake, eps, seed, reinterpret_cast<const long long*>(dev_counter), offset, (int)B, (long long)P,
                     xhat, eps_out, vec);
  return check_launch("gp_mix_kernel");
}

extern "C" int ali_gp_penalty(const float* g0, int32_t B, int64_t P, float lambda, float* out2, float* v, void* ws,
                              size_t ws_bytes, ali_stream_t stream) {
  if (!g0 || !out2) { set_error("ali_gp_penalty: g0 and out2 must not be NULL"); return ALI_ERR_BAD_ARG; }
  if (B < 1 || B > 65535 || P < 1 || (long long)B * P >= (1LL << 40)) {
    set_error("ali_gp_penalty: B = %d outside [1, 65535] or P = %lld outside [1, 2^40 / B)", (int)B, (long long)P);
    return ALI_ERR_BAD_ARG;
  }
  GpPart* part;
  int* ctr;
  const int rc = fold_workspace("ali_gp_penalty", ws, ws_bytes, (size_t)B, &part, &ctr);
  if (rc != ALI_OK) return rc;
  const int vec = (P % 4) == 0 && aligned16(g0) && (!v || aligned16(v));
  hipLaunchKernelGGL(gp_penalty_kernel, dim3((unsigned)B), dim3(kGpThreads), 0, ST(stream), g0, (int)B, (long long)P,
                     lambda, out2, v, part, ctr, vec);
  return check_launch("gp_penalty_kernel");
}

extern "C" int ali_wgan_critic(const float* d_fake, const float* d_real, int32_t B, float gscale, float* out3,
                               float* g_fake, float* g_real, ali_stream_t stream) {
  if ((!d_fake && !d_real) || !out3 || B < 1) {
    set_error("ali_wgan_critic: needs d_fake or d_real, out3 and B >= 1");
    return ALI_ERR_BAD_ARG;
  }
  if ((g_fake && !d_fake) || (g_real && !d_real)) {
    set_error("ali_wgan_critic: a gradient was asked for logits that were not given");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(wgan_critic_kernel, dim3(1), dim3(kMixThreads), 0, (hipStream_t)stream, d_fake, d_real, (int)B, gscale,
                     out3, g_fake, g_real);
  return check_launch("wgan_critic_kernel");
}
