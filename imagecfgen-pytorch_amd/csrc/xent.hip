// Softmax cross-entropy against probability targets, its gradient, the arg-max prediction and the hit count of a
// [B][C] logit batch in ONE launch (include/ali_hip.h: ali_softmax_xent) -- nn.CrossEntropyLoss() with float one-hot /
// soft rows plus the `.argmax(1) == .argmax(1)).sum()` of the classifier loops (classifiers/mnist.py:48-56,
// audiomnist_generator_score.py:90-98).
//
// One 64-lane wave per row, lanes strided over the C columns, four waves per block, rows grid-strided.  Three passes
// over the row (it stays in L1 / L2: C <= 4096):
//   1. max and first arg-max of the logits, first arg-max of the targets, sum of the targets
//   2. sum exp(z - max)                                 -> lse = max + log(sum)
//   3. loss_b = sum t * (lse - z),  glogit = gscale * (exp(z - lse) * sum t - t) / B
// The row arithmetic is fp64 (exp and log included): the kernel is launch bound at every size the callers have, and
// every fp32 result is then the rounding of an fp64 evaluation, whatever |logit| <= 1e4 does to z - max.
// Cross-lane reductions are xor butterflies (a + b == b + a bit for bit, so all lanes agree); the arg-max butterfly
// carries the index and prefers the lower one on equal values, which is torch.argmax's first maximum.
// Rows -> wave partials (fixed row order) -> block partial (waves 0..3 in order) -> 8-byte write-through stores into
// the workspace; the block that arrives last at the counter adds the block partials in block order.  No float atomics:
// the same inputs give the same bits on every run.  The counter is the last int of the workspace's reserved head
// (zero between launches, like the split-K counters in front of it) and is left at zero.
//
// NaN logits (what falls out, untested): comparisons with NaN are false, so a NaN never becomes the maximum or the
// prediction -- torch.argmax would pick it --; exp(NaN - max) makes the row's loss and gradient NaN, and with them out2[0].
#include "ali_common.h"

#include <limits.h>

namespace ali {

constexpr int kXentWaves = 4;
constexpr int kXentMaxBlocks = 1024;
constexpr int kXentCtr = (int)(kWsReserved / sizeof(int)) - 1;

struct XentPart { unsigned long long loss_bits; unsigned long long hits; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

__global__ void __launch_bounds__(kXentWaves * 64)
softmax_xent_kernel(const float* __restrict__ logit, const float* __restrict__ target, int B, int C, float gscale,
                    float* __restrict__ out2, float* __restrict__ glogit, int* __restrict__ pred,
                    long long* __restrict__ hits_accum, XentPart* part, int* ctr) {
  __shared__ double s_loss[kXentWaves];
  __shared__ int s_hits[kXentWaves];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double loss_w = 0.0;
  int hits_w = 0;
  for (long long b = (long long)blockIdx.x * kXentWaves + wave; b < B; b += (long long)gridDim.x * kXentWaves) {
    const float* z = logit + b * C;
    const float* t = target + b * C;
    float zmax = -INFINITY, tmax = -INFINITY;
    int zi = lane < C ? lane : INT_MAX, ti = zi;   // (a row of -inf / NaN only: the lane's first column)
    double tsum = 0.0;
    for (int j = lane; j < C; j += 64) {           // ascending j per lane: a strict > keeps the lane's first maximum
      const float zv = z[j], tv = t[j];
      if (zv > zmax) { zmax = zv; zi = j; }
      if (tv > tmax) { tmax = tv; ti = j; }
      tsum += (double)tv;
    }
    wave_argmax(zmax, zi);
    wave_argmax(tmax, ti);
    tsum = wave_sum(tsum);
    double esum = 0.0;
    for (int j = lane; j < C; j += 64) esum += exp((double)z[j] - (double)zmax);
    esum = wave_sum(esum);
    const double lse = (double)zmax + log(esum);
    const double gs = (double)gscale / (double)B;
    double loss = 0.0;
    for (int j = lane; j < C; j += 64) {
      const double zv = (double)z[j], tv = (double)t[j];
      loss += tv * (lse - zv);
      if (glogit) glogit[b * C + j] = (float)(gs * (exp(zv - lse) * tsum - tv));
    }
    loss = wave_sum(loss);
    loss_w += loss;
    hits_w += (zi == ti) ? 1 : 0;
    if (pred && lane == 0) pred[b] = zi;
  }
  if (lane == 0) { s_loss[wave] = loss_w; s_hits[wave] = hits_w; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    long long h = 0;
    for (int w = 0; w < kXentWaves; ++w) { l += s_loss[w]; h += s_hits[w]; }
    // write-through (device-scope) stores, drained before the arrival: the reducer's device-scope loads see them on
    // whichever XCD it runs
    __hip_atomic_store(&part[blockIdx.x].loss_bits, (unsigned long long)__double_as_longlong(l), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&part[blockIdx.x].hits, (unsigned long long)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int arrived = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = arrived == (int)gridDim.x - 1;
    if (s_last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // all blocks have arrived
  }
  __syncthreads();
  if (!s_last || threadIdx.x != 0) return;
  double total = 0.0;
  long long hits = 0;
  for (int i = 0; i < (int)gridDim.x; ++i) {       // block order, whichever block this is
    total += __longlong_as_double((long long)__hip_atomic_load(&part[i].loss_bits, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT));
    hits += (long long)__hip_atomic_load(&part[i].hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  out2[0] = (float)(total / (double)B);
  out2[1] = (float)hits;
  if (hits_accum) *hits_accum += hits;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_softmax_xent(const float* logit, const float* target, int32_t B, int32_t C, float gscale,
                                float* out2, float* glogit, int32_t* pred, int64_t* hits_accum, void* ws,
                                size_t ws_bytes, ali_stream_t stream) {
  if (C < 1 || C > 4096) {
    set_error("ali_softmax_xent: C = %d outside [1, 4096]", (int)C);
    return ALI_ERR_BAD_ARG;
  }
  if (B < 1 || (long long)B * C >= (1LL << 31)) {
    set_error("ali_softmax_xent: B = %d outside [1, 2^31 / C)", (int)B);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !target || !out2) {
    set_error("ali_softmax_xent: logit, target and out2 must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  int blocks = (B + kXentWaves - 1) / kXentWaves;
  if (blocks > kXentMaxBlocks) blocks = kXentMaxBlocks;
  if (!ws || ws_payload_bytes(ws_bytes) < (size_t)blocks * sizeof(XentPart)) {
    set_error("ali_softmax_xent: workspace too small (%zu bytes behind the reserved head needed)",
              (size_t)blocks * sizeof(XentPart));
    return ALI_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(blocks), dim3(kXentWaves * 64), 0, (hipStream_t)stream, logit, target,
                     (int)B, (int)C, gscale, out2, glogit, reinterpret_cast<int*>(pred),
                     reinterpret_cast<long long*>(hits_accum), reinterpret_cast<XentPart*>(ws_payload(ws)),
                     reinterpret_cast<int*>(ws) + kXentCtr);
  return check_launch("softmax_xent_kernel");
}
