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
// Reductions and the hand-off between blocks: ali_reduce.h.  Here: rows -> wave partials (fixed row order) -> block
// partial (waves 0..3 in order) -> the block that arrives last adds the block partials, thread 0, blocks ascending.
//
// NaN logits (what falls out, untested): comparisons with NaN are false, so a NaN never becomes the maximum or the
// prediction -- torch.argmax would pick it --; exp(NaN - max) makes the row's loss and gradient NaN, and with them out2[0].
#include "ali_reduce.h"

#include <limits.h>

namespace ali {

constexpr int kXentWaves = 4;
constexpr int kXentMaxBlocks = 1024;

struct XentPart { unsigned long long loss_bits; unsigned long long hits; };

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
  const double l = waves_sum<kXentWaves>(loss_w, s_loss);
  const int h = waves_sum<kXentWaves>(hits_w, s_hits);
  if (threadIdx.x == 0) {
    partial_store(&part[blockIdx.x].loss_bits, l);
    partial_store_int(&part[blockIdx.x].hits, (unsigned long long)h);
  }
  if (!arrive_last(ctr, (int)gridDim.x, &s_last) || threadIdx.x != 0) return;
  double total = 0.0;
  long long hits = 0;
  for (int i = 0; i < (int)gridDim.x; ++i) {       // block order, whichever block this is
    total += partial_load(&part[i].loss_bits);
    hits += (long long)partial_load_int(&part[i].hits);
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
  XentPart* part;
  int* ctr;
  const int rc = fold_workspace("ali_softmax_xent", ws, ws_bytes, (size_t)blocks, &part, &ctr);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(blocks), dim3(kXentWaves * 64), 0, ST(stream), logit, target, (int)B,
                     (int)C, gscale, out2, glogit, reinterpret_cast<int*>(pred),
                     reinterpret_cast<long long*>(hits_accum), part, ctr);
  return check_launch("softmax_xent_kernel");
}
