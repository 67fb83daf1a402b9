// The deterministic reductions of the loss and family kernels (xent.hip, vae.hip, gan.hip, explain.hip), once.
//
// Every sum runs in a fixed order, without float atomics, so the same inputs give the same bits on every run:
//   lanes   xor butterflies: a + b == b + a bit for bit, so all 64 lanes end with the same value
//   waves   lane 0 of each wave writes s[wave]; every thread adds s[0] .. s[WAVES-1] ascending
//   blocks  each block publishes its partial in the workspace and arrives at a counter; the block that arrives last
//           folds the partials in an order of the kernel's own (it is part of the result, so it stays in the kernel)
//
// The hand-off between blocks is the one piece whose correctness rests on the MI355X memory model: the L2s are private
// per XCD, so a partial must be stored write-through (a relaxed agent-scope atomic store) and drained (s_waitcnt
// vmcnt(0)) before the arrival is signalled, and every load of the fold must bypass L1 (a relaxed agent-scope atomic
// load), whichever XCD the last block runs on.  The order here is the protocol; change none of it without measuring.
#pragma once
#include "ali_common.h"

namespace ali {

// ---------------------------------------------------------------------------------------------------------- lanes
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// the maximum and its index; the lower index on equal values (torch.argmax's first maximum)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// ---------------------------------------------------------------------------------------------------------- waves
// Called by all WAVES * 64 threads of the block; every thread gets the same value.  `s` holds WAVES elements.  One
// barrier discipline: write, barrier, read, barrier -- `s` is free again when a call returns, so calls may follow each
// other on the same `s`, and nothing needs to be known about what ran before.
//
// waves_sum: v is already the same in every lane of a wave (a butterfly's result, or a count the wave agrees on).
template <int WAVES, typename T>
__device__ __forceinline__ T waves_sum(T v, T* s) {
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += s[w];
  __syncthreads();
  return t;
}

template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* s) {
  return waves_sum<WAVES>(wave_sum(v), s);
}

template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* s) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = -INFINITY;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t = fmaxf(t, s[w]);
  __syncthreads();
  return t;
}

// --------------------------------------------------------------------------------------------------------- blocks
// One thread of a block (thread 0) stores the block's partials; then all threads call arrive_last, which tells every
// thread whether this block arrived last; that block folds with partial_load.
__device__ __forceinline__ void partial_store_int(unsigned long long* slot, unsigned long long v) {
  __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void partial_store(unsigned long long* slot, double v) {
  partial_store_int(slot, (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ unsigned long long partial_load_int(const unsigned long long* slot) {
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double partial_load(const unsigned long long* slot) {
  return __longlong_as_double((long long)partial_load_int(slot));
}

// `expected` blocks arrive at *ctr; `s_last` is one int of LDS.  Thread 0 drains its partial stores, arrives, and --
// when it is the last, so that all have arrived -- puts the counter back to zero for the next launch.
__device__ __forceinline__ bool arrive_last(int* ctr, int expected, int* s_last) {
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int arrived = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = arrived == expected - 1;
    if (*s_last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return *s_last != 0;
}

// The arrival counter: the last int of the workspace's reserved head.  That int is also the split-K arrival counter of
// tile kWsReserved / sizeof(int) - 1 of a GEMM launch (gconv.hip: one counter per tile), and every kernel here uses the
// same one.  Sharing is safe because every user of a workspace slab runs stream-ordered on it -- no two of these
// launches overlap -- and each leaves the word at zero, which is all the next one needs to find.
constexpr int kFoldCtr = (int)(kWsReserved / sizeof(int)) - 1;

// The partials (n of type T behind the reserved head) and the counter of workspace `ws`, or the error of entry point
// `who` when the workspace is missing or too small.
template <typename T>
inline int fold_workspace(const char* who, void* ws, size_t ws_bytes, size_t n, T** part, int** ctr) {
  if (!ws || ws_payload_bytes(ws_bytes) < n * sizeof(T)) {
    set_error("%s: workspace too small (%zu bytes behind the reserved head needed)", who, n * sizeof(T));
    return ALI_ERR_WORKSPACE;
  }
  *part = reinterpret_cast<T*>(ws_payload(ws));
  *ctr = reinterpret_cast<int*>(ws) + kFoldCtr;
  return ALI_OK;
}

}  // namespace ali
