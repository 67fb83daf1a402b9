// The distance arithmetic of the cf_eval family (include/ali_hip.h: ali_group_moments, ali_manifold_err) -- the
// "mean squared distance to the same subject's recordings over the mean squared distance to every other subject's" of
// audiomnist_cf_eval.py:93-131 without the [M][n][D] pair tensor.  For a cell of n rows b_j with column sums S and
// column sums of squares Q,
//     sum_j ||a - b_j||^2 = sum_k (n a_k^2 - 2 a_k S_k + Q_k),
// every term of the right-hand sum being sum_j (a_k - b_jk)^2 >= 0 itself: cancellation stays inside a column, where
// fp64 holds it (the products of two fp32 values are exact in fp64), and nothing cancels across columns.
//
// Both are bytes-moved kernels:
//   ali_group_moments  grid (column chunks, cells): a thread owns 4 columns (16-byte loads) or 1, walks its cell's rows
//                      in ascending row order, four row loads in flight, and writes S and Q once; a second launch of
//                      (column chunks, classes) folds the cells of a class in ascending owner order from 0.  Reads
//                      4 N D bytes, writes 16 (O C + C) D.  No sum crosses a thread: no workspace.
//   ali_manifold_err   grid (split, M) like ali_row_dist: block (k, m) adds chunk k of row m, two fp64 partials per
//                      block; the block that arrives last folds every row's partials in block order.  Reads 4 D bytes
//                      of the row and 32 D of its cell's and class's moments (shared by the rows of a cell: L2).
// Every sum runs in a fixed order without float atomics: the same inputs give the same bits on every run.  The row and
// cell indices are device data: one outside its range reads nothing (see the NaN corners in the header).
#include "ali_reduce.h"

namespace ali {

constexpr int kEvBlock = 256;
constexpr int kEvWaves = kEvBlock / 64;
constexpr int kEvChunk = 4096;                                       // elements of a row one block adds up
constexpr int kEvMaxSplit = 64;
constexpr int kEvRowsInFlight = 4;

// -------------------------------------------------------------------------------------------------- group_moments
template <int W> struct EvLoad;
template <> struct EvLoad<1> {
  float v[1];
  __device__ __forceinline__ void get(const float* p) { v[0] = p[0]; }
};
template <> struct EvLoad<4> {
  float v[4];
  __device__ __forceinline__ void get(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
};

// block (x, y): columns [x * kEvBlock * W, ...) of cell y; thread t owns W consecutive columns
template <int W>
__global__ void __launch_bounds__(kEvBlock)
group_moments_kernel(const float* __restrict__ rows, long long ld, int N, int D, const int* __restrict__ order,
                     int n_order, const int* __restrict__ start, double* __restrict__ S, double* __restrict__ Q) {
  const int cell = blockIdx.y;
  const long long col = ((long long)blockIdx.x * kEvBlock + threadIdx.x) * W;
  if (col >= D) return;
  int lo = start[cell], hi = start[cell + 1];
  if (lo < 0) lo = 0;
  if (hi > n_order) hi = n_order;
  double s[W], q[W];
#pragma unroll
  for (int w = 0; w < W; ++w) s[w] = q[w] = 0.0;
  auto add = [&](const EvLoad<W>& x) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const double d = (double)x.v[w];
      s[w] += d;
      q[w] += d * d;
    }
  };
  auto row_ok = [&](int r) { return r >= 0 && r < N; };              // (an index outside the table adds nothing)
  int j = lo;
  for (; j + kEvRowsInFlight <= hi; j += kEvRowsInFlight) {
    int r[kEvRowsInFlight];
    EvLoad<W> x[kEvRowsInFlight];
#pragma unroll
    for (int u = 0; u < kEvRowsInFlight; ++u) r[u] = order[j + u];
#pragma unroll
    for (int u = 0; u < kEvRowsInFlight; ++u)
      if (row_ok(r[u])) x[u].get(rows + (long long)r[u] * ld + col);
#pragma unroll
    for (int u = 0; u < kEvRowsInFlight; ++u)                        // ascending position: ascending row
      if (row_ok(r[u])) add(x[u]);
  }
  for (; j < hi; ++j) {
    const int r = order[j];
    if (!row_ok(r)) continue;
    EvLoad<W> x;
    x.get(rows + (long long)r * ld + col);
    add(x);
  }
  double* sp = S + (long long)cell * D + col;
  double* qp = Q + (long long)cell * D + col;
  if constexpr (W == 4) {
    reinterpret_cast<double2*>(sp)[0] = make_double2(s[0], s[1]);
    reinterpret_cast<double2*>(sp)[1] = make_double2(s[2], s[3]);
    reinterpret_cast<double2*>(qp)[0] = make_double2(q[0], q[1]);
    reinterpret_cast<double2*>(qp)[1] = make_double2(q[2], q[3]);
  } else {
#pragma unroll
    for (int w = 0; w < W; ++w) { sp[w] = s[w]; qp[w] = q[w]; }
  }
}

// block (x, y): columns of class y; the fold over the owners starts from 0 and runs in ascending owner order, so a
// class held by one owner gives that owner's sums bit for bit (the other cells are +0)
__global__ void __launch_bounds__(kEvBlock)
class_totals_kernel(const double* __restrict__ S, const double* __restrict__ Q, int O, int C, int D,
                    double* __restrict__ TS, double* __restrict__ TQ) {
  const int c = blockIdx.y;
  const long long col = (long long)blockIdx.x * kEvBlock + threadIdx.x;
  if (col >= D) return;
  double ts = 0.0, tq = 0.0;
  for (int o = 0; o < O; ++o) {
    const long long at = ((long long)o * C + c) * D + col;
    ts += S[at];
    tq += Q[at];
  }
  TS[(long long)c * D + col] = ts;
  TQ[(long long)c * D + col] = tq;
}

// --------------------------------------------------------------------------------------------------- manifold_err
// what a row compares with: its cell (same) and its class less its cell (other)
struct EvRow {
  bool cls_ok, own_ok;
  long long cell, klass;
  int n, m;                                                          // rows in the cell, rows of the class outside it
};

__device__ __forceinline__ EvRow ev_row(const int* owner, const int* cls, const int* cnt, const int* tcnt, int O, int C,
                                        int r) {
  EvRow e;
  const int o = owner[r], c = cls[r];
  e.cls_ok = c >= 0 && c < C;
  e.own_ok = e.cls_ok && o >= 0 && o < O;
  e.cell = e.own_ok ? (long long)o * C + c : 0;
  e.klass = e.cls_ok ? c : 0;
  e.n = e.own_ok ? cnt[e.cell] : 0;
  e.m = e.cls_ok ? tcnt[e.klass] - e.n : 0;
  return e;
}

// one column of both sums: (n a^2 - 2 a S + Q, m a^2 - 2 a (TS - S) + (TQ - Q))
__device__ __forceinline__ void ev_col(double a, double s, double q, double ts, double tq, double n, double m,
                                       double& same, double& other) {
  const double a2 = a * a;
  same += (n * a2 - 2.0 * a * s) + q;
  other += (m * a2 - 2.0 * a * (ts - s)) + (tq - q);
}

template <bool VEC>
__global__ void __launch_bounds__(kEvBlock)
manifold_err_kernel(const float* __restrict__ cf, long long ld, int M, int D, long long chunk,
                    const int* __restrict__ owner, const int* __restrict__ cls, const double* __restrict__ S,
                    const double* __restrict__ Q, const double* __restrict__ TS, const double* __restrict__ TQ,
                    const int* __restrict__ cnt, const int* __restrict__ tcnt, int O, int C, float* __restrict__ out3,
                    unsigned long long* part, int* ctr) {
  __shared__ double s_red[kEvWaves];
  __shared__ int s_last;
  const int r = blockIdx.y, k = blockIdx.x, split = gridDim.x;
  const EvRow e = ev_row(owner, cls, cnt, tcnt, O, C, r);           // (the row is the block's: uniform branches)
  const float* a = cf + (long long)r * ld;
  const double* s = S + e.cell * D;
  const double* q = Q + e.cell * D;
  const double* ts = TS + e.klass * D;
  const double* tq = TQ + e.klass * D;
  const long long lo = (long long)k * chunk;
  long long hi = lo + chunk;
  if (hi > D) hi = D;
  const double n = (double)e.n, m = (double)e.m;
  double same = 0.0, other = 0.0;
  if (e.cls_ok) {                                                    // (a class outside the bank reads nothing)
    if (VEC) {
      for (long long i = lo + 4 * threadIdx.x; i < hi; i += 4 * kEvBlock) {
        const float4 av = *reinterpret_cast<const float4*>(a + i);
        double2 s0 = make_double2(0.0, 0.0), s1 = s0, q0 = s0, q1 = s0;
        if (e.own_ok) {
          s0 = *reinterpret_cast<const double2*>(s + i);
          s1 = *reinterpret_cast<const double2*>(s + i + 2);
          q0 = *reinterpret_cast<const double2*>(q + i);
          q1 = *reinterpret_cast<const double2*>(q + i + 2);
        }
        const double2 t0 = *reinterpret_cast<const double2*>(ts + i), t1 = *reinterpret_cast<const double2*>(ts + i + 2);
        const double2 u0 = *reinterpret_cast<const double2*>(tq + i), u1 = *reinterpret_cast<const double2*>(tq + i + 2);
        ev_col((double)av.x, s0.x, q0.x, t0.x, u0.x, n, m, same, other);
        ev_col((double)av.y, s0.y, q0.y, t0.y, u0.y, n, m, same, other);
        ev_col((double)av.z, s1.x, q1.x, t1.x, u1.x, n, m, same, other);
        ev_col((double)av.w, s1.y, q1.y, t1.y, u1.y, n, m, same, other);
      }
    } else {
      for (long long i = lo + threadIdx.x; i < hi; i += kEvBlock)
        ev_col((double)a[i], e.own_ok ? s[i] : 0.0, e.own_ok ? q[i] : 0.0, ts[i], tq[i], n, m, same, other);
    }
  }
  same = block_sum<kEvWaves>(same, s_red);
  other = block_sum<kEvWaves>(other, s_red);
  if (threadIdx.x == 0) {
    partial_store(&part[((long long)r * split + k) * 2], same);
    partial_store(&part[((long long)r * split + k) * 2 + 1], other);
  }
  if (!arrive_last(ctr, (int)(gridDim.x * gridDim.y), &s_last)) return;
  const float nan = __int_as_float(0x7fc00000);
  for (int row = threadIdx.x; row < M; row += kEvBlock) {
    const EvRow f = ev_row(owner, cls, cnt, tcnt, O, C, row);
    double t_same = 0.0, t_other = 0.0;
    for (int i = 0; i < split; ++i) {                                // block order
      t_same += partial_load(&part[((long long)row * split + i) * 2]);
      t_other += partial_load(&part[((long long)row * split + i) * 2 + 1]);
    }
    // the reference's 0 / 0, written out: an empty cell, an empty rest of the class
    const bool has_same = f.n > 0, has_other = f.m > 0;
    const double ds = t_same / (double)f.n, dn = t_other / (double)f.m;
    out3[3 * (long long)row] = has_same ? (float)ds : nan;
    out3[3 * (long long)row + 1] = has_other ? (float)dn : nan;
    out3[3 * (long long)row + 2] = has_same && has_other ? (float)(ds / dn) : nan;
  }
}

}  // namespace ali

using namespace ali;

extern "C" int ali_group_moments(const float* rows, int64_t ld, int32_t N, int32_t D, const int32_t* order,
                                 int32_t n_order, const int32_t* start, int32_t O, int32_t C, double* S, double* Q,
                                 double* TS, double* TQ, ali_stream_t stream) {
  if (!rows || !order || !start || !S || !Q || !TS || !TQ) {
    set_error("ali_group_moments: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (N < 1 || D < 1 || ld < D || n_order < 0 || n_order > N || O < 1 || C < 1 || (long long)O * C > 65535) {
    set_error("ali_group_moments: N = %d < 1, D = %d < 1, ld = %lld < D, n_order = %d outside [0, N] or O * C = %lld "
              "outside [1, 65535]", (int)N, (int)D, (long long)ld, (int)n_order, (long long)O * C);
    return ALI_ERR_BAD_ARG;
  }
  const bool vec = D % 4 == 0 && ld % 4 == 0 && aligned16(rows) && aligned16(S) && aligned16(Q);
  const int per_block = kEvBlock * (vec ? 4 : 1);
  const dim3 grid((unsigned)((D + per_block - 1) / per_block), (unsigned)(O * C));
  const int* ord = reinterpret_cast<const int*>(order);
  const int* st = reinterpret_cast<const int*>(start);
  if (vec)
    hipLaunchKernelGGL(group_moments_kernel<4>, grid, dim3(kEvBlock), 0, ST(stream), rows, (long long)ld, (int)N,
                       (int)D, ord, (int)n_order, st, S, Q);
  else
    hipLaunchKernelGGL(group_moments_kernel<1>, grid, dim3(kEvBlock), 0, ST(stream), rows, (long long)ld, (int)N,
                       (int)D, ord, (int)n_order, st, S, Q);
  int rc = check_launch("group_moments_kernel");
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(class_totals_kernel, dim3((unsigned)((D + kEvBlock - 1) / kEvBlock), (unsigned)C), dim3(kEvBlock),
                     0, ST(stream), S, Q, (int)O, (int)C, (int)D, TS, TQ);
  return check_launch("class_totals_kernel");
}

extern "C" int ali_manifold_err(const float* cf, int64_t ld, int32_t M, int32_t D, const int32_t* owner,
                                const int32_t* cls, const double* S, const double* Q, const double* TS,
                                const double* TQ, const int32_t* cnt, const int32_t* tcnt, int32_t O, int32_t C,
                                float* out3, void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (!cf || !owner || !cls || !S || !Q || !TS || !TQ || !cnt || !tcnt || !out3) {
    set_error("ali_manifold_err: NULL argument");
    return ALI_ERR_BAD_ARG;
  }
  if (M < 1 || M > 65535 || D < 1 || ld < D || O < 1 || C < 1 || (long long)O * C > 65535) {
    set_error("ali_manifold_err: M = %d outside [1, 65535], D = %d < 1, ld = %lld < D or O * C = %lld outside "
              "[1, 65535]", (int)M, (int)D, (long long)ld, (long long)O * C);
    return ALI_ERR_BAD_ARG;
  }
  long long split = ((long long)D + kEvChunk - 1) / kEvChunk;
  if (split > kEvMaxSplit) split = kEvMaxSplit;
  const bool vec = D % 4 == 0 && ld % 4 == 0 && aligned16(cf) && aligned16(S) && aligned16(Q) && aligned16(TS) &&
                   aligned16(TQ);
  long long chunk = ((long long)D + split - 1) / split;
  if (vec) chunk = (chunk + 3) & ~3LL;                               // (a block's range starts on a 16-byte boundary)
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_manifold_err", ws, ws_bytes, (size_t)M * (size_t)split * 2, &part, &ctr);
  if (rc != ALI_OK) return rc;
  const dim3 grid((unsigned)split, (unsigned)M);
  const int* ow = reinterpret_cast<const int*>(owner);
  const int* cl = reinterpret_cast<const int*>(cls);
  const int* cn = reinterpret_cast<const int*>(cnt);
  const int* tc = reinterpret_cast<const int*>(tcnt);
  if (vec)
    hipLaunchKernelGGL(manifold_err_kernel<true>, grid, dim3(kEvBlock), 0, ST(stream), cf, (long long)ld, (int)M,
                       (int)D, chunk, ow, cl, S, Q, TS, TQ, cn, tc, (int)O, (int)C, out3, part, ctr);
  else
    hipLaunchKernelGGL(manifold_err_kernel<false>, grid, dim3(kEvBlock), 0, ST(stream), cf, (long long)ld, (int)M,
                       (int)D, chunk, ow, cl, S, Q, TS, TQ, cn, tc, (int)O, (int)C, out3, part, ctr);
  return check_launch("manifold_err_kernel");
}
