// The counterfactual explainers' own arithmetic (explain/cf_example.py; include/ali_hip.h: ali_row_dist, ali_cf_hinge,
// ali_cf_join, ali_cf_input_fwd, ali_cf_input_step, ali_cf_select): what sits between the generator's and the
// classifier's conv chains in one step of HingeLossCFExplainer.explain and at the tail of
// DeepCounterfactualExplainer.explain's sweep.  Every one of them is launch bound at the callers' sizes (batch 1 .. 64,
// 10-class logits, 28x28 .. 128x128 images), so the row arithmetic is fp64 -- every fp32 result is the rounding of an
// fp64 evaluation -- and every reduction runs in a fixed order (ali_reduce.h): lanes -> waves 0..3 in order -> blocks in
// block order.  No float atomics, no host reads, no allocation: the same inputs give the same bits, and every launch can
// be recorded into a HIP graph.
//
// NaN (what falls out, untested unless said otherwise):
//   ali_row_dist    a NaN element makes its row's distance NaN.
//   ali_cf_hinge    comparisons with NaN are false, so a NaN logit never becomes the maximum (max_excluding's `>` skips
//                   it as well); a NaN target logit makes h NaN.  A row whose other logits are all NaN / -inf has
//                   h = -inf - logit[t] and only the -c entry in its gradient.
//   ali_cf_join     a NaN difference gives a NaN gradient entry (torch.sign(NaN) is NaN).
//   ali_cf_select   a NaN logit never becomes the prediction (torch.argmax would pick it); NaN metrics sort behind every
//                   number among the hits, in row order among themselves -- torch.argsort's order (tested).
#include "ali_reduce.h"

#include <limits.h>
#include <string.h>

namespace ali {

constexpr int kCfBlock = 256;
constexpr int kCfWaves = kCfBlock / 64;
constexpr int kDistChunk = 4096;                                     // elements of a row one block adds up
constexpr int kDistMaxSplit = 64;
constexpr int kCfMaxCat = 1024;                                      // widest segment that goes through LDS
constexpr int kSelMax = 1024;

// ---------------------------------------------------------------------------------------------------- ali_row_dist
// grid (split, S): block (k, s) adds elements [k * chunk, (k + 1) * chunk) of row s; the block that arrives last at the
// counter adds every row's partials in block order (thread per row).
__global__ void __launch_bounds__(kCfBlock)
row_dist_kernel(const float* __restrict__ x, int xB, const float* __restrict__ y, int S, long long N, long long chunk,
                int mode, float* __restrict__ out, unsigned long long* part, int* ctr) {
  __shared__ double s_red[kCfWaves];
  __shared__ int s_last;
  const int s = blockIdx.y, k = blockIdx.x, split = gridDim.x;
  const float* xr = x + (xB == 1 ? 0 : (long long)s * N);
  const float* yr = y + (long long)s * N;
  const long long lo = (long long)k * chunk;
  long long hi = lo + chunk;
  if (hi > N) hi = N;
  double acc = 0.0;
  for (long long n = lo + threadIdx.x; n < hi; n += kCfBlock) {
    const double d = (double)yr[n] - (double)xr[n];
    acc += mode == ALI_DIST_L1 ? fabs(d) : d * d;
  }
  acc = block_sum<kCfWaves>(acc, s_red);
  if (threadIdx.x == 0) partial_store(&part[(long long)s * split + k], acc);
  if (!arrive_last(ctr, (int)(gridDim.x * gridDim.y), &s_last)) return;
  for (int r = threadIdx.x; r < S; r += kCfBlock) {
    double total = 0.0;
    for (int i = 0; i < split; ++i) total += partial_load(&part[(long long)r * split + i]);   // block order
    out[r] = (float)(total / (double)N);
  }
}

// ---------------------------------------------------------------------------------------------------- ali_cf_hinge
// One wave per row, lanes strided over the C columns.
__global__ void __launch_bounds__(kCfBlock)
cf_hinge_kernel(const float* __restrict__ logit, const int* __restrict__ target, const float* __restrict__ orig_pred,
                const float* __restrict__ m, float c, int B, int C, float* __restrict__ out3,
                float* __restrict__ glogit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kCfWaves + wave;
  if (b >= B) return;
  const float* z = logit + (long long)b * C;
  float* g = glogit ? glogit + (long long)b * C : nullptr;
  const int t = target[b];
  const double cd = (double)c, md = (double)m[b];
  double h;
  if (t >= 0) {
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int j = lane; j < C; j += 64) {             // ascending j per lane: a strict > keeps the lane's first maximum
      const float zv = z[j];
      if (j != t && zv > best) { best = zv; bi = j; }
    }
    wave_argmax(best, bi);
    const bool ok = t < C;                            // (a target past the row: h = NaN, no gradient)
    h = ok ? (double)best - (double)z[t] : (double)NAN;
    if (g)
      for (int j = lane; j < C; j += 64) g[j] = !ok ? 0.f : (j == t ? -c : (j == bi ? c : 0.f));
  } else if (orig_pred) {
    const float* o = orig_pred + (long long)b * C;
    double acc = 0.0;
    const double gs = 2.0 * cd / (double)C;
    for (int j = lane; j < C; j += 64) {
      const double d = (double)z[j] - (double)o[j];
      acc += d * d;
      if (g) g[j] = (float)(gs * d);
    }
    h = wave_sum(acc) / (double)C;
  } else {                                            // (no target and nothing to compare with)
    h = (double)NAN;
    if (g)
      for (int j = lane; j < C; j += 64) g[j] = 0.f;
  }
  if (lane == 0) {
    out3[b * 3 + 0] = (float)(cd * h + md);
    out3[b * 3 + 1] = (float)h;
    out3[b * 3 + 2] = (float)md;
  }
}

// ----------------------------------------------------------------------------------------------------- ali_cf_join
__global__ void __launch_bounds__(kCfBlock)
cf_join_kernel(const float* __restrict__ gx, int cpad, const float* __restrict__ x_cf, const float* __restrict__ x,
               int xB, long long N, long long total, float* __restrict__ gy) {
  const float r = 1.0f / (float)N;                    // IEEE division: what mean's backward hands abs's
  for (long long i = (long long)blockIdx.x * kCfBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kCfBlock) {
    const float d = x_cf[i] - x[xB == 1 ? i % N : i];
    const float sg = d > 0.f ? r : (d < 0.f ? -r : (d == 0.f ? 0.f : d));
    gy[i] = gx[i * cpad] + sg;
  }
}

// ------------------------------------------------------------------------------- ali_cf_input_fwd / ali_cf_input_step
struct CfSegs {
  AliCfSegment seg[ALI_CF_MAX_SEGMENTS];
  const float* table[ALI_CF_MAX_SEGMENTS];           // per segment; nullptr: the columns are written directly
  int n;
};

// One block per row.  A segment that needs the whole of its transformed values at once (softmax, or a table product)
// keeps them in LDS as doubles; the others stream.
__global__ void __launch_bounds__(kCfBlock)
cf_input_fwd_kernel(const float* __restrict__ raw, int raw_ld, const float* __restrict__ given, int given_ld, CfSegs sg,
                    int n_log, int ld, float* __restrict__ rows, float* __restrict__ attrs, int attrs_ld) {
  __shared__ double s_p[kCfMaxCat];
  __shared__ double s_red[kCfWaves];
  __shared__ float s_max[kCfWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* row = rows + (long long)b * ld;
  float* arow = attrs ? attrs + (long long)b * attrs_ld : nullptr;
  for (int q = 0; q < sg.n; ++q) {
    const AliCfSegment s = sg.seg[q];
    const float* tab = sg.table[q];
    const float* src = s.kind == ALI_CF_COPY ? given + (long long)b * given_ld + s.src_off
                                             : raw + (long long)b * raw_ld + s.src_off;
    if (!tab && s.kind != ALI_CF_SOFTMAX) {
      for (int i = tid; i < s.width; i += kCfBlock) {
        const float v = s.kind == ALI_CF_TANH ? (float)tanh((double)src[i]) : src[i];
        row[s.dst_off + i] = v;
        if (arow && s.attr_off >= 0) arow[s.attr_off + i] = v;
      }
      continue;
    }
    if (s.kind == ALI_CF_SOFTMAX) {
      float mx = -INFINITY;
      for (int i = tid; i < s.width; i += kCfBlock) mx = fmaxf(mx, src[i]);
      mx = block_max<kCfWaves>(mx, s_max);
      double e = 0.0;
      for (int i = tid; i < s.width; i += kCfBlock) {
        const double ev = exp((double)src[i] - (double)mx);
        s_p[i] = ev;
        e += ev;
      }
      e = block_sum<kCfWaves>(e, s_red);
      for (int i = tid; i < s.width; i += kCfBlock) s_p[i] = s_p[i] / e;     // (the thread's own entries)
    } else {
      for (int i = tid; i < s.width; i += kCfBlock)
        s_p[i] = s.kind == ALI_CF_TANH ? tanh((double)src[i]) : (double)src[i];
    }
    // the attribute row holds the fp32 values; the product below and the step's Jacobian both start from them
    for (int i = tid; i < s.width; i += kCfBlock) {
      const float pf = (float)s_p[i];
      s_p[i] = (double)pf;
      if (arow && s.attr_off >= 0) arow[s.attr_off + i] = pf;
      if (!tab) row[s.dst_off + i] = pf;
    }
    __syncthreads();
    if (tab)
      for (int j = tid; j < ALI_CF_EMB; j += kCfBlock) {
        double acc = 0.0;
        for (int k = 0; k < s.width; ++k) acc += s_p[k] * (double)tab[(long long)k * ALI_CF_EMB + j];   // ascending k
        row[s.dst_off + j] = (float)acc;
      }
    __syncthreads();
  }
  for (int i = n_log + tid; i < ld; i += kCfBlock) row[i] = 0.f;
}

// torch.optim.Adam (no weight decay, no amsgrad) on one element, step t >= 1, in fp64 from the fp32 state and the
// fp32 gradient (the value graw receives: the update is Adam's at exactly that gradient)
__device__ __forceinline__ void cf_adam(float* p, float* m, float* v, double g, double lr, double b1, double b2,
                                        double eps, double bc1, double bc2_sqrt) {
  const double mm = b1 * (double)*m + (1.0 - b1) * g;
  const double vv = b2 * (double)*v + (1.0 - b2) * g * g;
  const double denom = sqrt(vv) / bc2_sqrt + eps;
  *m = (float)mm;
  *v = (float)vv;
  *p = (float)((double)*p - (lr / bc1) * (mm / denom));
}

__global__ void __launch_bounds__(kCfBlock)
cf_input_step_kernel(const float* __restrict__ g_rows, int ld, const float* __restrict__ rows,
                     const float* __restrict__ attrs, int attrs_ld, CfSegs sg, float* __restrict__ raw,
                     float* __restrict__ m, float* __restrict__ v, int raw_ld, int* __restrict__ step, double lr,
                     double b1, double b2, double eps, float* __restrict__ graw) {
  __shared__ double s_g[kCfMaxCat];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = step[b] + 1;                          // this row's own counter: only this block touches it
  const double bc1 = 1.0 - pow(b1, (double)t), bc2_sqrt = sqrt(1.0 - pow(b2, (double)t));
  const float* grow = g_rows + (long long)b * ld;
  const float* row = rows + (long long)b * ld;
  const float* arow = attrs + (long long)b * attrs_ld;
  const long long r0 = (long long)b * raw_ld;
  for (int q = 0; q < sg.n; ++q) {
    const AliCfSegment s = sg.seg[q];
    if (s.kind == ALI_CF_COPY) continue;
    const float* tab = sg.table[q];
    const float* val = s.attr_off >= 0 ? arow + s.attr_off : row + s.dst_off;   // the transformed values
    if (!tab && s.kind == ALI_CF_TANH) {
      for (int i = tid; i < s.width; i += kCfBlock) {
        const double tv = (double)val[i];
        const double g = (double)grow[s.dst_off + i] * (1.0 - tv * tv);
        const long long at = r0 + s.src_off + i;
        if (graw) graw[at] = (float)g;
        cf_adam(raw + at, m + at, v + at, (double)(float)g, lr, b1, b2, eps, bc1, bc2_sqrt);
      }
      continue;
    }
    // gradient of the transformed values: the row's columns, or their products with the table's rows (wave per k)
    if (tab) {
      for (int k = wave; k < s.width; k += kCfWaves) {
        double acc = 0.0;
        for (int j = lane; j < ALI_CF_EMB; j += 64)
          acc += (double)grow[s.dst_off + j] * (double)tab[(long long)k * ALI_CF_EMB + j];
        acc = wave_sum(acc);
        if (lane == 0) s_g[k] = acc;
      }
    } else {
      for (int i = tid; i < s.width; i += kCfBlock) s_g[i] = (double)grow[s.dst_off + i];
    }
    __syncthreads();
    double dot = 0.0;
    if (s.kind == ALI_CF_SOFTMAX)
      for (int k = 0; k < s.width; ++k) dot += (double)val[k] * s_g[k];          // ascending k in every thread
    for (int i = tid; i < s.width; i += kCfBlock) {
      const double pv = (double)val[i];
      const double g = s.kind == ALI_CF_SOFTMAX ? pv * (s_g[i] - dot) : s_g[i] * (1.0 - pv * pv);
      const long long at = r0 + s.src_off + i;
      if (graw) graw[at] = (float)g;
      cf_adam(raw + at, m + at, v + at, (double)(float)g, lr, b1, b2, eps, bc1, bc2_sqrt);
    }
    __syncthreads();
  }
  __syncthreads();                                    // every thread has read the counter
  if (tid == 0) step[b] = t;
}

// --------------------------------------------------------------------------------------------------- ali_cf_select
// One block, one thread per row; rank by counting.
__device__ __forceinline__ bool sel_before(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return bn;                            // a number comes before a NaN
  if (!an && a != b) return a < b;
  return ia < ib;
}

__global__ void __launch_bounds__(kSelMax)
cf_select_kernel(const float* __restrict__ logit, const float* __restrict__ metric, const int* __restrict__ target,
                 int S, int C, int* __restrict__ pred, int* __restrict__ order, int* __restrict__ n_hit) {
  __shared__ float s_key[kSelMax];
  __shared__ unsigned char s_hit[kSelMax];
  const int s = threadIdx.x;
  const int tgt = target[0];
  bool hit = false;
  float key = 0.f;
  if (s < S) {
    const float* z = logit + (long long)s * C;
    float best = z[0];
    int bi = 0;
    for (int j = 1; j < C; ++j)                       // strict >: the first maximum
      if (z[j] > best || best != best) { best = z[j]; bi = j; }
    pred[s] = bi;
    hit = bi == tgt;
    key = metric[s];
    s_key[s] = key;
    s_hit[s] = hit ? 1 : 0;
  }
  __syncthreads();
  if (s >= S) return;
  int hits = 0, rank = 0;
  for (int j = 0; j < S; ++j) {
    const bool hj = s_hit[j] != 0;
    hits += hj ? 1 : 0;
    if (hit) rank += (hj && j != s && sel_before(s_key[j], j, key, s)) ? 1 : 0;
    else rank += (!hj && j < s) ? 1 : 0;
  }
  order[hit ? rank : hits + rank] = s;
  if (s == 0) n_hit[0] = hits;
}

static int fill_segs(const char* who, const AliCfSegment* segs, int n_seg, const float* const* tables, int n_tables,
                     int raw_ld, int given_ld, int ld, int attrs_ld, bool have_given, bool have_attrs, bool step,
                     CfSegs* out) {
  if (!segs || n_seg < 1 || n_seg > ALI_CF_MAX_SEGMENTS) {
    set_error("%s: n_seg = %d outside [1, %d]", who, n_seg, ALI_CF_MAX_SEGMENTS);
    return ALI_ERR_BAD_ARG;
  }
  memset(out, 0, sizeof(*out));
  out->n = n_seg;
  for (int q = 0; q < n_seg; ++q) {
    const AliCfSegment s = segs[q];
    const bool copy = s.kind == ALI_CF_COPY;
    if (s.kind != ALI_CF_COPY && s.kind != ALI_CF_TANH && s.kind != ALI_CF_SOFTMAX) {
      set_error("%s: segment %d has kind %d", who, q, (int)s.kind);
      return ALI_ERR_BAD_ARG;
    }
    if (step && copy) {                               // (nothing of it is differentiated or updated)
      out->seg[q] = s;
      continue;
    }
    const bool lds = s.table >= 0 || s.kind == ALI_CF_SOFTMAX;
    if (s.width < 1 || (lds && s.width > kCfMaxCat)) {
      set_error("%s: segment %d has width %d (softmax / table segments: at most %d)", who, q, (int)s.width, kCfMaxCat);
      return ALI_ERR_BAD_ARG;
    }
    if (s.table >= n_tables || (s.table >= 0 && (!tables || !tables[s.table]))) {
      set_error("%s: segment %d names table %d of %d", who, q, (int)s.table, n_tables);
      return ALI_ERR_BAD_ARG;
    }
    const int src_ld = copy ? given_ld : raw_ld;
    const int dst_w = s.table >= 0 ? ALI_CF_EMB : s.width;
    if (s.src_off < 0 || s.src_off + s.width > src_ld || s.dst_off < 0 || s.dst_off + dst_w > ld ||
        (s.attr_off >= 0 && s.attr_off + s.width > attrs_ld) || (copy && !have_given) ||
        (s.attr_off >= 0 && !have_attrs)) {
      set_error("%s: segment %d (kind %d, width %d, src %d, dst %d, attr %d) leaves its rows (raw %d, given %d, row %d, "
                "attrs %d)", who, q, (int)s.kind, (int)s.width, (int)s.src_off, (int)s.dst_off, (int)s.attr_off, raw_ld,
                given_ld, ld, attrs_ld);
      return ALI_ERR_BAD_ARG;
    }
    if (s.table >= 0 && s.attr_off < 0) {
      set_error("%s: segment %d goes through a table and keeps no attribute row (its values are needed again)", who, q);
      return ALI_ERR_BAD_ARG;
    }
    out->seg[q] = s;
    out->table[q] = s.table >= 0 ? tables[s.table] : nullptr;
  }
  return ALI_OK;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_row_dist(const float* x, int32_t xB, const float* y, int32_t S, int64_t N, int32_t mode, float* out,
                            void* ws, size_t ws_bytes, ali_stream_t stream) {
  if (S < 1 || S > 65535 || N < 1 || (xB != 1 && xB != S)) {
    set_error("ali_row_dist: S = %d outside [1, 65535], N = %lld < 1 or xB = %d not in {1, S}", (int)S, (long long)N,
              (int)xB);
    return ALI_ERR_BAD_ARG;
  }
  if (mode != ALI_DIST_L1 && mode != ALI_DIST_L2) {
    set_error("ali_row_dist: mode %d", (int)mode);
    return ALI_ERR_BAD_ARG;
  }
  if (!x || !y || !out) {
    set_error("ali_row_dist: x, y and out must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  long long split = (N + kDistChunk - 1) / kDistChunk;
  if (split > kDistMaxSplit) split = kDistMaxSplit;
  const long long chunk = (N + split - 1) / split;
  unsigned long long* part;
  int* ctr;
  const int rc = fold_workspace("ali_row_dist", ws, ws_bytes, (size_t)S * (size_t)split, &part, &ctr);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(row_dist_kernel, dim3((unsigned)split, (unsigned)S), dim3(kCfBlock), 0, ST(stream), x, (int)xB, y,
                     (int)S, (long long)N, chunk, (int)mode, out, part, ctr);
  return check_launch("row_dist_kernel");
}

extern "C" int ali_cf_hinge(const float* logit, const int32_t* target, const float* orig_pred, const float* m, float c,
                            int32_t B, int32_t C, float* out3, float* glogit, ali_stream_t stream) {
  if (C < 2 || C > 4096) {
    set_error("ali_cf_hinge: C = %d outside [2, 4096]", (int)C);
    return ALI_ERR_BAD_ARG;
  }
  if (B < 1 || (long long)B * C >= (1LL << 31)) {
    set_error("ali_cf_hinge: B = %d outside [1, 2^31 / C)", (int)B);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !target || !m || !out3) {
    set_error("ali_cf_hinge: logit, target, m and out3 must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(cf_hinge_kernel, dim3((B + kCfWaves - 1) / kCfWaves), dim3(kCfBlock), 0, (hipStream_t)stream, logit,
                     reinterpret_cast<const int*>(target), orig_pred, m, c, (int)B, (int)C, out3, glogit);
  return check_launch("cf_hinge_kernel");
}

extern "C" int ali_cf_join(const float* gx_clf, int32_t cpad, const float* x_cf, const float* x, int32_t xB, int32_t B,
                           int64_t N, float* gy, ali_stream_t stream) {
  if (B < 1 || N < 1 || N >= (1LL << 24) || cpad < 1 || (xB != 1 && xB != B) || (long long)B * N * cpad >= (1LL << 40)) {
    set_error("ali_cf_join: B = %d, N = %lld (needs 1 <= N < 2^24), cpad = %d, xB = %d (needs 1 or B)", (int)B,
              (long long)N, (int)cpad, (int)xB);
    return ALI_ERR_BAD_ARG;
  }
  if (!gx_clf || !x_cf || !x || !gy) {
    set_error("ali_cf_join: gx_clf, x_cf, x and gy must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  const long long total = (long long)B * N;
  long long blocks = (total + kCfBlock - 1) / kCfBlock;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cf_join_kernel, dim3((unsigned)blocks), dim3(kCfBlock), 0, (hipStream_t)stream, gx_clf, (int)cpad,
                     x_cf, x, (int)xB, (long long)N, total, gy);
  return check_launch("cf_join_kernel");
}

extern "C" int ali_cf_input_fwd(const float* raw, int32_t raw_ld, const float* given, int32_t given_ld,
                                const AliCfSegment* segs, int32_t n_seg, const float* const* tables, int32_t n_tables,
                                int32_t B, int32_t n_log, int32_t ld, float* rows, float* attrs_out, int32_t attrs_ld,
                                ali_stream_t stream) {
  if (B < 1 || n_log < 1 || ld < n_log || !rows || raw_ld < 0 || given_ld < 0 || attrs_ld < 0 || (raw_ld > 0 && !raw)) {
    set_error("ali_cf_input_fwd: B = %d, n_log = %d, ld = %d, raw_ld = %d, given_ld = %d or a NULL buffer", (int)B,
              (int)n_log, (int)ld, (int)raw_ld, (int)given_ld);
    return ALI_ERR_BAD_ARG;
  }
  CfSegs sg;
  const int rc = fill_segs("ali_cf_input_fwd", segs, n_seg, tables, n_tables, raw_ld, given_ld, ld, attrs_ld,
                           given != nullptr, attrs_out != nullptr, false, &sg);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(cf_input_fwd_kernel, dim3(B), dim3(kCfBlock), 0, (hipStream_t)stream, raw, (int)raw_ld, given,
                     (int)given_ld, sg, (int)n_log, (int)ld, rows, attrs_out, (int)attrs_ld);
  return check_launch("cf_input_fwd_kernel");
}

extern "C" int ali_cf_input_step(const float* g_rows, int32_t ld, const float* rows, const float* attrs,
                                 int32_t attrs_ld, const AliCfSegment* segs, int32_t n_seg, const float* const* tables,
                                 int32_t n_tables, int32_t B, float* raw, float* m, float* v, int32_t raw_ld,
                                 int32_t given_ld, int32_t* step, double lr, double beta1, double beta2, double eps,
                                 float* graw, ali_stream_t stream) {
  if (B < 1 || ld < 1 || raw_ld < 1 || given_ld < 0 || attrs_ld < 0 || !g_rows || !rows || !raw || !m || !v || !step ||
      (attrs_ld > 0 && !attrs)) {
    set_error("ali_cf_input_step: B = %d, ld = %d, raw_ld = %d or a NULL buffer", (int)B, (int)ld, (int)raw_ld);
    return ALI_ERR_BAD_ARG;
  }
  CfSegs sg;
  const int rc = fill_segs("ali_cf_input_step", segs, n_seg, tables, n_tables, raw_ld, given_ld, ld, attrs_ld, false,
                           attrs != nullptr, true, &sg);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(cf_input_step_kernel, dim3(B), dim3(kCfBlock), 0, (hipStream_t)stream, g_rows, (int)ld, rows, attrs,
                     (int)attrs_ld, sg, raw, m, v, (int)raw_ld, reinterpret_cast<int*>(step), lr, beta1, beta2, eps,
                     graw);
  return check_launch("cf_input_step_kernel");
}

extern "C" int ali_cf_select(const float* logit, const float* metric, const int32_t* target, int32_t S, int32_t C,
                             int32_t* pred, int32_t* order, int32_t* n_hit, ali_stream_t stream) {
  if (S < 1 || S > kSelMax) {
    set_error("ali_cf_select: S = %d outside [1, %d]", (int)S, kSelMax);
    return ALI_ERR_BAD_ARG;
  }
  if (C < 1 || C > 4096) {
    set_error("ali_cf_select: C = %d outside [1, 4096]", (int)C);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !metric || !target || !pred || !order || !n_hit) {
    set_error("ali_cf_select: no argument may be NULL");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(cf_select_kernel, dim3(1), dim3((S + 63) / 64 * 64), 0, (hipStream_t)stream, logit, metric,
                     reinterpret_cast<const int*>(target), (int)S, (int)C, reinterpret_cast<int*>(pred),
                     reinterpret_cast<int*>(order), reinterpret_cast<int*>(n_hit));
  return check_launch("cf_select_kernel");
}
