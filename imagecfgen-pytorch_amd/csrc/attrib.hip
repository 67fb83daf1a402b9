// Expected-gradients attributions (morphomnist_attribute_shap.py; include/ali_hip.h: ali_eg_input, ali_eg_seed,
// ali_eg_reduce): what sits around the generator's and the classifier's conv chains when shap.GradientExplainer
// explains f(a) = mean_z softmax(clf(decoder(z, a))).  The chains carry all the arithmetic that matters; these three are
// bound by their memory traffic (ali_eg_input writes, ali_eg_reduce reads one generator-input row per sample) or by the
// launch (ali_eg_seed), so the row arithmetic is fp64 -- every fp32 result is the rounding of an fp64 evaluation -- and
// every sum runs in a fixed order (ali_reduce.h).  No float atomics, no host reads, no allocation: the same inputs give
// the same bits, and every launch can be recorded into a HIP graph.
//
// NaN (what falls out, untested): a NaN attribute, logit or gradient makes what is computed from it NaN; nothing
// branches on a value except the clamp of a given background index into [0, Nb).
#include "ali_reduce.h"
#include "ali_rng.h"

#include <string.h>

namespace ali {

constexpr int kEgBlock = 256;
constexpr int kEgWaves = kEgBlock / 64;
constexpr int kEgMaxA = 1024;                                        // attribute columns ali_eg_input mixes in LDS
constexpr int kEgRedMaxA = 256;                                      // attribute columns ali_eg_reduce accumulates in LDS
constexpr int kEgChunk = 64;                                         // (k, s) rows of one explained row per block

struct EgSegs {
  AliCfSegment seg[ALI_CF_MAX_SEGMENTS];
  const float* table[ALI_CF_MAX_SEGMENTS];                           // per segment; nullptr: the columns are copied
  int n;
};

// ---------------------------------------------------------------------------------------------------- ali_eg_input
// grid R * S: block (r, k) mixes the attribute row once and writes its n_draws generator-input rows.
__global__ void __launch_bounds__(kEgBlock)
eg_input_kernel(const float* __restrict__ x, const float* __restrict__ bg, const int* __restrict__ idx,
                const float* __restrict__ t, const float* __restrict__ z, unsigned long long seed,
                const long long* dev_counter, unsigned long long offset, EgSegs sg, int S, int n_draws, int Nb, int A,
                int latent, int n_log, int ld, float* __restrict__ rows, float* __restrict__ delta,
                int* __restrict__ idx_out, float* __restrict__ t_out) {
  __shared__ float s_a[kEgMaxA];
  const int tid = threadIdx.x;
  const long long rk = blockIdx.x;                                   // r * S + k
  const long long r = rk / S;
  const uint64_t base = rng_base_key(seed, dev_counter);
  const uint64_t e = (uint64_t)offset * (uint64_t)S + (uint64_t)rk;  // (offset + r) * S + k
  const uint64_t h = hash_at(eg_key(base), e);
  int bi = idx ? idx[rk] : (int)(((uint64_t)hi24(h) * (uint64_t)Nb) >> 24);
  bi = bi < 0 ? 0 : (bi >= Nb ? Nb - 1 : bi);
  const float tv = t ? t[rk] : (float)lo24(h) * kInv24;
  if (tid == 0) {
    if (idx_out) idx_out[rk] = bi;
    if (t_out) t_out[rk] = tv;
  }
  const float* xr = x + r * A;
  const float* br = bg + (long long)bi * A;
  const double td = (double)tv;
  for (int i = tid; i < A; i += kEgBlock) {
    const float xv = xr[i], bv = br[i];
    const float mixed = (float)(td * (double)xv + (1.0 - td) * (double)bv);
    s_a[i] = tv == 0.f ? bv : (tv == 1.f ? xv : mixed);             // (the ends bit for bit, a -0 included)
    delta[rk * A + i] = xv - bv;
  }
  __syncthreads();
  float* row0 = rows + rk * n_draws * ld;
  // z: given, or element (row * latent + l) of the latent stream, row counted over the whole call
  const uint64_t zkey = latent_key(base);
  for (int i = tid; i < n_draws * latent; i += kEgBlock) {
    const int s = i / latent, l = i - s * latent;
    const uint64_t grow = e * (uint64_t)n_draws + (uint64_t)s;
    row0[(long long)s * ld + l] = z ? z[(rk * n_draws + s) * latent + l]
                                    : normal_at(zkey, grow * (uint64_t)latent + (uint64_t)l);
  }
  for (int q = 0; q < sg.n; ++q) {
    const AliCfSegment sq = sg.seg[q];
    const float* tab = sg.table[q];
    const int dst_w = tab ? ALI_CF_EMB : sq.width;
    for (int j = tid; j < dst_w; j += kEgBlock) {
      float v;
      if (tab) {
        double acc = 0.0;
        for (int k = 0; k < sq.width; ++k)                           // ascending k
          acc += (double)s_a[sq.src_off + k] * (double)tab[(long long)k * ALI_CF_EMB + j];
        v = (float)acc;
      } else {
        v = s_a[sq.src_off + j];
      }
      for (int s = 0; s < n_draws; ++s) row0[(long long)s * ld + sq.dst_off + j] = v;
    }
  }
  const int pad = ld - n_log;
  for (int i = tid; i < n_draws * pad; i += kEgBlock) {
    const int s = i / pad, l = i - s * pad;
    row0[(long long)s * ld + n_log + l] = 0.f;
  }
}

// ----------------------------------------------------------------------------------------------------- ali_eg_seed
// One thread per row.  At the callers' K = 10 a wave per row would leave 54 lanes idle and spend twelve butterfly steps
// on the maximum and the sum; a thread per row needs no cross-lane step, and the 64 rows of a wave are one contiguous
// 64 * K * 4 byte range, every byte of which is used.  The row is read three times (maximum, sum, values): the second and
// third read hit L1.
__global__ void __launch_bounds__(kEgBlock)
eg_seed_kernel(const float* __restrict__ logit, long long N, int K, int c, double scale, float* __restrict__ glogit,
               float* __restrict__ p_out) {
  const long long n = (long long)blockIdx.x * kEgBlock + threadIdx.x;
  if (n >= N) return;
  const float* zr = logit + n * K;
  float mx = zr[0];
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, zr[k]);
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += exp((double)zr[k] - (double)mx);           // ascending k
  const double pc = exp((double)zr[c] - (double)mx) / sum;
  for (int k = 0; k < K; ++k) {
    const double pk = exp((double)zr[k] - (double)mx) / sum;
    glogit[n * K + k] = (float)(scale * pc * ((k == c ? 1.0 : 0.0) - pk));
    if (p_out) p_out[n * K + k] = (float)pk;
  }
}

// --------------------------------------------------------------------------------------------------- ali_eg_reduce
// grid (split, R): block (p, r) takes the (k, s) rows [p * kEgChunk, (p + 1) * kEgChunk) of explained row r, wave w the
// rows w, w + 4, ... of them in ascending order; lane 0 of the wave adds delta * gradient per attribute column into the
// wave's LDS row.  Waves 0..3 in order give the block's partial; the block that arrives last adds every row's partials
// in block order (thread per (r, column)).  `split` depends on S * n_draws alone, so a row's bits do not depend on R.
__global__ void __launch_bounds__(kEgBlock)
eg_reduce_kernel(const float* __restrict__ g_rows, int ld, const float* __restrict__ delta, EgSegs sg, int R, int S,
                 int n_draws, int A, int C, int c, float* __restrict__ phi, unsigned long long* part, int* ctr) {
  __shared__ double s_acc[kEgWaves][kEgRedMaxA];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = blockIdx.x, split = gridDim.x;
  const long long r = blockIdx.y;
  const int per_row = S * n_draws;
  for (int i = tid; i < kEgWaves * kEgRedMaxA; i += kEgBlock) (&s_acc[0][0])[i] = 0.0;
  __syncthreads();
  int hi = (p + 1) * kEgChunk;
  if (hi > per_row) hi = per_row;
  for (int i = p * kEgChunk + wave; i < hi; i += kEgWaves) {
    const float* grow = g_rows + (r * per_row + i) * ld;
    const float* drow = delta + (r * S + i / n_draws) * A;
    for (int q = 0; q < sg.n; ++q) {
      const AliCfSegment sq = sg.seg[q];
      const float* tab = sg.table[q];
      if (!tab) {
        if (lane == 0)
          for (int j = 0; j < sq.width; ++j)
            s_acc[wave][sq.src_off + j] += (double)drow[sq.src_off + j] * (double)grow[sq.dst_off + j];
        continue;
      }
      float gv[ALI_CF_EMB / 64];
#pragma unroll
      for (int u = 0; u < ALI_CF_EMB / 64; ++u) gv[u] = grow[sq.dst_off + u * 64 + lane];
      for (int j = 0; j < sq.width; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < ALI_CF_EMB / 64; ++u)
          acc += (double)gv[u] * (double)tab[(long long)j * ALI_CF_EMB + u * 64 + lane];
        acc = wave_sum(acc);
        if (lane == 0) s_acc[wave][sq.src_off + j] += (double)drow[sq.src_off + j] * acc;
      }
    }
  }
  __syncthreads();
  if (tid == 0)
    for (int j = 0; j < A; ++j) {
      double total = 0.0;
      for (int w = 0; w < kEgWaves; ++w) total += s_acc[w][j];                   // waves in order
      partial_store(&part[(r * split + p) * A + j], total);
    }
  if (!arrive_last(ctr, (int)(gridDim.x * gridDim.y), &s_last)) return;
  for (long long o = tid; o < (long long)R * A; o += kEgBlock) {
    const long long rr = o / A;
    const int j = (int)(o - rr * A);
    double total = 0.0;
    for (int i = 0; i < split; ++i) total += partial_load(&part[(rr * split + i) * A + j]);   // block order
    phi[(rr * C + c) * A + j] = (float)total;
  }
}

// The segments of `who` as the kernels take them, or its error: ALI_CF_COPY entries whose attribute columns lie in
// [0, A) (at most max_width per table segment), whose row columns lie in [latent, n_log) and, when `fill`, add up to it.
static int eg_segments(const char* who, const AliCfSegment* segs, int n_seg, const float* const* tables, int n_tables,
                       int A, int latent, int n_log, bool fill, EgSegs* out) {
  if (!segs || n_seg < 1 || n_seg > ALI_CF_MAX_SEGMENTS) {
    set_error("%s: n_seg = %d outside [1, %d]", who, n_seg, ALI_CF_MAX_SEGMENTS);
    return ALI_ERR_BAD_ARG;
  }
  memset(out, 0, sizeof(*out));
  out->n = n_seg;
  long long covered = 0;
  for (int q = 0; q < n_seg; ++q) {
    const AliCfSegment s = segs[q];
    if (s.kind != ALI_CF_COPY) {
      set_error("%s: segment %d has kind %d (the attributes are given: ALI_CF_COPY)", who, q, (int)s.kind);
      return ALI_ERR_BAD_ARG;
    }
    if (s.table >= n_tables || (s.table >= 0 && (!tables || !tables[s.table]))) {
      set_error("%s: segment %d names table %d of %d", who, q, (int)s.table, n_tables);
      return ALI_ERR_BAD_ARG;
    }
    const int dst_w = s.table >= 0 ? ALI_CF_EMB : s.width;
    if (s.width < 1 || s.src_off < 0 || (long long)s.src_off + s.width > A || s.dst_off < latent ||
        (long long)s.dst_off + dst_w > n_log) {
      set_error("%s: segment %d (width %d, src %d, dst %d) leaves the attribute row (%d columns) or the input row's "
                "columns [%d, %d)", who, q, (int)s.width, (int)s.src_off, (int)s.dst_off, A, latent, n_log);
      return ALI_ERR_BAD_ARG;
    }
    covered += dst_w;
    out->seg[q] = s;
    out->table[q] = s.table >= 0 ? tables[s.table] : nullptr;
  }
  if (fill && covered != (long long)n_log - latent) {
    set_error("%s: the segments write %lld of the input row's %d attribute columns", who, covered, n_log - latent);
    return ALI_ERR_BAD_ARG;
  }
  return ALI_OK;
}

}  // namespace ali

using namespace ali;

extern "C" int ali_eg_input(const float* x, const float* bg, const int32_t* idx, const float* t, const float* z,
                            uint64_t seed, const int64_t* dev_counter, uint64_t offset, const AliCfSegment* segs,
                            int32_t n_seg, const float* const* tables, int32_t n_tables, int32_t R, int32_t S,
                            int32_t n_draws, int32_t Nb, int32_t A, int32_t latent, int32_t n_log, int32_t ld,
                            float* rows, float* delta, int32_t* idx_out, float* t_out, ali_stream_t stream) {
  if (R < 1 || S < 1 || n_draws < 1 || Nb < 1 || A < 1 || A > kEgMaxA || latent < 0 || n_log <= latent || ld < n_log ||
      (long long)R * S >= (1LL << 31) || (long long)n_draws * ld >= (1LL << 31)) {
    set_error("ali_eg_input: R = %d, S = %d, n_draws = %d, Nb = %d, A = %d (at most %d), latent = %d, n_log = %d, "
              "ld = %d", (int)R, (int)S, (int)n_draws, (int)Nb, (int)A, kEgMaxA, (int)latent, (int)n_log, (int)ld);
    return ALI_ERR_BAD_ARG;
  }
  if (!x || !bg || !rows || !delta) {
    set_error("ali_eg_input: x, bg, rows and delta must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  EgSegs sg;
  const int rc = eg_segments("ali_eg_input", segs, n_seg, tables, n_tables, A, latent, n_log, true, &sg);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(eg_input_kernel, dim3((unsigned)((long long)R * S)), dim3(kEgBlock), 0, ST(stream), x, bg,
                     reinterpret_cast<const int*>(idx), t, z, (unsigned long long)seed,
                     reinterpret_cast<const long long*>(dev_counter), (unsigned long long)offset, sg, (int)S,
                     (int)n_draws, (int)Nb, (int)A, (int)latent, (int)n_log, (int)ld, rows, delta,
                     reinterpret_cast<int*>(idx_out), t_out);
  return check_launch("eg_input_kernel");
}

extern "C" int ali_eg_seed(const float* logit, int64_t N, int32_t K, int32_t c, double scale, float* glogit,
                           float* p_out, ali_stream_t stream) {
  if (N < 1 || K < 1 || K > 1024 || c < 0 || c >= K || (N + kEgBlock - 1) / kEgBlock >= (1LL << 31)) {
    set_error("ali_eg_seed: N = %lld, K = %d outside [1, 1024] or c = %d outside [0, K)", (long long)N, (int)K, (int)c);
    return ALI_ERR_BAD_ARG;
  }
  if (!logit || !glogit) {
    set_error("ali_eg_seed: logit and glogit must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(eg_seed_kernel, dim3((unsigned)((N + kEgBlock - 1) / kEgBlock)), dim3(kEgBlock), 0, ST(stream),
                     logit, (long long)N, (int)K, (int)c, scale, glogit, p_out);
  return check_launch("eg_seed_kernel");
}

extern "C" int ali_eg_reduce(const float* g_rows, int32_t ld, const float* delta, const AliCfSegment* segs,
                             int32_t n_seg, const float* const* tables, int32_t n_tables, int32_t R, int32_t S,
                             int32_t n_draws, int32_t A, int32_t C, int32_t c, float* phi, void* ws, size_t ws_bytes,
                             ali_stream_t stream) {
  if (R < 1 || R > 65535 || S < 1 || n_draws < 1 || (long long)S * n_draws >= (1LL << 24) || A < 1 || A > kEgRedMaxA ||
      C < 1 || c < 0 || c >= C || ld < 1) {
    set_error("ali_eg_reduce: R = %d outside [1, 65535], S = %d, n_draws = %d, A = %d (at most %d), C = %d, c = %d or "
              "ld = %d", (int)R, (int)S, (int)n_draws, (int)A, kEgRedMaxA, (int)C, (int)c, (int)ld);
    return ALI_ERR_BAD_ARG;
  }
  if (!g_rows || !delta || !phi) {
    set_error("ali_eg_reduce: g_rows, delta and phi must not be NULL");
    return ALI_ERR_BAD_ARG;
  }
  EgSegs sg;
  int rc = eg_segments("ali_eg_reduce", segs, n_seg, tables, n_tables, A, 0, ld, false, &sg);
  if (rc != ALI_OK) return rc;
  const int split = (S * n_draws + kEgChunk - 1) / kEgChunk;
  unsigned long long* part;
  int* ctr;
  rc = fold_workspace("ali_eg_reduce", ws, ws_bytes, (size_t)R * (size_t)split * (size_t)A, &part, &ctr);
  if (rc != ALI_OK) return rc;
  hipLaunchKernelGGL(eg_reduce_kernel, dim3((unsigned)split, (unsigned)R), dim3(kEgBlock), 0, ST(stream), g_rows,
                     (int)ld, delta, sg, (int)R, (int)S, (int)n_draws, (int)A, (int)C, (int)c, phi, part, ctr);
  return check_launch("eg_reduce_kernel");
}
