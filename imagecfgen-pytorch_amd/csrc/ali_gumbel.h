// The Gumbel-max draws and their posterior, once: ali_gumbel_posterior (flow.hip) and ali_cat_map (cat.hip) share them.
#pragma once
#include "ali_rng.h"

namespace ali {

// Gumbel(0, 1) = -log(-log u), u = (k + 0.5) / 2^24 strictly inside (0, 1): the top 24 bits of the hash of element e
__device__ __forceinline__ float gumbel_at(uint64_t key, uint64_t e) {
  const double u = ((double)hi24(hash_at(key, e)) + 0.5) * (double)kInv24;
  return (float)-log(-log(u));
}

// Posterior noise of one class of a row whose observed class is y: g, z this class's prior draw and logit; gy, zy
// those of y; ey = exp(-gy - zy); lse = log sum exp of the row's logits.  argmax(z + noise) is y.
__device__ __forceinline__ double gumbel_posterior_at(bool is_y, double g, double z, double gy, double zy, double ey,
                                                      double lse) {
  return is_y ? gy + lse - zy : -log(exp(-g - z) + ey) - z;
}

}  // namespace ali
