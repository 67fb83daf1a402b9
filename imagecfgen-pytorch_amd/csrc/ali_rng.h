// The counter RNG of libali_hip.so: every random number the kernels draw is a 24-bit field of splitmix64's finaliser
// over a stream key and an element index.  This is the one place that states the key schedule (ali_hip/rng.py follows
// it on the host; tests/golden/rng_streams.npz pins the bits captured graphs, checkpoints and host references rely on):
//
//   base    = mix64(mix64(seed) ^ (dev_counter ? (uint64)dev_counter[0] * kCounterMul : 0))    masks
//   latent  = mix64(base   ^ kLatentStream)      ali_normal_fill, ali_vae_latent_fwd
//   gp      = mix64(latent ^ kGpStream)          ali_gp_mix (eps)
//   gumbel  = mix64(latent ^ kGumbelStream)      ali_gumbel_posterior
//   phase   = mix64(base   ^ kPhaseStream)       ali_gl_init
//   thin    = mix64(base   ^ kThinStream)       ali_morpho_thin (the tiebreak of the thinning order; no counter)
//   eg      = mix64(base   ^ kEgStream)         ali_eg_input (background index from hi24, mixing weight t from lo24)
//   locate  = mix64(base   ^ kLocateStream)     ali_morpho_locate (candidate index from hi24 of hash row * 8 + draw)
//   hash(e) = mix64(key ^ e)
//   hi24    = bits 40..63 of a hash
//   lo24    = bits 16..39 of a hash
//
// A NULL counter and a counter holding 0 give the same key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ali {
constexpr uint64_t kCounterMul = 0xD1B54A32D192ED03ull;
constexpr uint64_t kLatentStream = 0x4C4154454E545A31ull, kGpStream = 0x47504D4958455053ull;      // "LATENTZ1", "GPMIXEPS"
constexpr uint64_t kGumbelStream = 0x47554D42454C3031ull, kPhaseStream = 0x474C504841534531ull;   // "GUMBEL01", "GLPHASE1"
constexpr uint64_t kThinStream = 0x5448494E4B455931ull;                                           // "THINKEY1"
constexpr uint64_t kEgStream = 0x4547425249445831ull;                                             // "EGBRIDX1"
constexpr uint64_t kLocateStream = 0x534B454C4C4F4331ull;                                         // "SKELLOC1"
constexpr float kInv24 = 1.f / 16777216.f;   // a 24-bit field times this is exact in fp32, in [0, 1)

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t rng_base_key(uint64_t seed, const long long* dev_counter) {
  return mix64(mix64(seed) ^ (dev_counter ? (uint64_t)dev_counter[0] * kCounterMul : 0ull));
}
__device__ __forceinline__ uint64_t sub_key(uint64_t key, uint64_t tag) { return mix64(key ^ tag); }
__device__ __forceinline__ uint64_t latent_key(uint64_t base) { return sub_key(base, kLatentStream); }
__device__ __forceinline__ uint64_t gp_key(uint64_t base) { return sub_key(latent_key(base), kGpStream); }
__device__ __forceinline__ uint64_t gumbel_key(uint64_t base) { return sub_key(latent_key(base), kGumbelStream); }
__device__ __forceinline__ uint64_t phase_key(uint64_t base) { return sub_key(base, kPhaseStream); }
__device__ __forceinline__ uint64_t thin_key(uint64_t base) { return sub_key(base, kThinStream); }
__device__ __forceinline__ uint64_t eg_key(uint64_t base) { return sub_key(base, kEgStream); }
__device__ __forceinline__ uint64_t locate_key(uint64_t base) { return sub_key(base, kLocateStream); }
__device__ __forceinline__ uint64_t hash_at(uint64_t key, uint64_t e) { return mix64(key ^ e); }
__device__ __forceinline__ uint32_t hi24(uint64_t r) { return (uint32_t)(r >> 40); }
__device__ __forceinline__ uint32_t lo24(uint64_t r) { return (uint32_t)(r >> 16) & 0xFFFFFFu; }

// The latent stream (ali_hip/rng.py: normal_reference): element g is one half of the Box-Muller pair of hash g >> 1
// (even g: cosine, odd g: sine), u1 in (0, 1] from hi24 and u2 in [0, 1) from lo24.
__device__ __forceinline__ void normal_pair(uint64_t key, uint64_t pair, float& c, float& s) {
  const uint64_t r = hash_at(key, pair);
  const float u1 = (float)(hi24(r) + 1u) * kInv24;
  const float u2 = (float)lo24(r) * kInv24;
  const float rad = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(2.f * u2, &sn, &cs);        // (the angle 2*pi*u2 without rounding 2*pi*u2 itself)
  c = rad * cs;
  s = rad * sn;
}
__device__ __forceinline__ float normal_at(uint64_t key, uint64_t g) {
  float c, s;
  normal_pair(key, g >> 1, c, s);
  return (g & 1) ? s : c;
}

}  // namespace ali
