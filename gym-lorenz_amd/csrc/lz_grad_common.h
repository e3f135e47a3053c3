// What the two gradient translation units (lz_a2c.hip, lz_ppo.hip) share besides the kernel
// body (lz_grad_body.inc): the tile constants, the layout of the flat parameter vector, the
// MFMA helpers and the grid / shape rules of the entry points.  Both files pull the names
// into their own namespace (lz::a2c, lz::ppo), where the kernels and their GradArgs stay.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lz {
namespace grad {

typedef float v16 __attribute__((ext_vector_type(16)));

constexpr int kH = 128;          // hidden units of the first form (LZ_POLICY_HIDDEN)
constexpr int kH64 = 64;         // hidden units of the _h64 form (SB3's default MlpPolicy)
constexpr int kTile = 32;        // samples per workgroup tile
constexpr int kLd = 33;          // row stride of the [unit][sample] images
constexpr int kMaxO = 8, kMaxA = 4;
constexpr int kFlushTiles = 64;  // float32 chains end after 64 * 32 samples
constexpr int kDefaultWgs = 128; // workgroups per net when the caller sets no cap
constexpr int kMaxWgs = 4096;

// offsets of the 13 tensors (gym_lorenz.policy.KEYS order, nn.Linear layout) in the flat
// parameter vector of a net with H hidden units, and its length (lz_a2c_param_count_hidden)
struct Layout {
  int64_t off[13];
  int64_t P;
};

__host__ __device__ inline Layout layout(int O, int A, int H = kH) {
  Layout L;
  const int64_t n[13] = {(int64_t)H * O, H, (int64_t)H * H, H, (int64_t)H * O, H,
                         (int64_t)H * H, H, (int64_t)A * H, A, H, 1, A};
  int64_t o = 0;
  for (int i = 0; i < 13; ++i) {
    L.off[i] = o;
    o += n[i];
  }
  L.P = o;
  return L;
}

__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

__device__ __forceinline__ v16 mfma(float a, float b, v16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void put(double* p, float v, bool first) {
  *p = first ? (double)v : *p + (double)v;
}

inline int wgs_per_net(int64_t n, int cap) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t lim = cap > 0 ? cap : kDefaultWgs;
  return (int)(tiles < lim ? tiles : lim);
}

inline bool dims_ok(int O, int A) { return O >= 1 && O <= kMaxO && A >= 1 && A <= kMaxA; }

// the hidden sizes a gradient kernel is built for
inline bool hidden_ok(int H) { return H == kH || H == kH64; }

}  // namespace grad
}  // namespace lz
