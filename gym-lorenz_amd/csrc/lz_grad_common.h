// What the two gradient translation units (lz_a2c.hip, lz_ppo.hip) share besides the kernel
// body (lz_grad_body.inc): the tile constants, the layout of the flat parameter vector, the
// MFMA helpers and, for the host, the table row of a built kernel form (Form), the rule of
// an exported gradient entry point (Rule) with its size functions and refusals, and the two
// helpers every entry point of the two files ends in (fail, launched).  Both files pull the
// names into their own namespace (lz::a2c, lz::ppo), where the kernels, their GradArgs, the
// form table and the rules stay.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "lz_internal.h"

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

// "<who>: <what>" as the library's last error; returns s
__attribute__((format(printf, 3, 4))) inline lz_status fail(lz_status s, const char* who,
                                                            const char* what, ...) {
  char w[128], m[192];
  va_list ap;
  va_start(ap, what);
  vsnprintf(w, sizeof w, what, ap);
  va_end(ap);
  snprintf(m, sizeof m, "%s: %s", who, w);
  return lz::set_error(s, m);
}

// what an entry point returns after its launches
inline lz_status launched() {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lz::set_error(LZ_ERR_HIP, hipGetErrorString(e)) : LZ_OK;
}

// One built instantiation of lz_grad_body.inc (Args: the file's GradArgs), a row of the file's
// kForms; a launch takes the first row with hidden == H and O <= max_obs.
template <class Args>
struct Form {
  int hidden, max_obs;  // LZ_GRAD_H, LZ_GRAD_MAXO
  int threads;          // 2 * hidden
  void (*kernel)(Args);
};

template <class Args, int N>
const Form<Args>* pick_form(const Form<Args> (&forms)[N], int H, int O) {
  for (const Form<Args>& f : forms)
    if (f.hidden == H && O <= f.max_obs) return &f;
  return nullptr;
}

// the fields every GradArgs has, from a lz_a2c_grad_args or lz_ppo_grad_args
template <class Args, class Api>
void common_args(Args& a, const Api& g) {
  a.params = g.params;
  a.obs = g.observations;
  a.act = g.actions;
  a.adv = g.advantages;
  a.ret = g.returns;
  a.n = g.n_samples;
  a.O = g.obs_dim;
  a.A = g.act_dim;
  a.vf_coef = (float)g.vf_coef;
  a.ent_coef = (float)g.ent_coef;
  a.part = static_cast<double*>(g.workspace);
}

// One exported gradient entry point: what it accepts and how its refusals name it.  The
// refusals' order is the same for all of them: NULL args, NULL buffer, [PPO: old_values],
// check_shape, [PPO: n_rows, indices, clip ranges], check_launch, hipSetDevice.
struct Rule {
  const char* who;      // the entry point
  const char* ws_name;  // its workspace function, as the refusal names it
  int max_obs;          // obs_dim 1..max_obs
  int h_lo, h_hi;       // the hidden sizes it takes (one size: both the same)
  bool dims_ok(int O, int A) const { return O >= 1 && O <= max_obs && A >= 1 && A <= kMaxA; }
  bool hidden_ok(int H) const { return H == h_lo || H == h_hi; }
};

// length of the flat parameter vector, -1 where the rule refuses
inline int64_t param_count(const Rule& r, int O, int A, int H) {
  return r.dims_ok(O, A) && r.hidden_ok(H) ? layout(O, A, H).P : -1;
}

// bytes of the per-workgroup float64 slots ([workgroups per net][P + tail]), -1 where the
// rule or the grid refuses
inline int64_t workspace_bytes(const Rule& r, int64_t n, int O, int A, int H, int cap, int tail) {
  if (!r.dims_ok(O, A) || !r.hidden_ok(H) || n < 1 || cap < 0 || cap > kMaxWgs) return -1;
  return (int64_t)wgs_per_net(n, cap) * (layout(O, A, H).P + tail) * (int64_t)sizeof(double);
}

inline lz_status check_shape(const Rule& r, int O, int A, int64_t n) {
  if (!r.dims_ok(O, A))
    return fail(LZ_ERR_INVALID, r.who, "obs_dim must be 1..%d and act_dim 1..%d", r.max_obs, kMaxA);
  if (n < 1) return fail(LZ_ERR_INVALID, r.who, "n_samples < 1");
  return LZ_OK;
}

// after check_shape: the grid cap, the hidden size, the caller's workspace (`have` bytes)
inline lz_status check_launch(const Rule& r, int64_t n, int O, int A, int H, int cap, int tail,
                              int64_t have) {
  if (cap < 0 || cap > kMaxWgs)
    return fail(LZ_ERR_INVALID, r.who, "max_workgroups must be 0..%d", kMaxWgs);
  if (!r.hidden_ok(H)) {
    char more[16] = "";
    if (r.h_hi != r.h_lo) snprintf(more, sizeof more, " or %d", r.h_hi);
    return fail(LZ_ERR_UNSUPPORTED, r.who, "hidden must be %d%s", r.h_lo, more);
  }
  if (have < workspace_bytes(r, n, O, A, H, cap, tail))
    return fail(LZ_ERR_INVALID, r.who, "workspace smaller than %s", r.ws_name);
  return LZ_OK;
}

}  // namespace grad
}  // namespace lz
