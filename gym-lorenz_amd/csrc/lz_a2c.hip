// One A2C gradient step for the float32 MlpPolicy on a rollout batch that is already on
// the device: lz_a2c_grad_f32 (forward + backward of the two obs -> 128 -> 128 Tanh nets,
// per-workgroup partial sums, a fixed-order float64 reduction) and lz_a2c_apply_f32
// (clip_grad_norm_ + RMSpropTFLike).  Restates SB3 2.7.1 A2C.train()
// (stable_baselines3/a2c/a2c.py:134-190: evaluate_actions, policy_loss = -(adv * log_prob)
// .mean(), value_loss = F.mse_loss(returns, values), entropy_loss = -mean(entropy),
// clip_grad_norm_(max_grad_norm), optimizer.step()), DiagGaussianDistribution.log_prob /
// entropy (common/distributions.py) and RMSpropTFLike (common/sb2_compat/
// rmsprop_tf_like.py: square_avg starts at ones, eps inside the root) as the reference's
// learner uses them (code/lorenz_pmsm/train.py:151-185).
//
// k_a2c_grad is lz_grad_body.inc with LZ_GRAD_PPO 0 (the dataflow is described there; the
// same text with LZ_GRAD_PPO 1 is lz_ppo.hip's k_ppo_grad).  k_a2c_grad_h64 is the same text
// with LZ_GRAD_H 64, the obs -> 64 -> 64 net of SB3's default MlpPolicy: what
// code/lorenz_pmsm/train.py:130-139 trains (its policy_kwargs are commented out) and half of
// code/lorenz_pmsm/optimize.py:38-42's trials (net_dim in {64, 128}); lz_a2c_grad_hidden_f32
// launches either form.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "lz_grad_common.h"
#include "lz_internal.h"

namespace lz {
namespace a2c {

using namespace grad;

constexpr int kTail = 4;      // loss sums and the count after the P gradient sums
constexpr int kLaneSums = 2;  // policy / value loss sum, entropy sum

struct GradArgs {
  const float* params;
  const float* obs;
  const float* act;
  const float* adv;
  const float* ret;
  int64_t n;
  int O, A;
  float vf_coef, ent_coef;
  double* part;  // [workgroups per net][P + 4]
};

#define LZ_GRAD_PPO 0
#define LZ_GRAD_H 128
#define LZ_GRAD_KERNEL k_a2c_grad
#include "lz_grad_body.inc"
#undef LZ_GRAD_KERNEL
#undef LZ_GRAD_H
// the same text for SB3's default 64 x 64 net: 2 waves, 128 threads (lz_a2c_grad_hidden_f32)
#define LZ_GRAD_H 64
#define LZ_GRAD_KERNEL k_a2c_grad_h64
#include "lz_grad_body.inc"
#undef LZ_GRAD_KERNEL
#undef LZ_GRAD_H
#undef LZ_GRAD_PPO

// out[i] = the slots' entries i added in slot order
__global__ __launch_bounds__(256) void k_a2c_reduce(const double* __restrict__ part, int nwg,
                                                    int64_t len, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s += part[(int64_t)g * len + i];
  out[i] = s;
}

struct ApplyArgs {
  const double* sums;
  float* params;
  float* sq;
  int64_t P;
  double lr, max_norm, alpha, eps, vf_coef, ent_coef;
  double* stats;
};

// one workgroup: the mean gradient rounded to float32 (what torch's .grad holds), its
// global norm (float64, a fixed tree), the clip coefficient, the RMSpropTFLike step
__global__ __launch_bounds__(1024) void k_a2c_apply(ApplyArgs a) {
  __shared__ double sN[1024];
  const int tid = (int)threadIdx.x;
  const double cnt = a.sums[a.P + 3];
  double loc = 0.0;
  for (int64_t i = tid; i < a.P; i += 1024) {
    const double g = (double)(float)(a.sums[i] / cnt);
    loc += g * g;
  }
  sN[tid] = loc;
  __syncthreads();
  for (int m = 512; m > 0; m >>= 1) {
    if (tid < m) sN[tid] += sN[tid + m];
    __syncthreads();
  }
  const double total = sqrt(sN[0]);
  const double c0 = a.max_norm / (total + 1e-6);
  const double coef = c0 > 1.0 ? 1.0 : c0;  // NaN stays NaN, as torch.clamp(max=1.0) keeps it
  for (int64_t i = tid; i < a.P; i += 1024) {
    const double g = (double)(float)(a.sums[i] / cnt) * coef;
    const double s = a.alpha * (double)a.sq[i] + (1.0 - a.alpha) * (g * g);
    const double p = (double)a.params[i] - a.lr * g / sqrt(s + a.eps);
    a.sq[i] = (float)s;
    a.params[i] = (float)p;
  }
  if (tid == 0) {
    const double pl = a.sums[a.P + 0] / cnt, vl = a.sums[a.P + 1] / cnt, el = a.sums[a.P + 2] / cnt;
    a.stats[0] = pl;
    a.stats[1] = vl;
    a.stats[2] = el;
    a.stats[3] = (pl + a.ent_coef * el) + a.vf_coef * vl;
    a.stats[4] = total;
    a.stats[5] = coef;
    a.stats[6] = cnt;
    a.stats[7] = a.lr;
  }
}

}  // namespace a2c
}  // namespace lz

extern "C" int64_t lz_a2c_param_count(int32_t obs_dim, int32_t act_dim) {
  if (!lz::a2c::dims_ok(obs_dim, act_dim)) return -1;
  return lz::a2c::layout(obs_dim, act_dim).P;
}

extern "C" int64_t lz_a2c_workspace_bytes(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                          int32_t max_workgroups) {
  if (!lz::a2c::dims_ok(obs_dim, act_dim) || n_samples < 1 || max_workgroups < 0 ||
      max_workgroups > lz::a2c::kMaxWgs)
    return -1;
  const int64_t P = lz::a2c::layout(obs_dim, act_dim).P;
  return (int64_t)lz::a2c::wgs_per_net(n_samples, max_workgroups) * (P + 4) * (int64_t)sizeof(double);
}

extern "C" int64_t lz_a2c_param_count_hidden(int32_t obs_dim, int32_t act_dim, int32_t hidden) {
  if (!lz::a2c::dims_ok(obs_dim, act_dim) || !lz::a2c::hidden_ok(hidden)) return -1;
  return lz::a2c::layout(obs_dim, act_dim, hidden).P;
}

extern "C" int64_t lz_a2c_workspace_bytes_hidden(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                                 int32_t hidden, int32_t max_workgroups) {
  using namespace lz::a2c;
  if (!dims_ok(obs_dim, act_dim) || !hidden_ok(hidden) || n_samples < 1 || max_workgroups < 0 ||
      max_workgroups > kMaxWgs)
    return -1;
  const int64_t P = layout(obs_dim, act_dim, hidden).P;
  return (int64_t)wgs_per_net(n_samples, max_workgroups) * (P + kTail) * (int64_t)sizeof(double);
}

namespace {

lz_status fail(lz_status s, const char* who, const char* what) {
  char m[160];
  snprintf(m, sizeof m, "%s: %s", who, what);
  return lz::set_error(s, m);
}

// lz_a2c_grad_f32 (any_hidden false: 128 units only) and lz_a2c_grad_hidden_f32: the same
// refusals in the same order, then the launch of the form built for g->hidden
lz_status grad_entry(const lz_a2c_grad_args* g, int32_t device, void* stream, const char* who,
                     bool any_hidden) {
  using namespace lz::a2c;
  if (!g) return fail(LZ_ERR_INVALID, who, "NULL args");
  if (!g->params || !g->observations || !g->actions || !g->advantages || !g->returns ||
      !g->workspace || !g->grad_sums)
    return fail(LZ_ERR_INVALID, who, "NULL buffer");
  if (!dims_ok(g->obs_dim, g->act_dim))
    return fail(LZ_ERR_INVALID, who, "obs_dim must be 1..8 and act_dim 1..4");
  if (g->n_samples < 1) return fail(LZ_ERR_INVALID, who, "n_samples < 1");
  if (g->max_workgroups < 0 || g->max_workgroups > kMaxWgs)
    return fail(LZ_ERR_INVALID, who, "max_workgroups must be 0..4096");
  if (any_hidden ? !hidden_ok(g->hidden) : g->hidden != kH)
    return fail(LZ_ERR_UNSUPPORTED, who, any_hidden ? "hidden must be 64 or 128" : "hidden must be 128");
  const int64_t need = lz_a2c_workspace_bytes_hidden(g->n_samples, g->obs_dim, g->act_dim, g->hidden,
                                                     g->max_workgroups);
  if (g->workspace_bytes < need)
    return fail(LZ_ERR_INVALID, who, any_hidden ? "workspace smaller than lz_a2c_workspace_bytes_hidden"
                                                : "workspace smaller than lz_a2c_workspace_bytes");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nwg = wgs_per_net(g->n_samples, g->max_workgroups);
  const int64_t len = layout(g->obs_dim, g->act_dim, g->hidden).P + kTail;
  GradArgs a;
  a.params = g->params;
  a.obs = g->observations;
  a.act = g->actions;
  a.adv = g->advantages;
  a.ret = g->returns;
  a.n = g->n_samples;
  a.O = g->obs_dim;
  a.A = g->act_dim;
  a.vf_coef = (float)g->vf_coef;
  a.ent_coef = (float)g->ent_coef;
  a.part = static_cast<double*>(g->workspace);
  if (g->hidden == kH64)
    hipLaunchKernelGGL(k_a2c_grad_h64, dim3(2u * (unsigned)nwg), dim3(2 * kH64), 0, s, a);
  else
    hipLaunchKernelGGL(k_a2c_grad, dim3(2u * (unsigned)nwg), dim3(2 * kH), 0, s, a);
  hipLaunchKernelGGL(k_a2c_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s,
                     static_cast<const double*>(g->workspace), nwg, len, g->grad_sums);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
}

}  // namespace

extern "C" lz_status lz_a2c_grad_f32(const lz_a2c_grad_args* g, int32_t device, void* stream) {
  return grad_entry(g, device, stream, "lz_a2c_grad_f32", false);
}

extern "C" lz_status lz_a2c_grad_hidden_f32(const lz_a2c_grad_args* g, int32_t device, void* stream) {
  return grad_entry(g, device, stream, "lz_a2c_grad_hidden_f32", true);
}

extern "C" lz_status lz_a2c_apply_f32(const lz_a2c_apply_args* p, int32_t device, void* stream) {
  using namespace lz::a2c;
  if (!p) return lz::set_error(LZ_ERR_INVALID, "lz_a2c_apply_f32: NULL args");
  if (!p->grad_sums || !p->params || !p->square_avg || !p->stats)
    return lz::set_error(LZ_ERR_INVALID, "lz_a2c_apply_f32: NULL buffer");
  if (p->n_params < 1) return lz::set_error(LZ_ERR_INVALID, "lz_a2c_apply_f32: n_params < 1");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  ApplyArgs a;
  a.sums = p->grad_sums;
  a.params = p->params;
  a.sq = p->square_avg;
  a.P = p->n_params;
  a.lr = p->lr;
  a.max_norm = p->max_grad_norm;
  a.alpha = p->alpha;
  a.eps = p->eps;
  a.vf_coef = p->vf_coef;
  a.ent_coef = p->ent_coef;
  a.stats = p->stats;
  hipLaunchKernelGGL(k_a2c_apply, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
}
