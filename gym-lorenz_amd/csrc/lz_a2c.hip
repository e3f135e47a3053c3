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

#include "lz_grad_common.h"

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

// the forms above and the two entry points' rules
constexpr Form<GradArgs> kForms[] = {{kH, kMaxO, 2 * kH, k_a2c_grad}, {kH64, kMaxO, 2 * kH64, k_a2c_grad_h64}};
constexpr Rule kGrad = {"lz_a2c_grad_f32", "lz_a2c_workspace_bytes", kMaxO, kH, kH};
constexpr Rule kGradHidden = {"lz_a2c_grad_hidden_f32", "lz_a2c_workspace_bytes_hidden", kMaxO, kH64, kH};

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

using namespace lz::a2c;  // the entry points below

extern "C" int64_t lz_a2c_param_count(int32_t obs_dim, int32_t act_dim) {
  return param_count(kGrad, obs_dim, act_dim, kH);
}

extern "C" int64_t lz_a2c_workspace_bytes(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                          int32_t max_workgroups) {
  return workspace_bytes(kGrad, n_samples, obs_dim, act_dim, kH, max_workgroups, kTail);
}

extern "C" int64_t lz_a2c_param_count_hidden(int32_t obs_dim, int32_t act_dim, int32_t hidden) {
  return param_count(kGradHidden, obs_dim, act_dim, hidden);
}

extern "C" int64_t lz_a2c_workspace_bytes_hidden(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                                 int32_t hidden, int32_t max_workgroups) {
  return workspace_bytes(kGradHidden, n_samples, obs_dim, act_dim, hidden, max_workgroups, kTail);
}

namespace {

// every A2C gradient entry point: the refusals in Rule's order, then the launch of the form
// built for g->hidden
lz_status grad_entry(const Rule& r, const lz_a2c_grad_args* g, int32_t device, void* stream) {
  if (!g) return fail(LZ_ERR_INVALID, r.who, "NULL args");
  if (!g->params || !g->observations || !g->actions || !g->advantages || !g->returns ||
      !g->workspace || !g->grad_sums)
    return fail(LZ_ERR_INVALID, r.who, "NULL buffer");
  if (lz_status e = check_shape(r, g->obs_dim, g->act_dim, g->n_samples)) return e;
  if (lz_status e = check_launch(r, g->n_samples, g->obs_dim, g->act_dim, g->hidden, g->max_workgroups,
                                 kTail, g->workspace_bytes))
    return e;
  const Form<GradArgs>* form = pick_form(kForms, g->hidden, g->obs_dim);
  if (!form) return fail(LZ_ERR_UNSUPPORTED, r.who, "no kernel is built for this net");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nwg = wgs_per_net(g->n_samples, g->max_workgroups);
  const int64_t len = layout(g->obs_dim, g->act_dim, g->hidden).P + kTail;
  GradArgs a;
  common_args(a, *g);
  hipLaunchKernelGGL(form->kernel, dim3(2u * (unsigned)nwg), dim3(form->threads), 0, s, a);
  hipLaunchKernelGGL(k_a2c_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s,
                     static_cast<const double*>(g->workspace), nwg, len, g->grad_sums);
  return launched();
}

}  // namespace

extern "C" lz_status lz_a2c_grad_f32(const lz_a2c_grad_args* g, int32_t device, void* stream) {
  return grad_entry(kGrad, g, device, stream);
}

extern "C" lz_status lz_a2c_grad_hidden_f32(const lz_a2c_grad_args* g, int32_t device, void* stream) {
  return grad_entry(kGradHidden, g, device, stream);
}

extern "C" lz_status lz_a2c_apply_f32(const lz_a2c_apply_args* p, int32_t device, void* stream) {
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
  return launched();
}
