// One PPO minibatch step for the float32 MlpPolicy on a rollout that is already on the
// device: lz_ppo_adv_moments (the minibatch's advantage mean and unbiased std),
// lz_ppo_grad_f32 (forward + backward of the two obs -> 128 -> 128 Tanh nets on the rows an
// index list names, the clipped surrogate and the clipped value loss, per-workgroup partial
// sums, a fixed-order float64 reduction) and lz_adam_apply_f32 (clip_grad_norm_ + Adam with
// the step count and the target_kl stop flag on the device).  Restates SB3 2.7.1
// PPO.train() (stable_baselines3/ppo/ppo.py:181-300: advantages = (advantages - mean) /
// (std + 1e-8), ratio = exp(log_prob - old_log_prob), policy_loss = -min(adv ratio,
// adv clamp(ratio, 1 - clip, 1 + clip)).mean(), values_pred = old_values + clamp(values -
// old_values, -clip_range_vf, clip_range_vf), value_loss = F.mse_loss(returns, values_pred),
// entropy_loss = -mean(entropy), clip_fraction, approx_kl = mean((ratio - 1) - log_ratio),
// the target_kl break, clip_grad_norm_(max_grad_norm), optimizer.step()), RolloutBuffer.get
// (common/buffers.py: a permutation of the flattened rows cut into minibatches),
// ActorCriticPolicy.evaluate_actions (common/policies.py), DiagGaussianDistribution.log_prob
// / entropy (common/distributions.py), torch.optim.Adam (betas (0.9, 0.999), eps 1e-5 from
// ActorCriticPolicy's optimizer_kwargs, no weight decay, no amsgrad) and
// torch.nn.utils.clip_grad_norm_, as the reference's learners use them (code/train.py:97-129,
// code/lorenz_filter/train.py, code/gym_run.py:83).
//
// k_ppo_grad is lz_grad_body.inc with LZ_GRAD_PPO 1: k_a2c_grad's text and dataflow (one
// net per workgroup, pi on the even and vf on the odd workgroups, 4 waves, 32-sample tiles as
// [unit][sample] LDS images with row stride 33, v_mfma_f32_32x32x2_f32 in natural k order,
// float32 chains of at most 2048 samples flushed into the workgroup's own float64 slot,
// k_ppo_reduce adds the slots in slot order, no atomics).  What differs, each a block under
// LZ_GRAD_PPO there:
//   rows            sample i of the minibatch is row indices[i] of the flat [n_rows] arrays
//                   (x, actions, adv, ret, old_log_prob, old_values are gathered); a row
//                   outside [0, n_rows) is never dereferenced: the sample adds nothing to the
//                   gradient and NaN to the three loss sums
//   pi head phase   log_prob of the whole sample first (the sum over the action dims), then
//                   ratio = expf(log_prob - old_log_prob), c = active ? -adv_n ratio : 0 with
//                   active = !((ratio > 1 + clip and adv_n > 0) or (ratio < 1 - clip and
//                   adv_n < 0)) (torch autograd's derivative of the min / clamp: the clip
//                   edges are active), d_out[j] = c (a_j - mu_j) / sigma_j^2,
//                   dlog_std[j] += c (q_j - 1) - ent_coef
//   vf head phase   d_out = -2 vf_coef (ret - v_pred), 0 where |v - old_v| > clip_range_vf
//   two more float64 per-lane sums: [|ratio - 1| > clip] and (ratio - 1) - log_ratio
//   the launch returns at entry while ctrl[1] (the target_kl stop) is set
//
// k_ppo_grad_h64 is the same text with LZ_GRAD_H 64, the obs -> 64 -> 64 net of SB3's default
// MlpPolicy: what code/train.py:106-118 and code/lorenz_filter/train.py:117-129 train (both
// build a policy_kwargs dict and never pass it on) and what the reference's shipped PPO
// policies hold (hr_sync_agent.zip: (64, 6) / (64, 64) / (1, 64));
// lz_ppo_grad_hidden_f32 launches either form.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lz_grad_common.h"

namespace lz {
namespace ppo {

using namespace grad;

constexpr int kTail = 6;      // loss sums, count, clip count, kl sum after the P gradient sums
constexpr int kLaneSums = 3;  // policy / value loss sum, entropy sum, kl sum

struct GradArgs {
  const float* params;
  const float* obs;
  const float* act;
  const float* adv;
  const float* ret;
  const float* old_logp;
  const float* old_val;     // nullptr: no value clipping
  const int32_t* idx;       // nullptr: rows 0 .. n - 1
  const double* moments;    // nullptr: no advantage normalisation
  const int64_t* ctrl;      // nullptr, or {step, stopped}: a set flag ends the launch at entry
  int64_t n, n_rows;
  int O, A;
  float vf_coef, ent_coef;
  float clip, clip_lo, clip_hi;  // (float)clip, (float)(1 - clip), (float)(1 + clip)
  float clip_vf;                 // <= 0: none
  double* part;  // [workgroups per net][P + 6]
};

#define LZ_GRAD_PPO 1
#define LZ_GRAD_H 128
#define LZ_GRAD_KERNEL k_ppo_grad
#include "lz_grad_body.inc"
#undef LZ_GRAD_KERNEL
#undef LZ_GRAD_H
// the same text for SB3's default 64 x 64 net: 2 waves, 128 threads (lz_ppo_grad_hidden_f32)
#define LZ_GRAD_H 64
#define LZ_GRAD_KERNEL k_ppo_grad_h64
#include "lz_grad_body.inc"
#undef LZ_GRAD_KERNEL
#undef LZ_GRAD_H
// ... and for that net on a frame-stacked observation of up to 24 inputs
// (code/lorenz_filter/train.py:109-131: VecFrameStack(n_stack=4) on HR's 6, tensors
// (64, 24) / (64, 64) / (A, 64)): the x and W1 images 24 wide, 12 layer-1 MFMA steps
// (lz_ppo_grad_wide_f32 for obs_dim > 8)
#define LZ_GRAD_H 64
#define LZ_GRAD_MAXO 24
#define LZ_GRAD_KERNEL k_ppo_grad_h64_wide
#include "lz_grad_body.inc"
#undef LZ_GRAD_KERNEL
#undef LZ_GRAD_MAXO
#undef LZ_GRAD_H
#undef LZ_GRAD_PPO

// the forms above (the wide one after the narrow one it falls back to at obs_dim <= 8) and
// the three entry points' rules (24: the wide form's LZ_GRAD_MAXO, the wide rule's limit)
constexpr Form<GradArgs> kForms[] = {{kH, kMaxO, 2 * kH, k_ppo_grad},
                                     {kH64, kMaxO, 2 * kH64, k_ppo_grad_h64},
                                     {kH64, 24, 2 * kH64, k_ppo_grad_h64_wide}};
constexpr Rule kGrad = {"lz_ppo_grad_f32", "lz_ppo_workspace_bytes", kMaxO, kH, kH};
constexpr Rule kGradHidden = {"lz_ppo_grad_hidden_f32", "lz_ppo_workspace_bytes_hidden", kMaxO, kH64, kH};
constexpr Rule kGradWide = {"lz_ppo_grad_wide_f32", "lz_ppo_workspace_bytes_wide", kForms[2].max_obs, kH64, kH64};

// out[i] = the slots' entries i added in slot order (nothing after the stop, as k_ppo_grad)
__global__ __launch_bounds__(256) void k_ppo_reduce(const double* __restrict__ part, int nwg,
                                                    int64_t len, const int64_t* __restrict__ ctrl,
                                                    double* __restrict__ out) {
  if (ctrl && ctrl[1] != 0) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  double s = 0.0;
  // (unrolled: eight slots' loads in flight per thread; the order of the adds is the slots')
#pragma unroll 8
  for (int g = 0; g < nwg; ++g) s += part[(int64_t)g * len + i];
  out[i] = s;
}

// s + e (e the running error term) += x, exactly (Knuth's two-sum): the centred squares of
// 65,536 advantages then sum to within an ulp of their true sum in any order
__device__ __forceinline__ void dd_add(double& s, double& e, double x) {
  const double t = s + x;
  const double bb = t - s;
  e += (s - (t - bb)) + (x - bb);
  s = t;
}

// one workgroup: thread t adds samples t, t + 1024, ... in that order, then a fixed tree;
// out = {mean, sqrt(sum((adv - mean)^2) / (M - 1))} (torch.mean / torch.std, in float64)
__global__ __launch_bounds__(1024) void k_ppo_adv_moments(const float* __restrict__ adv,
                                                          const int32_t* __restrict__ idx, int64_t m,
                                                          int64_t n_rows, double* __restrict__ out) {
  __shared__ double sS[1024], sE[1024];
  const int tid = (int)threadIdx.x;
  double mean = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double s = 0.0, e = 0.0;
    for (int64_t i = tid; i < m; i += 1024) {
      const int64_t row = idx ? (int64_t)idx[i] : i;
      // a row outside the array is not read: the moments are NaN
      const double x = (row >= 0 && row < n_rows) ? (double)adv[row] : (double)NAN;
      const double d = x - mean;
      dd_add(s, e, pass == 0 ? x : d * d);
    }
    sS[tid] = s;
    sE[tid] = e;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
      if (tid < k) {
        double s0 = sS[tid], e0 = sE[tid] + sE[tid + k];
        dd_add(s0, e0, sS[tid + k]);
        sS[tid] = s0;
        sE[tid] = e0;
      }
      __syncthreads();
    }
    const double total = sS[0] + sE[0];
    __syncthreads();
    if (pass == 0) {
      mean = total / (double)m;
    } else if (tid == 0) {
      out[0] = mean;
      out[1] = sqrt(total / (double)(m - 1));
    }
  }
}

struct AdamArgs {
  const double* sums;
  float* params;
  float* m;
  float* v;
  int64_t P;
  double lr, max_norm, b1, b2, eps, vf_coef, ent_coef, target_kl;
  int64_t* ctrl;
  double* stats;
};

// one workgroup: the early-stop decision, the mean gradient rounded to float32 (what torch's
// .grad holds), its global norm (float64, a fixed tree), the clip coefficient, torch's Adam
__global__ __launch_bounds__(1024) void k_adam_apply(AdamArgs a) {
  __shared__ double sN[1024];
  const int tid = (int)threadIdx.x;
  const int64_t step0 = a.ctrl[0];
  const bool was_stopped = a.ctrl[1] != 0;
  const double nan = (double)NAN;
  if (was_stopped) {  // the sums are not this minibatch's: k_ppo_grad left at entry
    if (tid == 0) {
      for (int i = 0; i < 10; ++i) a.stats[i] = nan;
      a.stats[7] = a.lr;
      a.stats[10] = (double)step0;
      a.stats[11] = 1.0;
    }
    return;
  }
  const double cnt = a.sums[a.P + 3];
  const double pl = a.sums[a.P + 0] / cnt, vl = a.sums[a.P + 1] / cnt, el = a.sums[a.P + 2] / cnt;
  const double kl = a.sums[a.P + 5] / cnt;
  const bool stop = a.target_kl > 0.0 && kl > 1.5 * a.target_kl;
  double total = nan, coef = nan;
  if (!stop) {
    double loc = 0.0;
    for (int64_t i = tid; i < a.P; i += 1024) {
      const double g = (double)(float)(a.sums[i] / cnt);
      loc += g * g;
    }
    sN[tid] = loc;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
      if (tid < k) sN[tid] += sN[tid + k];
      __syncthreads();
    }
    total = sqrt(sN[0]);
    const double c0 = a.max_norm / (total + 1e-6);
    coef = c0 > 1.0 ? 1.0 : c0;  // NaN stays NaN, as torch.clamp(max=1.0) keeps it
    const double t = (double)(step0 + 1);
    const double step_size = a.lr / (1.0 - pow(a.b1, t));
    const double bc2_sqrt = sqrt(1.0 - pow(a.b2, t));
    for (int64_t i = tid; i < a.P; i += 1024) {
      const double g = (double)(float)(a.sums[i] / cnt) * coef;
      const double m = a.b1 * (double)a.m[i] + (1.0 - a.b1) * g;
      const double v = a.b2 * (double)a.v[i] + (1.0 - a.b2) * (g * g);
      const double p = (double)a.params[i] - step_size * m / (sqrt(v) / bc2_sqrt + a.eps);
      a.m[i] = (float)m;
      a.v[i] = (float)v;
      a.params[i] = (float)p;
    }
  }
  // every thread has read ctrl before thread 0 writes it
  __syncthreads();
  if (tid == 0) {
    const int64_t step1 = stop ? step0 : step0 + 1;
    a.ctrl[0] = step1;
    if (stop) a.ctrl[1] = 1;
    a.stats[0] = pl;
    a.stats[1] = vl;
    a.stats[2] = el;
    a.stats[3] = (pl + a.ent_coef * el) + a.vf_coef * vl;
    a.stats[4] = total;
    a.stats[5] = coef;
    a.stats[6] = cnt;
    a.stats[7] = a.lr;
    a.stats[8] = a.sums[a.P + 4] / cnt;
    a.stats[9] = kl;
    a.stats[10] = (double)step1;
    a.stats[11] = stop ? 1.0 : 0.0;
  }
}

}  // namespace ppo
}  // namespace lz

using namespace lz::ppo;  // the entry points below

extern "C" int64_t lz_ppo_workspace_bytes(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                          int32_t max_workgroups) {
  return workspace_bytes(kGrad, n_samples, obs_dim, act_dim, kH, max_workgroups, kTail);
}

extern "C" int64_t lz_ppo_workspace_bytes_hidden(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                                 int32_t hidden, int32_t max_workgroups) {
  return workspace_bytes(kGradHidden, n_samples, obs_dim, act_dim, hidden, max_workgroups, kTail);
}

extern "C" int64_t lz_ppo_param_count_wide(int32_t obs_dim, int32_t act_dim, int32_t hidden) {
  return param_count(kGradWide, obs_dim, act_dim, hidden);
}

extern "C" int64_t lz_ppo_workspace_bytes_wide(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                               int32_t hidden, int32_t max_workgroups) {
  return workspace_bytes(kGradWide, n_samples, obs_dim, act_dim, hidden, max_workgroups, kTail);
}

extern "C" lz_status lz_ppo_adv_moments(const float* advantages, const int32_t* indices,
                                        int64_t n_samples, int64_t n_rows, void* workspace,
                                        double* out, int32_t device, void* stream) {
  (void)workspace;
  if (!advantages || !out) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: NULL buffer");
  if (n_samples < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_samples < 1");
  if (n_rows < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_rows < 1");
  if (!indices && n_samples > n_rows)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_samples > n_rows without indices");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(k_ppo_adv_moments, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream),
                     advantages, indices, n_samples, n_rows, out);
  return launched();
}

namespace {

// every PPO gradient entry point: the refusals in Rule's order, then the launch of the form
// built for g->hidden and g->obs_dim
lz_status grad_entry(const Rule& r, const lz_ppo_grad_args* g, int32_t device, void* stream) {
  if (!g) return fail(LZ_ERR_INVALID, r.who, "NULL args");
  if (!g->params || !g->observations || !g->actions || !g->advantages || !g->returns ||
      !g->old_log_prob || !g->workspace || !g->grad_sums)
    return fail(LZ_ERR_INVALID, r.who, "NULL buffer");
  if (g->clip_range_vf > 0.0 && !g->old_values)
    return fail(LZ_ERR_INVALID, r.who, "NULL old_values with clip_range_vf > 0");
  if (lz_status e = check_shape(r, g->obs_dim, g->act_dim, g->n_samples)) return e;
  if (g->n_rows < 1) return fail(LZ_ERR_INVALID, r.who, "n_rows < 1");
  if (!g->indices && g->n_samples > g->n_rows)
    return fail(LZ_ERR_INVALID, r.who, "n_samples > n_rows without indices");
  if (!(g->clip_range >= 0.0) || std::isinf(g->clip_range))
    return fail(LZ_ERR_INVALID, r.who, "clip_range must be finite and >= 0");
  if (g->clip_range_vf != g->clip_range_vf || std::isinf(g->clip_range_vf))
    return fail(LZ_ERR_INVALID, r.who, "clip_range_vf must be finite");
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
  a.old_logp = g->old_log_prob;
  a.old_val = g->clip_range_vf > 0.0 ? g->old_values : nullptr;
  a.idx = g->indices;
  a.moments = g->adv_moments;
  a.ctrl = g->ctrl;
  a.n_rows = g->n_rows;
  // torch compares and clamps the float32 ratio with the Python floats rounded to float32
  a.clip = (float)g->clip_range;
  a.clip_lo = (float)(1.0 - g->clip_range);
  a.clip_hi = (float)(1.0 + g->clip_range);
  a.clip_vf = (float)g->clip_range_vf;
  hipLaunchKernelGGL(form->kernel, dim3(2u * (unsigned)nwg), dim3(form->threads), 0, s, a);
  hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s,
                     static_cast<const double*>(g->workspace), nwg, len, g->ctrl, g->grad_sums);
  return launched();
}

}  // namespace

extern "C" lz_status lz_ppo_grad_f32(const lz_ppo_grad_args* g, int32_t device, void* stream) {
  return grad_entry(kGrad, g, device, stream);
}

extern "C" lz_status lz_ppo_grad_hidden_f32(const lz_ppo_grad_args* g, int32_t device, void* stream) {
  return grad_entry(kGradHidden, g, device, stream);
}

extern "C" lz_status lz_ppo_grad_wide_f32(const lz_ppo_grad_args* g, int32_t device, void* stream) {
  return grad_entry(kGradWide, g, device, stream);
}

extern "C" lz_status lz_adam_apply_f32(const lz_adam_apply_args* p, int32_t device, void* stream) {
  if (!p) return lz::set_error(LZ_ERR_INVALID, "lz_adam_apply_f32: NULL args");
  if (!p->grad_sums || !p->params || !p->exp_avg || !p->exp_avg_sq || !p->ctrl || !p->stats)
    return lz::set_error(LZ_ERR_INVALID, "lz_adam_apply_f32: NULL buffer");
  if (p->n_params < 1) return lz::set_error(LZ_ERR_INVALID, "lz_adam_apply_f32: n_params < 1");
  if (!(p->beta1 >= 0.0 && p->beta1 < 1.0) || !(p->beta2 >= 0.0 && p->beta2 < 1.0))
    return lz::set_error(LZ_ERR_INVALID, "lz_adam_apply_f32: betas must lie in [0, 1)");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  AdamArgs a;
  a.sums = p->grad_sums;
  a.params = p->params;
  a.m = p->exp_avg;
  a.v = p->exp_avg_sq;
  a.P = p->n_params;
  a.lr = p->lr;
  a.max_norm = p->max_grad_norm;
  a.b1 = p->beta1;
  a.b2 = p->beta2;
  a.eps = p->eps;
  a.vf_coef = p->vf_coef;
  a.ent_coef = p->ent_coef;
  a.target_kl = p->target_kl;
  a.ctrl = p->ctrl;
  a.stats = p->stats;
  hipLaunchKernelGGL(k_adam_apply, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
  return launched();
}
