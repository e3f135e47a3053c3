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
// k_ppo_grad keeps k_a2c_grad's dataflow (lz_a2c.hip:12-35: one net per workgroup, pi on
// the even and vf on the odd workgroups, 4 waves, 32-sample tiles as [unit][sample] LDS
// images with row stride 33, v_mfma_f32_32x32x2_f32 in natural k order, float32 chains of at
// most 2048 samples flushed into the workgroup's own float64 slot, k_ppo_reduce adds the
// slots in slot order, no atomics).  What differs:
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
// The file restates k_a2c_grad's text instead of sharing it: lz_a2c.hip stays byte for byte
// what it was, so k_a2c_grad keeps its machine code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lz_internal.h"

namespace lz {
namespace ppo {

typedef float v16 __attribute__((ext_vector_type(16)));

constexpr int kH = 128;          // hidden units (LZ_POLICY_HIDDEN)
constexpr int kTile = 32;        // samples per workgroup tile
constexpr int kLd = 33;          // row stride of the [unit][sample] images
constexpr int kW2Ld = 129;       // row stride of the W2 image
constexpr int kMaxO = 8, kMaxA = 4;
constexpr int kFlushTiles = 64;  // float32 chains end after 64 * 32 samples
constexpr int kDefaultWgs = 128; // workgroups per net when the caller sets no cap
constexpr int kMaxWgs = 4096;
constexpr int kTail = 6;         // loss sums, count, clip count, kl sum after the P gradient sums

// lz_a2c.hip's layout of the flat parameter vector (lz_a2c_param_count is its length)
struct Layout {
  int64_t off[13];
  int64_t P;
};

__host__ __device__ inline Layout layout(int O, int A) {
  Layout L;
  const int64_t n[13] = {(int64_t)kH * O, kH, (int64_t)kH * kH, kH, (int64_t)kH * O, kH,
                         (int64_t)kH * kH, kH, (int64_t)A * kH, A, kH, 1, A};
  int64_t o = 0;
  for (int i = 0; i < 13; ++i) {
    L.off[i] = o;
    o += n[i];
  }
  L.P = o;
  return L;
}

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

__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

__device__ __forceinline__ v16 mfma(float a, float b, v16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void put(double* p, float v, bool first) {
  *p = first ? (double)v : *p + (double)v;
}

__global__ __launch_bounds__(256) void k_ppo_grad(GradArgs a) {
  __shared__ float sW2[kH * kW2Ld];
  __shared__ float sW1[kH * kMaxO];
  __shared__ float sB1[kH], sB2[kH];
  __shared__ float sWh[kMaxA * kH];
  __shared__ float sX[kMaxO * kTile];
  __shared__ float sH1[kH * kLd], sH2[kH * kLd], sD2[kH * kLd], sD1[kH * kLd];
  __shared__ float sHP[4 * kMaxA * kTile];
  __shared__ float sDO[kMaxA * kTile];
  __shared__ double sRed[kTile * (3 + 2 * kMaxA)];

  // SB3's early stop: nothing is computed for a minibatch after the stop (uniform)
  if (a.ctrl && a.ctrl[1] != 0) return;

  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const bool pi = (blockIdx.x & 1u) == 0;
  const int wg = (int)(blockIdx.x >> 1), nwg = (int)(gridDim.x >> 1);
  const int O = a.O, A = a.A, NH = pi ? A : 1;
  const Layout L = layout(O, A);
  // (selected, not indexed: a runtime index would put the table in scratch)
  const int64_t oW1 = pi ? L.off[0] : L.off[4], oB1 = pi ? L.off[1] : L.off[5];
  const int64_t oW2 = pi ? L.off[2] : L.off[6], oB2 = pi ? L.off[3] : L.off[7];
  const int64_t oWh = pi ? L.off[8] : L.off[10], oBh = pi ? L.off[9] : L.off[11];
  const int64_t oLs = L.off[12], P = L.P;
  const float* gW1 = a.params + oW1;
  const float* gB1 = a.params + oB1;
  const float* gW2 = a.params + oW2;
  const float* gB2 = a.params + oB2;
  const float* gWh = a.params + oWh;
  const float* gBh = a.params + oBh;
  const float* gLs = a.params + oLs;

  for (int e = tid; e < kH * kH; e += 256) sW2[(e >> 7) * kW2Ld + (e & 127)] = gW2[e];
  for (int e = tid; e < kH * kMaxO; e += 256) {
    const int u = e >> 3, k = e & 7;
    sW1[e] = k < O ? gW1[u * O + k] : 0.0f;
  }
  for (int e = tid; e < kH; e += 256) {
    sB1[e] = gB1[e];
    sB2[e] = gB2[e];
  }
  for (int e = tid; e < kMaxA * kH; e += 256) sWh[e] = e < NH * kH ? gWh[e] : 0.0f;
  for (int e = tid; e < kMaxA * kTile; e += 256) sDO[e] = 0.0f;
  float bh[kMaxA], ls[kMaxA], inv_var[kMaxA];
#pragma unroll
  for (int j = 0; j < kMaxA; ++j) {
    bh[j] = j < NH ? gBh[j] : 0.0f;
    ls[j] = (pi && j < A) ? gLs[j] : 0.0f;
    const float sd = expf(ls[j]);
    inv_var[j] = 1.0f / (sd * sd);
  }
  // torch forms (adv - mean) / (std + 1e-8) on float32 tensors
  const bool norm = a.moments != nullptr;
  const float adv_mean = norm ? (float)a.moments[0] : 0.0f;
  const float adv_den = norm ? (float)a.moments[1] + 1e-8f : 1.0f;
  __syncthreads();

  v16 accW2[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) accW2[t][g] = 0.0f;
  float accS[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) accS[i] = 0.0f;
  double lossS = 0.0, entS = 0.0, klS = 0.0, cntS = 0.0, clipS = 0.0, dbh[kMaxA], dls[kMaxA];
#pragma unroll
  for (int j = 0; j < kMaxA; ++j) dbh[j] = dls[j] = 0.0;

  double* slot = a.part + (int64_t)wg * (P + kTail);
  bool first = true;
  int since = 0;

  // the workgroup's float32 accumulators into its float64 slot, then zeroed
  auto flush = [&]() __attribute__((always_inline)) {
    double* pW2 = slot + oW2;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        put(pW2 + (32 * w + acc_row(g, h)) * kH + 32 * t + r, accW2[t][g], first);
        accW2[t][g] = 0.0f;
        // eight read-modify-writes in flight at a time, not all 64 (registers)
        if ((g & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
    if (tid < kH) {
#pragma unroll
      for (int o = 0; o < kMaxO; ++o)
        if (o < O) put(slot + oW1 + tid * O + o, accS[o], first);
      put(slot + oB1 + tid, accS[8], first);
    } else {
      const int u = tid - kH;
      put(slot + oB2 + u, accS[8], first);
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < NH) put(slot + oWh + j * kH + u, accS[j], first);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) accS[i] = 0.0f;
    first = false;
    since = 0;
  };

  const int64_t ntiles = (a.n + kTile - 1) / kTile;
  for (int64_t tile = wg; tile < ntiles; tile += nwg) {
    const int64_t base = tile * kTile;
    // sample r of the tile (tid & 31 == r): its row of the flat arrays.  `valid`: a row that
    // may be read; `bad`: a sample whose index lies outside the arrays
    const int64_t si = base + r;
    int64_t row = si;
    if (a.idx && si < a.n) row = (int64_t)a.idx[si];
    const bool valid = si < a.n && row >= 0 && row < a.n_rows;
    const bool bad = si < a.n && !valid;
    {  // x as [k][sample]; rows k >= O and samples that are not read are 0
      const int k = tid >> 5;
      sX[k * kTile + r] = (k < O && valid) ? a.obs[row * O + k] : 0.0f;
    }
    __syncthreads();

    // layer 1
    v16 c, h1, h2;
#pragma unroll
    for (int g = 0; g < 16; ++g) c[g] = sB1[32 * w + acc_row(g, h)];
#pragma unroll
    for (int st = 0; st < kMaxO / 2; ++st)
      c = mfma(sW1[(32 * w + r) * kMaxO + 2 * st + h], sX[(2 * st + h) * kTile + r], c);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      h1[g] = tanhf(c[g]);
      sH1[(32 * w + acc_row(g, h)) * kLd + r] = h1[g];
    }
    __syncthreads();

    // layer 2
#pragma unroll
    for (int g = 0; g < 16; ++g) c[g] = sB2[32 * w + acc_row(g, h)];
#pragma unroll 8
    for (int st = 0; st < kH / 2; ++st)
      c = mfma(sW2[(32 * w + r) * kW2Ld + 2 * st + h], sH1[(2 * st + h) * kLd + r], c);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      h2[g] = tanhf(c[g]);
      sH2[(32 * w + acc_row(g, h)) * kLd + r] = h2[g];
    }
    // this wave's share of the head rows
#pragma unroll
    for (int j = 0; j < kMaxA; ++j) {
      if (j < NH) {
        float p = 0.0f;
#pragma unroll
        for (int g = 0; g < 16; ++g) p = fmaf(sWh[j * kH + 32 * w + acc_row(g, h)], h2[g], p);
        p += __shfl_xor(p, 32, 64);
        if (h == 0) sHP[(w * kMaxA + j) * kTile + r] = p;
      }
    }
    __syncthreads();

    // heads, the loss terms and d_out of sample r (every wave computes the same values)
    float dout[kMaxA];
    {
      float out[kMaxA];
#pragma unroll
      for (int j = 0; j < kMaxA; ++j) {
        out[j] = 0.0f;
        if (j < NH)
          out[j] = (((sHP[(0 * kMaxA + j) * kTile + r] + sHP[(1 * kMaxA + j) * kTile + r]) +
                     sHP[(2 * kMaxA + j) * kTile + r]) + sHP[(3 * kMaxA + j) * kTile + r]) + bh[j];
        dout[j] = 0.0f;
      }
      const bool own = w == 0 && h == 0;
      if (pi) {
        const float adv_n = valid ? (a.adv[row] - adv_mean) / adv_den : 0.0f;
        const float old_lp = valid ? a.old_logp[row] : 0.0f;
        // log_prob of the whole sample before the ratio
        float diff[kMaxA], q[kMaxA], logp = 0.0f;
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) {
          diff[j] = q[j] = 0.0f;
          if (j < A) {
            const float act = valid ? a.act[row * A + j] : 0.0f;
            diff[j] = act - out[j];
            q[j] = diff[j] * diff[j] * inv_var[j];
            logp += (-0.5f * q[j] - ls[j]) - 0.91893853320467274f;
          }
        }
        const float log_ratio = logp - old_lp;
        const float ratio = expf(log_ratio);
        const float s1 = adv_n * ratio;
        const float s2 = adv_n * fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
        const float pl = -((s1 < s2 || s1 != s1) ? s1 : s2);  // torch.min keeps a NaN
        const bool zeroed = (ratio > a.clip_hi && adv_n > 0.0f) || (ratio < a.clip_lo && adv_n < 0.0f);
        const float cf = (valid && !zeroed) ? -adv_n * ratio : 0.0f;
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) {
          if (j < A) {
            dout[j] = cf * (diff[j] * inv_var[j]);
            if (own && valid) {
              dbh[j] += (double)dout[j];
              dls[j] += (double)(cf * (q[j] - 1.0f) - a.ent_coef);
            }
          }
        }
        if (own && valid) {
          lossS += (double)pl;
          float ent = 0.0f;
#pragma unroll
          for (int j = 0; j < kMaxA; ++j)
            if (j < A) ent += 1.4189385332046727f + ls[j];
          entS += (double)(-ent);
          klS += (double)((ratio - 1.0f) - log_ratio);
          clipS += fabsf(ratio - 1.0f) > a.clip ? 1.0 : 0.0;
        }
        if (own && bad) {
          lossS += (double)NAN;
          entS += (double)NAN;
        }
        if (own && si < a.n) cntS += 1.0;
      } else {
        const float ret = valid ? a.ret[row] : 0.0f;
        float v_pred = out[0];
        bool act_v = valid;
        if (a.old_val) {
          const float ov = valid ? a.old_val[row] : 0.0f;
          const float d = out[0] - ov;
          v_pred = ov + fminf(fmaxf(d, -a.clip_vf), a.clip_vf);
          act_v = valid && !(fabsf(d) > a.clip_vf);
        }
        const float e = ret - v_pred;
        dout[0] = act_v ? -2.0f * a.vf_coef * e : 0.0f;
        if (own && valid) {
          dbh[0] += (double)dout[0];
          lossS += (double)(e * e);
        }
        if (own && bad) lossS += (double)NAN;
      }
      if (w == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < kMaxA; ++j)
          if (j < NH) sDO[j * kTile + r] = dout[j];
      }
    }
    // d2 in place of h2
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int u = 32 * w + acc_row(g, h);
      float cc = 0.0f;
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < NH) cc = fmaf(sWh[j * kH + u], dout[j], cc);
      sD2[u * kLd + r] = cc * (1.0f - h2[g] * h2[g]);
    }
    __syncthreads();

    // d1 = (W2^T d2) (1 - h1^2)
#pragma unroll
    for (int g = 0; g < 16; ++g) c[g] = 0.0f;
#pragma unroll 8
    for (int st = 0; st < kH / 2; ++st)
      c = mfma(sW2[(2 * st + h) * kW2Ld + 32 * w + r], sD2[(2 * st + h) * kLd + r], c);
#pragma unroll
    for (int g = 0; g < 16; ++g)
      sD1[(32 * w + acc_row(g, h)) * kLd + r] = c[g] * (1.0f - h1[g] * h1[g]);
    // dW2 rows 32 w .. 32 w + 31
#pragma unroll 4
    for (int st = 0; st < kTile / 2; ++st) {
      const float av = sD2[(32 * w + r) * kLd + 2 * st + h];
#pragma unroll
      for (int t = 0; t < 4; ++t) accW2[t] = mfma(av, sH1[(32 * t + r) * kLd + 2 * st + h], accW2[t]);
    }
    __syncthreads();

    // the sample sums of the small tensors, one thread per unit
    if (tid < kH) {  // dW1 row and db1 of unit tid
#pragma unroll 4
      for (int s = 0; s < kTile; ++s) {
        const float d = sD1[tid * kLd + s];
        accS[8] += d;
#pragma unroll
        for (int o = 0; o < kMaxO; ++o) accS[o] = fmaf(d, sX[o * kTile + s], accS[o]);
      }
    } else {  // db2 and the head rows' column of unit tid - 128
      const int u = tid - kH;
#pragma unroll 4
      for (int s = 0; s < kTile; ++s) {
        accS[8] += sD2[u * kLd + s];
        const float hv = sH2[u * kLd + s];
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) accS[j] = fmaf(sDO[j * kTile + s], hv, accS[j]);
      }
    }
    // every workgroup has at least one tile (the grid is no larger than the tile count),
    // so the last tile's flush writes every entry of the slot at least once
    if (++since == kFlushTiles || tile + nwg >= ntiles) flush();
    __syncthreads();
  }

  // the float64 per-lane sums of wave 0's lower half, added in lane order
  constexpr int kRedLd = 3 + 2 * kMaxA;
  if (w == 0 && h == 0) {
    double* p = sRed + r * kRedLd;
    p[0] = lossS;
    p[1] = entS;
    p[2] = klS;
#pragma unroll
    for (int j = 0; j < kMaxA; ++j) {
      p[3 + j] = dbh[j];
      p[3 + kMaxA + j] = dls[j];
    }
  }
  // the two counts are exact in any order
  double cnt = cntS, ncl = clipS;
  if (w == 0) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
      cnt += __shfl_xor(cnt, m, 64);
      ncl += __shfl_xor(ncl, m, 64);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double t[kRedLd];
#pragma unroll
    for (int i = 0; i < kRedLd; ++i) t[i] = 0.0;
#pragma unroll 1
    for (int s = 0; s < kTile; ++s)
#pragma unroll
      for (int i = 0; i < kRedLd; ++i) t[i] += sRed[s * kRedLd + i];
#pragma unroll
    for (int j = 0; j < kMaxA; ++j)
      if (j < NH) slot[oBh + j] = t[3 + j];
    if (pi) {
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < A) slot[oLs + j] = t[3 + kMaxA + j];
      slot[P + 0] = t[0];
      slot[P + 2] = t[1];
      slot[P + 3] = cnt;
      slot[P + 4] = ncl;
      slot[P + 5] = t[2];
    } else {
      slot[P + 1] = t[0];
    }
  }
}

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

static int wgs_per_net(int64_t n, int cap) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t lim = cap > 0 ? cap : kDefaultWgs;
  return (int)(tiles < lim ? tiles : lim);
}

static bool dims_ok(int O, int A) { return O >= 1 && O <= kMaxO && A >= 1 && A <= kMaxA; }

}  // namespace ppo
}  // namespace lz

extern "C" int64_t lz_ppo_workspace_bytes(int64_t n_samples, int32_t obs_dim, int32_t act_dim,
                                          int32_t max_workgroups) {
  using namespace lz::ppo;
  if (!dims_ok(obs_dim, act_dim) || n_samples < 1 || max_workgroups < 0 || max_workgroups > kMaxWgs)
    return -1;
  const int64_t P = layout(obs_dim, act_dim).P;
  return (int64_t)wgs_per_net(n_samples, max_workgroups) * (P + kTail) * (int64_t)sizeof(double);
}

extern "C" lz_status lz_ppo_adv_moments(const float* advantages, const int32_t* indices,
                                        int64_t n_samples, int64_t n_rows, void* workspace,
                                        double* out, int32_t device, void* stream) {
  using namespace lz::ppo;
  (void)workspace;
  if (!advantages || !out) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: NULL buffer");
  if (n_samples < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_samples < 1");
  if (n_rows < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_rows < 1");
  if (!indices && n_samples > n_rows)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_adv_moments: n_samples > n_rows without indices");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(k_ppo_adv_moments, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream),
                     advantages, indices, n_samples, n_rows, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
}

extern "C" lz_status lz_ppo_grad_f32(const lz_ppo_grad_args* g, int32_t device, void* stream) {
  using namespace lz::ppo;
  if (!g) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: NULL args");
  if (!g->params || !g->observations || !g->actions || !g->advantages || !g->returns ||
      !g->old_log_prob || !g->workspace || !g->grad_sums)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: NULL buffer");
  if (g->clip_range_vf > 0.0 && !g->old_values)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: NULL old_values with clip_range_vf > 0");
  if (!dims_ok(g->obs_dim, g->act_dim))
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: obs_dim must be 1..8 and act_dim 1..4");
  if (g->n_samples < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: n_samples < 1");
  if (g->n_rows < 1) return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: n_rows < 1");
  if (!g->indices && g->n_samples > g->n_rows)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: n_samples > n_rows without indices");
  if (!(g->clip_range >= 0.0) || std::isinf(g->clip_range))
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: clip_range must be finite and >= 0");
  if (g->clip_range_vf != g->clip_range_vf || std::isinf(g->clip_range_vf))
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: clip_range_vf must be finite");
  if (g->max_workgroups < 0 || g->max_workgroups > kMaxWgs)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: max_workgroups must be 0..4096");
  if (g->hidden != kH)
    return lz::set_error(LZ_ERR_UNSUPPORTED, "lz_ppo_grad_f32: hidden must be 128");
  const int64_t need = lz_ppo_workspace_bytes(g->n_samples, g->obs_dim, g->act_dim, g->max_workgroups);
  if (g->workspace_bytes < need)
    return lz::set_error(LZ_ERR_INVALID, "lz_ppo_grad_f32: workspace smaller than lz_ppo_workspace_bytes");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nwg = wgs_per_net(g->n_samples, g->max_workgroups);
  const int64_t len = layout(g->obs_dim, g->act_dim).P + kTail;
  GradArgs a;
  a.params = g->params;
  a.obs = g->observations;
  a.act = g->actions;
  a.adv = g->advantages;
  a.ret = g->returns;
  a.old_logp = g->old_log_prob;
  a.old_val = g->clip_range_vf > 0.0 ? g->old_values : nullptr;
  a.idx = g->indices;
  a.moments = g->adv_moments;
  a.ctrl = g->ctrl;
  a.n = g->n_samples;
  a.n_rows = g->n_rows;
  a.O = g->obs_dim;
  a.A = g->act_dim;
  a.vf_coef = (float)g->vf_coef;
  a.ent_coef = (float)g->ent_coef;
  // torch compares and clamps the float32 ratio with the Python floats rounded to float32
  a.clip = (float)g->clip_range;
  a.clip_lo = (float)(1.0 - g->clip_range);
  a.clip_hi = (float)(1.0 + g->clip_range);
  a.clip_vf = (float)g->clip_range_vf;
  a.part = static_cast<double*>(g->workspace);
  hipLaunchKernelGGL(k_ppo_grad, dim3(2u * (unsigned)nwg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s,
                     static_cast<const double*>(g->workspace), nwg, len, g->ctrl, g->grad_sums);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
}

extern "C" lz_status lz_adam_apply_f32(const lz_adam_apply_args* p, int32_t device, void* stream) {
  using namespace lz::ppo;
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
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
}
