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
// Dataflow of k_a2c_grad (one net per workgroup: pi on the even, vf on the odd workgroups;
// 4 waves; a tile = 32 samples; grid-stride over the tiles).  Every matrix of a tile lives
// in LDS as a [unit][sample] image with row stride 33 (any row or column of 32 is then
// conflict-free), and wave w owns unit tile w (32 units) of every product on
// v_mfma_f32_32x32x2_f32 (A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31],
// D[i = (g & 3) + 8 (g >> 2) + 4 (lane >> 5)][j = lane & 31] in register g):
//   h1 = tanh(W1 x + b1)            A = W1 (LDS [unit][8], zero padded), B = x [k][sample]
//   h2 = tanh(W2 h1 + b2)           A = W2 rows (LDS, row stride 129),  B = h1 image
//   out = W_head h2 + b_head        each wave's 32 units from its registers, the four
//                                   partial sums added in wave order
//   d_out per sample                (-adv (a - mu) / sigma^2 | -2 vf_coef (ret - v)); 0 for
//                                   lanes past the last sample, whose x is 0 too
//   d2 = (W_head^T d_out) (1 - h2^2)    in the registers that hold h2
//   d1 = (W2^T d2) (1 - h1^2)       A = W2 columns (the same LDS image), B = d2 image
//   dW2 += d2 h1^T                  A = d2 image [unit][sample], B = h1 image read along
//                                   the sample: wave w accumulates rows 32 w .. 32 w + 31
//                                   of dW2 (4 accumulator tiles) over all the workgroup's
//                                   samples
//   dW1, db1, db2, dW_head          sample sums by one thread per unit over the images
//   db_head, dlog_std, the loss sums  float64 per lane, reduced once at the end
// The float32 accumulators are added into the workgroup's float64 partial vector (its own
// slot of the workspace, no atomics) every kFlushTiles tiles, so no float32 chain is longer
// than 2048 samples whatever the batch; k_a2c_reduce adds the slots in slot order.  Two
// launches on the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lz_internal.h"

namespace lz {
namespace a2c {

typedef float v16 __attribute__((ext_vector_type(16)));

constexpr int kH = 128;          // hidden units (LZ_POLICY_HIDDEN)
constexpr int kTile = 32;        // samples per workgroup tile
constexpr int kLd = 33;          // row stride of the [unit][sample] images
constexpr int kW2Ld = 129;       // row stride of the W2 image
constexpr int kMaxO = 8, kMaxA = 4;
constexpr int kFlushTiles = 64;  // float32 chains end after 64 * 32 samples
constexpr int kDefaultWgs = 128; // workgroups per net when the caller sets no cap
constexpr int kMaxWgs = 4096;

// offsets of the 13 tensors (gym_lorenz.policy.KEYS order, nn.Linear layout) in the flat
// parameter vector, and its length
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
  int64_t n;
  int O, A;
  float vf_coef, ent_coef;
  double* part;  // [workgroups per net][P + 4]
};

__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

__device__ __forceinline__ v16 mfma(float a, float b, v16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void put(double* p, float v, bool first) {
  *p = first ? (double)v : *p + (double)v;
}

__global__ __launch_bounds__(256) void k_a2c_grad(GradArgs a) {
  __shared__ float sW2[kH * kW2Ld];
  __shared__ float sW1[kH * kMaxO];
  __shared__ float sB1[kH], sB2[kH];
  __shared__ float sWh[kMaxA * kH];
  __shared__ float sX[kMaxO * kTile];
  __shared__ float sH1[kH * kLd], sH2[kH * kLd], sD2[kH * kLd], sD1[kH * kLd];
  __shared__ float sHP[4 * kMaxA * kTile];
  __shared__ float sDO[kMaxA * kTile];
  __shared__ double sRed[kTile * (2 + 2 * kMaxA)];

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
  __syncthreads();

  v16 accW2[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) accW2[t][g] = 0.0f;
  float accS[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) accS[i] = 0.0f;
  double lossS = 0.0, entS = 0.0, cntS = 0.0, dbh[kMaxA], dls[kMaxA];
#pragma unroll
  for (int j = 0; j < kMaxA; ++j) dbh[j] = dls[j] = 0.0;

  double* slot = a.part + (int64_t)wg * (P + 4);
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
    {  // x as [k][sample]; rows k >= O and samples past the end are 0
      const int k = tid >> 5, s = tid & 31;
      const int64_t i = base + s;
      sX[k * kTile + s] = (k < O && i < a.n) ? a.obs[i * O + k] : 0.0f;
    }
    const int64_t si = base + r;
    const bool valid = si < a.n;
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
      const bool own = valid && w == 0 && h == 0;
      if (pi) {
        const float adv = valid ? a.adv[si] : 0.0f;
        float logp = 0.0f;
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) {
          if (j < A) {
            const float act = valid ? a.act[si * A + j] : 0.0f;
            const float diff = act - out[j];
            const float q = diff * diff * inv_var[j];
            logp += (-0.5f * q - ls[j]) - 0.91893853320467274f;
            dout[j] = valid ? -adv * (diff * inv_var[j]) : 0.0f;
            if (own) {
              dbh[j] += (double)dout[j];
              dls[j] += (double)(-adv * (q - 1.0f) - a.ent_coef);
            }
          }
        }
        if (own) {
          lossS += (double)(-adv * logp);
          float ent = 0.0f;
#pragma unroll
          for (int j = 0; j < kMaxA; ++j)
            if (j < A) ent += 1.4189385332046727f + ls[j];
          entS += (double)(-ent);
          cntS += 1.0;
        }
      } else {
        const float ret = valid ? a.ret[si] : 0.0f;
        const float e = ret - out[0];
        dout[0] = valid ? -2.0f * a.vf_coef * e : 0.0f;
        if (own) {
          dbh[0] += (double)dout[0];
          lossS += (double)(e * e);
        }
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
  constexpr int kRedLd = 2 + 2 * kMaxA;
  if (w == 0 && h == 0) {
    double* p = sRed + r * kRedLd;
    p[0] = lossS;
    p[1] = entS;
#pragma unroll
    for (int j = 0; j < kMaxA; ++j) {
      p[2 + j] = dbh[j];
      p[2 + kMaxA + j] = dls[j];
    }
  }
  // the count is exact in any order
  double cnt = cntS;
  if (w == 0) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) cnt += __shfl_xor(cnt, m, 64);
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
      if (j < NH) slot[oBh + j] = t[2 + j];
    if (pi) {
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < A) slot[oLs + j] = t[2 + kMaxA + j];
      slot[P + 0] = t[0];
      slot[P + 2] = t[1];
      slot[P + 3] = cnt;
    } else {
      slot[P + 1] = t[0];
    }
  }
}

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

static int wgs_per_net(int64_t n, int cap) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t lim = cap > 0 ? cap : kDefaultWgs;
  return (int)(tiles < lim ? tiles : lim);
}

static bool dims_ok(int O, int A) { return O >= 1 && O <= kMaxO && A >= 1 && A <= kMaxA; }

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

extern "C" lz_status lz_a2c_grad_f32(const lz_a2c_grad_args* g, int32_t device, void* stream) {
  using namespace lz::a2c;
  if (!g) return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: NULL args");
  if (!g->params || !g->observations || !g->actions || !g->advantages || !g->returns ||
      !g->workspace || !g->grad_sums)
    return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: NULL buffer");
  if (!dims_ok(g->obs_dim, g->act_dim))
    return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: obs_dim must be 1..8 and act_dim 1..4");
  if (g->n_samples < 1) return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: n_samples < 1");
  if (g->max_workgroups < 0 || g->max_workgroups > kMaxWgs)
    return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: max_workgroups must be 0..4096");
  if (g->hidden != kH)
    return lz::set_error(LZ_ERR_UNSUPPORTED, "lz_a2c_grad_f32: hidden must be 128");
  const int64_t need = lz_a2c_workspace_bytes(g->n_samples, g->obs_dim, g->act_dim, g->max_workgroups);
  if (g->workspace_bytes < need)
    return lz::set_error(LZ_ERR_INVALID, "lz_a2c_grad_f32: workspace smaller than lz_a2c_workspace_bytes");
  if (hipSetDevice(device) != hipSuccess) return lz::set_error(LZ_ERR_HIP, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nwg = wgs_per_net(g->n_samples, g->max_workgroups);
  const int64_t len = layout(g->obs_dim, g->act_dim).P + 4;
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
  hipLaunchKernelGGL(k_a2c_grad, dim3(2u * (unsigned)nwg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_a2c_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s,
                     static_cast<const double*>(g->workspace), nwg, len, g->grad_sums);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return lz::set_error(LZ_ERR_HIP, hipGetErrorString(e));
  return LZ_OK;
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
