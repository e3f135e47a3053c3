// The gradient kernel of the float32 MlpPolicy, from __global__ to its closing brace.
// lz_a2c.hip (inside lz::a2c) and lz_ppo.hip (inside lz::ppo) each include this file once
// per hidden size, after their GradArgs and after defining
//   LZ_GRAD_PPO     0: k_a2c_grad, 1: k_ppo_grad
//   LZ_GRAD_H       hidden units: 128, or 64 (the _h64 kernels)
//   LZ_GRAD_KERNEL  the kernel's name
//   kTail           doubles after the P gradient sums in a workgroup's slot
//   kLaneSums       float64 per-lane loss sums that go through the lane-order reduction
//   LZ_GRAD_MAXO    (optional, default 8) the widest input: 24 for k_ppo_grad_h64_wide, the
//                   frame-stacked MlpPolicy (code/lorenz_filter/train.py:109-131); every
//                   constant that depends on it is kMO / kW1Ld below, and with the default
//                   they are the numbers the text had before
// One text, so the two forms cannot drift apart -- and the preprocessor, not a template
// parameter, picks the form: each kernel keeps its name and its machine code (measurements
// are tied to kernel code hashes, tools/kernel_hash.py; DESIGN.md 4.6).  The forms differ in
// the blocks under LZ_GRAD_PPO and nowhere else; lz_ppo.hip's header says what its side of
// each block computes.
//
// Dataflow (one net per workgroup: pi on the even, vf on the odd workgroups; 4 waves; a
// tile = 32 samples; grid-stride over the tiles).  Every matrix of a tile lives in LDS as a
// [unit][sample] image with row stride 33 (any row or column of 32 is then conflict-free),
// and wave w owns unit tile w (32 units) of every product on v_mfma_f32_32x32x2_f32
// (A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31],
// D[i = (g & 3) + 8 (g >> 2) + 4 (lane >> 5)][j = lane & 31] in register g):
//   h1 = tanh(W1 x + b1)            A = W1 (LDS [unit][8], zero padded), B = x [k][sample]
//   h2 = tanh(W2 h1 + b2)           A = W2 rows (LDS, row stride 129),  B = h1 image
//   out = W_head h2 + b_head        each wave's 32 units from its registers, the four
//                                   partial sums added in wave order
//   d_out per sample                A2C: (-adv (a - mu) / sigma^2 | -2 vf_coef (ret - v)); 0
//                                   for lanes past the last sample, whose x is 0 too
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
// than 2048 samples whatever the batch; the reduce kernel adds the slots in slot order.  Two
// launches on the same inputs give the same bits.
//
// The hidden size is the including file's too: LZ_GRAD_H is 128 (k_a2c_grad, k_ppo_grad: the
// figures above) or 64 (k_a2c_grad_h64, k_ppo_grad_h64: SB3's default MlpPolicy).  Everything
// that depends on it is a constant below: kWaves = kH / 32 waves, kThreads = 2 kH threads (one
// per unit for each of the two per-unit sample sums), W2 row stride kH + 1, kWaves accumulator
// tiles of dW2 and kWaves head partials per sample.  The 64-unit form computes what the
// 128-unit form computes on the zero-padded net: the padded units add exact zeros to every
// chain, and the tiles, flushes and slots are the same.
#if !defined(LZ_GRAD_PPO) || !defined(LZ_GRAD_KERNEL) || !defined(LZ_GRAD_H)
#error "lz_grad_body.inc: define LZ_GRAD_PPO to 0 or 1, LZ_GRAD_KERNEL to the kernel's name, LZ_GRAD_H to 128 or 64"
#endif
#if LZ_GRAD_H != 128 && LZ_GRAD_H != 64
#error "lz_grad_body.inc: LZ_GRAD_H must be 128 or 64"
#endif
#ifndef LZ_GRAD_MAXO
#define LZ_GRAD_MAXO 8
#define LZ_GRAD_MAXO_DEFAULTED 1
#endif
#if LZ_GRAD_MAXO % 2 != 0 || (32 * LZ_GRAD_MAXO) % (2 * LZ_GRAD_H) != 0
#error "lz_grad_body.inc: LZ_GRAD_MAXO must be even and fill whole passes of the x image"
#endif

__global__ __launch_bounds__(2 * LZ_GRAD_H) void LZ_GRAD_KERNEL(GradArgs a) {
  constexpr int kH = LZ_GRAD_H;         // hidden units (hides grad::kH)
  constexpr int kLogH = kH == 128 ? 7 : 6;
  constexpr int kW2Ld = kH + 1;         // row stride of the W2 image
  constexpr int kWaves = kH / 32;       // wave w owns units 32 w .. 32 w + 31
  constexpr int kThreads = 2 * kH;      // = 64 kWaves
  constexpr int kMO = LZ_GRAD_MAXO;     // widest input (the x and W1 images, accS)
  // row stride of the W1 image: 8 as it always was; the wide form an odd one as W2's (24
  // words would put the 32 rows of a column read on 8 banks)
  constexpr int kW1Ld = kMO == 8 ? 8 : kMO + 1;
  __shared__ float sW2[kH * kW2Ld];
  __shared__ float sW1[kH * kW1Ld];
  __shared__ float sB1[kH], sB2[kH];
  __shared__ float sWh[kMaxA * kH];
  __shared__ float sX[kMO * kTile];
  __shared__ float sH1[kH * kLd], sH2[kH * kLd], sD2[kH * kLd], sD1[kH * kLd];
  __shared__ float sHP[kWaves * kMaxA * kTile];
  __shared__ float sDO[kMaxA * kTile];
  constexpr int kRedLd = kLaneSums + 2 * kMaxA;
  __shared__ double sRed[kTile * kRedLd];

#if LZ_GRAD_PPO
  // SB3's early stop: nothing is computed for a minibatch after the stop (uniform)
  if (a.ctrl && a.ctrl[1] != 0) return;
#endif

  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const bool pi = (blockIdx.x & 1u) == 0;
  const int wg = (int)(blockIdx.x >> 1), nwg = (int)(gridDim.x >> 1);
  const int O = a.O, A = a.A, NH = pi ? A : 1;
  const Layout L = layout(O, A, kH);
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

  for (int e = tid; e < kH * kH; e += kThreads) sW2[(e >> kLogH) * kW2Ld + (e & (kH - 1))] = gW2[e];
  for (int e = tid; e < kH * kMO; e += kThreads) {
    const int u = kMO == 8 ? e >> 3 : e / kMO, k = kMO == 8 ? e & 7 : e % kMO;
    sW1[kMO == 8 ? e : u * kW1Ld + k] = k < O ? gW1[u * O + k] : 0.0f;
  }
  for (int e = tid; e < kH; e += kThreads) {
    sB1[e] = gB1[e];
    sB2[e] = gB2[e];
  }
  for (int e = tid; e < kMaxA * kH; e += kThreads) sWh[e] = e < NH * kH ? gWh[e] : 0.0f;
  for (int e = tid; e < kMaxA * kTile; e += kThreads) sDO[e] = 0.0f;
  float bh[kMaxA], ls[kMaxA], inv_var[kMaxA];
#pragma unroll
  for (int j = 0; j < kMaxA; ++j) {
    bh[j] = j < NH ? gBh[j] : 0.0f;
    ls[j] = (pi && j < A) ? gLs[j] : 0.0f;
    const float sd = expf(ls[j]);
    inv_var[j] = 1.0f / (sd * sd);
  }
#if LZ_GRAD_PPO
  // torch forms (adv - mean) / (std + 1e-8) on float32 tensors
  const bool norm = a.moments != nullptr;
  const float adv_mean = norm ? (float)a.moments[0] : 0.0f;
  const float adv_den = norm ? (float)a.moments[1] + 1e-8f : 1.0f;
#endif
  __syncthreads();

  v16 accW2[kWaves];
#pragma unroll
  for (int t = 0; t < kWaves; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) accW2[t][g] = 0.0f;
  float accS[kMO + 1];
#pragma unroll
  for (int i = 0; i < kMO + 1; ++i) accS[i] = 0.0f;
#if LZ_GRAD_PPO
  double lossS = 0.0, entS = 0.0, klS = 0.0, cntS = 0.0, clipS = 0.0, dbh[kMaxA], dls[kMaxA];
#else
  double lossS = 0.0, entS = 0.0, cntS = 0.0, dbh[kMaxA], dls[kMaxA];
#endif
#pragma unroll
  for (int j = 0; j < kMaxA; ++j) dbh[j] = dls[j] = 0.0;

  double* slot = a.part + (int64_t)wg * (P + kTail);
  bool first = true;
  int since = 0;

  // the workgroup's float32 accumulators into its float64 slot, then zeroed
  auto flush = [&]() __attribute__((always_inline)) {
    double* pW2 = slot + oW2;
#pragma unroll
    for (int t = 0; t < kWaves; ++t)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        put(pW2 + (32 * w + acc_row(g, h)) * kH + 32 * t + r, accW2[t][g], first);
        accW2[t][g] = 0.0f;
        // eight read-modify-writes in flight at a time, not all 64 (registers)
        if ((g & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
    if (tid < kH) {
#pragma unroll
      for (int o = 0; o < kMO; ++o)
        if (o < O) put(slot + oW1 + tid * O + o, accS[o], first);
      put(slot + oB1 + tid, accS[kMO], first);
    } else {
      const int u = tid - kH;
      put(slot + oB2 + u, accS[kMO], first);
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < NH) put(slot + oWh + j * kH + u, accS[j], first);
    }
#pragma unroll
    for (int i = 0; i < kMO + 1; ++i) accS[i] = 0.0f;
    first = false;
    since = 0;
  };

  const int64_t ntiles = (a.n + kTile - 1) / kTile;
  for (int64_t tile = wg; tile < ntiles; tile += nwg) {
    const int64_t base = tile * kTile;
#if LZ_GRAD_PPO
    // sample r of the tile (tid & 31 == r): its row of the flat arrays.  `valid`: a row that
    // may be read; `bad`: a sample whose index lies outside the arrays
    const int64_t si = base + r;
    int64_t row = si;
    if (a.idx && si < a.n) row = (int64_t)a.idx[si];
    const bool valid = si < a.n && row >= 0 && row < a.n_rows;
    const bool bad = si < a.n && !valid;
    // x as [k][sample]; rows k >= O and samples that are not read are 0 (kThreads / 32 rows
    // a pass: one pass with 256 threads, two with 128)
#pragma unroll
    for (int k0 = 0; k0 < kMO; k0 += kThreads / 32) {
      const int k = k0 + (tid >> 5);
      sX[k * kTile + r] = (k < O && valid) ? a.obs[row * O + k] : 0.0f;
    }
#else
    // x as [k][sample]; rows k >= O and samples past the end are 0 (kThreads / 32 rows a
    // pass: one pass with 256 threads, two with 128)
#pragma unroll
    for (int k0 = 0; k0 < kMO; k0 += kThreads / 32) {
      const int k = k0 + (tid >> 5), s = tid & 31;
      const int64_t i = base + s;
      sX[k * kTile + s] = (k < O && i < a.n) ? a.obs[i * O + k] : 0.0f;
    }
    const int64_t si = base + r;
    const bool valid = si < a.n;
#endif
    __syncthreads();

    // layer 1
    v16 c, h1, h2;
#pragma unroll
    for (int g = 0; g < 16; ++g) c[g] = sB1[32 * w + acc_row(g, h)];
#pragma unroll
    for (int st = 0; st < kMO / 2; ++st)
      c = mfma(sW1[(32 * w + r) * kW1Ld + 2 * st + h], sX[(2 * st + h) * kTile + r], c);
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
        if (j < NH) {  // the waves' partials in wave order, then the bias
          float p = sHP[(0 * kMaxA + j) * kTile + r];
#pragma unroll
          for (int ww = 1; ww < kWaves; ++ww) p += sHP[(ww * kMaxA + j) * kTile + r];
          out[j] = p + bh[j];
        }
        dout[j] = 0.0f;
      }
      // wave 0's lower half keeps the float64 sums (PPO tells `valid` from `bad` per sum)
      const bool own = (LZ_GRAD_PPO || valid) && w == 0 && h == 0;
      if (pi) {
#if LZ_GRAD_PPO
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
#else
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
#endif
      } else {
#if LZ_GRAD_PPO
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
#else
        const float ret = valid ? a.ret[si] : 0.0f;
        const float e = ret - out[0];
        dout[0] = valid ? -2.0f * a.vf_coef * e : 0.0f;
        if (own) {
          dbh[0] += (double)dout[0];
          lossS += (double)(e * e);
        }
#endif
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
      for (int t = 0; t < kWaves; ++t) accW2[t] = mfma(av, sH1[(32 * t + r) * kLd + 2 * st + h], accW2[t]);
    }
    __syncthreads();

    // the sample sums of the small tensors, one thread per unit
    if (tid < kH) {  // dW1 row and db1 of unit tid
#pragma unroll 4
      for (int s = 0; s < kTile; ++s) {
        const float d = sD1[tid * kLd + s];
        accS[kMO] += d;
#pragma unroll
        for (int o = 0; o < kMO; ++o) accS[o] = fmaf(d, sX[o * kTile + s], accS[o]);
      }
    } else {  // db2 and the head rows' column of unit tid - kH
      const int u = tid - kH;
#pragma unroll 4
      for (int s = 0; s < kTile; ++s) {
        accS[kMO] += sD2[u * kLd + s];
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
  if (w == 0 && h == 0) {
    double* p = sRed + r * kRedLd;
    p[0] = lossS;
    p[1] = entS;
#if LZ_GRAD_PPO
    p[2] = klS;
#endif
#pragma unroll
    for (int j = 0; j < kMaxA; ++j) {
      p[kLaneSums + j] = dbh[j];
      p[kLaneSums + kMaxA + j] = dls[j];
    }
  }
  // the counts are exact in any order
  double cnt = cntS;
#if LZ_GRAD_PPO
  double ncl = clipS;
#endif
  if (w == 0) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
      cnt += __shfl_xor(cnt, m, 64);
#if LZ_GRAD_PPO
      ncl += __shfl_xor(ncl, m, 64);
#endif
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
      if (j < NH) slot[oBh + j] = t[kLaneSums + j];
    if (pi) {
#pragma unroll
      for (int j = 0; j < kMaxA; ++j)
        if (j < A) slot[oLs + j] = t[kLaneSums + kMaxA + j];
      slot[P + 0] = t[0];
      slot[P + 2] = t[1];
      slot[P + 3] = cnt;
#if LZ_GRAD_PPO
      slot[P + 4] = ncl;
      slot[P + 5] = t[2];
#endif
    } else {
      slot[P + 1] = t[0];
    }
  }
}
#ifdef LZ_GRAD_MAXO_DEFAULTED
#undef LZ_GRAD_MAXO
#undef LZ_GRAD_MAXO_DEFAULTED
#endif
