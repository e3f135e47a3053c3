// The two evaluation kernels (lz_policy.hip includes this file inside namespace lz, twice):
// with LZ_EVAL_TRACE 0 it defines k_evaluate_policy_f32 / k_evaluate_policy_attn_f32, with
// LZ_EVAL_TRACE 1 their traced forms k_evaluate_policy_f32_trace / k_evaluate_policy_attn_
// f32_trace, which take the trace (TArgs) as a fourth kernel parameter.  One text, so the
// two forms cannot drift apart -- and the preprocessor, not a template parameter, picks
// the form, because the untraced kernels must keep their names and their machine code (a
// PMC figure or an A/B number recorded for a kernel is tied to its code hash,
// tools/kernel_hash.py): an extra template parameter renames them, and the same body as an
// inlined function template instantiated both ways changed the register allocation of all
// seventeen of them.
#ifndef LZ_EVAL_TRACE
#error "lz_eval_kernels.inc: define LZ_EVAL_TRACE to 0 or 1"
#endif

// The float32 MlpPolicy (kF32* blob): one wave per 32-env tile as k_rollout_policy's
// kMlpF32 path, the pi net, the Normal constants and the tanh table alone in LDS (75 KB
// of the blob's 148).
template <class Sys, int W>
#if LZ_EVAL_TRACE
__global__ __launch_bounds__(W * 64) void k_evaluate_policy_f32_trace(KArgs a, PArgs p, EArgs ev, TArgs tr) {
#else
__global__ __launch_bounds__(W * 64) void k_evaluate_policy_f32(KArgs a, PArgs p, EArgs ev) {
#endif
  constexpr int E = 32;
  constexpr int O = Sys::O, A = Sys::A, ED = O / 2;
  constexpr int kCst = 64 + kTanhSegs * 32;
  static_assert(O <= kPolMaxObs && A <= kPolMaxAct && ED <= 4, "policy tile shape");
  static_assert(kF32Net % 16 == 0 && kF32LogStd % 16 == 0 && kCst % 16 == 0 && kF32Tag + 16 <= kF32Net,
                "16-B pieces");
  __shared__ __attribute__((aligned(64))) uint8_t s_net[kF32Net];
  __shared__ __attribute__((aligned(16))) uint8_t s_cst[kCst];
  __shared__ double s_norm[2 * kPolMaxObs];
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int slot = lane & 31;
  const bool owner = h == 0;
  const bool bad = !blob_is(p.blob, kF32Tag, LZ_BLOB_MLP_F32);
  blob_to_lds(reinterpret_cast<f4v*>(s_net), reinterpret_cast<const f4v*>(p.blob), kF32Net / 16, tid,
              W * 64, bad);
  blob_to_lds(reinterpret_cast<f4v*>(s_cst), reinterpret_cast<const f4v*>(p.blob + kF32LogStd), kCst / 16,
              tid, W * 64, bad);
  const uint64_t tick = pol_prologue<O>(a, p, s_norm, tid);
  __syncthreads();
  const float* g_scale = reinterpret_cast<const float*>(s_cst) + 4;
  const float* ttab = reinterpret_cast<const float*>(s_cst + 64);
  const bool norm = p.norm != nullptr;
  const double* mu = s_norm;
  const double* sd = s_norm + kPolMaxObs;
  const bool det = (p.pflags & LZ_POLICY_DETERMINISTIC) != 0;
  const bool autoreset = (a.flags & LZ_FLAG_AUTORESET) != 0;
  Sys sys;
  sys.setup(a);
  const int64_t ntiles = (a.n + E - 1) / E;
  for (int64_t tile = (int64_t)blockIdx.x * W + wave; tile < ntiles; tile += (int64_t)gridDim.x * W) {
    const int64_t i = tile * E + slot;
    const bool live = owner && i < a.n;
    int32_t steps;
    bool any_reset = false;
    double q[4][4];  // this tile's accumulators: zeroed per grid-stride tile
    EvalCount c;
    eval_zero<4>(q, c);
    float o[O];
    tile_open(sys, a, p, i, live, steps, o);
#if LZ_EVAL_TRACE
    TraceCursor tc;  // the owner lane stores the env's rows
    tc.open(tr, i, live);
#endif
    for (int k = 0; k < a.K; ++k) {
      float x[O];
      normalize<O>(o, x, norm, mu, sd, p.clip);
      float mean[A];
      float xs[(O + 1) / 2];
      f32_inputs<O, (O + 1) / 2>(x, lane, xs);
      mlp_f32<(O + 1) / 2, A>(s_net, xs, lane, mean, ttab);
      float act_c[A];
      if (live) {
        float act[A];
        policy_sample<A, false>(a, p, i, tick + (uint64_t)k, det, mean, g_scale, act, act_c);
      }
      float on[O], ot[O];
      float rew = 0.0f;
      bool did_reset;
      const uint8_t df = step_body<Sys, float, true, true>(sys, steps, a, i, live, act_c,
                                                           tick + (uint64_t)k, k, on, rew, did_reset, ot);
      any_reset = any_reset || did_reset;
      if (live) eval_step<4, ED>(q, c, 0, ot, rew, df, k, autoreset, ev.skip, ev.max_episodes);
#if LZ_EVAL_TRACE
      tc.step(tr, sys, k, ot, act_c, rew, df, bad);
#endif
#pragma unroll
      for (int j = 0; j < O; ++j) o[j] = on[j];
    }
    tile_close(sys, a, p, i, live, steps, any_reset, o);
    if (live) eval_store<4>(ev.stats, a.n, i, q, c, 0, true, bad);
  }
}

// The float32 attention actor-critics (kAF* blob; kLn: the residual + LayerNorm extractor
// on an S-frame VecFrameStack): 16-env waves as k_rollout_policy_attn_f32.  There is one
// net to run, so the pi net is DMA'd into the slot once per launch and stays: the step
// loop has no barrier and no slot swap.  The stack lives distributed over the lane groups
// and follows the rollout's order exactly (the zeroing of a done env's older frames is
// applied when the next input is formed).
template <class Sys, bool kLn, int S, int W>
#if LZ_EVAL_TRACE
__global__ __launch_bounds__(W * 64) void k_evaluate_policy_attn_f32_trace(KArgs a, PArgs p, EArgs ev,
                                                                           TArgs tr) {
#else
__global__ __launch_bounds__(W * 64) void k_evaluate_policy_attn_f32(KArgs a, PArgs p, EArgs ev) {
#endif
  constexpr int E = 16;
  constexpr int O = Sys::O, A = Sys::A, ED = O / 2;
  using Stack = AttnStack<O, S>;
  constexpr int SO = Stack::SO, KS = Stack::KS;
  static_assert(kLn || S == 1, "frame stacking is the LayerNorm variant's");
  static_assert(SO <= kAFMaxIn && O <= kPolMaxObs && A <= kPolMaxAct && ED <= 4, "policy tile shape");
  __shared__ __attribute__((aligned(16))) uint8_t s_lds[kAFLdsBytes];
  __shared__ double s_norm[2 * kPolMaxObs];
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, G = lane >> 4, col = lane & 15;
  const bool bad = !blob_is(p.blob, kAFTag, kLn ? LZ_BLOB_ATTN_LN_F32 : LZ_BLOB_ATTN_F32);
  blob_to_lds(reinterpret_cast<f4v*>(s_lds), reinterpret_cast<const f4v*>(p.blob), kAFExt / 16, tid, W * 64,
              bad);
  blob_to_lds(reinterpret_cast<f4v*>(s_lds + kAFExt), reinterpret_cast<const f4v*>(p.blob + kAFLogStd),
              kAFConst / 16, tid, W * 64, bad);
  const uint64_t tick = pol_prologue<O>(a, p, s_norm, tid);
  const uint8_t* s_ext = s_lds;
  const float* cst = reinterpret_cast<const float*>(s_lds + kAFExt);
  const float* g_scale = cst + 4;
  const float* ttab = cst + 16;
  const uint8_t* s_net = s_lds + kAFExt + kAFConst;
  net_dma<W>(p.blob + kAFPi, s_net, wave, lane);  // the pi net into the slot, once
  __builtin_amdgcn_s_waitcnt(0x0F70);  // this wave's DMA pieces have landed
  __syncthreads();
  const bool norm = p.norm != nullptr;
  const double* mu = s_norm;
  const double* sd = s_norm + kPolMaxObs;
  const bool det = (p.pflags & LZ_POLICY_DETERMINISTIC) != 0;
  const bool autoreset = (a.flags & LZ_FLAG_AUTORESET) != 0;
  Sys sys;
  sys.setup(a);
  const int64_t ntiles = (a.n + E - 1) / E;
  const Stack stk = {G, col};
  for (int64_t tile = (int64_t)blockIdx.x * W + wave; tile < ntiles; tile += (int64_t)gridDim.x * W) {
    const int64_t i = tile * E + col;
    const bool valid = i < a.n;        // all four lanes of the env compute it
    const bool own = valid && G == 0;  // ... lane group 0 stores it
    int32_t steps;
    bool any_reset = false;
    double q[1][4];  // lane group G's part of this tile's accumulators, zeroed per tile
    EvalCount c;
    eval_zero<1>(q, c);
    float o[O], st[kLn ? KS : 1];
    bool zf = false;
    // tile_open written out: called, the HR instance of this kernel measured 0.27 % slower
    // (five alternating rounds against the previous code, its spread 0.22 %); with this
    // block in place and every other shared step called, -0.02 %
    steps = 0;
#pragma unroll
    for (int j = 0; j < O; ++j) o[j] = 0.0f;
    if (valid) {
      sys.load(a, i);
      if (a.count_steps) steps = static_cast<const int32_t*>(a.pl[Sys::kStepPlane])[i];
#pragma unroll
      for (int j = 0; j < O; ++j) o[j] = p.obs_in[i * O + j];
    }
    if constexpr (kLn) stk.load(p.stack_in, i, valid, st);
#if LZ_EVAL_TRACE
    TraceCursor tc;  // the four lanes of an env all compute the row, lane group 0 stores it
    tc.open(tr, i, own);
#endif
    for (int k = 0; k < a.K; ++k) {
      f32x4 F[4];
      float xs[KS];
      if constexpr (kLn) {
        stk.cur_stack(st, zf, xs);
      } else {
        float x[O];
        normalize<O>(o, x, norm, mu, sd, p.clip);
        stk.inputs(x, xs);
      }
      attn16_extract<KS, kLn>(s_ext, xs, lane, F);
      float mean[A];
      attn16_net<A>(s_net, F, lane, mean, ttab);
      float act_c[A];
#pragma unroll
      for (int j = 0; j < A; ++j) act_c[j] = 0.0f;
      if (valid) {  // every lane of the env: the same Philox draw
        float act[A];
        policy_sample<A, false>(a, p, i, tick + (uint64_t)k, det, mean, g_scale, act, act_c);
      }
      // the deferred zeroing of a done env's older frames
      if constexpr (kLn) stk.cur_stack(st, zf, st);
      float on[O], ot[O];
      float rew = 0.0f;
      bool did_reset;
      const uint8_t df = step_body<Sys, float, true, true>(sys, steps, a, i, valid, act_c,
                                                           tick + (uint64_t)k, k, on, rew, did_reset, ot,
                                                           G == 0);
      any_reset = any_reset || did_reset;
      if (valid) eval_step<1, ED>(q, c, G, ot, rew, df, k, autoreset, ev.skip, ev.max_episodes);
#if LZ_EVAL_TRACE
      tc.step(tr, sys, k, ot, act_c, rew, df, bad);
#endif
      if constexpr (kLn) {
        stk.roll_stack(st, on);
        zf = df != 0;
      }
#pragma unroll
      for (int j = 0; j < O; ++j) o[j] = on[j];
    }
    tile_close(sys, a, p, i, own, steps, any_reset, o);
    if (valid) {
      eval_store<1>(ev.stats, a.n, i, q, c, G, G == 0, bad);
      if constexpr (kLn) {
        float xs[KS];
        stk.cur_stack(st, zf, xs);
        stk.store(p.stack_out, i, xs);
      }
    }
  }
}
