"""GPU tests of the evaluation trace (lz_evaluate_policy_*_f32_trace, FusedEvaluator.evaluate
(..., trace=ids) -> EvalTrace).  Every comparison is bit for bit (NaN equal to NaN) against
tests/trace_ref.py fed

  * the per-step outputs of the rollout collector on a twin handle with the same seed
    (test_gpu_eval._transitive's construction: terminal-substituted observations, rewards,
    done bytes, clip(actions, low, high)), gathered at the traced ids and recorded steps;
  * for the state columns a third handle stepped K times by lz_step with those clipped
    actions, lz_get_state read after each step;
  * the oracle closed loop of the reference's eight PMSM policies, and the reference's own
    cpu_e traces at the bounds of test_policy_f32_host.test_f2_free_running_vs_reference.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_eval as tge
import trace_ref as tr
from test_policy_f32_host import GOLD, normalize_obs

pytestmark = pytest.mark.gpu

_np, _teq = tge._np, tge._teq


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


@pytest.fixture(scope="module")
def pol():
    from gym_lorenz import policy

    return policy


@pytest.fixture(scope="module")
def nat():
    from gym_lorenz import _native

    return _native


def _sd(pol, system, attention=False, ln=False, stack=1, seed=7):
    O, A, _ = tr.DIMS[system]
    if attention or ln:
        return tge._attn(pol, O * stack, A, seed=seed, ln=ln)
    return tge._mlp(pol, O, A, seed=seed)


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:5].tolist()


def _traced_vs_collector(gl, pol, system, n, K, ids, sd, kw, det=True, frame_stack=1, start=0, every=1,
                         state=True):
    """One traced launch against the collector twin (and the lz_step twin for the state):
    returns (EvalResult, the reference trace)."""
    O, A, S = tr.DIMS[system]
    ea = gl.BatchedEnv(system, n, seed=11, **kw)
    eb = gl.BatchedEnv(system, n, seed=11, **kw)
    ev = pol.FusedEvaluator(ea, sd, deterministic=det, frame_stack=frame_stack)
    col = pol.FusedRolloutCollector(eb, sd, bootstrap=False, deterministic=det, capture_terminal=K * n,
                                    frame_stack=frame_stack, precision="fp32")
    ev.reset()
    col.reset()
    res = ev.evaluate(K, skip=2, trace=ids, trace_every=every, trace_start=start, trace_state=state)
    b = col.collect(K)
    o, r, d = tge._steps_of_batch(b, n, O)
    lo, hi = pol.action_bounds(system)
    a = np.clip(_np(b.actions), np.float32(lo), np.float32(hi))
    st = None
    if state:
        ec = gl.BatchedEnv(system, n, seed=11, **kw)
        ec.reset()
        st = np.zeros((K, n, S), np.float32)
        for k in range(K):
            ec.step(torch.from_numpy(a[k]))
            for j in range(S):
                st[k, ids, j] = _np(ec.get_state(j, indices=ids))
        ec.close()
    want = tr.trace_ref(o, a, r, d, ids, start, every, state=st)
    t = res.trace
    got = _np(t.data)
    T, C = tr.shape(system, K, start, every, tr.TRACE_STATE if state else 0)
    assert got.shape == want.shape == (T, len(ids), C)
    assert _teq(got, want), _diff(got, want)
    ks = tr.recorded_steps(K, start, every)
    assert _np(t.steps).tolist() == ks.tolist() and _np(t.env_ids).tolist() == list(ids)
    assert _teq(_np(t.obs), o[ks][:, ids]) and _teq(_np(t.actions), a[ks][:, ids])
    assert _teq(_np(t.rewards), r[ks][:, ids]) and np.array_equal(_np(t.dones), d[ks][:, ids])
    assert (t.state is None) if not state else _teq(_np(t.state), st[ks][:, ids])
    # the table of the same launch is the untraced semantics' (skip = 2)
    T_ref = tge.er.eval_ref(o, r, d, kw.get("autoreset", True), 2, 0, tge.er.ERR_DIMS[system])
    assert _teq(_np(res.stats), T_ref)
    assert _teq(_np(ev.last_obs), _np(b.last_obs))
    ea.close()
    eb.close()
    return res, want, d


MLP_IDS = [0, 31, 32, 63, 64, 69]     # n = 70: two 32-env tiles plus a ragged 6
ATTN_IDS = [0, 15, 16, 31, 32, 36]    # n = 37: two 16-env tiles plus a ragged 5


@pytest.mark.parametrize("system,kw,K,det,start,every,state", [
    ("pmsm", dict(add_noise=True, max_episode_steps=5), 12, True, 0, 1, True),
    ("pmsm", dict(add_noise=True, max_episode_steps=5), 12, False, 0, 1, True),
    ("lorenz4", dict(max_episode_steps=3), 7, True, 2, 3, True),
    ("lorenz4", dict(max_episode_steps=3), 7, True, 2, 3, False),
    ("hr", dict(add_noise=True, add_filter=True, autoreset=False), 12, False, 0, 1, True),
])
def test_mlp_trace_equals_collector(gl, pol, system, kw, K, det, start, every, state):
    res, want, d = _traced_vs_collector(gl, pol, system, 70, K, MLP_IDS, _sd(pol, system), kw, det=det,
                                        start=start, every=every, state=state)
    if kw.get("max_episode_steps"):  # done steps (terminal observation, post-reset state) were traced
        assert (d[tr.recorded_steps(K, start, every)][:, MLP_IDS] != 0).any()
    if system == "lorenz4":
        assert want.shape[0] == 2  # steps 2 and 5


@pytest.mark.parametrize("system,kw,n,K,ln,stack", [
    ("hr", dict(max_episode_steps=5), 37, 12, False, 1),
    ("pmsm", dict(), 17, 10, False, 1),
    ("hr", dict(max_episode_steps=5), 37, 12, True, 4),      # lorenz_filter: LayerNorm + VecFrameStack(4)
    ("lorenz3", dict(max_episode_steps=2), 17, 5, True, 1),
])
def test_attention_trace_equals_collector(gl, pol, system, kw, n, K, ln, stack):
    ids = ATTN_IDS if n == 37 else [0, 15, 16]
    sd = _sd(pol, system, attention=True, ln=ln, stack=stack, seed=4)
    res, want, d = _traced_vs_collector(gl, pol, system, n, K, ids, sd, kw, frame_stack=stack)
    assert res.trace.obs.shape[2] == 6  # the raw frame, not the stack
    if kw.get("max_episode_steps"):
        assert (d[:, ids] != 0).any()


@pytest.mark.parametrize("attention", [False, True])
def test_grid_stride_tiles_find_their_slots(gl, pol, nat, attention):
    """More tiles than grid x waves: a wave opens a second tile and reads that tile's slots."""
    n = 32787
    probe = gl.BatchedEnv("lorenz3", n, seed=11, max_episode_steps=2)
    sh = nat.launch_shape(probe._h, nat.CALL_EVALUATE_POLICY_ATTN_F32 if attention
                          else nat.CALL_EVALUATE_POLICY_F32)
    probe.close()
    epw, first_pass = sh["envs_per_wave"], sh["grid"] * sh["waves"]
    tiles = -(-n // epw)
    assert tiles > first_pass and sh["grid_stride"]
    ids = [3 * epw + 5, first_pass * epw + 7, n - 1]  # a first-pass tile, a later tile, the last env
    assert ids[0] // epw < first_pass <= ids[1] // epw and ids[1] < n - 1
    sd = _sd(pol, "lorenz3", attention=attention, seed=3)
    _traced_vs_collector(gl, pol, "lorenz3", n, 3, ids, sd, dict(max_episode_steps=2))


def test_every_env_traced_in_reverse(gl, pol):
    """M = N: slot m holds env 69 - m."""
    n = 70
    ids = list(range(n - 1, -1, -1))
    res, want, _ = _traced_vs_collector(gl, pol, "pmsm", n, 6, ids, _sd(pol, "pmsm"),
                                        dict(add_noise=True, max_episode_steps=5))
    assert _np(res.trace.env_ids).tolist() == ids
    fwd = _np(res.trace.data)[:, ::-1]  # env order
    assert _teq(fwd, want[:, ::-1]) and not _teq(fwd[:, 0], fwd[:, 1])


@pytest.mark.parametrize("system,kw,n,attention", [
    ("pmsm", dict(add_noise=True, max_episode_steps=5), 70, False),
    ("hr", dict(max_episode_steps=5), 37, True),
])
def test_trace_moves_nothing_else(gl, pol, system, kw, n, attention):
    """Twin handles, one launch traced and one not: the same table, planes and last_obs,
    and a following collect(2) on both agrees (tick and call parity advanced alike)."""
    sd = _sd(pol, system, attention=attention)
    ea = gl.BatchedEnv(system, n, seed=11, **kw)
    eb = gl.BatchedEnv(system, n, seed=11, **kw)
    eva, evb = pol.FusedEvaluator(ea, sd, deterministic=False), pol.FusedEvaluator(eb, sd, deterministic=False)
    eva.reset()
    evb.reset()
    ra = eva.evaluate(12, skip=2, max_episodes=2, trace=[0, n - 1], trace_every=5, trace_state=True)
    rb = evb.evaluate(12, skip=2, max_episodes=2)
    assert rb.trace is None and ra.trace.data.shape[:2] == (3, 2)
    assert _teq(_np(ra.stats), _np(rb.stats))
    assert _teq(_np(eva.last_obs), _np(evb.last_obs))
    for pa, pb in zip(tge._planes(ea), tge._planes(eb)):
        assert _teq(pa, pb)
    ck = dict(bootstrap=False, deterministic=False, capture_terminal=2 * n, precision="fp32")
    ca, cb = pol.FusedRolloutCollector(ea, sd, **ck), pol.FusedRolloutCollector(eb, sd, **ck)
    ca.last_obs, cb.last_obs = eva.last_obs, evb.last_obs
    ca.last_stack, cb.last_stack = eva.last_stack, evb.last_stack
    b1, b2 = ca.collect(2), cb.collect(2)
    for f in ("observations", "actions", "log_probs", "values", "rewards", "dones", "last_obs"):
        assert _teq(_np(getattr(b1, f)), _np(getattr(b2, f))), f
    ea.close()
    eb.close()


@pytest.mark.parametrize("j", range(8))
def test_reference_pmsm_policies_error_curves(gl, pol, orc, nat, j):
    """code/lorenz_pmsm/test_evaluate.py:113-134: the state1 - state2 columns of its sheet
    from one traced launch per policy.  The reference's fixed initial state sits in env 33
    of a 40-env handle.  Observation rows == the oracle closed loop's bit for bit; errors()
    against the reference's own run (cpu_e) at the bounds the oracle loop is held to
    (test_f2_free_running_vs_reference: max |de| <= 5e-4, steady RMS within 1e-4)."""
    from gym_lorenz.vec_normalize import DeviceRunningMeanStd

    gold = np.load(GOLD)
    K, n, env_id = 1999, 40, 33
    alpha = float(gold["alphas"][j])
    sd = {k: torch.from_numpy(gold["a%d/%s" % (j, k)]) for k in orc.POLICY_KEYS + ("log_std",)}
    env = gl.BatchedEnv("pmsm", n, seed=0, alpha=alpha, add_noise=False)
    rms = DeviceRunningMeanStd(6, env.device)
    rms.set_state(gold["a%d/obs_rms.mean" % j], gold["a%d/obs_rms.var" % j],
                  float(gold["a%d/obs_rms.count" % j]))
    ev = pol.FusedEvaluator(env, sd, obs_rms=rms, clip_obs=float(gold["a%d/clip_obs" % j]),
                            norm_eps=float(gold["a%d/epsilon" % j]))
    ev.reset()
    s1, s2 = gold["init_state1"], gold["init_state2"]
    for i in range(3):
        env.set_state(nat.PMSM_S1 + i, [s1[i]], indices=[env_id])
        env.set_state(nat.PMSM_S2 + i, [s2[i]], indices=[env_id])
    S = orc.PmsmState(1)
    S.st[0, :3], S.st[0, 3:] = s1, s2
    raw = orc.pmsm_reset_obs(S.st)
    ev.last_obs[env_id] = torch.from_numpy(raw[0]).to(env.device)
    res = ev.evaluate(K, skip=1000, trace=[env_id])
    psd = {k: gold["a%d/%s" % (j, k)] for k in orc.POLICY_KEYS}
    os_ = []
    for _ in range(K):
        m, _ = orc.mlp_f32(psd, normalize_obs(gold, j, raw))
        raw, r, te, trc = orc.pmsm_step(S, np.clip(m, np.float32(-1), np.float32(1)), None, False,
                                        alpha, orc.DEV)
        os_.append(raw[0].copy())
    t = res.trace
    assert t.obs.shape == (K, 1, 6) and _teq(_np(t.obs)[:, 0], np.array(os_))
    e = _np(t.errors())[:, 0]
    ref = gold["cpu_e"][j][:K]
    dmax = np.abs(e - ref).max()
    rms_e, rms_ref = (np.sqrt(np.mean(v[999:1999].astype(np.float64) ** 2)) for v in (e, ref))
    print("alpha=%.3f: max |de| %.2e, steady RMS %.5f vs %.5f" % (alpha, dmax, rms_e, rms_ref))
    assert dmax <= 5e-4
    assert abs(rms_e - rms_ref) <= 1e-4 * rms_ref
    env.close()


def test_wrong_blob_gives_nan_trace(gl, pol):
    env = gl.BatchedEnv("pmsm", 300, seed=3)
    sd = tge._mlp(pol, 6, 2, seed=2)
    ev = pol.FusedEvaluator(env, sd)
    ev.reset()
    good = ev.evaluate(4, trace=[0, 299], trace_state=True)
    assert np.isfinite(_np(good.trace.data)).all() and np.isfinite(_np(good.stats)).all()
    ev.blob = torch.from_numpy(pol.pack_policy_i8x4(sd, 6, 2)).to(env.device)  # behind the host check
    bad = ev.evaluate(4, trace=[0, 299], trace_state=True)
    assert np.isnan(_np(bad.trace.data)).all() and np.isnan(_np(bad.stats)).all()
    env.close()


def test_traced_launch_is_graph_capturable(gl, pol, nat):
    """A traced launch allocates nothing (the slot map is the caller's): two of them (an
    even number of calls, the header's hipGraph note) captured and replayed once write what
    the same two calls write eagerly on a twin handle."""
    n, K, ids = 70, 6, [69, 0, 33]
    sd = tge._mlp(pol, 6, 2, seed=7)
    kw = dict(add_noise=True, max_episode_steps=5)

    def setup():
        env = gl.BatchedEnv("pmsm", n, seed=11, **kw)
        ev = pol.FusedEvaluator(env, sd, deterministic=False)
        ev.reset()
        dev = env.device
        buf = dict(obs=[ev.last_obs.clone(), torch.zeros((n, 6), device=dev)],
                   stats=[torch.zeros((nat.EVAL_COLS, n), dtype=torch.float64, device=dev) for _ in range(2)],
                   out=[torch.zeros((K, 3, 16), device=dev) for _ in range(2)],
                   ids=torch.tensor(ids, dtype=torch.int64, device=dev),
                   slots=torch.zeros((n,), dtype=torch.int32, device=dev))
        calls = []
        for c in range(2):
            e = nat.LzPolicyEvalArgs()
            e.K, e.flags = K, 0
            e.blob, e.obs_in, e.obs_last = ev.blob.data_ptr(), buf["obs"][c].data_ptr(), buf["obs"][1 - c].data_ptr()
            e.norm_eps, e.clip_obs, e.act_low, e.act_high = 1e-8, 10.0, ev.act_low, ev.act_high
            e.skip, e.stats = 1, buf["stats"][c].data_ptr()
            t = nat.LzEvalTrace()
            t.ids, t.count, t.slot_map = buf["ids"].data_ptr(), 3, buf["slots"].data_ptr()
            t.start, t.every, t.flags = 0, 1, nat.TRACE_STATE
            t.out, t.out_capacity_bytes = buf["out"][c].data_ptr(), K * 3 * 16 * 4
            calls.append((e, t))
        return env, ev, buf, calls

    def launch(env, calls):
        for e, t in calls:
            nat.check(nat.lib.lz_evaluate_policy_f32_trace(env._h, ctypes.byref(e), ctypes.byref(t)))

    ea, eva, ba, ca = setup()
    launch(ea, ca)  # eager (and the kernels' code is loaded before the capture below)
    torch.cuda.synchronize()
    eb, evb, bb, cb = setup()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    nat.check(nat.lib.lz_set_stream(eb._h, ctypes.c_void_p(s.cuda_stream)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(eb, cb)
    torch.cuda.synchronize()
    assert not _np(bb["out"][0]).any()  # captured, not run
    with torch.cuda.stream(s):
        g.replay()
    torch.cuda.synchronize()
    for k in ("out", "stats", "obs"):
        for c in range(2):
            assert _teq(_np(ba[k][c]), _np(bb[k][c])), (k, c)
    assert _np(ba["out"][1]).any() and not _teq(_np(ba["out"][0]), _np(ba["out"][1]))
    nat.check(nat.lib.lz_set_stream(eb._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for pa, pb in zip(tge._planes(ea), tge._planes(eb)):
        assert _teq(pa, pb)
    ea.close()
    eb.close()


def test_trace_refusals(gl, pol, nat):
    n, K = 64, 6
    env = gl.BatchedEnv("pmsm", n, seed=1)
    sd = tge._mlp(pol, 6, 2, seed=1)
    ev = pol.FusedEvaluator(env, sd)
    ev.reset()
    for kw in (dict(trace=[1, 5, 1]), dict(trace=[-1]), dict(trace=[n]), dict(trace=[]),
               dict(trace=[0], trace_start=K), dict(trace=[0], trace_start=-1), dict(trace=[0], trace_every=0),
               dict(trace_every=2), dict(trace_state=True)):
        with pytest.raises(ValueError):
            ev.evaluate(K, **kw)
    short = torch.empty((K * 2 * 10 - 1,), dtype=torch.float32, device=env.device)
    with pytest.raises(nat.LorenzEnvError):
        ev.evaluate(K, trace=[0, 1], trace_out=short)
    with pytest.raises(nat.LorenzEnvError):
        ev.evaluate(K, trace=[0, 1], trace_out=torch.empty((K * 2 * 10,), dtype=torch.float64, device=env.device))
    with pytest.raises(nat.LorenzEnvError):
        ev.evaluate(K, trace=[0, 1], trace_slot_map=torch.empty((n - 1,), dtype=torch.int32, device=env.device))
    # a caller-owned buffer with room to spare is used in place
    big = torch.full((K * 2 * 10 + 7,), -5.0, dtype=torch.float32, device=env.device)
    res = ev.evaluate(K, trace=[0, 1], trace_out=big)
    assert res.trace.data.data_ptr() == big.data_ptr() and (_np(big)[K * 2 * 10:] == -5.0).all()
    with pytest.raises(ValueError):
        pol.FusedEvaluator(gl.BatchedEnv("lorenz3", n, dtype="float64"), tge._mlp(pol, 6, 3, seed=1))

    # the C entry itself
    def args(e_, **over):
        keep = [torch.zeros((e_.num_envs, e_.obs_dim), device=e_.device),
                torch.zeros((e_.num_envs, e_.obs_dim), device=e_.device),
                torch.zeros((nat.EVAL_COLS, e_.num_envs), dtype=torch.float64, device=e_.device),
                torch.tensor([0, 1], dtype=torch.int64, device=e_.device),
                torch.zeros((e_.num_envs,), dtype=torch.int32, device=e_.device),
                torch.zeros((K * 2 * 10,), dtype=torch.float32, device=e_.device)]
        e = nat.LzPolicyEvalArgs()
        e.K, e.flags = K, nat.POLICY_DETERMINISTIC
        e.blob, e.obs_in, e.obs_last, e.stats = (ev.blob.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(),
                                                 keep[2].data_ptr())
        e.norm_eps, e.clip_obs, e.act_low, e.act_high = 1e-8, 10.0, -1.0, 1.0
        t = nat.LzEvalTrace()
        t.ids, t.count, t.slot_map, t.out = keep[3].data_ptr(), 2, keep[4].data_ptr(), keep[5].data_ptr()
        t.start, t.every, t.flags, t.out_capacity_bytes = 0, 1, 0, K * 2 * 10 * 4
        for k, v in over.items():
            setattr(t, k, v)
        return e, t, keep

    def call(e_, a):
        return nat.lib.lz_evaluate_policy_f32_trace(e_._h, ctypes.byref(a[0]), ctypes.byref(a[1]))

    assert call(env, args(env)) == nat.LZ_OK
    assert call(env, args(env, count=0, ids=None, slot_map=None, out=None)) == nat.LZ_OK  # untraced
    for over in (dict(start=K), dict(start=-1), dict(every=0), dict(ids=None), dict(slot_map=None),
                 dict(out=None), dict(count=-1), dict(flags=2), dict(out_capacity_bytes=K * 2 * 10 * 4 - 1),
                 dict(flags=nat.TRACE_STATE)):  # the state columns need 6 more floats per row
        assert call(env, args(env, **over)) == nat.LZ_ERR_INVALID, over
        assert nat.lib.lz_last_error()
    e, t, keep = args(env)
    assert nat.lib.lz_evaluate_policy_f32_trace(env._h, ctypes.byref(e), None) == nat.LZ_ERR_INVALID
    assert nat.lib.lz_evaluate_policy_attn_stack_f32_trace(env._h, ctypes.byref(e), 3, None, None,
                                                           ctypes.byref(t)) == nat.LZ_ERR_UNSUPPORTED
    env.close()
    e64 = gl.BatchedEnv("lorenz3", n, seed=1, dtype="float64")
    e64.reset()
    assert call(e64, args(e64)) == nat.LZ_ERR_UNSUPPORTED
    e64.close()
