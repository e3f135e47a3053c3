"""GPU: the frame-stacked 64-unit MlpPolicy (code/lorenz_filter/train.py:109-131: PPO(
"MlpPolicy") on VecFrameStack(n_stack=4); test_evaluate.py:94-157 evaluates it) --
lz_stack_rollout_policy_f32 / lz_stack_evaluate_policy_f32 behind FusedRolloutCollector /
FusedEvaluator(frame_stack=4) with a (64, 24) layer 1.

Bars:
  * forward: every deterministic action (= the policy mean), value and last value is
    VALUE-equal (==, NaNs matching) to the unchanged oracle.mlp_f32 of the [.., 24]
    observation the kernel recorded: the oracle zero-pads the 64 units to 128, and the
    kernel's two-tile chains are the padded chains without their zero steps, so the two
    can differ in a zero's sign and in nothing else;
  * env part: vs lz_rollout fed the policy's own clipped actions (rewards, dones, compact
    done list, last obs, state planes); stacks, stacked terminal observations and
    last_stack vs the SB3 StackedObservations restatement (oracle/sb3_framestack.py);
  * truncation bootstrap: reward = env reward + float32(gamma * V(stacked terminal obs));
  * sampling: every sampled action against the Philox stream of (seed, env, tick), the
    log_prob by the kernel's float32 formula;
  * evaluation: the [24, N] table bit-equal to tests/eval_ref.py over the collector twin;
  * an LZ_BLOB_MLP_F32 blob swapped in behind the host check: all-NaN outputs;
  * every launcher branch through lz_get_launch_shape, the entry points' refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

import device_normals as dn
import eval_ref as er

pytestmark = pytest.mark.gpu

STK_LOGSTD = 2 * 24128  # lz_internal.h kStkLogStd


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


def _np(t):
    return t.detach().cpu().numpy()


def value_equal(a, b):
    """a == b elementwise with NaNs matching (a zero's sign is free)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _sd(pol, A, seed, scale=0.4, in_dim=24, hidden=64):
    net = pol.ActorCriticMlp(in_dim, A, hidden=hidden, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (scale if p.dim() > 1 else 0.3))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _col(pol, env, sd, **kw):
    kw.setdefault("precision", "fp32")
    col = pol.FusedRolloutCollector(env, sd, frame_stack=4, **kw)
    assert col.mlp_stack and col.f32 and col.family == "mlp_stack"
    return col


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sb3_stacks(obs0, obs_r, done_r, didx, tobs, n, n_stack):
    from oracle.sb3_framestack import StackedObservations

    K, O = obs_r.shape[0], obs_r.shape[2]
    term = {int(i): tobs[m] for m, i in enumerate(didx)}
    so = StackedObservations(n, n_stack, O)
    seen = [so.reset(obs0).copy()]
    stacked_term = {}
    for k in range(K):
        d = done_r[k] != 0
        infos = [{"terminal_observation": term[k * n + e]} if d[e] else {} for e in range(n)]
        st, infos = so.update(obs_r[k], d, infos)
        for e in np.nonzero(d)[0]:
            stacked_term[(k, int(e))] = infos[e]["terminal_observation"]
        seen.append(st.copy())
    return np.stack(seen[:-1]), stacked_term, seen[-1]


def _grid_stride_n(gl, nat):
    """The smallest n at which a wave of the rollout walks a second tile."""
    probe = gl.BatchedEnv("hr", 1 << 20, seed=1)
    sh = nat.launch_shape(probe._h, nat.CALL_ROLLOUT_POLICY_STACK_F32)
    probe.close()
    assert sh["grid"] == 2 * _cus() and sh["grid_stride"]
    return sh["grid"] * sh["waves"] * sh["envs_per_wave"] + 1


@pytest.mark.parametrize("system,n,K,kw", [
    ("hr", 70, 9, dict(add_noise=True, add_filter=True, max_episode_steps=4)),  # a ragged tile
    ("pmsm", 1500, 9, dict(add_noise=True, max_episode_steps=4)),
    ("lorenz3", 333, 6, dict(max_episode_steps=5)),                             # A = 3
    ("hr", None, 5, dict(max_episode_steps=4)),                                 # groups > grid
])
def test_stack_f32_rollout_value_equal(gl, pol, nat, orc, system, n, K, kw):
    stride = n is None
    if stride:
        n = _grid_stride_n(gl, nat)
    envp = gl.BatchedEnv(system, n, seed=11, **kw)
    envr = gl.BatchedEnv(system, n, seed=11, **kw)
    O, A = envp.obs_dim, envp.action_dim
    assert O == 6
    # the launcher branch (one kernel, one shape function) through lz_get_launch_shape
    groups = -(-(-(-n // 32)) // 4)
    for call, kernel in ((nat.CALL_ROLLOUT_POLICY_STACK_F32, "policy_stack_f32"),
                         (nat.CALL_EVALUATE_POLICY_STACK_F32, "eval_stack_f32")):
        sh = nat.launch_shape(envp._h, call)
        assert (sh["kernel"], sh["envs_per_wave"], sh["waves"]) == (kernel, 32, 4)
        assert sh["groups"] == groups and sh["grid"] == min(groups, 2 * _cus())
        assert sh["grid_stride"] == stride
        if stride:
            assert groups == sh["grid"] + 1
    sd = _sd(pol, A, seed=3)
    col = _col(pol, envp, sd, bootstrap=False, deterministic=True, capture_terminal=K * n)
    obs0 = _np(col.reset())
    assert np.array_equal(obs0, _np(envr.reset()))
    b = col.collect(K)
    lo, hi = pol.action_bounds(envp.system_name)
    acts = torch.clamp(b.actions, lo, hi).contiguous()
    obs_r, rew_r, done_r, (didx, tobs, nd) = envr.rollout(acts, capture_terminal=K * n)
    assert torch.equal(b.rewards, rew_r)
    assert torch.equal(b.dones, done_r)
    assert torch.equal(b.last_obs, obs_r[-1])
    m = int(nd.item())
    assert m > 0 and int(b.n_done.item()) == m
    o1, o2 = np.argsort(_np(b.done_idx[:m])), np.argsort(_np(didx[:m]))
    assert np.array_equal(_np(b.done_idx[:m])[o1], _np(didx[:m])[o2])
    assert np.array_equal(_np(b.terminal_obs[:m])[o1], _np(tobs[:m])[o2])
    for p in range(3):
        assert torch.equal(envp.get_state(p), envr.get_state(p))
    seen, _, final = _sb3_stacks(obs0, _np(obs_r), _np(done_r), _np(didx[:m]), _np(tobs[:m]), n, 4)
    assert b.observations.shape == (K, n, 24)
    assert np.array_equal(_np(b.observations), seen)
    assert np.array_equal(_np(b.last_stack), final) and np.array_equal(_np(col.last_stack), final)
    # the stack filled, rolled and restarted
    d = _np(done_r) != 0
    assert (seen[0][:, :18] == 0).all() and (seen[1:][d[:-1]][:, :18] == 0).all()
    assert (seen[:, :, :6] != 0).any()
    obs = _np(b.observations).reshape(-1, 24)
    act, val = _np(b.actions).reshape(-1, A), _np(b.values).reshape(-1)
    if n * K > 20000:  # the last tiles (the second round of the grid) and a sample of the rest
        rows = np.unique(np.concatenate([np.random.default_rng(0).choice(n * K, 3000, replace=False),
                                         np.arange(n * K - 200, n * K)]))
        obs, act, val = obs[rows], act[rows], val[rows]
    mean, v = orc.mlp_f32(sd, obs)
    assert np.isfinite(mean).all() and np.abs(mean).max() > 0.05
    assert value_equal(act, mean), np.nanmax(np.abs(act - mean))
    assert value_equal(val, v), np.nanmax(np.abs(val - v))
    _, vl = orc.mlp_f32(sd, final)
    assert value_equal(_np(b.last_values), vl)
    # a second collect carries the stack on
    b2 = col.collect(2)
    assert np.array_equal(_np(b2.observations[0]), final)
    envp.close()
    envr.close()


def test_stack_f32_bootstrap_values_the_stacked_terminal_obs(gl, pol, orc):
    n, K, gamma = 1500, 9, 0.97
    kw = dict(max_episode_steps=4, add_filter=True)
    ea = gl.BatchedEnv("hr", n, seed=21, **kw)
    eb = gl.BatchedEnv("hr", n, seed=21, **kw)
    sd = _sd(pol, 2, seed=4)
    ca = _col(pol, ea, sd, gamma=gamma, bootstrap=True, deterministic=True, capture_terminal=K * n)
    cb = _col(pol, eb, sd, gamma=gamma, bootstrap=False, deterministic=True)
    obs0 = _np(ca.reset())
    cb.reset()
    ba, bb = ca.collect(K), cb.collect(K)
    assert torch.equal(ba.actions, bb.actions) and torch.equal(ba.values, bb.values)
    d = _np(ba.dones)
    trunc = (d & 2 != 0) & (d & 1 == 0)
    assert trunc.sum() > 0
    ra, rb = _np(ba.rewards), _np(bb.rewards)
    assert np.array_equal(ra[~trunc], rb[~trunc])
    m = int(ba.n_done.item())
    raw = np.concatenate([_np(ba.observations)[1:, :, -6:], _np(ba.last_obs)[None]], 0)
    _, sterm, _ = _sb3_stacks(obs0, raw, d, _np(ba.done_idx[:m]), _np(ba.terminal_obs[:m]), n, 4)
    keys = [(k, e) for (k, e) in sterm if trunc[k, e]]
    _, vt = orc.mlp_f32(sd, np.stack([sterm[key] for key in keys]))
    want = np.array([rb[k, e] for (k, e) in keys], np.float32) + (np.float32(gamma) * vt).astype(np.float32)
    got = np.array([ra[k, e] for (k, e) in keys], np.float32)
    assert (vt != 0).all() and value_equal(got, want.astype(np.float32))
    ea.close()
    eb.close()


def test_stack_f32_sampling_follows_the_philox_stream(gl, pol, orc):
    n, K = 700, 5
    env = gl.BatchedEnv("lorenz3", n, seed=21, max_episode_steps=3)
    sd = _sd(pol, 3, seed=6)
    sd["log_std"] = torch.tensor([-0.5, 0.25, 0.1])
    col = _col(pol, env, sd, bootstrap=False)
    col.reset()
    b = col.collect(K)
    obs = _np(b.observations).reshape(-1, 24)
    mean, val = orc.mlp_f32(sd, obs)
    assert value_equal(_np(b.values).reshape(-1), val)
    act = _np(b.actions).reshape(-1, 3)
    f = np.frombuffer(_np(col.blob).tobytes(), np.float32)[STK_LOGSTD // 4: STK_LOGSTD // 4 + 16]
    scale, var2, lscale = f[4:8], f[8:12], f[12:16]
    for k in range(K):  # sample by sample the normal of (seed, env, tick = step + 1)
        r = slice(k * n, (k + 1) * n)
        dn.check_action(act[r], mean[r], scale[:3], orc.policy_normals(21, np.arange(n), k + 1)[:, :3],
                        "step %d" % k)
    dd = (act - mean).astype(np.float32)
    lp = None
    for j in range(3):
        lpj = ((-(dd[:, j] * dd[:, j])) / var2[j] - lscale[j]) - np.float32(0.91893853320467274)
        lp = lpj if lp is None else (lp + lpj).astype(np.float32)
    assert np.array_equal(_np(b.log_probs).reshape(-1), lp)
    env.close()


def _planes(env):
    out = []
    for j in range(64):
        try:
            out.append(_np(env.get_state(j)))
        except ValueError:
            break
    assert out
    return out


@pytest.mark.parametrize("system,n,kw,det,max_ep", [
    ("hr", 70, dict(add_noise=True, add_filter=True, max_episode_steps=4), True, 0),
    ("pmsm", 1500, dict(add_noise=True, max_episode_steps=4), False, 2),
])
def test_stack_f32_evaluation_table_equals_collector_twin(gl, pol, system, n, kw, det, max_ep):
    K, skip = 9, 2
    ea = gl.BatchedEnv(system, n, seed=11, **kw)
    eb = gl.BatchedEnv(system, n, seed=11, **kw)
    sd = _sd(pol, 2, seed=7)
    ev = pol.FusedEvaluator(ea, sd, deterministic=det, frame_stack=4)
    assert ev.mlp_stack and ev.family == "mlp_stack"
    col = _col(pol, eb, sd, bootstrap=False, deterministic=det, capture_terminal=K * n)
    ev.reset()
    col.reset()
    res = ev.evaluate(K, skip=skip, max_episodes=max_ep)
    b = col.collect(K)
    obs = _np(b.observations)[..., -6:]
    o = np.concatenate([obs[1:], _np(b.last_obs)[None]]).copy()
    m = int(b.n_done.item())
    idx = _np(b.done_idx[:m])
    o[idx // n, idx % n] = _np(b.terminal_obs[:m])
    d = _np(b.dones)
    assert m == int((d != 0).sum()) and m > 0
    T = er.eval_ref(o, _np(b.rewards), d, True, skip, max_ep, er.ERR_DIMS[system])
    got = _np(res.stats)
    assert got.shape == (24, n) and np.isfinite(got).all()
    for c in range(er.COLS):
        assert np.array_equal(got[c], T[c], equal_nan=True), c
    assert T[er.N_EP].min() >= 1
    assert np.array_equal(_np(ev.last_obs), _np(b.last_obs))
    assert np.array_equal(_np(ev.last_stack), _np(b.last_stack))
    for pa, pb in zip(_planes(ea), _planes(eb)):
        assert np.array_equal(pa, pb, equal_nan=True)
    with pytest.raises(ValueError, match="no traced form"):
        ev.evaluate(K, trace=[0])
    ea.close()
    eb.close()


def test_stack_f32_wrong_blob_gives_nan(gl, pol, nat):
    n, K = 100, 3
    env = gl.BatchedEnv("hr", n, seed=3)
    sd = _sd(pol, 2, seed=2)
    wrong = pol.pack_policy_f32(_sd(pol, 2, seed=2, in_dim=6, hidden=128), 6, 2)  # LZ_BLOB_MLP_F32
    assert nat.lib.lz_policy_blob_format(wrong.ctypes.data, wrong.size) == nat.BLOB_MLP_F32
    col = _col(pol, env, sd, deterministic=True)
    col.reset()
    good = col.collect(K)
    assert all(torch.isfinite(t).all() for t in (good.actions, good.values, good.log_probs, good.rewards))
    with pytest.raises(nat.LorenzEnvError):
        col._set_blob(wrong)  # the host check itself
    col.blob = torch.from_numpy(wrong).to(env.device)  # behind the host check
    bad = col.collect(K)
    for name in ("actions", "values", "log_probs", "last_values", "rewards"):
        assert torch.isnan(getattr(bad, name)).all(), name
    ev = pol.FusedEvaluator(env, sd, frame_stack=4)
    ev.reset()
    assert np.isfinite(_np(ev.evaluate(K).stats)).all()
    ev.blob = torch.from_numpy(wrong).to(env.device)
    assert np.isnan(_np(ev.evaluate(K).stats)).all()
    env.close()


def test_stack_f32_entry_point_refusals(gl, pol, nat):
    sd = _sd(pol, 2, seed=2)
    env = gl.BatchedEnv("hr", 64, seed=3)
    col = _col(pol, env, sd)
    col.reset()
    # n_stack: the reference's 4 alone
    col.frame_stack = 1
    with pytest.raises(nat.LorenzEnvError, match="n_stack must be 4"):
        col.collect(2)
    col.frame_stack = 4
    col.i8x4 = True
    with pytest.raises(nat.LorenzEnvError, match="LZ_POLICY_I8X4"):
        col.collect(2)
    col.i8x4 = False
    assert torch.isfinite(col.collect(2).values).all()
    env.close()
    # the other systems, float64 handles and RK4: refused as the other stacked entry points
    for system, kw in (("lorenz4", {}), ("hr", dict(dtype="float64")), ("lorenz3", dict(integrator="rk4"))):
        e = gl.BatchedEnv(system, 64, seed=3, **kw)
        e.reset()
        r, ea = nat.LzPolicyRolloutArgs(), nat.LzPolicyEvalArgs()
        r.K = ea.K = 2
        buf = torch.zeros(64 * 24 * 4, dtype=torch.float32, device=e.device)
        for fn, args in ((nat.lib.lz_stack_rollout_policy_f32, r), (nat.lib.lz_stack_evaluate_policy_f32, ea)):
            st = fn(e._h, ctypes.byref(args), 4, buf.data_ptr(), buf.data_ptr())
            assert st == nat.LZ_ERR_UNSUPPORTED, (system, kw, nat.lib.lz_last_error())
        e.close()
    # what the Python layer refuses before any launch
    e = gl.BatchedEnv("hr", 64, seed=3)
    with pytest.raises(ValueError, match="LayerNorm attention extractor"):
        pol.FusedRolloutCollector(e, _sd(pol, 2, seed=2, hidden=128), frame_stack=4)
    with pytest.raises(ValueError, match="precision='fp32' only"):
        pol.FusedRolloutCollector(e, sd, frame_stack=4, precision="bf16")
    e.close()
