"""GPU tests of the fused policy evaluation (lz_evaluate_policy_f32 / _attn_f32 /
_attn_stack_f32, gym_lorenz.FusedEvaluator).  Every comparison of the [24, N] table is bit
for bit against tests/eval_ref.py (the header's semantics in NumPy float64) fed

  * the per-step outputs of the rollout collector on a twin handle (transitive: the
    collector is pinned to the oracle by the policy tests) -- every mode, every kernel
    family, partial tiles and grid-stride tiles;
  * the C oracle directly (orc.mlp_f32 / attn_f32 + the DEV-mode env steps, rewards held
    bit for bit as tests/test_gpu_parity.py holds the env's), with and without frozen
    VecNormalize statistics, and through tests/oracle_tl.OracleTL for auto-reset;
  * the reference's own closed loop (code/lorenz_pmsm/test_evaluate.py, the eight trained
    policies): table == the oracle loop's, MAE / RMSE within 1e-4 of the reference traces.
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as er
from oracle_tl import OracleTL
from test_policy_f32_host import GOLD, normalize_obs

pytestmark = pytest.mark.gpu

ORC_KEY = {"lorenz3": "l3", "lorenz4": "l4", "pmsm": "pmsm", "hr": "hr"}


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


def _teq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _mlp(pol, O, A, seed, scale=0.4):
    net = pol.ActorCriticMlp(O, A, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (scale if p.dim() > 1 else 0.3))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _attn(pol, I, A, seed, ln=False, scale=0.3):
    net = pol.ActorCriticAttn(I, A, seed=seed, layer_norm=ln)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "layer_norm" in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (scale if p.dim() > 1 else 0.3))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _planes(env):
    out = []
    for j in range(64):  # every state plane (lz_plane_elem_size 0 ends the list)
        try:
            out.append(_np(env.get_state(j)))
        except ValueError:
            break
    assert out
    return out


def _steps_of_batch(b, n, O):
    """(o [K, n, O] pre-reset observations, r, d) from a collector batch: observations[1:]
    and last_obs are what each step left (post-reset on a done step), the done rows come
    back from the compact terminal list."""
    obs = _np(b.observations)[..., -O:]  # a frame stack's newest frame is its last O columns
    o = np.concatenate([obs[1:], _np(b.last_obs)[None]]).copy()
    m = int(b.n_done.item())
    idx = _np(b.done_idx[:m])
    o[idx // n, idx % n] = _np(b.terminal_obs[:m])
    d = _np(b.dones)
    assert m == int((d != 0).sum())
    return o, _np(b.rewards), d


def _transitive(gl, pol, system, n, K, skip, max_episodes, sd, kw, deterministic=True, frame_stack=1):
    ea = gl.BatchedEnv(system, n, seed=11, **kw)
    eb = gl.BatchedEnv(system, n, seed=11, **kw)
    O = ea.obs_dim
    ev = pol.FusedEvaluator(ea, sd, deterministic=deterministic, frame_stack=frame_stack)
    ck = dict(bootstrap=False, deterministic=deterministic, capture_terminal=K * n,
              frame_stack=frame_stack, precision="fp32")
    col = pol.FusedRolloutCollector(eb, sd, **ck)
    ev.reset()
    col.reset()
    res = ev.evaluate(K, skip=skip, max_episodes=max_episodes)
    b = col.collect(K)
    o, r, d = _steps_of_batch(b, n, O)
    autoreset = kw.get("autoreset", True)
    T = er.eval_ref(o, r, d, autoreset, skip, max_episodes, er.ERR_DIMS[system])
    got = _np(res.stats)
    for c in range(er.COLS):
        assert _teq(got[c], T[c]), (c, np.nonzero(~((got[c] == T[c]) | (np.isnan(got[c]) & np.isnan(T[c]))))[0][:5])
    assert _teq(_np(ev.last_obs), _np(b.last_obs))
    if frame_stack > 1:
        assert _teq(_np(ev.last_stack), _np(b.last_stack))
    for pa, pb in zip(_planes(ea), _planes(eb)):
        assert _teq(pa, pb)
    # tick and call parity advanced alike: a following collect on both handles agrees
    col2 = pol.FusedRolloutCollector(ea, sd, **ck)
    col2.last_obs = ev.last_obs
    col2.last_stack = ev.last_stack
    b1, b2 = col2.collect(2), col.collect(2)
    for f in ("observations", "actions", "log_probs", "values", "rewards", "dones", "last_obs"):
        assert _teq(_np(getattr(b1, f)), _np(getattr(b2, f))), f
    ea.close()
    eb.close()
    return T


@pytest.mark.parametrize("system,kw,n,K,skip,max_ep,det", [
    ("pmsm", dict(add_noise=True, max_episode_steps=5), 4099, 12, 2, 0, True),
    ("pmsm", dict(add_noise=True, max_episode_steps=5), 4099, 12, 2, 2, True),
    ("hr", dict(add_noise=True, add_filter=True, autoreset=False), 4099, 12, 5, 0, False),
    ("lorenz4", dict(max_episode_steps=3), 70, 7, 0, 0, True),
] + [  # 2,048 tiles = 8 per CU: the 8-wave kernel of every system, sampled actions
    (system, dict(max_episode_steps=2), 65536, 5, 2, 0, False) for system in ("pmsm", "hr", "lorenz3", "lorenz4")
])
def test_mlp_table_equals_collector(gl, pol, system, kw, n, K, skip, max_ep, det):
    O, A = {"pmsm": (6, 2), "hr": (6, 2), "lorenz3": (6, 3), "lorenz4": (8, 3)}[system]
    T = _transitive(gl, pol, system, n, K, skip, max_ep, _mlp(pol, O, A, seed=7), kw, deterministic=det)
    if kw.get("max_episode_steps"):
        assert T[er.N_EP].min() >= 1 and (T[er.N_DONE_STEPS] >= 2).all()
    if max_ep:
        assert (T[er.N_STEPS] < K).any()  # the cut-off left uncounted steps


@pytest.mark.parametrize("system,kw,n,K,ln,stack", [
    ("hr", dict(max_episode_steps=5), 1000, 12, False, 1),
    ("pmsm", dict(), 777, 10, False, 1),
    ("hr", dict(), 5, 6, False, 1),                     # one partial 16-env tile
    ("hr", dict(max_episode_steps=5), 1000, 12, True, 4),   # lorenz_filter: LayerNorm + VecFrameStack(4)
    # the other LayerNorm kernels: a full 16-env tile plus a ragged one, 2-step episodes
    ("hr", dict(max_episode_steps=2), 17, 5, True, 1),
    ("lorenz3", dict(max_episode_steps=2), 17, 5, True, 1),
    ("lorenz3", dict(max_episode_steps=2), 17, 5, True, 4),
    ("pmsm", dict(max_episode_steps=2), 17, 5, True, 1),
    ("pmsm", dict(max_episode_steps=2), 17, 5, True, 4),
])
def test_attention_table_equals_collector(gl, pol, system, kw, n, K, ln, stack):
    sd = _attn(pol, 6 * stack, 3 if system == "lorenz3" else 2, seed=4, ln=ln)
    _transitive(gl, pol, system, n, K, 2, 0, sd, kw, frame_stack=stack)


@pytest.mark.parametrize("attention", [False, True])
def test_grid_stride_tiles_start_from_zero(gl, pol, nat, attention):
    """More tiles than grid x waves: a wave runs a second tile, whose accumulators must
    start from zero again (K = 3 with 2-step episodes: every column is populated)."""
    n = 32787
    probe = gl.BatchedEnv("lorenz3", n, seed=11, max_episode_steps=2)
    sh = nat.launch_shape(probe._h, nat.CALL_EVALUATE_POLICY_ATTN_F32 if attention
                          else nat.CALL_EVALUATE_POLICY_F32)
    probe.close()
    assert sh["kernel"] == ("eval_attn_f32" if attention else "eval")
    tiles = -(-n // sh["envs_per_wave"])
    assert tiles > sh["grid"] * sh["waves"] and sh["grid_stride"]
    sd = _attn(pol, 6, 3, seed=3) if attention else _mlp(pol, 6, 3, seed=3)
    T = _transitive(gl, pol, "lorenz3", n, 3, 0, 0, sd, dict(max_episode_steps=2))
    assert (T[er.N_STEPS] == 3).all() and (T[er.N_EP] == 1).all() and (T[er.TAIL_LEN] == 1).all()


# ------------------------------------------------------------------------- oracle-direct
def _oracle_loop(orc, system, n, seed, K, fwd, norm, lo, hi, add_filter=False, alpha=0.5):
    """K closed-loop steps of the DEV oracle without auto-reset from the seed's reset draw:
    (o [K, n, O], r [K, n], d [K, n], last raw obs)."""
    key = ORC_KEY[system]
    init = orc.reset_draw(key, np.float32, n, 0, seed, 0)
    f32 = np.float32
    if system == "pmsm":
        S = orc.PmsmState(n)
        S.st[:] = init
        raw = orc.pmsm_reset_obs(S.st)
    elif system == "hr":
        st = np.ascontiguousarray(init[:, :6])
        fa = np.zeros((n, 2), f32)
        raw = orc.hr_reset_obs(st)
    else:
        st = np.ascontiguousarray(init.copy())
        raw = orc.l3_reset_obs(st) if system == "lorenz3" else orc.l4_reset_obs(st)
    os_, rs, ds = [], [], []
    with np.errstate(all="ignore"):
        for _ in range(K):
            m = fwd(norm(raw))
            a = np.clip(m, f32(lo), f32(hi))
            tr = np.zeros(n, bool)
            if system == "pmsm":
                raw, r, te, tr = orc.pmsm_step(S, a, None, False, alpha, orc.DEV)
            elif system == "hr":
                raw, r, te = orc.hr_step(st, fa, a, None, False, add_filter, orc.DEV)
            elif system == "lorenz3":
                raw, r = orc.l3_step(st, a)
                te = np.zeros(n, bool)
            else:
                raw, r, te = orc.l4_step(st)
            os_.append(raw.copy())
            rs.append(r.copy())
            ds.append(te.astype(np.uint8) | (tr.astype(np.uint8) << 1))
    return np.array(os_), np.array(rs), np.array(ds), raw


@pytest.mark.parametrize("vecnorm", [False, True])
@pytest.mark.parametrize("system,attention", [("pmsm", False), ("hr", False), ("lorenz3", False),
                                              ("lorenz4", False), ("hr", True)])
def test_table_equals_oracle_closed_loop(gl, pol, orc, system, attention, vecnorm):
    from gym_lorenz.vec_normalize import DeviceRunningMeanStd

    n, K, skip, seed = 4099, 12, 5, 5
    kw = dict(add_filter=True) if system == "hr" else {}
    env = gl.BatchedEnv(system, n, seed=seed, autoreset=False, **kw)
    O, A = env.obs_dim, env.action_dim
    sd = _attn(pol, O, A, seed=7) if attention else _mlp(pol, O, A, seed=7)
    rms = None
    norm = lambda x: x  # noqa: E731
    if vecnorm:
        rms = DeviceRunningMeanStd(O, env.device)
        rng = np.random.default_rng(1)
        rms.set_state(rng.normal(0, 2, O), rng.uniform(0.5, 30, O), 1e4)
        mean, var = rms.mean.copy(), rms.var.copy()
        norm = lambda x: np.clip((x.astype(np.float64) - mean) / np.sqrt(var + 1e-8),  # noqa: E731
                                 -10.0, 10.0).astype(np.float32)
    ev = pol.FusedEvaluator(env, sd, obs_rms=rms)
    ev.reset()
    res = ev.evaluate(K, skip=skip)
    fwd = (lambda x: orc.attn_f32(sd, x)[0]) if attention else (lambda x: orc.mlp_f32(sd, x)[0])
    lo, hi = pol.action_bounds(system)
    o, r, d, last = _oracle_loop(orc, system, n, seed, K, fwd, norm, lo, hi, add_filter=system == "hr")
    T = er.eval_ref(o, r, d, False, skip, 0, er.ERR_DIMS[system])
    got = _np(res.stats)
    for c in range(er.COLS):
        assert _teq(got[c], T[c]), c
    assert _teq(_np(ev.last_obs), last)
    assert (T[er.N_WIN] == K - skip).all() and (T[er.N_EP] == 0).all()
    env.close()


@pytest.mark.parametrize("system", ["lorenz3", "lorenz4"])
def test_autoreset_episode_returns_vs_oracle(gl, pol, orc, system):
    n, L, seed = 1000, 4, 9
    O, A = (6, 3) if system == "lorenz3" else (8, 3)
    sd = _mlp(pol, O, A, seed=5)
    lo, hi = pol.action_bounds(system)
    key = ORC_KEY[system]

    def run(K):
        tl = OracleTL(orc, key, np.float32, n, seed, L)
        raw = orc.l3_reset_obs(tl.st) if key == "l3" else orc.l4_reset_obs(tl.st)
        os_, rs, ds = [], [], []
        for _ in range(K):
            a = np.clip(orc.mlp_f32(sd, raw)[0], np.float32(lo), np.float32(hi))
            raw, r, d, idx, term = tl.step(a) if key == "l3" else tl.step()
            pre = raw.copy()
            pre[idx] = term
            os_.append(pre)
            rs.append(r.copy())
            ds.append(d.copy())
        return np.array(os_), np.array(rs), np.array(ds)

    # the table: K = 10, two counted episodes per env, then two uncounted steps
    env = gl.BatchedEnv(system, n, seed=seed, max_episode_steps=L)
    ev = pol.FusedEvaluator(env, sd)
    ev.reset()
    res = ev.evaluate(10, skip=1, max_episodes=2)
    o, r, d = run(10)
    T = er.eval_ref(o, r, d, True, 1, 2, er.ERR_DIMS[system])
    got = _np(res.stats)
    for c in range(er.COLS):
        assert _teq(got[c], T[c]), c
    assert (T[er.N_EP] == 2).all() and (T[er.N_STEPS] <= 8).all() and (T[er.N_DONE_STEPS] >= 2).all()
    env.close()
    # SB3 evaluate_policy: 2000 episodes = 2 per env
    env = gl.BatchedEnv(system, n, seed=seed, max_episode_steps=L)
    mean, std = gl.evaluate_policy(env, sd, 2000)
    o, r, d = run(8)
    T = er.eval_ref(o, r, d, True, 0, 2, er.ERR_DIMS[system])
    assert (T[er.N_EP] == 2).all()
    # the oracle's episode returns, one by one
    rets, acc = [], np.zeros(n, np.float64)
    cnt = np.zeros(n, int)
    for k in range(8):
        acc = acc + np.where(cnt < 2, r[k].astype(np.float64), 0.0)
        fin = (d[k] != 0) & (cnt < 2)
        rets.extend(acc[fin])
        acc[d[k] != 0] = 0.0
        cnt += d[k] != 0
    rets = np.array(rets)
    assert rets.size == 2000 and ((rets < 0).all() or (rets > 0).all())  # one sign: the bound below
    assert abs(mean - np.mean(rets)) <= 2000 * 2.0 ** -52 * abs(np.mean(rets))
    want_std = np.sqrt(max(T[er.EP_RET_SQ].sum() / 2000 - (T[er.EP_RET_SUM].sum() / 2000) ** 2, 0.0))
    assert abs(std - want_std) <= 1e-9 * max(want_std, 1e-300)
    # sqrt(E[R^2] - mean^2) against the two-pass np.std: the subtraction cancels
    # (mean^2 + var) / var of the 2^-52 relative error of each term, far inside 1e-6 here
    assert abs(std - np.std(rets)) <= 1e-6 * np.std(rets)
    with pytest.raises(ValueError):
        gl.evaluate_policy(env, sd, 1500)  # N does not divide it
    env.close()


@pytest.mark.parametrize("j", range(8))
def test_reference_closed_loop_pmsm_policies(gl, pol, orc, nat, j):
    """code/lorenz_pmsm/test_evaluate.py:61-166 in one launch per policy (the reference's
    eight trained A2C policies): K = 1999, the window from step 1000."""
    from gym_lorenz.vec_normalize import DeviceRunningMeanStd

    gold = np.load(GOLD)
    K, skip = 1999, 1000
    alpha = float(gold["alphas"][j])
    sd = {k: torch.from_numpy(gold["a%d/%s" % (j, k)]) for k in orc.POLICY_KEYS + ("log_std",)}
    env = gl.BatchedEnv("pmsm", 1, seed=0, alpha=alpha, add_noise=False)
    rms = DeviceRunningMeanStd(6, env.device)
    rms.set_state(gold["a%d/obs_rms.mean" % j], gold["a%d/obs_rms.var" % j],
                  float(gold["a%d/obs_rms.count" % j]))
    ev = pol.FusedEvaluator(env, sd, obs_rms=rms, clip_obs=float(gold["a%d/clip_obs" % j]),
                            norm_eps=float(gold["a%d/epsilon" % j]))
    ev.reset()
    s1, s2 = gold["init_state1"], gold["init_state2"]
    for i in range(3):
        env.set_state(nat.PMSM_S1 + i, torch.tensor([s1[i]], device=env.device))
        env.set_state(nat.PMSM_S2 + i, torch.tensor([s2[i]], device=env.device))
    S = orc.PmsmState(1)
    S.st[0, :3], S.st[0, 3:] = s1, s2
    raw = orc.pmsm_reset_obs(S.st)
    ev.last_obs = torch.from_numpy(raw).to(env.device)
    res = ev.evaluate(K, skip=skip)
    os_, rs, ds = [], [], []
    psd = {k: gold["a%d/%s" % (j, k)] for k in orc.POLICY_KEYS}
    for _ in range(K):
        m, _ = orc.mlp_f32(psd, normalize_obs(gold, j, raw))
        raw, r, te, tr = orc.pmsm_step(S, np.clip(m, np.float32(-1), np.float32(1)), None, False,
                                       alpha, orc.DEV)
        os_.append(raw.copy())
        rs.append(r.copy())
        ds.append(te.astype(np.uint8) | (tr.astype(np.uint8) << 1))
    T = er.eval_ref(np.array(os_), np.array(rs), np.array(ds), True, skip, 0, 3)
    got = _np(res.stats)
    for c in range(er.COLS):
        assert _teq(got[c], T[c]), (j, c)
    ref = gold["cpu_e"][j][skip:K].astype(np.float64)
    mae, rmse = np.mean(np.abs(ref)), np.sqrt(np.mean(ref ** 2))
    print("alpha=%.3f: MAE %.6f (reference %.6f), RMSE %.6f (reference %.6f), max %.4f"
          % (alpha, res.mae, mae, res.rmse, rmse, res.max_abs))
    assert abs(res.mae - mae) <= 1e-4 * mae and abs(res.rmse - rmse) <= 1e-4 * rmse
    env.close()


def test_wrong_blob_gives_nan_table(gl, pol):
    env = gl.BatchedEnv("pmsm", 300, seed=3)
    sd = _mlp(pol, 6, 2, seed=2)
    ev = pol.FusedEvaluator(env, sd)
    ev.reset()
    good = _np(ev.evaluate(4).stats)
    assert np.isfinite(good).all()
    ev.blob = torch.from_numpy(pol.pack_policy_i8x4(sd, 6, 2)).to(env.device)  # behind the host check
    bad = _np(ev.evaluate(4).stats)
    assert np.isnan(bad).all()
    with pytest.raises(Exception):
        ev._set_blob(pol.pack_policy_i8x4(sd, 6, 2))  # the host check itself
    env.close()


def test_pooled_values(gl, pol, nat):
    n, K, skip = 3001, 9, 2
    env = gl.BatchedEnv("hr", n, seed=4, max_episode_steps=4)
    ev = pol.FusedEvaluator(env, _mlp(pol, 6, 2, seed=8))
    ev.reset()
    res = ev.evaluate(K, skip=skip)
    T = _np(res.stats)
    s = _np(res.pooled_sums)
    assert s.shape == (er.COLS,) and res.n_win.data_ptr() == res.stats[er.N_WIN].data_ptr()
    assert tuple(res.columns) == nat.EVAL_COLUMNS
    tol = n * 2.0 ** -52
    for c in list(range(12)) + [er.N_WIN, er.RET_SUM, er.N_STEPS, er.N_EP, er.EP_RET_SUM, er.EP_RET_SQ,
                                er.EP_LEN_SUM]:
        if er.MAX_ABS0 <= c < er.MAX_ABS0 + 4:
            continue
        assert abs(s[c] - T[c].sum()) <= tol * np.abs(T[c]).sum(), c
    want = er.pooled(T, 3, 50.0)
    for k in ("mae", "rmse", "max_abs", "mean_reward", "std_reward", "mean_ep_length", "mean_step_reward"):
        assert abs(getattr(res, k) - want[k]) <= 4 * tol * abs(want[k]) + 1e-300, k
    np.testing.assert_allclose(res.mae_per_dim, want["mae_per_dim"], rtol=4 * tol)
    np.testing.assert_allclose(res.rmse_per_dim, want["rmse_per_dim"], rtol=4 * tol)
    assert res.max_abs == 50.0 * T[er.MAX_ABS0:er.MAX_ABS0 + 3].max()
    env.close()


def test_refusals(gl, pol, nat):
    def args(env, pblob, **over):
        n, O = env.num_envs, env.obs_dim
        keep = [torch.zeros((n, O), device=env.device), torch.zeros((n, O), device=env.device),
                torch.zeros((nat.EVAL_COLS, n), dtype=torch.float64, device=env.device)]
        e = nat.LzPolicyEvalArgs()
        e.K, e.flags = 2, nat.POLICY_DETERMINISTIC
        e.blob, e.obs_in, e.obs_last, e.stats = (pblob.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(),
                                                 keep[2].data_ptr())
        e.norm_eps, e.clip_obs, e.act_low, e.act_high = 1e-8, 10.0, -1.0, 1.0
        for k, v in over.items():
            setattr(e, k, v)
        return e, keep

    def call(env, e, fn="lz_evaluate_policy_f32"):
        return getattr(nat.lib, fn)(env._h, ctypes.byref(e[0]))

    env = gl.BatchedEnv("pmsm", 64, seed=1)
    blob = torch.from_numpy(pol.pack_policy_f32(_mlp(pol, 6, 2, seed=1), 6, 2)).to(env.device)
    assert call(env, args(env, blob)) == nat.LZ_ERR_STATE  # before the first reset
    env.reset()
    assert call(env, args(env, blob)) == nat.LZ_OK
    assert call(env, args(env, blob, flags=nat.POLICY_BOOTSTRAP)) == nat.LZ_ERR_INVALID
    assert call(env, args(env, blob, flags=nat.POLICY_I8X4)) == nat.LZ_ERR_UNSUPPORTED
    for over in (dict(K=0), dict(skip=-1), dict(max_episodes=-1), dict(blob=None), dict(obs_in=None),
                 dict(obs_last=None), dict(stats=None)):
        assert call(env, args(env, blob, **over)) == nat.LZ_ERR_INVALID, over
    e = args(env, blob)
    assert nat.lib.lz_evaluate_policy_attn_stack_f32(env._h, ctypes.byref(e[0]), 4, None, None) == nat.LZ_ERR_INVALID
    assert nat.lib.lz_evaluate_policy_attn_stack_f32(env._h, ctypes.byref(e[0]), 3, None, None) == nat.LZ_ERR_UNSUPPORTED
    env.close()
    for system, kw, fn in (("lorenz3", dict(dtype="float64"), "lz_evaluate_policy_f32"),
                           ("lorenz3", dict(integrator="rk4"), "lz_evaluate_policy_f32"),
                           ("lorenz4", dict(), "lz_evaluate_policy_attn_f32"),
                           ("transient1", dict(), "lz_evaluate_policy_f32"),
                           ("transient2", dict(), "lz_evaluate_policy_f32"),
                           ("transient_pmsm", dict(), "lz_evaluate_policy_f32"),
                           ("singlecontrol", dict(), "lz_evaluate_policy_f32")):
        env = gl.BatchedEnv(system, 64, seed=1, **kw)
        env.reset()
        assert call(env, args(env, blob), fn) == nat.LZ_ERR_UNSUPPORTED, (system, kw)
        assert nat.lib.lz_last_error()
        env.close()
