"""GPU: every action sample the policy kernels draw is the normal its Philox stream
prescribes (lz_philox.h normal2 / normal4: purpose 3, keyed by seed, global env id and the
tick of the step), sample by sample, in every kernel family -- not only N(0, 1) in
distribution, which a replayed tick, a tile-local env id, the process noise's block or a
mispaired third component would pass.

The mean is made exactly known in every kind, bf16 included: action_net.weight is zero, its
bias holds distinct bf16-representable values and log_std distinct values per component, so
a deterministic collect must return the bias bit for bit (asserted: the premise), and on a
twin handle z = (action - bias) / scale -- the scale read from the blob's float32 Normal
constants -- is held to oracle.policy_normals(seed, gid0 + env, tick)[:A] by
tests/device_normals.py's check_action, no row excluded.

  * test_action_samples_family: one case per kernel family of test_gpu_policy_branches.py's
    table at its smallest forcing size, on PMSM (A = 2, process noise on) and LORENZ3
    (A = 3: normal4's third component), the launch shape asserted.
  * test_ticks_across_launches: collect(3), one plain BatchedEnv.step, collect(2) use ticks
    1..6 in order -- the plain step consumes its tick and no policy draw -- and PMSM's
    process noise of the same launches is purpose 2 of the same ticks: a twin handle steps
    the clipped actions one lz_step at a time, every step held to oracle.noise_normals
    (device_normals.pmsm_step_check), and ends each launch in the policy handle's state bit
    for bit.
  * test_shards_and_seeds: global env ids straddling and above 2^32 (the counter's c1 carries
    gid[39:32]) and a seed with a non-zero high word (the key's k1): reset draws bit for bit,
    process noise and action samples against their prescriptions, all different from
    offset 0's / seed 3's."""
import numpy as np
import pytest
import torch

import device_normals as dn
from conftest import bits_equal
from test_gpu_policy_branches import (BF16_ATTN, BF16_LN, BF16_MLP, CALL, F32_ATTN, F32_LN, F32_LN_I8,
                                      F32_MLP, F32_MLP_I8, F32_STEP, _attn_sd, _mlp_sd)

pytestmark = pytest.mark.gpu

SEED = 3
BIAS = np.array([0.75, -1.25, 0.40625], np.float32)     # bf16-representable, distinct
LOG_STD = np.array([-0.5, 0.25, -0.25], np.float32)
# where each kind's blob keeps [log_std(4)][scale(4)][2 scale^2(4)][log scale(4)] in float32
# (lz_internal.h kPolLogStd / kAttLogStd / kLnLogStd / kF32LogStd / kAFLogStd)
CONSTS = {BF16_MLP: 2 * 46208, BF16_ATTN: 23552 + 2 * 58496, BF16_LN: 28928 + 2 * 58496,
          F32_MLP: 2 * 73024, F32_STEP: 2 * 73024, F32_MLP_I8: 2 * 73024,
          F32_ATTN: 54400 + 2 * 102400, F32_LN: 54400 + 2 * 102400, F32_LN_I8: 54400 + 2 * 102400}
PRECISION = {BF16_MLP: "bf16", BF16_ATTN: "bf16", BF16_LN: "bf16", F32_MLP_I8: "i8x4", F32_LN_I8: "i8x4"}

# (kind, n, variant, n_stack, the kernel the launcher must report): the families of
# test_gpu_policy_branches.py's table at their smallest forcing sizes (33 envs: a full tile
# plus a ragged one; 17 for the 16-env attention waves; 129: four split tiles plus one;
# 65,536: 8 tiles per CU, where the float32 launcher switches to 8 waves)
FAMILIES = [
    (F32_MLP, 129, 0, 1, "policy_split"),
    (F32_MLP, 65536, 0, 1, "policy"),           # 8 waves
    (F32_MLP, 33, 8192, 1, "policy"),           # 4 waves
    (F32_STEP, 33, 0, 1, "policy_step"),        # per-step VecNormalize
    (BF16_MLP, 33, 0, 1, "policy_pair_pipe"),
    (BF16_MLP, 33, 128, 1, "policy_pair"),
    (BF16_MLP, 33, 32, 1, "policy"),            # serial
    (BF16_ATTN, 33, 0, 1, "policy_attn"),
    (BF16_LN, 33, 0, 4, "policy_attn"),
    (F32_ATTN, 17, 0, 1, "policy_attn_f32"),
    (F32_LN, 17, 0, 4, "policy_attn_f32"),
    (F32_MLP_I8, 33, 0, 1, "policy_split"),
    (F32_LN_I8, 17, 0, 4, "policy_attn_f32"),
]
FAMILY_CASES = [c + (s,) for c in FAMILIES for s in ("pmsm", "lorenz3")]


def family_case_id(c):
    return "-".join(str(v) for v in (c[0], c[5], c[1], c[2], c[3], c[4]))


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


@pytest.fixture(scope="module")
def pol():
    from gym_lorenz import policy

    return policy


def _np(t):
    return t.detach().cpu().numpy()


def known_mean_sd(pol, kind, O, A, n_stack):
    """A random actor-critic of `kind` whose action mean is BIAS[:A] whatever it sees."""
    if kind in (F32_MLP, F32_STEP, BF16_MLP, F32_MLP_I8):
        sd = _mlp_sd(pol, O, A, seed=7, scale=0.2 if kind == BF16_MLP else 0.4)
    else:
        ln = kind in (BF16_LN, F32_LN, F32_LN_I8)
        sd = _attn_sd(pol, n_stack * O if ln else O, A, seed=3, ln=ln)
    sd["action_net.weight"] = torch.zeros_like(sd["action_net.weight"])
    sd["action_net.bias"] = torch.from_numpy(BIAS[:A].copy())
    sd["log_std"] = torch.from_numpy(LOG_STD[:A].copy())
    return sd


def make_collector(gl, pol, kind, system, n, variant=0, n_stack=1, deterministic=False, seed=SEED,
                   gid0=0, max_episode_steps=2):
    from gym_lorenz.vec_normalize import DeviceRunningMeanStd

    kw = {"add_noise": True} if system == "pmsm" else {}
    env = gl.BatchedEnv(system, n, seed=seed, variant=variant, global_env_offset=gid0,
                        max_episode_steps=max_episode_steps, **kw)
    sd = known_mean_sd(pol, kind, env.obs_dim, env.action_dim, n_stack)
    rms = DeviceRunningMeanStd(env.obs_dim, env.device) if kind == F32_STEP else None
    ln = kind in (BF16_LN, F32_LN, F32_LN_I8)
    col = pol.FusedRolloutCollector(env, sd, bootstrap=False, deterministic=deterministic, obs_rms=rms,
                                    training=True, frame_stack=n_stack if ln else 1,
                                    precision=PRECISION.get(kind, "fp32"))
    if kind == F32_STEP:
        assert col.per_step_vecnorm
    return env, col


def blob_scale(col, kind, A):
    """exp(log_std) as the kernel reads it: the blob's float32 Normal constants."""
    off = CONSTS[kind]
    c = np.frombuffer(_np(col.blob).tobytes()[off: off + 64], np.float32)
    assert np.array_equal(c[:A], LOG_STD[:A]), (kind, off)  # the offset is the constants'
    scale = c[4:4 + A].copy()
    assert (np.abs(scale - np.exp(LOG_STD[:A].astype(np.float64))) <= np.spacing(scale)).all()  # float32 exp
    return scale


def check_samples(orc, actions, scale, seed, gids, tick0, what):
    """actions [K, n, A] of one collect whose first step has tick `tick0`."""
    A = actions.shape[2]
    worst = 0.0
    for k in range(actions.shape[0]):
        z = orc.policy_normals(seed, gids, tick0 + k)[:, :A]
        worst = max(worst, dn.check_action(actions[k], BIAS[:A], scale, z, "%s tick %d" % (what, tick0 + k)))
    return worst


def run_family_case(gl, pol, orc, case):
    """One FAMILY_CASES row; returns the worst err / tol over all samples."""
    from gym_lorenz import _native as nat

    kind, n, variant, n_stack, kernel, system = case
    K = 3 if n > 1000 else 4
    env, col = make_collector(gl, pol, kind, system, n, variant, n_stack, deterministic=True)
    A = env.action_dim
    col.reset()
    b = col.collect(K)
    assert np.isfinite(_np(b.observations)).all()
    # the premise: the mean is the bias, bit for bit
    assert bits_equal(_np(b.actions), np.broadcast_to(BIAS[:A], (K, n, A))), family_case_id(case)
    env.close()
    env, col = make_collector(gl, pol, kind, system, n, variant, n_stack)
    sh = nat.launch_shape(env._h, CALL[kind])
    assert sh["kernel"] == kernel, sh
    if kind == F32_MLP and kernel == "policy":
        assert sh["waves"] == (8 if n >= 65536 else 4), sh
    col.reset()
    b = col.collect(K)
    assert (_np(b.dones) & 2).any()  # auto-resets inside the rollout
    worst = check_samples(orc, _np(b.actions), blob_scale(col, kind, A), SEED, np.arange(n), 1,
                          family_case_id(case))
    env.close()
    return worst


@pytest.mark.parametrize("case", FAMILY_CASES, ids=family_case_id)
def test_action_samples_family(gl, pol, orc, case):
    worst = run_family_case(gl, pol, orc, case)
    print("action samples %s: worst err / tol %.3f" % (family_case_id(case), worst))
    assert worst <= 1.0


# ------------------------------------------------------------------ the process noise of the same launches
def _planes(be):
    return [_np(be.get_state(p)) for p in range(dn.PMSM_PLANES)]


def twin_steps(orc, twin, actions, seed, gids, tick0, what):
    """Step the PMSM handle `twin` through the clipped actions [K, n, 2], one lz_step at a
    time: an env the step reset holds that tick's reset draw bit for bit, every other env's
    slave moved by that tick's process noise.  Returns the worst err / tol."""
    worst = 0.0
    for k in range(actions.shape[0]):
        tick = tick0 + k
        pre = _planes(twin)
        a = _np(actions[k])
        done = _np(twin.step(actions[k].contiguous())[2]) != 0
        post = _planes(twin)
        if done.any():
            fresh = orc.reset_draw_idx("pmsm", np.float32, gids[done], seed, tick)
            assert bits_equal(np.stack(post[:6], 1)[done], fresh), (what, tick)
        live = ~done
        if live.any():
            z = orc.noise_normals(seed, gids[live], tick)
            worst = max(worst, dn.pmsm_step_check(orc, [p[live] for p in pre], a[live],
                                                  [p[live] for p in post], z, what="%s tick %d" % (what, tick)))
    return worst


def same_state(a, b):
    return all(torch.equal(a.get_state(p), b.get_state(p)) for p in range(dn.PMSM_PLANES))


def run_ticks_case(gl, pol, orc, kind):
    """collect(3), a plain step, collect(2) on PMSM with process noise on; returns
    {"action": worst err / tol of the action samples, "noise": of the process noise}."""
    n = 129
    env, col = make_collector(gl, pol, kind, "pmsm", n, max_episode_steps=0)
    twin = gl.BatchedEnv("pmsm", n, seed=SEED, add_noise=True)
    scale = blob_scale(col, kind, 2)
    lo, hi = pol.action_bounds("pmsm")
    gids = np.arange(n)
    assert torch.equal(col.reset(), twin.reset()) and same_state(env, twin)
    out = {"action": 0.0, "noise": 0.0}

    def collect(K, tick0):
        b = col.collect(K)
        out["action"] = max(out["action"], check_samples(orc, _np(b.actions), scale, SEED, gids, tick0, kind))
        out["noise"] = max(out["noise"], twin_steps(orc, twin, torch.clamp(b.actions, lo, hi), SEED, gids,
                                                    tick0, kind))
        assert same_state(env, twin), (kind, tick0)
        return _np(b.actions)

    first = collect(3, 1)                                   # ticks 1, 2, 3
    a4 = torch.from_numpy(np.random.default_rng(4).uniform(-1.2, 1.2, (1, n, 2)).astype(np.float32)).cuda()
    obs4 = env.step(a4[0])[0].clone()                       # tick 4: no policy draw
    out["noise"] = max(out["noise"], twin_steps(orc, twin, a4, SEED, gids, 4, kind + " plain step"))
    assert same_state(env, twin)
    col.last_obs = obs4                                     # the collector carries on from the step's obs
    second = collect(2, 5)                                  # ticks 5, 6
    for s in second:  # no replayed tick: no sample of the second collect is one of the first
        for f in first:
            assert (s != f).all()
    env.close()
    twin.close()
    return out


@pytest.mark.parametrize("kind", [F32_MLP, F32_STEP])
def test_ticks_across_launches(gl, pol, orc, kind):
    out = run_ticks_case(gl, pol, orc, kind)
    print("ticks across launches %s: action samples worst err / tol %.3f, process noise %.3f"
          % (kind, out["action"], out["noise"]))
    assert out["action"] <= 1.0 and out["noise"] <= 1.0


# ------------------------------------------------------------------ ids and seeds at and above 2^32
SEED_HI = (5 << 32) | 3
SHARDS = [(2 ** 32 - 16, SEED), (2 ** 32 + 7, SEED), (0, SEED_HI)]  # (global_env_offset, seed)


def run_shard_case(gl, pol, orc, gid0, seed):
    """The float32 split kernel on 33 PMSM envs with ids gid0 .. gid0 + 32: reset draws, the
    process noise of a twin handle, the action samples.  Returns (figures, the collect's
    actions, the reset states)."""
    from gym_lorenz import _native as nat

    n, K = 33, 3
    env, col = make_collector(gl, pol, F32_MLP, "pmsm", n, seed=seed, gid0=gid0)
    assert nat.launch_shape(env._h, CALL[F32_MLP])["kernel"] == "policy_split"
    twin = gl.BatchedEnv("pmsm", n, seed=seed, add_noise=True, global_env_offset=gid0, max_episode_steps=2)
    gids = gid0 + np.arange(n, dtype=np.int64)
    assert torch.equal(col.reset(), twin.reset())
    state0 = np.stack(_planes(env)[:6], 1)
    assert bits_equal(state0, orc.reset_draw_idx("pmsm", np.float32, gids, seed, 0))
    b = col.collect(K)
    what = "offset %d seed %d" % (gid0, seed)
    lo, hi = pol.action_bounds("pmsm")
    out = {"action": check_samples(orc, _np(b.actions), blob_scale(col, F32_MLP, 2), seed, gids, 1, what),
           # step 2 truncates every env (2-step episodes): its reset draws, bit for bit
           "noise": twin_steps(orc, twin, torch.clamp(b.actions, lo, hi), seed, gids, 1, what)}
    assert (_np(b.dones)[1] == 2).all() and same_state(env, twin)
    env.close()
    twin.close()
    return out, _np(b.actions), state0


@pytest.fixture(scope="module")
def shard_base(gl, pol, orc):
    return run_shard_case(gl, pol, orc, 0, SEED)


@pytest.mark.parametrize("gid0,seed", SHARDS, ids=["straddle_2p32", "above_2p32", "seed_high_word"])
def test_shards_and_seeds(gl, pol, orc, shard_base, gid0, seed):
    out, actions, state0 = run_shard_case(gl, pol, orc, gid0, seed)
    print("shard offset %d seed %d: action samples worst err / tol %.3f, process noise %.3f"
          % (gid0, seed, out["action"], out["noise"]))
    assert out["action"] <= 1.0 and out["noise"] <= 1.0
    # the high bits reach the counter and the key: not offset 0's / seed 3's draws
    assert (actions != shard_base[1]).all() and (state0 != shard_base[2]).all()
