"""Every launcher branch of the policy-in-the-loop kernels, each with a
GPU case at a size that forces it and an assertion that the launcher chose it
(lz_get_launch_shape, the launchers' own decision functions: lz_internal.h
policy_shape / f32_policy_shape / attn_policy_shape / attn_f32_policy_shape).  The
round-3 race (DESIGN §5 "Round 3c") lived in a rollout branch no test reached at its
size; this file is the policy kernels' branch table.

Per case: the env part of the collect is bit-exact against lz_rollout fed the policy's
own clipped actions (observations, rewards, dones, the compact done list, the final
state), and the forward is checked on every recorded row --
  * float32 kernels: bit for bit vs oracle.mlp_f32 / oracle.attn_f32 of the input the
    kernel recorded (deterministic actions = the mean, values, last values);
  * bf16 kernels: vs the torch restatements with the same bf16 roundings (policy.
    reference_forward_*_bf16) within the tolerance of tests/test_gpu_policy.py, and
    the three bf16 MLP shapes are bit-identical to one another.

Branches (MI355X: 256 CUs):
  f32 MlpPolicy   split actor/critic waves (tiles < 8 x CUs): n < 32, ragged, grid-stride;
                  one wave per tile, 8 waves: exact fit, grid-stride + ragged; 4 waves
                  (variant bit 8192)
  f32 SB3-exact   per-step kernel, 4 waves / 8 waves + grid-stride
  bf16 MlpPolicy  interleaved nets + pipelined weights / interleaved / serial 32-env waves
                  (variant bits 128, 32) / serial 32-env x 8 grid-stride / 64-env waves
                  grid-stride + ragged
  bf16 attention  32-env waves x 4, grid-stride; LayerNorm + VecFrameStack(4 / 1)
  f32 attention   16-env waves x 8: n < 16, ragged, grid-stride; LayerNorm + stack(4)
                  grid-stride + ragged
  i8x4            the float32 launchers' kI8 kernels (precision="i8x4"): MlpPolicy 8 waves,
                  LayerNorm attention stack 1 / 4
  every system    the rows after the table: each remaining (kernel, system) instantiation at
                  its smallest size (33 / 17 envs; 129 = four split tiles plus one; 65,536 /
                  131,072 where only the size picks the kernel), with sampled actions, the
                  truncation bootstrap and 2-step episodes; those rows also check the
                  log-probs, on the exact kinds every sample against the normal its Philox
                  stream prescribes, and the bootstrapped rewards, and the ones above 20,000 recorded
                  rows check the forward on 6,000 sampled rows plus the ragged tail
"""
import numpy as np
import pytest
import torch

import device_normals as dn
from conftest import bits_equal

pytestmark = pytest.mark.gpu

F32_MLP, F32_STEP, BF16_MLP, BF16_ATTN, BF16_LN, F32_ATTN, F32_LN = (
    "f32_mlp", "f32_step", "bf16_mlp", "bf16_attn", "bf16_ln", "f32_attn", "f32_ln")
F32_MLP_I8, F32_LN_I8 = "f32_mlp_i8", "f32_ln_i8"  # precision="i8x4": the same launchers' kI8 kernels
# A row with a ninth field True collects with sampled actions, the truncation bootstrap and
# 2-step episodes (K = 5: two truncations and auto-resets inside the rollout) and also checks
# the log-probs, the noise and the bootstrapped rewards (see test_policy_branch).
from test_gpu_policy_attn_f32 import AF_LOGSTD  # noqa: E402  (the blobs' Normal constants)
from test_gpu_policy_f32 import F32_LOGSTD  # noqa: E402

GAMMA = 0.97


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


def _mlp_sd(pol, O, A, seed, scale=0.4):
    net = pol.ActorCriticMlp(O, A, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (scale if p.dim() > 1 else 0.3))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _attn_sd(pol, I, A, seed, ln=False, scale=0.2):
    net = pol.ActorCriticAttn(I, A, seed=seed, layer_norm=ln)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "layer_norm" in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (scale if p.dim() > 1 else 0.3))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


# (kind, system, n, K, variant, n_stack, expected kernel, grid_stride)
CASES = [
    (F32_MLP, "pmsm", 20, 4, 0, 1, "policy_split", False),         # n < 32: one partial tile
    (F32_MLP, "pmsm", 1000, 6, 0, 1, "policy_split", False),       # ragged last tile
    (F32_MLP, "lorenz3", 40001, 3, 0, 1, "policy_split", True),    # 313 groups on 256 CUs
    (F32_MLP, "pmsm", 65536, 3, 0, 1, "policy", False),            # 8 waves, 256 groups exactly
    (F32_MLP, "hr", 70001, 3, 0, 1, "policy", True),               # 8 waves, grid-stride, ragged
    (F32_MLP, "pmsm", 1000, 4, 8192, 1, "policy", False),          # 4 waves, one per tile
    (F32_STEP, "pmsm", 1000, 4, 0, 1, "policy_step", False),       # 4 waves
    (F32_STEP, "lorenz4", 70001, 3, 0, 1, "policy_step", True),    # 8 waves, grid-stride
    (BF16_MLP, "pmsm", 1000, 5, 0, 1, "policy_pair_pipe", False),  # nets interleaved, pipelined
    (BF16_MLP, "pmsm", 1000, 5, 128, 1, "policy_pair", False),     # interleaved
    (BF16_MLP, "pmsm", 1000, 5, 32, 1, "policy", False),           # serial 32-env waves x 8
    (BF16_MLP, "lorenz3", 70000, 3, 0, 1, "policy", True),         # serial x 8, grid-stride
    (BF16_MLP, "pmsm", 262147, 3, 0, 1, "policy", True),           # 64-env waves, ragged
    (BF16_ATTN, "hr", 1000, 4, 0, 1, "policy_attn", False),
    (BF16_ATTN, "hr", 40000, 3, 0, 1, "policy_attn", True),
    (BF16_LN, "hr", 1000, 4, 0, 4, "policy_attn", False),
    (BF16_LN, "hr", 40001, 3, 0, 1, "policy_attn", True),
    (F32_ATTN, "hr", 5, 4, 0, 1, "policy_attn_f32", False),        # n < 16
    (F32_ATTN, "pmsm", 1000, 4, 0, 1, "policy_attn_f32", False),   # ragged
    (F32_ATTN, "hr", 40000, 3, 0, 1, "policy_attn_f32", True),     # 313 groups
    (F32_LN, "hr", 1000, 4, 0, 4, "policy_attn_f32", False),
    (F32_LN, "hr", 33001, 3, 0, 4, "policy_attn_f32", True),       # 258 groups, ragged
]
# Every (family, system) arm the library builds runs at least once: the systems the rows
# above leave out, at a small ragged size (a mis-wired arm steps another system's env).
CASES += [(kind, system, 333, 4, 0, 1, kernel, False) for kind, kernel, systems in (
    (F32_MLP, "policy_split", ("transient1", "transient2", "transient_pmsm", "singlecontrol")),
    (F32_STEP, "policy_step", ("lorenz3", "hr", "transient1", "transient2", "transient_pmsm",
                               "singlecontrol")),
    (BF16_MLP, "policy_pair_pipe", ("transient1",)),
    (BF16_ATTN, "policy_attn", ("lorenz4", "transient1", "transient2", "transient_pmsm",
                                "singlecontrol")),
) for system in systems]
CASES += [  # the LORENZ3 / PMSM arms of the kinds built for LORENZ3 / PMSM / HR only
    (BF16_LN, "lorenz3", 333, 4, 0, 4, "policy_attn", False),
    (BF16_LN, "pmsm", 333, 4, 0, 4, "policy_attn", False),
    (F32_ATTN, "lorenz3", 333, 4, 0, 1, "policy_attn_f32", False),
    (F32_LN, "lorenz3", 333, 4, 0, 4, "policy_attn_f32", False),
    (F32_LN, "pmsm", 333, 4, 0, 4, "policy_attn_f32", False),
]
# Every remaining template instantiation of the policy kernels (one per system the kind is
# built for), at the smallest size that reaches it: a full tile plus a ragged one where a
# variant bit or the default picks the kernel (33 envs; 17 for the 16-env attention waves;
# 129 = four tiles per split workgroup plus one), else the size its launcher switches at
# (8 tiles per CU on 256 CUs = 65,536 envs; 64-env waves from 131,072).  These rows sample
# (ninth field); the ones above 20,000 recorded rows check the forward on 6,000 sampled rows
# and the ragged tail instead of on every row.
_ALL = ("lorenz3", "lorenz4", "pmsm", "hr", "transient1", "transient2", "transient_pmsm", "singlecontrol")
CASES += [(F32_MLP, "pmsm", 129, 5, 0, 1, "policy_split", False, True)]
CASES += [(BF16_MLP, s, 33, 5, 128, 1, "policy_pair", False, True) for s in _ALL if s != "pmsm"]
CASES += [(BF16_MLP, s, 33, 5, 32, 1, "policy", False, True) for s in _ALL if s not in ("pmsm", "lorenz3")]
CASES += [(BF16_LN, s, 33, 5, 0, 1, "policy_attn", False, True) for s in ("lorenz3", "pmsm")]
CASES += [(F32_MLP, s, 33, 5, 8192, 1, "policy", False, True) for s in _ALL if s not in ("pmsm", "lorenz4")]
CASES += [(F32_STEP, "lorenz4", 33, 5, 0, 1, "policy_step", False, True)]
CASES += [(F32_LN, s, 17, 5, 0, 1, "policy_attn_f32", False, True) for s in ("hr", "lorenz3", "pmsm")]
CASES += [(F32_LN_I8, s, 17, 5, 0, 1, "policy_attn_f32", False, True) for s in ("hr", "lorenz3", "pmsm")]
CASES += [(F32_LN_I8, s, 17, 5, 0, 4, "policy_attn_f32", False, True) for s in ("lorenz3", "pmsm")]
CASES += [(BF16_MLP, s, 131072, 3, 0, 1, "policy", False, True) for s in _ALL if s != "pmsm"]
CASES += [(F32_MLP, s, 65536, 3, 0, 1, "policy", False, True) for s in _ALL if s not in ("pmsm", "hr")]
CASES += [(F32_MLP_I8, s, 65536, 3, 0, 1, "policy", False, True) for s in ("hr", "lorenz3", "lorenz4")]
CASES += [(F32_STEP, s, 65536, 3, 0, 1, "policy_step", False, True) for s in _ALL if s != "lorenz4"]
CALL = {F32_MLP: 3, F32_STEP: 4, BF16_MLP: 2, BF16_ATTN: 5, BF16_LN: 6, F32_ATTN: 7, F32_LN: 8,
        F32_MLP_I8: 3, F32_LN_I8: 8}


def _collector(gl, pol, kind, system, n, variant, n_stack, seed=5, sampled=False):
    from gym_lorenz.vec_normalize import DeviceRunningMeanStd

    kw = dict(max_episode_steps=2 if sampled else 3)
    if system in ("pmsm", "hr"):
        kw["add_noise"] = True
    envp = gl.BatchedEnv(system, n, seed=seed, variant=variant, **kw)
    envr = gl.BatchedEnv(system, n, seed=seed, **kw)
    O, A = envp.obs_dim, envp.action_dim
    i8 = kind in (F32_MLP_I8, F32_LN_I8)
    f32 = kind in (F32_MLP, F32_STEP, F32_ATTN, F32_LN)
    ln = kind in (BF16_LN, F32_LN, F32_LN_I8)
    if kind in (F32_MLP, F32_STEP, BF16_MLP, F32_MLP_I8):
        sd = _mlp_sd(pol, O, A, seed=7, scale=0.2 if kind == BF16_MLP else 0.4)
    else:
        sd = _attn_sd(pol, n_stack * O if ln else O, A, seed=3, ln=ln)
    rms = None
    if kind == F32_STEP:  # SB3-exact VecNormalize: one launch per step
        rms = DeviceRunningMeanStd(O, envp.device)
    if sampled:
        sd["log_std"] = torch.tensor([-0.5, 0.25, -0.25, 0.1][:A])
    col = pol.FusedRolloutCollector(envp, sd, bootstrap=sampled, deterministic=not sampled, gamma=GAMMA,
                                    obs_rms=rms, training=True, capture_terminal=4 * n, frame_stack=n_stack if ln else 1,
                                    precision="i8x4" if i8 else "fp32" if f32 else "bf16")
    if kind == F32_STEP:
        assert col.per_step_vecnorm
    return envp, envr, col, sd, O, A


def _case_id(c):  # the ids the eight-field rows always had; "-sampled" for the others
    return "-".join(str(v) for v in c[:8]) + ("-sampled" if len(c) > 8 and c[8] else "")


@pytest.mark.parametrize("kind,system,n,K,variant,n_stack,kernel,stride,sampled",
                         [tuple(c[:8]) + (len(c) > 8 and c[8],) for c in CASES],
                         ids=[_case_id(c) for c in CASES])
def test_policy_branch(gl, pol, orc, kind, system, n, K, variant, n_stack, kernel, stride, sampled):
    from gym_lorenz import _native as nat

    envp, envr, col, sd, O, A = _collector(gl, pol, kind, system, n, variant, n_stack, sampled=sampled)
    i8 = kind in (F32_MLP_I8, F32_LN_I8)
    exact = kind not in (BF16_MLP, BF16_ATTN, BF16_LN)
    sh = nat.launch_shape(envp._h, CALL[kind])
    assert sh["kernel"] == kernel, sh
    assert sh["grid_stride"] == stride, sh
    assert sh["grid"] <= sh["groups"] and (stride or sh["grid"] == sh["groups"]), sh
    obs0 = _np(col.reset())
    assert np.array_equal(obs0, _np(envr.reset()))
    b = col.collect(K)
    lo, hi = pol.action_bounds(system)
    acts = torch.clamp(b.actions, lo, hi).contiguous()
    obs_r, rew_r, done_r, (didx, tobs, nd) = envr.rollout(acts, capture_terminal=4 * n)
    # env part: bit-exact
    assert torch.equal(b.dones, done_r)
    d = _np(b.dones)
    trunc = (d & 2 != 0) & (d & 1 == 0)
    assert np.array_equal(_np(b.rewards)[~trunc], _np(rew_r)[~trunc])  # no bootstrap there
    assert sampled or torch.equal(b.rewards, rew_r)
    assert torch.equal(b.last_obs.view(torch.int32), obs_r[-1].view(torch.int32))
    m = int(nd.item())
    assert m > 0 and int(b.n_done.item()) == m
    o1, o2 = np.argsort(_np(b.done_idx[:m])), np.argsort(_np(didx[:m]))
    assert np.array_equal(_np(b.done_idx[:m])[o1], _np(didx[:m])[o2])
    assert bits_equal(_np(b.terminal_obs[:m])[o1], _np(tobs[:m])[o2])
    for p in range(3):
        assert torch.equal(envp.get_state(p), envr.get_state(p))
    # forward on every recorded row
    I = b.observations.shape[-1]
    x = _np(b.observations).reshape(-1, I)
    act = _np(b.actions).reshape(-1, A)
    val = _np(b.values).reshape(-1)
    logp = _np(b.log_probs).reshape(-1)
    rows = np.arange(x.shape[0])  # row r = (step r // n, env r % n)
    if sampled and x.shape[0] > 20000:  # sampled rows and the ragged tail
        rows = np.concatenate([np.random.default_rng(0).choice(x.shape[0], 6000, replace=False),
                               np.arange(x.shape[0] - 70, x.shape[0])])
        x, act, val, logp = x[rows], act[rows], val[rows], logp[rows]
    if kind in (F32_MLP, F32_STEP):
        mref, vref = orc.mlp_f32(sd, x)
    elif kind in (F32_ATTN, F32_LN):
        mref, vref = orc.attn_f32(sd, x)
    elif kind == F32_MLP_I8:
        mref, vref = orc.mlp_f32(sd, x, precision="i8x4")
    elif kind == F32_LN_I8:
        mref, vref = orc.attn_f32(sd, x, precision="i8x4")
    if exact:
        assert sampled or bits_equal(act, mref), np.nanmax(np.abs(act - mref))
        assert bits_equal(val, vref), np.nanmax(np.abs(val - vref))
    else:
        ref = {BF16_MLP: pol.reference_forward_bf16, BF16_ATTN: pol.reference_forward_attn_bf16,
               BF16_LN: pol.reference_forward_attn_ln_bf16}[kind]
        mt, vt = ref(sd, torch.from_numpy(x))
        f = np.isfinite(x).all(1)
        tol = 2e-2 if kind == BF16_MLP else 3e-2
        mref = _np(mt)
        if not sampled:
            np.testing.assert_allclose(act[f], _np(mt)[f], atol=tol, rtol=tol)
        np.testing.assert_allclose(val[f], _np(vt)[f], atol=tol, rtol=tol)
        assert np.median(np.abs(val[f] - _np(vt)[f])) < 2e-3
    if sampled:
        _check_sampled(pol, orc, kind, exact, sd, col, b, x, act, mref, logp, trunc, _np(rew_r), n, O, A,
                       rows, "%s-%s-%d" % (kind, system, n))
    envp.close()
    envr.close()


def _check_sampled(pol, orc, kind, exact, sd, col, b, x, act, mref, logp, trunc, rew_r, n, O, A, rows, what):
    """The sampled rows' extra checks: the noise z = (action - mean) / scale is finite and
    differs between rows (env, step: the Philox counter) and, on the exact kinds (mref is the
    oracle's bit-exact mean, the scale the blob's), it is the normal the Philox stream
    prescribes for the row's (step, env) = divmod(rows, n): oracle.policy_normals(seed 5, env,
    tick = step + 1) under tests/device_normals.py's check_action, on every finite row, which
    at least 90 % of a case's rows must be; the log-prob is the kernel's formula
    on action - mean, bit for bit on the float32 kinds (the blob's Normal constants), within
    tests/test_gpu_policy.py's tolerance of torch's Normal on the bf16 ones; every truncated
    step's reward is the env's plus gamma * V(stacked terminal observation)."""
    if exact:
        off = AF_LOGSTD if kind in (F32_ATTN, F32_LN, F32_LN_I8) else F32_LOGSTD
        c = np.frombuffer(_np(col.blob).tobytes(), np.float32)[off // 4: off // 4 + 16]
        scale, var2, lscale = c[4:8], c[8:12], c[12:16]
    else:
        scale = np.exp(_np(sd["log_std"])).astype(np.float32)
    f = np.isfinite(x).all(1) & np.isfinite(mref).all(1)
    z = (act - mref)[f] / scale[:A]
    assert np.isfinite(z).all() and len(np.unique(z[:, 0])) > 0.9 * len(z)
    if exact:
        assert f.mean() >= 0.9, (what, f.mean())
        step, env = np.divmod(rows[f], n)
        zp = np.empty((len(step), A))
        for k in np.unique(step):  # one collect after reset(): step k draws at tick k + 1
            zp[step == k] = orc.policy_normals(5, env[step == k], int(k) + 1)[:, :A]
        worst = dn.check_action(act[f], mref[f], scale[:A], zp, what)
        print("sampled rows %s: worst err / tol %.3f (%d of %d rows finite)" % (what, worst, f.sum(), f.size))
        dd = (act - mref).astype(np.float32)
        lp = None
        for j in range(A):
            lpj = ((-(dd[:, j] * dd[:, j])) / var2[j] - lscale[j]) - np.float32(0.91893853320467274)
            lp = lpj if lp is None else (lp + lpj).astype(np.float32)
        assert bits_equal(logp, lp)
    else:
        lp = torch.distributions.Normal(torch.from_numpy(mref), torch.from_numpy(scale[:A])).log_prob(
            torch.from_numpy(act)).sum(-1).numpy()
        np.testing.assert_allclose(logp[f], lp[f], atol=5e-2, rtol=2e-2)
    assert trunc.sum() > 0
    if kind == F32_STEP:  # (its bootstrap input is normalised by the next step's statistics:
        return            # tests/test_gpu_vecnorm_step.py restates that)
    m = int(b.n_done.item())
    idx = _np(b.done_idx[:m])
    k, e = idx // n, idx % n
    sel = trunc[k, e]
    k, e = k[sel], e[sel]
    if len(k) > 4000:
        k, e, sel = k[:4000], e[:4000], np.nonzero(sel)[0][:4000]
    # SB3's stacked terminal observation: the step's input stack rolled by one frame, the
    # terminal frame last (one frame: the terminal observation itself)
    st = np.concatenate([_np(b.observations)[k, e][:, O:], _np(b.terminal_obs[:m])[sel]], 1)
    if exact:
        fwd = orc.mlp_f32 if kind in (F32_MLP, F32_MLP_I8) else orc.attn_f32
        _, vt = fwd(sd, st, **({"precision": "i8x4"} if kind in (F32_MLP_I8, F32_LN_I8) else {}))
        want = (rew_r[k, e] + (np.float32(GAMMA) * vt).astype(np.float32)).astype(np.float32)
        assert bits_equal(_np(b.rewards)[k, e], want)
    else:
        ref = {BF16_MLP: pol.reference_forward_bf16, BF16_ATTN: pol.reference_forward_attn_bf16,
               BF16_LN: pol.reference_forward_attn_ln_bf16}[kind]
        _, vt = ref(sd, torch.from_numpy(st))
        want = np.float32(GAMMA) * _np(vt)
        g = np.isfinite(want)
        np.testing.assert_allclose((_np(b.rewards)[k, e] - rew_r[k, e])[g], want[g], atol=3e-2, rtol=3e-2)


def test_bf16_mlp_shapes_bit_identical(gl, pol):
    """The bf16 MlpPolicy shapes reachable at one size (interleaved + pipelined,
    interleaved, serial 32-env waves) give bit-identical collects."""
    outs = []
    for var in (0, 128, 32):
        envp, _, col, _, _, _ = _collector(gl, pol, BF16_MLP, "pmsm", 1000, var, 1, seed=9)
        col.reset()
        outs.append(col.collect(5))
        envp.close()
    for b in outs[1:]:
        for f in ("observations", "actions", "log_probs", "values", "rewards", "dones", "last_values"):
            assert torch.equal(getattr(b, f), getattr(outs[0], f)), f


@pytest.mark.parametrize("system,n,variant,kernel,no_done", [
    ("lorenz3", 16384, 0, "rollout_wave", False),    # one-wave, below 32,768: no split
    ("lorenz3", 32768, 0, "rollout_split", True),    # two lanes per env, done-free (no TimeLimit)
    ("lorenz3", 65536, 0, "rollout", True),          # 256-lane from 256 x CUs
    ("lorenz3", 32768, 2048, "rollout_split", False),  # variant 2048: the done path
    ("lorenz4", 49152, 0, "rollout", False),         # LORENZ4 f32: 256-lane from 3/4 x 256 x CUs
    ("lorenz4", 40960, 0, "rollout_wave", False),
    ("pmsm", 100000, 0, "rollout_wave", False),      # PMSM / HR: one-wave below 131,072
    ("pmsm", 32768, 0, "rollout_pair", False),       # PMSM: lane pairs at 2 < waves / CU <= 4
    ("pmsm", 16385, 0, "rollout_pair", False),
    ("pmsm", 16384, 0, "rollout_wave", False),
    ("pmsm", 32769, 0, "rollout_wave", False),
    ("pmsm", 200000, 1 << 27, "rollout_pair", False),  # forced at any N
    ("pmsm", 4097, 1 << 28, "rollout_wave", False),    # disabled
    ("hr", 32768, 0, "rollout_wave", False),          # (HR has no lane-pair step)
    ("hr", 131072, 0, "rollout", False),
])
def test_env_rollout_branch_reported(gl, system, n, variant, kernel, no_done):
    """lz_get_launch_shape reports the rollout branch launch_rollout_d takes (the
    rollout == steps cases of test_gpu_parity.py cover each branch's arithmetic)."""
    from gym_lorenz import _native as nat

    kw = {"add_noise": True} if system in ("pmsm", "hr") else {}
    be = gl.BatchedEnv(system, n, seed=1, variant=variant, **kw)
    sh = nat.launch_shape(be._h, nat.CALL_ROLLOUT)
    assert sh["kernel"] == kernel and sh["no_done"] == no_done, sh
    st = nat.launch_shape(be._h, nat.CALL_STEP)
    assert st["kernel"] in ("step", "step_multi") and st["envs_per_wave"] == 64
    be.close()
