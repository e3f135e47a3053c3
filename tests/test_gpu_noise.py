"""GPU: cfg4's on-device process noise (PMSM add_noise=True: N(0, 3) into the slave's
Euler update, lorenz_env_try_pmsm.py:80-93) over all 262,144 envs and many steps.

Each step is teacher-forced: the oracle steps the device's own pre-step state without
noise, so (state2_device - state2_noiseless) / dt recovers the device's noise sample to
within the float32 rounding of the two updates.  Every recovered sample is checked
against the normal the Philox stream prescribes for that env and tick (oracle.
noise_normals: the exact 24-bit uniforms through Box-Muller in float64; the device uses
hardware v_log_f32 / v_sqrt_f32 / v_cos_f32 / v_sin_f32) -- so the tails (u1 -> 0, where
v_log_f32 matters) are checked sample by sample, not only in distribution -- and the
recovered samples as a whole against N(0, 3): KS, moments, kurtosis, the 1e-5 and
1 - 1e-5 quantiles, and independence across components, neighbouring envs and steps.

The other noisy systems -- HR (SysHR::noise_from_normals: sigma * z with sigma a per-env
plane redrawn on auto-reset, onto the master as nz * dt), TP and SC (prm[6] * z onto the
slave's / the system's derivative) -- are held to the same prescription by
test_device_noise_step (tests/device_normals.py computes the per-sample tolerance, term by
term): 4,099 envs, 6 teacher-forced lz_step calls with staggered 3-step episodes, so every
step has auto-resets (bit for bit the reset draws of that tick, HR's new sigma included)
next to live envs (the noise of that tick, with the env's current sigma), once per
step-kernel family lz_get_launch_shape can report for the system.

The rollout kernels need no cases of their own here: with lz_step's draw pinned, the
bit-for-bit "rollout == K steps, noise on" tests (test_gpu_parity.py, test_gpu_legacy.py,
test_gpu_ragged.py, test_gpu_rollout_pair.py, test_gpu_resident.py and the policy tests'
env part) carry the pin to every rollout family."""
import numpy as np
import pytest
import torch

import device_normals as dn
from conftest import bits_equal

pytestmark = pytest.mark.gpu


def _planes(be, first, cnt):
    return np.stack([be.get_state(first + j).cpu().numpy() for j in range(cnt)], 1)


def test_device_noise_pmsm_262k_many_steps(orc):
    import gym_lorenz as gl
    from scipy import stats

    n, T, seed = 1 << 18, 8, 3
    dt = float(orc._params("pmsm")[2])
    be = gl.BatchedEnv("pmsm", n, seed=seed, add_noise=True, autoreset=False, compact=False)
    be.reset()
    rng = np.random.default_rng(1)
    rec = np.empty((T, n, 3))
    worst = 0.0
    for t in range(T):
        S = orc.PmsmState(n)
        S.st[:] = _planes(be, 0, 6)
        S.lam[:] = be.get_state(6).cpu().numpy()
        S.m[:] = be.get_state(7).cpu().numpy()
        S.v[:] = be.get_state(8).cpu().numpy()
        S.adam_step[:] = be.get_state(9).cpu().numpy()
        S.cur_step[:] = be.get_state(10).cpu().numpy()
        a = rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32)
        be.step(torch.from_numpy(a))
        with np.errstate(all="ignore"):
            orc.pmsm_step(S, a, None, False, 0.5, orc.DEV)
        s1 = _planes(be, 0, 3)
        assert np.array_equal(s1.view(np.int32), S.st[:, :3].view(np.int32)), t  # master noiseless
        s2d = _planes(be, 3, 3)
        s2o = S.st[:, 3:]
        r = (s2d.astype(np.float64) - s2o.astype(np.float64)) / dt
        nz = 3.0 * orc.noise_normals(seed, np.arange(n), t + 1)  # reset was tick 0
        tol = ((np.spacing(np.abs(s2d)).astype(np.float64) + np.spacing(np.abs(s2o)))
               / dt * 1.01 + 1e-3 + 1e-5 * np.abs(nz))
        err = np.abs(r - nz)
        assert (err <= tol).all(), (t, float((err / tol).max()), np.argwhere(err > tol)[:5])
        worst = max(worst, float((err / tol).max()))
        rec[t] = r
    z = (rec / 3.0).reshape(-1)
    N = z.size
    ks = stats.kstest(z, "norm")
    kurt = stats.kurtosis(z)  # excess
    q_lo, q_hi = np.quantile(z, [1e-5, 1 - 1e-5])
    qt = stats.norm.ppf(1 - 1e-5)
    tail = int((np.abs(z) > 4).sum())
    tail_exp = 2 * stats.norm.sf(4) * N
    print("device noise: %d samples, KS D %.2e (p %.3f), mean %.1e, std %.5f, excess kurtosis "
          "%.4f, q(1e-5) %.3f / q(1-1e-5) %.3f (N(0,1): -/+%.3f), |z|>4: %d (exp %.0f), "
          "worst err/tol %.3f" % (N, ks.statistic, ks.pvalue, z.mean(), z.std(), kurt, q_lo, q_hi,
                                  qt, tail, tail_exp, worst))
    assert ks.statistic < 2.3 / np.sqrt(N)
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.std() - 1) < 5 / np.sqrt(2 * N)
    assert abs(kurt) < 5 * np.sqrt(24 / N)
    assert abs(q_lo + qt) < 0.15 and abs(q_hi - qt) < 0.15
    assert abs(tail - tail_exp) < 5 * np.sqrt(tail_exp)
    lim = 5 / np.sqrt(n * T)
    c = np.corrcoef(rec.reshape(-1, 3).T)  # across components
    assert np.abs(c - np.eye(3)).max() < lim
    for j in range(3):
        lag = np.corrcoef(rec[1:, :, j].ravel(), rec[:-1, :, j].ravel())[0, 1]  # across steps
        nb = np.corrcoef(rec[:, 1:, j].ravel(), rec[:, :-1, j].ravel())[0, 1]  # neighbour envs
        assert abs(lag) < lim and abs(nb) < lim, (j, lag, nb)
    be.close()


# ------------------------------------------------------------------ HR / TP / SC, per step-kernel family
E1, E2, E4 = 16384, 32768, 49152  # tests/test_gpu_step_multi.py's variant bits: tiles per workgroup
TILES = {0: 1, E1: 1, E2: 2, E4: 4}
N, T_STEPS, SEED, L = 4099, 6, 3, 3
KEY = {"hr": "hr", "transient_pmsm": "tp", "singlecontrol": "sc"}
HR_EVAL = {"eval_mode": True, "add_filter": True}
# (system, dtype, constructor arguments, variant, the step kernel it must report)
STEP_CASES = [
    ("hr", "float32", {}, E1, "step"),
    ("hr", "float32", {}, E2, "step_multi"),
    ("hr", "float32", {}, E4, "step_multi"),
    ("hr", "float32", HR_EVAL, E1, "step"),
    ("hr", "float32", HR_EVAL, E4, "step_multi"),
    ("hr", "float64", {}, 0, "step"),
    ("transient_pmsm", "float32", {}, 0, "step"),
    ("transient_pmsm", "float64", {}, 0, "step"),
    ("singlecontrol", "float32", {}, 0, "step"),
    ("singlecontrol", "float64", {}, 0, "step"),
]


def step_case_id(c):
    return "%s-%s%s-%s%d" % (c[0], c[1][-2:], "-eval-filter" if c[2] else "", c[4], TILES[c[3]])


def run_step_case(gl, orc, case):
    """One STEP_CASES row; returns {"worst": the worst err / tol over the live envs of all
    steps, "z_err": (HR float64, whose rounding terms are near 1e-12: the hardware
    transcendentals' error itself) the largest recovered error in units of z}."""
    from gym_lorenz import _native as nat

    system, dtype, kw, variant, kernel = case
    key, T = KEY[system], np.dtype(dtype)
    be = gl.BatchedEnv(system, N, dtype=dtype, seed=SEED, max_episode_steps=L, variant=variant,
                       add_noise=True, **kw)
    sh = nat.launch_shape(be._h, nat.CALL_STEP)
    assert sh["kernel"] == kernel and sh["grid"] == -(-N // (256 * TILES[variant])), sh
    if not variant:  # no other family to force: the tile bits leave this system on k_step
        b4 = gl.BatchedEnv(system, N, dtype=dtype, seed=SEED, max_episode_steps=L, variant=E4,
                           add_noise=True, **kw)
        assert nat.launch_shape(b4._h, nat.CALL_STEP)["kernel"] == "step"
        b4.close()
    be.reset()
    P = be.info.n_planes
    ns = {"hr": 6, "tp": 6, "sc": 3}[key]

    def planes():
        return [be.get_state(p).cpu().numpy() for p in range(P)]

    # staggered step counters (tests/test_gpu_rollout_oracle.py): every step truncates some envs
    steps = np.random.default_rng(SEED).integers(0, L, N).astype(np.int32)
    be.set_state(P - 1, torch.from_numpy(steps))
    gids = np.arange(N)
    rng = np.random.default_rng(1)
    out = {"worst": 0.0}
    for k in range(T_STEPS):
        tick = k + 1  # the global step count since reset(), which took tick 0
        pre = planes()
        assert np.array_equal(pre[P - 1], steps), k
        a = rng.uniform(-1.2, 1.2, (N, be.action_dim)).astype(np.float32)
        d = be.step(torch.from_numpy(a))[2].cpu().numpy()
        post = planes()
        done = steps + 1 >= L
        assert 0 < done.mean() <= 0.4, (k, done.mean())  # from the fixed stagger alone
        assert np.array_equal(d, np.where(done, 2, 0).astype(np.uint8)), k
        steps = np.where(done, 0, steps + 1).astype(np.int32)
        assert np.array_equal(post[P - 1], steps), k
        # done envs: every plane is that tick's reset draw (HR: the new sigma too, the filter zeroed)
        fresh = orc.reset_draw_idx(key, T, gids[done], SEED, tick, add_noise=True,
                                   eval_mode=kw.get("eval_mode", False))
        assert bits_equal(np.stack(post[:fresh.shape[1]], 1)[done], fresh), k
        if key == "hr":
            assert not post[7][done].any() and not post[8][done].any(), k
        # live envs: the noise of (seed, gid, tick), sample by sample
        live = ~done
        z = orc.noise_normals(SEED, gids[live], tick)
        s0 = np.ascontiguousarray(np.stack(pre[:ns], 1)[live])
        s1 = np.ascontiguousarray(np.stack(post[:ns], 1)[live])
        what = "%s step %d" % (step_case_id(case), k)
        if key == "hr":
            sigma = pre[6][live]  # the env's current sigma
            assert bits_equal(post[6][live], sigma), k
            assert (sigma == 2).all() if kw.get("eval_mode") else len(np.unique(sigma)) > 0.99 * sigma.size
            fa = np.ascontiguousarray(np.stack(pre[7:9], 1)[live])
            w = dn.hr_step_check(orc, s0, fa, a[live], s1, sigma, z, kw.get("add_filter", False),
                                 what, out if T == np.float64 else None)
        else:
            w = dn.euler_step_check(orc, key, s0, a[live], s1, z, what)
            if key == "sc" and k == 0:  # one fixed start: only the gid keying tells the envs apart
                assert len(np.unique(s0, axis=0)) == 1 and len(np.unique(s1, axis=0)) == live.sum()
        out["worst"] = max(out["worst"], w)
    be.close()
    return out


@pytest.mark.parametrize("case", STEP_CASES, ids=step_case_id)
def test_device_noise_step(orc, case):
    import gym_lorenz as gl

    out = run_step_case(gl, orc, case)
    print("device noise %s: worst err / tol %.3f%s" % (
        step_case_id(case), out["worst"],
        ", largest recovered error %.3g in units of z" % out["z_err"] if "z_err" in out else ""))
    assert out["worst"] <= 1.0
