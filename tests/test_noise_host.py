"""The vectorised Philox4x32-10 and the normals the GPU tests check against
(oracle.philox_np / oracle.noise_normals / oracle.policy_normals), on the host: philox_np
equals the C restatement orc_philox4x32_10 (itself pinned to the device by the bit-exact
reset draws, tests/test_gpu_parity.py) word for word; policy_normals' words are those of
the counter lz_philox.h documents.

And the sample-by-sample check itself (tests/device_normals.py), before it goes near a
GPU: a simulated device -- the oracle stepped with the injected noise std * float32(z64)
for HR (float32 and float64), TP and SC, float32(mean + float32(z64) * scale) for action
samples -- passes it with worst err / tol below 1 and no row excluded, and every way a
kernel could draw the wrong normal (a neighbour env's or tick's, the other purpose's, a
permuted or mispaired component, a 2 % wrong scale, a neighbour's sigma, the other
subsystem) makes it raise."""
import numpy as np
import pytest

import device_normals as dn

SEED_HI = (5 << 32) | 3
TAIL = np.sqrt(-2 * np.log(2.0 ** -24)) + 1e-9  # 24-bit u1 bound


def test_philox_np_equals_c(orc):
    rng = np.random.default_rng(0)
    C = rng.integers(0, 2 ** 32, (4, 300), dtype=np.uint64)
    for k in range(3):
        key = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        got = orc.philox_np(C, key)
        for i in range(0, 300, 7):
            want = orc.philox([int(C[j, i]) for j in range(4)], key)
            assert [int(got[j][i]) for j in range(4)] == want


def test_noise_normals_shape_and_range(orc):
    z = orc.noise_normals(3, np.arange(1 << 16), 1)
    assert z.shape == (1 << 16, 3)
    assert np.abs(z).max() <= TAIL
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    # keyed by (seed, gid, tick): another tick is another draw
    assert not np.array_equal(z, orc.noise_normals(3, np.arange(1 << 16), 2))


def test_policy_normals_words_counter_and_range(orc):
    """Words 0..3 of block 0 of (gid, purpose 3, tick) under key = seed, as lz_philox.h lays
    the counter out -- gids at and above 2^32 (c1 carries gid[39:32]), a seed and a tick with
    non-zero high words -- and not purpose 2's block."""
    gids = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, (1 << 39) + 1, (1 << 40) - 1], np.int64)
    two24 = 5.9604644775390625e-08
    for seed, tick in ((3, 1), (SEED_HI, 6), (SEED_HI, (7 << 32) | 2)):
        z, w = orc.policy_normals(seed, gids, tick, words=True)
        assert z.shape == (len(gids), 4) and z.dtype == np.float64
        for r, g in enumerate(int(v) for v in gids):
            ctr = [g & 0xFFFFFFFF, ((g >> 32) & 0xFF) | (0 << 8) | (3 << 24),
                   tick & 0xFFFFFFFF, tick >> 32]
            want = orc.philox(ctr, [seed & 0xFFFFFFFF, seed >> 32])
            assert [int(w[j][r]) for j in range(4)] == want, (seed, tick, g)
            for a, b, j in ((want[0], want[1], 0), (want[2], want[3], 2)):  # the two Box-Muller pairs
                rad = np.sqrt(-2.0 * np.log(((a >> 8) + 1.0) * two24))
                ang = 2 * np.pi * ((b >> 8) * two24)
                assert z[r, j] == rad * np.cos(ang) and z[r, j + 1] == rad * np.sin(ang)
        assert not np.array_equal(z[:, :3], orc.noise_normals(seed, gids, tick))
    assert not np.array_equal(orc.policy_normals(3, gids, 1), orc.policy_normals(SEED_HI, gids, 1))
    g = np.arange(2 ** 32 - (1 << 15), 2 ** 32 + (1 << 15))
    z = orc.policy_normals(SEED_HI, g, 4)
    assert np.abs(z).max() <= TAIL
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    # the first pair of noise_normals is the same function of purpose 2's words
    assert np.array_equal(orc._stream_normals(SEED_HI, g, 4, 2)[0][:, :3], orc.noise_normals(SEED_HI, g, 4))


# ------------------------------------------------------------------ the simulated device
N, SEED, TICK, GID0 = 1031, 3, 4, 2 ** 32 - 500  # the ids straddle 2^32

MUTATIONS = ("gid+1", "gid-1", "tick+1", "tick-1", "purpose", "components", "cos_sin",
             "z2_from_sin1", "std_2pct", "sigma_neighbour", "other_subsystem")


def _z4(orc, purpose, mutation=None):
    """The four normals a (mutated) device would use for envs GID0 .. GID0 + N - 1 at TICK."""
    gids = np.arange(GID0, GID0 + N)
    g = gids + {"gid+1": 1, "gid-1": -1}.get(mutation, 0)
    t = TICK + {"tick+1": 1, "tick-1": -1}.get(mutation, 0)
    if mutation == "purpose":
        purpose = 5 - purpose
    z = orc._stream_normals(SEED, g, t, purpose)[0]
    if mutation == "components":
        z = z[:, [2, 1, 0, 3]]
    elif mutation == "cos_sin":
        z = z[:, [1, 0, 3, 2]]
    elif mutation == "z2_from_sin1":
        z = z[:, [0, 1, 1, 3]]
    return z


def _sim_hr(orc, T, mutation):
    init = orc.reset_draw("hr", T, N, GID0, SEED, 0, add_noise=True)
    pre, sigma = np.ascontiguousarray(init[:, :6]), init[:, 6].copy()
    rng = np.random.default_rng(1)
    fa = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    act = rng.uniform(-1.2, 1.2, (N, 2)).astype(np.float32)
    zf = _z4(orc, 2, mutation)[:, :3].astype(np.float32)
    sg = np.roll(sigma, 1) if mutation == "sigma_neighbour" else sigma
    sg = sg * T(1.02) if mutation == "std_2pct" else sg
    nz = (sg.astype(np.float64)[:, None] * zf.astype(np.float64)).astype(T)  # SysHR::noise_from_normals
    post, f = pre.copy(), fa.copy()
    with np.errstate(all="ignore"):
        if mutation == "other_subsystem":
            orc.hr_step(post, f, act, None, False, True, orc.DEV)
            post[:, 3:] = post[:, 3:] + nz * T(orc.PARAMS["hr"][8])
        else:
            orc.hr_step(post, f, act, nz, True, True, orc.DEV)
    z = orc.noise_normals(SEED, np.arange(GID0, GID0 + N), TICK)
    return lambda: dn.hr_step_check(orc, pre, fa, act, post, sigma, z, True)


def _sim_euler(orc, key, T, mutation):
    pre = orc.reset_draw(key, T, N, GID0, SEED, 0)
    if key == "sc":  # SC starts every env at one fixed state: spread it
        pre = pre + np.random.default_rng(2).uniform(-3, 3, pre.shape).astype(T)
    act = np.random.default_rng(1).uniform(-2.5, 2.5, (N, 2)).astype(np.float32)
    zf = _z4(orc, 2, mutation)[:, :3].astype(np.float32)
    std = orc.PARAMS[key][6] * (1.02 if mutation == "std_2pct" else 1.0)
    nz = std * zf.astype(np.float64)                    # SysTP / SysSC::noise_from_normals
    post = np.ascontiguousarray(pre.copy())
    with np.errstate(all="ignore"):
        if mutation == "other_subsystem":
            orc.legacy_step(key, post, act, None)
            post[:, :3] = post[:, :3] + nz.astype(T) * T(orc.PARAMS[key][3])
        else:
            orc.legacy_step(key, post, None if key == "sc" else act, nz)
    z = orc.noise_normals(SEED, np.arange(GID0, GID0 + N), TICK)
    return lambda: dn.euler_step_check(orc, key, pre, act, post, z)


def _sim_pmsm(orc, mutation):
    S = orc.PmsmState(N)
    S.st[:] = orc.reset_draw("pmsm", np.float32, N, GID0, SEED, 0)
    pre = list(S.st.T.copy()) + [S.lam.copy(), S.m.copy(), S.v.copy(), S.adam_step.copy(), S.cur_step.copy()]
    act = np.random.default_rng(1).uniform(-1.2, 1.2, (N, 2)).astype(np.float32)
    zf = _z4(orc, 2, mutation)[:, :3].astype(np.float32)
    nz = (3.06 if mutation == "std_2pct" else 3.0) * zf.astype(np.float64)  # SysPMSM::noise_from_normals
    with np.errstate(all="ignore"):
        if mutation == "other_subsystem":
            orc.pmsm_step(S, act, None, False, 0.5, orc.DEV)
            S.st[:, :3] = S.st[:, :3] + nz.astype(np.float32) * np.float32(orc.PARAMS["pmsm"][2])
        else:
            orc.pmsm_step(S, act, nz, True, 0.5, orc.DEV)
    post = list(S.st.T.copy()) + [S.lam, S.m, S.v, S.adam_step, S.cur_step]
    z = orc.noise_normals(SEED, np.arange(GID0, GID0 + N), TICK)
    return lambda: dn.pmsm_step_check(orc, pre, act, post, z)


def _sim_action(orc, A, mutation):
    mean = np.array([0.75, -1.25, 0.40625], np.float32)[:A]
    scale = np.exp(np.array([-0.5, 0.25, -0.25], np.float32)[:A]).astype(np.float32)
    zf = _z4(orc, 3, mutation)[:, :A].astype(np.float32)
    used = scale * np.float32(1.02) if mutation == "std_2pct" else scale
    act = mean + zf * used                              # normal_rsample, float32
    z = orc.policy_normals(SEED, np.arange(GID0, GID0 + N), TICK)[:, :A]
    return lambda: dn.check_action(act, mean, scale, z)


SIMS = {
    "hr32": lambda orc, m: _sim_hr(orc, np.float32, m),
    "hr64": lambda orc, m: _sim_hr(orc, np.float64, m),
    "tp32": lambda orc, m: _sim_euler(orc, "tp", np.float32, m),
    "tp64": lambda orc, m: _sim_euler(orc, "tp", np.float64, m),
    "sc32": lambda orc, m: _sim_euler(orc, "sc", np.float32, m),
    "sc64": lambda orc, m: _sim_euler(orc, "sc", np.float64, m),
    "pmsm": lambda orc, m: _sim_pmsm(orc, m),
    "act2": lambda orc, m: _sim_action(orc, 2, m),
    "act3": lambda orc, m: _sim_action(orc, 3, m),
}


def _applies(sim, mutation):
    if mutation == "sigma_neighbour":
        return sim.startswith("hr")
    if mutation == "other_subsystem":  # SC and the action head have one place to add it
        return sim.startswith(("hr", "tp", "pmsm"))
    if mutation in ("components", "z2_from_sin1"):  # A = 2 has no third component
        return sim != "act2"
    return True


@pytest.mark.parametrize("sim", sorted(SIMS))
def test_simulated_device_passes(orc, sim):
    worst = SIMS[sim](orc, None)()
    print("simulated %s: worst err / tol %.3f" % (sim, worst))
    assert worst < 1.0


@pytest.mark.parametrize("sim,mutation", [(s, m) for s in sorted(SIMS) for m in MUTATIONS
                                          if _applies(s, m)])
def test_mutated_device_raises(orc, sim, mutation):
    check = SIMS[sim](orc, mutation)
    with pytest.raises(AssertionError):
        check()
