"""Every rollout kernel family against the CPU oracle directly, process noise off: one
lz_rollout launch of K = 41 steps under a TimeLimit of 13 with staggered per-env step
counters (truncations, auto-resets from device Philox and, where the case says so, the
system's own terminations inside the launch) == tests/oracle_tl.py's OracleTL stepped K
times, bit for bit and NaN-aware: every step's obs, reward and done byte, the captured done
list (ids sorted, terminal observations) and every final state plane.  The other rollout
tests compare a fused launch with K lz_step calls, which an error shared by both paths
(the auto-reset's ordering, the tick of the reset draw, what persists through a PMSM or HR
reset) passes; here the kernels' force bits (lz_kernels.hip rollout_plan: 512 split lanes,
1<<23 256-lane, 1<<24 one-wave, 1<<27 lane pair) make every family reachable at about a
thousand envs, and lz_get_launch_shape must name the intended one.

N = 1,028 is a multiple of 4 but not a whole group: the full DMA path with the ragged last
group (kRag for the noise-free systems, LORENZ3 float64 included); N = 1,031 is not a
multiple of 4: the staged path.

PMSM at alpha = 0.7 takes the reward's (float)pow((double)x, alpha) path, which
test_gpu_parity.py::test_pmsm_vs_reference_and_oracle already matches to the oracle's DEV
mode bit for bit (the fixture's alphas 0.25 / 0.14 / 0.33 / 0.11), so the reward is
compared bit for bit here too.  HR's own termination (|e| > 70) cannot fire within a 13-step
episode, so its branch runs with the threshold lowered (see CASES).
"""
import numpy as np
import pytest
import torch

from conftest import bits_equal
from oracle_tl import OracleTL, assert_same_trace, rollout_trace

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

K, L, SEED = 41, 13, 31
ONE_WAVE, SPLIT, WIDE, PAIR = 1 << 24, 512, 1 << 23, 1 << 27
KERNEL = {ONE_WAVE: "rollout_wave", SPLIT: "rollout_split", WIDE: "rollout", PAIR: "rollout_pair"}
ORC_NAME = {"lorenz3": "l3", "lorenz4": "l4", "pmsm": "pmsm", "hr": "hr"}

# (system, dtype, force bit, N, TimeLimit, constructor arguments, actions, own termination fires)
CASES = [
    ("lorenz3", "float32", ONE_WAVE, 1028, L, {}, "uniform", False),
    ("lorenz3", "float32", ONE_WAVE, 1031, L, {}, "uniform", False),
    ("lorenz3", "float32", SPLIT, 1028, L, {}, "uniform", False),
    ("lorenz3", "float32", SPLIT, 1031, L, {}, "uniform", False),
    ("lorenz3", "float32", WIDE, 1028, L, {}, "uniform", False),
    ("lorenz3", "float64", ONE_WAVE, 1028, L, {}, "uniform", False),
    # no TimeLimit: the done-free instantiation (rollout_plan no_done)
    ("lorenz3", "float32", SPLIT, 1028, 0, {}, "uniform", False),
    ("lorenz4", "float32", ONE_WAVE, 1028, L, {}, "zero", False),
    ("lorenz4", "float32", SPLIT, 1028, L, {}, "zero", False),
    ("lorenz4", "float32", WIDE, 1031, L, {}, "zero", False),
    ("pmsm", "float32", PAIR, 1028, L, {"alpha": 0.5}, "uniform", False),
    ("pmsm", "float32", PAIR, 1031, L, {"alpha": 0.5}, "uniform", False),
    ("pmsm", "float32", ONE_WAVE, 1028, L, {"alpha": 0.5}, "uniform", False),
    ("pmsm", "float32", PAIR, 1028, L, {"alpha": 0.7}, "uniform", False),
    # error-sum threshold 25 instead of 1000: the termination branch
    ("pmsm", "float32", PAIR, 1031, L, {"params": {10: 25.0}}, "zero", True),
    # half the envs' actions held at 1.0.  With the reference's threshold |e| > 70 no env can
    # terminate within a 13-step episode (the draws give |e| <= 30 and dt = 0.001 moves it by
    # a few units): those two cases pin the launch without a termination, and the same two
    # with the threshold at 25 (params[12]) fire the termination branch inside the launch.
    ("hr", "float32", ONE_WAVE, 1028, L, {"add_filter": True}, "half_one", False),
    ("hr", "float32", ONE_WAVE, 1031, L, {}, "half_one", False),
    ("hr", "float32", ONE_WAVE, 1028, L, {"add_filter": True, "params": {12: 25.0}}, "half_one", True),
    ("hr", "float32", ONE_WAVE, 1031, L, {"params": {12: 25.0}}, "half_one", True),
]


def _id(c):
    system, dtype, bit, n, lim, kw, acts, terminates = c
    extra = "".join("-%s%s" % (k, v if k == "alpha" else "") for k, v in kw.items())
    extra += ("-noTL" if not lim else "") + ("-term" if terminates else "")
    return "%s-%s-%s-%d%s" % (system, dtype[-2:], KERNEL[bit], n, extra)


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


def _np(t):
    return t.detach().cpu().numpy()


def make_actions(kind, n, a_dim):
    a = np.random.default_rng(7).uniform(-1.2, 1.2, (K, n, a_dim)).astype(np.float32)
    if kind == "zero":
        a[:] = 0
    elif kind == "half_one":
        a[:, ::2] = 1.0
    return a


def make_oracle(orc, system, dtype, n, lim, kw, steps0):
    return OracleTL(orc, ORC_NAME[system], np.dtype(dtype), n, SEED, lim, steps0,
                    alpha=kw.get("alpha", 0.5), params=kw.get("params"),
                    add_filter=kw.get("add_filter", False))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rollout_family_equals_oracle(gl, orc, case):
    from gym_lorenz import _native as nat

    system, dtype, bit, n, lim, kw, acts, terminates = case
    be = gl.BatchedEnv(system, n, dtype=dtype, seed=SEED, max_episode_steps=lim, variant=bit,
                       add_noise=False, **kw)
    sh = nat.launch_shape(be._h, nat.CALL_ROLLOUT)
    assert sh["kernel"] == KERNEL[bit], sh
    assert sh["no_done"] == (lim == 0), sh
    be.reset()
    n_planes = be.info.n_planes
    steps0 = None
    if lim:  # staggered step counters: the truncations fall on different steps per env
        steps0 = np.random.default_rng(SEED).integers(0, lim, n).astype(np.int32)
        be.set_state(n_planes - 1, torch.from_numpy(steps0))
    A = make_actions(acts, n, be.action_dim)
    obs, rew, done, (didx, tobs, nd) = be.rollout(torch.from_numpy(A).cuda(), capture_terminal=K * n)
    m = int(nd.item())
    order = torch.argsort(didx[:m])
    got = {"obs": _np(obs), "rew": _np(rew), "done": _np(done), "didx": _np(didx[:m][order]),
           "tobs": _np(tobs[:m][order]), "planes": [_np(be.get_state(p)) for p in range(n_planes)]}
    be.close()

    ref = make_oracle(orc, system, dtype, n, lim, kw, steps0)
    want = rollout_trace(ref, A)
    # without a TimeLimit the handle keeps no step counter: that plane is not compared
    assert_same_trace(got, want, bits_equal, planes=None if lim else range(n_planes - 1))
    if lim:
        assert (want["done"] & 2).any() and m == want["didx"].size > 0
    else:
        assert m == 0 and not want["done"].any()
    assert bool((want["done"] & 1).any()) == terminates, "the case's own termination"
