"""The launcher branches of lz_kernels.hip that only a tuning-variant bit reaches
(lz_config.reserved[0]; the table is in lz_internal.h and DESIGN.md): the prefetch
distances D = 3 / 15, the done-free split kernel's store policies, the 256-lane kernel's
non-temporal done bytes, the step variants V and k_step_multi<4>'s temporal done bytes.

A selector changes HOW a kernel moves its bytes, never what it computes.  So every case
launches twice from the same seed -- once with the selector, once with only the bit that
forces the same kernel family -- and the two must agree bit for bit (NaN-aware): obs,
reward, done bytes, the done count, the done ids sorted with their terminal rows, and
every final state plane; lz_get_launch_shape must report the same kernel for both.

Only LORENZ3 float32 and PMSM instantiate these variants (lz_kernels.hip has_variants), PMSM here with its
device-drawn process noise.

Rollout shapes: N = 1,028 = 16 whole 64-env groups + 4 envs, a multiple of 4 -- the full
DMA path and the ragged last group; N = 1,031 -- the staged path (no 16-B aligned slices).
K = 33 = 2 * 15 + 3: the wait ladder, the steady state and the tail's re-read of step K - 1
all run for D = 3, 7 and 15.  TimeLimit 5 for the done paths; none for the done-free
LORENZ3 kernels.
Step shapes: N = 1,031 = one whole 1,024-env group + 7 envs (six steps, TimeLimit 3);
N = 1,613 as test_gpu_step_multi.py for the four-tile kernel."""
import numpy as np
import pytest
import torch

from conftest import bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

K = 33
BLOCK, WAVE, SPLIT, PAIR = 1 << 23, 1 << 24, 512, 1 << 27  # the family force bits
SYSTEMS = {"lorenz3": dict(adim=3, arange=1.0, kw={}),
           "pmsm": dict(adim=2, arange=1.2, kw={"add_noise": True})}

# (system, TimeLimit, family bit, selector)
ROLLOUT_CASES = (
    # 1024: D = 3, every family
    [("lorenz3", tl, fam, 1024) for tl in (0, 5) for fam in (BLOCK, WAVE, SPLIT)]
    + [("pmsm", 5, fam, 1024) for fam in (BLOCK, WAVE, PAIR)]
    # 4096: D = 15 for the two-lanes-per-env kernels
    + [("lorenz3", 0, SPLIT, 4096), ("lorenz3", 5, SPLIT, 4096), ("pmsm", 5, PAIR, 4096)]
    # bits 18-20: the done-free split kernel's store policy
    + [("lorenz3", 0, SPLIT, sv << 18) for sv in (1, 3, 4, 7)]
    # 1 << 21: non-temporal done bytes of the 256-lane kernel
    + [("lorenz3", 5, BLOCK, 1 << 21), ("lorenz3", 0, BLOCK, 1 << 21), ("pmsm", 5, BLOCK, 1 << 21)]
)
ROLLOUT_SIZES = (1028, 1031)
STEP_V = (1, 2, 3, 4, 5, 8, 16, 24, 32)
E4 = 49152  # four tiles per step workgroup


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


def _np(t):
    return t.detach().cpu().numpy()


def _planes(be):
    return [_np(be.get_state(p)) for p in range(be.info.n_planes)]


def _actions(system, shape):
    s = SYSTEMS[system]
    return torch.from_numpy(np.random.default_rng(7).uniform(-s["arange"], s["arange"], shape + (s["adim"],))
                            .astype(np.float32)).cuda()


def run_rollout(gl, system, n, tl, variant):
    """One K-step launch: (launch shape, [arrays to compare])."""
    from gym_lorenz import _native as nat

    be = gl.BatchedEnv(system, n, seed=11, max_episode_steps=tl, variant=variant, **SYSTEMS[system]["kw"])
    shape = nat.launch_shape(be._h, nat.CALL_ROLLOUT)
    be.reset()
    obs, rew, done, (didx, tobs, nd) = be.rollout(_actions(system, (K, n)), capture_terminal=K * n)
    m = int(nd.item())
    ids = _np(didx[:m])
    order = np.argsort(ids, kind="stable")
    out = [_np(obs), _np(rew), _np(done), np.int64(m), ids[order], _np(tobs[:m])[order]] + _planes(be)
    be.close()
    return shape, out


def run_steps(gl, system, n, tl, variant, steps=6):
    """`steps` lz_step calls: (launch shape, [arrays to compare])."""
    from gym_lorenz import _native as nat

    be = gl.BatchedEnv(system, n, seed=11, max_episode_steps=tl, variant=variant, **SYSTEMS[system]["kw"])
    shape = nat.launch_shape(be._h, nat.CALL_STEP)
    be.reset()
    A = _actions(system, (steps, n))
    out = []
    for k in range(steps):
        o, r, d = be.step(A[k])
        idx, term = be.done_list()
        out += [_np(o), _np(r), _np(d), _np(idx), _np(term)]
    out += _planes(be)
    be.close()
    return shape, out


_REF = {}  # the family-only / V = 0 launches, computed once per (runner, system, n, tl, variant)


def _ref(run, gl, system, n, tl, variant):
    key = (run.__name__, system, n, tl, variant)
    if key not in _REF:
        _REF[key] = run(gl, system, n, tl, variant)
    return _REF[key]


def _same(got, want):
    assert got[0] == want[0], (got[0], want[0])  # lz_get_launch_shape
    assert len(got[1]) == len(want[1])
    for j, (x, y) in enumerate(zip(got[1], want[1])):
        assert bits_equal(x, y), j


@pytest.mark.parametrize("n", ROLLOUT_SIZES)
@pytest.mark.parametrize("system,tl,family,selector", ROLLOUT_CASES)
def test_rollout_selector_equals_family(gl, system, tl, family, selector, n):
    want = _ref(run_rollout, gl, system, n, tl, family)
    if tl:  # the done path ran: every episode ends within tl steps, inside the launch
        assert want[1][3] >= (K // tl) * n
    else:  # LORENZ3 with the reference's constants never ends an episode
        assert want[1][3] == 0
        assert want[0]["no_done"] == (family != WAVE), want[0]  # (no done-free one-wave kernel)
    _same(run_rollout(gl, system, n, tl, family | selector), want)


@pytest.mark.parametrize("v", STEP_V)
@pytest.mark.parametrize("system", sorted(SYSTEMS))
def test_step_variant_equals_default(gl, system, v):
    want = _ref(run_steps, gl, system, 1031, 3, 0)
    assert want[1][2 + 5 * 2].all() and want[1][2 + 5 * 5].all()  # TimeLimit 3: steps 3 and 6 end every episode
    _same(run_steps(gl, system, 1031, 3, v), want)


@pytest.mark.parametrize("system", sorted(SYSTEMS))
def test_step_multi_temporal_done_equals_default(gl, system):
    want = _ref(run_steps, gl, system, 1613, 3, E4)
    assert want[0]["kernel"] == "step_multi", want[0]
    _same(run_steps(gl, system, 1613, 3, E4 | (1 << 22)), want)
