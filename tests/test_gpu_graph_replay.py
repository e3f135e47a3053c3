"""Replayed hipGraphs of lz_reset / lz_step / lz_rollout and of the lz_step_vecnorm +
lz_vecnorm_apply pair against eager runs, bit for bit (no tolerance anywhere in this file).

Every per-step number bench.py reports comes from a captured loop replayed many times, and
include/lorenz_env.h promises that those calls can be captured.  What can break is the
two-slot ping-pong of the RNG tick and the done-list cursor (lz_api.cpp fill_common: a launch
reads ticks[p] / counters[p] and writes tick + tick_adv and a zeroed cursor into slot 1 - p,
p being the HOST's call parity, frozen into the captured node): the SECOND replay must start
on the slot the first one's last node wrote.  A stale or repeated tick is silent -- auto-resets
redraw the same initial states, PMSM / HR process noise repeats, and the output still looks
like a trajectory (test_stale_tick_would_be_seen shows the comparison sees it).

One harness (tests/graph_replay.py run_replay_case) for all cases: reset, E0 in {0, 1} eager
warm-up steps (so a capture starts once on each ping-pong slot), L calls (L even) captured on
a side stream with their OWN buffers each, three replays compared call by call with the
reference's steps r L .. r L + L - 1 (obs, reward, done bytes, n_done, the sorted done ids and
their terminal rows), two eager steps between replay 2 and 3 (bench.py's windows; an even
count keeps the parity), then every state plane and one more eager step.  max_episode_steps
= 3 with L = 4: every env is truncated and auto-reset from Philox (keyed by the tick) inside
every replay; n_done == N on exactly the steps where the TimeLimit fires and >= 4 N in all.

Reference: tests/oracle_tl.py OracleTL for the noise-free cases; an eager twin handle for the
device-noise ones (pinned sample by sample in test_gpu_noise.py).

Shapes: 777 = 3 whole 256-env groups + 9 envs; 1613 as test_gpu_step_multi.py (E = 4 tiles:
trailing empty tiles, a ragged live one); rollouts at 1000 (a multiple of 4, not a whole
group: the full path with the ragged last group) and 70 (not a multiple of 4: the staged
path); the lane-pair rollout at 2050 with an odd K = 5 (it draws normals two steps at a time,
so each launch must restart that schedule at its own tick).  vecnorm-split runs at 262,145
envs: lz_kernels.hip vn_fused(N) holds while ceil(N / kVnBlock) <= vn_fuse_max_wg(), that is
N <= 256 workgroups x 1024 envs = 262,144, so 262,145 is the smallest N on the split path
(256-env workgroups and a column-total launch).

The even-length rule itself is not enforced by the library (a refusal at
the first call after an odd-length capture was built, tested and left out for its host cost),
and no odd-length graph is ever replayed here.  The last test pins what an even-length capture
promises besides: it runs nothing and leaves the handle on the parity it began on, so eager
calls go on after it, before and after a replay.
"""
import numpy as np
import pytest
import torch

from conftest import bits_equal
from graph_replay import (OracleRef, PairCall, ResetCall, RolloutCall, StepCall, TwinRef, VnSide,
                          VnTwinRef, host, run_replay_case, same, set_stream)
from oracle_tl import OracleTL

gpu = pytest.mark.gpu
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

LIMIT, L, SEED = 3, 4, 29
E4, PAIR = 49152, 1 << 27  # variant bits: four tiles per step workgroup; the lane-pair rollout
VN_SPLIT_N = 256 * 1024 + 1  # the smallest N for which lz::vn_fused(N) is false (see above)


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


def _actions(env, shape_prefix, seed):
    """Fixed per-call actions (the graph replays the same ones; the state moves on)."""
    if not env.reads_actions:
        return None
    a = np.random.default_rng(seed).uniform(-1.2, 1.2, shape_prefix + (env.num_envs, env.action_dim))
    return torch.from_numpy(a.astype(np.float32)).to(env.device)


def _make(gl, system, n, dtype, kw):
    return gl.BatchedEnv(system, n, dtype=dtype, seed=SEED, max_episode_steps=LIMIT, **kw)


def _ref(gl, orc, system, n, dtype, kw, twin):
    if twin:
        return TwinRef(_make(gl, system, n, dtype, kw))
    return OracleRef(orc, system, dtype, n, SEED, LIMIT)


def _total_ok(tally, n):
    # the TimeLimit of 3 ends every episode after at most 3 steps and every case below takes
    # at least 15 steps after the reset (a masked reset inside the sequence restarts a third
    # of the envs, which still complete one episode per replay and one per eager window)
    assert tally.total >= 4 * n, tally.total


# (id, system, dtype, kwargs, N, kernel asserted for lz_step or None, eager twin?)
STEP_CASES = [
    ("l3-step", "lorenz3", "float32", {}, 777, None, False),
    ("l3-multi", "lorenz3", "float32", {"variant": E4}, 1613, "step_multi", False),
    ("l3-f64", "lorenz3", "float64", {}, 300, None, False),
    ("l4-step", "lorenz4", "float32", {}, 300, None, False),  # reads no actions: NULL
    ("pmsm-noise", "pmsm", "float32", {"add_noise": True}, 777, None, True),
    ("hr-noise-filter", "hr", "float32", {"add_noise": True, "add_filter": True}, 777, None, True),
]


@gpu
@pytest.mark.parametrize("e0", [0, 1])
@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_replayed_steps(gl, orc, case, e0):
    """4 x lz_step with n_done_out, captured once, replayed three times."""
    from gym_lorenz import _native as nat

    _, system, dtype, kw, n, kernel, twin = case
    G = _make(gl, system, n, dtype, kw)
    if kernel:
        assert nat.launch_shape(G._h, nat.CALL_STEP)["kernel"] == kernel
    ref = _ref(gl, orc, system, n, dtype, kw, twin)
    st = torch.cuda.Stream(G.device)
    tally = run_replay_case(
        G, G, st, ref, lambda: [StepCall(G, _actions(G, (), 100 + k)) for k in range(L)],
        lambda: StepCall(G, _actions(G, (), 99)), e0, LIMIT)
    _total_ok(tally, n)
    assert tally.s == e0 + 3 * L + 3
    ref.close()
    G.close()


# (id, system, kwargs, N, K, kernel asserted for lz_rollout or None, eager twin?)
ROLLOUT_CASES = [
    ("l3-rollout-1000", "lorenz3", {}, 1000, 5, None, False),
    ("l3-rollout-70", "lorenz3", {}, 70, 5, None, False),
    ("pmsm-pair-rollout", "pmsm", {"add_noise": True, "variant": PAIR}, 2050, 5, "rollout_pair", True),
]


@gpu
@pytest.mark.parametrize("e0", [0, 1])
@pytest.mark.parametrize("case", ROLLOUT_CASES, ids=[c[0] for c in ROLLOUT_CASES])
def test_replayed_rollouts(gl, orc, case, e0):
    """2 x lz_rollout(K = 5) with cap = K N and n_done: tick_adv = K per node."""
    from gym_lorenz import _native as nat

    _, system, kw, n, K, kernel, twin = case
    G = _make(gl, system, n, "float32", kw)
    if kernel:
        assert nat.launch_shape(G._h, nat.CALL_ROLLOUT)["kernel"] == kernel
    ref = _ref(gl, orc, system, n, "float32", kw, twin)
    st = torch.cuda.Stream(G.device)
    tally = run_replay_case(
        G, G, st, ref, lambda: [RolloutCall(G, _actions(G, (K,), 200 + k)) for k in range(2)],
        lambda: StepCall(G, _actions(G, (), 199)), e0, LIMIT)
    _total_ok(tally, n)
    assert tally.s == e0 + 3 * 2 * K + 3
    ref.close()
    G.close()


@gpu
@pytest.mark.parametrize("e0", [0, 1])
def test_replayed_mixed_sequence(gl, orc, e0):
    """lz_reset(mask = every 3rd env), lz_step, lz_rollout(K = 3), lz_step in one graph: four
    parity flips of three kinds; the reset's obs rows and the rollout's outputs are compared
    like the steps'."""
    n = 777
    G = _make(gl, "lorenz3", n, "float32", {})
    ref = OracleRef(orc, "lorenz3", "float32", n, SEED, LIMIT)
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    st = torch.cuda.Stream(G.device)
    tally = run_replay_case(
        G, G, st, ref,
        lambda: [ResetCall(G, mask), StepCall(G, _actions(G, (), 301)),
                 RolloutCall(G, _actions(G, (3,), 302)), StepCall(G, _actions(G, (), 303))],
        lambda: StepCall(G, _actions(G, (), 299)), e0, LIMIT, uniform=False)
    _total_ok(tally, n)
    G.close()


def _count(updates, n):
    """RunningMeanStd.count after `updates` batches of n rows from epsilon = 1e-4."""
    c = 1e-4
    for _ in range(updates):
        c = c + float(n)
    assert int(c) == updates * n  # 1e-4 + updates * n, exactly, up to the sum's own rounding
    return c


@gpu
@pytest.mark.parametrize("e0", [0, 1])
@pytest.mark.parametrize("n", [777, VN_SPLIT_N], ids=["vecnorm-fused", "vecnorm-split"])
def test_replayed_vecnorm_pairs(gl, n, e0):
    """4 x (lz_step_vecnorm + lz_vecnorm_apply), PMSM with device noise, laid out as
    bench.py::bench_vecnorm.  The RunningMeanStd states, `returns` and the moment partials all
    live on the device and accumulate across replays: after the reset, every eager pair and
    every replay obs_rms / ret_rms (mean, var, count) and returns equal the eager twin's bit
    for bit, and, independently of the twin, obs_rms.count is exactly 1e-4 + (steps so far + 1)
    N, the + 1 being the reset's update (ret_rms is updated by the steps only): the float64
    value of that sum as RunningMeanStd forms it, count = count + N once per update
    (lz_rms_math.h; SB3's update_from_moments) -- rounding 1e-4 + k N in one go differs from
    it in the last bit (N = 777, k = 11), so _count() folds.  G takes one eager pair before
    the capture besides the E0 ones: the first lz_step_vecnorm on a handle allocates its
    workspace."""
    kw = {"add_noise": True}
    st = torch.cuda.Stream(torch.device("cuda", torch.cuda.current_device()))
    G = VnSide(_make(gl, "pmsm", n, "float32", kw), stream=st)
    T = VnSide(_make(gl, "pmsm", n, "float32", kw))
    ref = VnTwinRef(T)

    def stats(tag, tally):
        g = G.stats()
        same(g, T.stats(), tag)
        assert g["obs_rms"][-1] == _count(tally.s + 1, n), (tag, tally.s)
        assert g["ret_rms"][-1] == _count(tally.s, n), (tag, tally.s)

    res = run_replay_case(
        G, G.env, st, ref, lambda: [PairCall(G.env, _actions(G.env, (), 400 + k)) for k in range(L)],
        lambda: PairCall(G.env, _actions(G.env, (), 399)), e0, LIMIT, warm=1, after_replay=stats)
    _total_ok(res, n)
    assert res.s == 1 + e0 + 3 * L + 3
    ref.close()
    G.close()


def test_stale_tick_would_be_seen(orc):
    """The power of the comparison above, on the CPU: l3-step's reference built a second time
    with the tick a bad replay would reuse -- replay 2 starting again on replay 1's tick, so
    its first auto-reset (step 6, every env) is drawn at tick 2 instead of 6.  The reset rows
    differ in bits from the true reference's for EVERY env, so any env would fail the test."""
    n = 777
    acts = [np.random.default_rng(100 + k).uniform(-1.2, 1.2, (n, 3)).astype(np.float32) for k in range(L)]
    true, stale = (OracleTL(orc, "l3", np.float32, n, SEED, LIMIT) for _ in range(2))
    rows = []
    for tl, rewind in ((true, 0), (stale, L)):
        for k in range(L):      # replay 1: steps 1 .. 4
            tl.step(acts[k])
        tl.tick -= rewind       # the stale start of replay 2
        tl.step(acts[0])        # step 5
        o, _, d, idx, _ = tl.step(acts[1])  # step 6: the TimeLimit resets every env
        assert (d == 2).all() and idx.size == n
        rows.append(o.copy())
    assert true.tick == 6 and stale.tick == 2
    differ = (rows[0].view(np.uint32) != rows[1].view(np.uint32)).any(axis=1)
    assert differ.all(), int(differ.sum())


# ------------------------------------------------------------------ capture, then eager calls
def _twins(gl, n=300):
    G = gl.BatchedEnv("lorenz3", n, seed=SEED, max_episode_steps=LIMIT)
    T = gl.BatchedEnv("lorenz3", n, seed=SEED, max_episode_steps=LIMIT)
    st = torch.cuda.Stream(G.device)
    torch.cuda.synchronize()
    set_stream(G, st)
    assert bits_equal(host(G.reset()), host(T.reset()))
    return G, T, st


def _capture(G, st, calls):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        for c in calls:
            c.launch(G)
    torch.cuda.synchronize()
    return gr


@gpu
@pytest.mark.parametrize("count", [2, 4])
def test_even_capture_then_eager_calls(gl, count):
    """A 2-call and a 4-call capture followed by eager calls, before and after one replay: the
    capture ran nothing and left the handle on its parity, so the handle continues the eager
    twin's sequence throughout (which crosses a TimeLimit reset, drawn from Philox at its tick)."""
    G, T, st = _twins(gl)
    calls = [StepCall(G, _actions(G, (), 540 + k)) for k in range(count)]
    gr = _capture(G, st, calls)
    eager = StepCall(G, _actions(G, (), 550))
    twin = eager.spawn(T)
    twins = [c.spawn(T) for c in calls]
    torch.cuda.synchronize()
    for _ in range(2):  # an even number of eager calls: the replay starts on the capture's slot
        eager.launch(G)
        twin.launch(T)
        same(eager.read(), twin.read(), "eager after the capture")
    with torch.cuda.stream(st):
        gr.replay()
    torch.cuda.synchronize()
    for c, t in zip(calls, twins):
        t.launch(T)
        same(c.read(), t.read(), "replay")
    eager.launch(G)
    twin.launch(T)
    same(eager.read(), twin.read(), "eager after the replay")
    G.close()
    T.close()
