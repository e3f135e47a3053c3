"""BASELINE.md's per-step float32 bar ("per-step fp32 state error < 1e-5 vs CPU reference")
for the kernels of every system but LORENZ3 (test_gpu_parity.py has that one): every kept
(env, step) pair of the reference's float64 trajectories (tests/teacher_forced.py: L4
12,000, HR 8,000, T1 4,800, T2 4,676 of 4,800, TP 4,800, SC 2,400) becomes its own env of a
float32 BatchedEnv -- reset(init=) from the rounded state, HR's filter memory through
set_state and its sigma in the init's seventh column, one handle per (add_noise,
add_filter) -- takes ONE lz_step with the fixture's action and injected noise, and its
next state is read back through the state planes.  Bars (teacher_forced.assert_gates):

  * state |d| / max(|s|, 1) < 1e-5 against the reference's float64 next state;
  * HR: the termination flag equals the reference's on every pair, and filtered_action is
    bit-equal to the float32 recurrence (lorenz_env_try.py:85-86);
  * reward and the non-cancelling observation components < 1e-5 by the same measure against
    the float64 formula evaluated at the kernel's own float32 next state (T2 / TP rewards,
    a pow: rtol 1e-6, the rule of test_gpu_legacy.py);
  * L4's cancelling derivative half, scaled by the sum of the absolute values of its terms:
    at most twice teacher_forced.L4_DERIV_SCALED_MAX = 1.20e-07, the float32 oracle's own
    maximum as tests/test_teacher_forced_host.py measures it (the kernel is expected
    bit-equal to that oracle; the margin covers only a differently contracted fma).

The bit-for-bit tests against the float32 oracle prove the kernel equals the project's
restatement; this one bounds how far either sits from what the reference computes.
The float32 oracle's own figures are in tests/test_teacher_forced_host.py's docstring.
"""
import numpy as np
import pytest
import torch

import teacher_forced as tf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gl():
    import gym_lorenz

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gym_lorenz


def _np(t):
    return t.detach().cpu().numpy()


def _one_step(gl, key, P, idx, **kw):
    """One float32 lz_step of the pairs `idx` as a batch of their own; returns after, obs,
    rew, term and (HR with the filter) fa for those rows."""
    from gym_lorenz import _native as nat

    n = idx.size
    be = gl.BatchedEnv(tf.NAMES[key], n, dtype="float32", autoreset=False, **kw)
    init = P["before"][idx].astype(np.float32)
    if key == "hr":
        init = np.concatenate([init, P["sigma"][idx, None].astype(np.float32)], 1)
    be.reset(init=torch.from_numpy(np.ascontiguousarray(init)))
    if key == "hr":
        for j in range(2):
            be.set_state(nat.HR_FA + j, torch.from_numpy(np.ascontiguousarray(P["fa"][idx, j])))
    act = np.zeros((n, be.action_dim), np.float32)
    if be.reads_actions:
        act[:] = P["act"][idx][:, :be.action_dim]
    noise = None
    if "noise" in P and (key != "hr" or kw["add_noise"]):
        noise = torch.from_numpy(np.ascontiguousarray(P["noise"][idx]))
    o, r, d = be.step(torch.from_numpy(act), noise)
    D = P["before"].shape[1]
    out = {"after": np.stack([_np(be.get_state(j)) for j in range(D)], 1), "obs": _np(o).copy(),
           "rew": _np(r).copy(), "term": (_np(d) & 1).astype(bool)}
    if key == "hr":
        out["fa"] = np.stack([_np(be.get_state(nat.HR_FA + j)) for j in range(2)], 1)
    be.close()
    return out


@pytest.mark.parametrize("key", tf.SYSTEMS)
def test_f32_kernel_step_vs_reference_f64(gl, orc, key):
    P = tf.pairs(orc, key)
    n = P["kept"]
    if key == "hr":
        got = {"after": np.empty((n, 6), np.float32), "obs": np.empty((n, 6), np.float32),
               "rew": np.empty(n, np.float32), "term": np.empty(n, bool),
               "fa": P["fa"].copy()}  # (rows without the filter keep theirs: not compared)
        for an, af, idx in tf.hr_groups(P):
            part = _one_step(gl, key, P, idx, add_noise=an, add_filter=af)
            for k, v in part.items():
                got[k][idx] = v
    else:
        got = _one_step(gl, key, P, np.arange(n))
    assert got["after"].dtype == np.float32 and got["obs"].dtype == np.float32
    tf.assert_gates(key, tf.measure(orc, key, P, got), deriv_factor=2.0)
