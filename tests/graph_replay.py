"""Test helper (not a test module): one harness that captures a sequence of env calls on a
handle into a hipGraph, replays it three times and compares every captured call's outputs,
replay by replay, with a reference that is advanced eagerly (test_gpu_graph_replay.py).

A captured call is a Call object that owns its buffers (each of the L captured calls gets
its OWN obs / reward / done / done-list / terminal-obs / n_done buffers, validated once
through BatchedEnv.step_args / rollout_args), so after a replay every call of the sequence
can still be inspected, its done list included.  The same Call classes drive

  * the graph handle G (capture + replays + the eager calls in between),
  * the eager twin T of the device-noise cases (TwinRef: a spawn() of each call, same
    actions, fresh buffers, launched eagerly on T),

and OracleRef answers the same calls from tests/oracle_tl.py's OracleTL on the CPU.

The tick bookkeeping this pins (lz_api.cpp fill_common; k_reset / k_step* / k_rollout*):
every launch reads ticks[p] / counters[p] and writes tick + tick_adv and a zeroed cursor
into slot 1 - p, p being a HOST parity baked into the captured node.  A replay therefore
only continues the sequence when it starts on the slot its predecessor's last node wrote.
"""
import ctypes

import numpy as np
import torch

from conftest import bits_equal
from oracle_tl import OracleTL, rollout_trace

SENTINEL = 12345.0  # prefill of a masked reset's obs buffer: rows of unselected envs keep it


def host(t):
    """Host copy of a device tensor after everything queued on any stream has finished."""
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def set_stream(env, stream):
    from gym_lorenz import _native as nat

    nat.check(nat.lib.lz_set_stream(env._h, ctypes.c_void_p(stream.cuda_stream)))


def _sorted_list(ids, tobs, m):
    order = np.argsort(ids[:m], kind="stable")
    return ids[:m][order].astype(np.int64), tobs[:m][order]


def same(got, want, where):
    """Two result dicts agree bit for bit (conftest.bits_equal: NaN-aware) key by key."""
    assert got.keys() == want.keys(), where
    for k in want:
        g, w = got[k], want[k]
        if np.isscalar(w) or np.ndim(w) == 0:
            assert int(g) == int(w), (where, k, int(g), int(w))
        elif np.asarray(w).dtype.kind in "iub":
            assert np.array_equal(g, w), (where, k)
        else:
            assert np.asarray(g).dtype == np.asarray(w).dtype, (where, k, "dtype")
            assert bits_equal(g, w), (where, k)


# ------------------------------------------------------------------ captured calls
class StepCall:
    """One lz_step into its own buffers (n_done_out included)."""
    kind, steps = "step", 1

    def __init__(self, env, actions):
        n, o, dev, td = env.num_envs, env.obs_dim, env.device, env.tdtype
        self.n, self.actions = n, actions  # actions: device float32 [N, A], or None (LORENZ4)
        self.obs = torch.empty((n, o), dtype=td, device=dev)
        self.rew = torch.empty((n,), dtype=td, device=dev)
        self.done = torch.empty((n,), dtype=torch.uint8, device=dev)
        self.didx = torch.empty((n,), dtype=torch.int32, device=dev)
        self.tobs = torch.empty((n, o), dtype=td, device=dev)
        self.nd = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.args = env.step_args(actions, self.obs, self.rew, self.done, self.didx, self.tobs, self.nd)

    def spawn(self, env):
        return StepCall(env, self.actions)

    def launch(self, env):
        from gym_lorenz import _native as nat

        nat.check(nat.lib.lz_step(env._h, *self.args))

    def ran(self):
        return int(host(self.nd)[0]) != -1

    def read(self):
        m = int(host(self.nd)[0])
        assert 0 <= m <= self.n, m
        ids, tobs = _sorted_list(host(self.didx), host(self.tobs), m)
        return {"obs": host(self.obs), "rew": host(self.rew), "done": host(self.done), "n_done": m,
                "didx": ids, "tobs": tobs}

    def done_per_step(self, res):
        return [int(np.count_nonzero(res["done"]))]


class RolloutCall:
    """One lz_rollout of K steps with the whole done list (cap = K * N) and n_done."""
    kind = "rollout"

    def __init__(self, env, actions):
        n, o, dev, td = env.num_envs, env.obs_dim, env.device, env.tdtype
        K = int(actions.shape[0])
        self.n, self.K, self.steps, self.actions = n, K, K, actions  # device float32 [K, N, A]
        self.obs = torch.empty((K, n, o), dtype=td, device=dev)
        self.rew = torch.empty((K, n), dtype=td, device=dev)
        self.done = torch.empty((K, n), dtype=torch.uint8, device=dev)
        self.didx = torch.empty((K * n,), dtype=torch.int64, device=dev)
        self.tobs = torch.empty((K * n, o), dtype=td, device=dev)
        self.nd = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.args = env.rollout_args(K, actions, self.obs, self.rew, self.done, self.didx, self.tobs,
                                     K * n, self.nd)

    def spawn(self, env):
        return RolloutCall(env, self.actions)

    def launch(self, env):
        from gym_lorenz import _native as nat

        nat.check(nat.lib.lz_rollout(env._h, *self.args))

    def ran(self):
        return int(host(self.nd)[0]) != -1

    def read(self):
        m = int(host(self.nd)[0])
        assert 0 <= m <= self.K * self.n, m
        ids, tobs = _sorted_list(host(self.didx), host(self.tobs), m)
        return {"obs": host(self.obs), "rew": host(self.rew), "done": host(self.done), "n_done": m,
                "didx": ids, "tobs": tobs}

    def done_per_step(self, res):
        return [int(np.count_nonzero(res["done"][k])) for k in range(self.K)]


class ResetCall:
    """lz_reset(mask) with device Philox draws into its own obs buffer; the rows of the
    unselected envs must keep the sentinel."""
    kind, steps = "reset", 0

    def __init__(self, env, mask):
        n, o, dev = env.num_envs, env.obs_dim, env.device
        self.n, self.mask_np = n, np.ascontiguousarray(mask, dtype=np.uint8)
        assert self.mask_np.shape == (n,)
        self.mask = torch.from_numpy(self.mask_np).to(dev)
        self.obs = torch.full((n, o), SENTINEL, dtype=env.tdtype, device=dev)

    def spawn(self, env):
        return ResetCall(env, self.mask_np)

    def launch(self, env):
        from gym_lorenz import _native as nat

        nat.check(nat.lib.lz_reset(env._h, ctypes.c_void_p(self.mask.data_ptr()), None,
                                   ctypes.c_void_p(self.obs.data_ptr())))

    def ran(self):
        return bool((host(self.obs) != SENTINEL).any())

    def read(self):
        o = host(self.obs)
        sel = self.mask_np != 0
        assert (o[~sel] == SENTINEL).all(), "a masked reset wrote the row of an unselected env"
        return {"obs_rows": o[sel]}

    def done_per_step(self, res):
        return []


class VnSide:
    """A handle with the VecNormalize state lz_step_vecnorm / lz_vecnorm_apply work on, all
    of it on the device: obs_rms, ret_rms (RunningMeanStd: mean, var, count) and returns.
    TRAINING | NORM_OBS | NORM_REWARD, clip 10 (bench.py::bench_vecnorm's settings)."""

    def __init__(self, env, stream=None):
        from gym_lorenz import _native as nat
        from gym_lorenz.vec_normalize import DeviceRunningMeanStd

        self.env = env
        self.obs_rms = DeviceRunningMeanStd(env.obs_dim, env.device, stream=stream)
        self.ret_rms = DeviceRunningMeanStd(1, env.device, stream=stream)
        self.returns = torch.zeros((env.num_envs,), dtype=torch.float64, device=env.device)
        vn = nat.LzVecNorm()
        vn.obs_rms, vn.ret_rms = self.obs_rms._h.value, self.ret_rms._h.value
        vn.returns = self.returns.data_ptr()
        vn.gamma, vn.epsilon, vn.clip_obs, vn.clip_reward = 0.99, 1e-8, 10.0, 10.0
        vn.flags = nat.VN_TRAINING | nat.VN_NORM_OBS | nat.VN_NORM_REWARD
        self.vn = vn

    def reset(self):
        """VecNormalize.reset: returns = 0 and the reset obs go into obs_rms (one update)."""
        obs = self.env.reset()
        self.returns.zero_()
        self.obs_rms.update(obs)
        return obs

    def stats(self):
        return {"obs_rms": host(self.obs_rms.state), "ret_rms": host(self.ret_rms.state),
                "returns": host(self.returns)}

    def close(self):
        self.obs_rms.close()
        self.ret_rms.close()
        self.env.close()


class PairCall:
    """lz_step_vecnorm + lz_vecnorm_apply as bench.py::bench_vecnorm lays them out: raw obs /
    reward / done, the done list int32 [N + 1] with the count in its last element, raw and
    normalised terminal rows, normalised obs / reward and the 0-1 dones -- all its own."""
    kind, steps = "pair", 1

    def __init__(self, env, actions):
        n, o, dev = env.num_envs, env.obs_dim, env.device
        self.n, self.actions = n, actions
        self.raw_o = torch.empty((n, o), device=dev)
        self.raw_r = torch.empty((n,), device=dev)
        self.done = torch.empty((n,), dtype=torch.uint8, device=dev)
        self.didx = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
        self.tobs = torch.empty((n, o), device=dev)
        self.obs_n = torch.empty((n, o), device=dev)
        self.rew_n = torch.empty((n,), device=dev)
        self.dones = torch.empty((n,), dtype=torch.uint8, device=dev)
        self.tn = torch.empty((n, o), device=dev)
        # lz_step_vecnorm takes lz_step's buffers: the same checked entry, as the bench
        env.step_args(actions, self.raw_o, self.raw_r, self.done, self.didx[:n], self.tobs, self.didx[n:])
        env.step_args(actions, self.obs_n, self.rew_n, self.dones)
        env.step_args(actions, self.tn, self.rew_n, self.dones)

    def spawn(self, env):
        return PairCall(env, self.actions)

    def launch(self, side):
        from gym_lorenz import _native as nat

        h, vn, nd = side.env._h, side.vn, self.didx.data_ptr() + 4 * self.n
        nat.check(nat.lib.lz_step_vecnorm(h, vn, self.actions.data_ptr(), self.raw_o.data_ptr(),
                                          self.raw_r.data_ptr(), self.done.data_ptr(), self.didx.data_ptr(),
                                          self.tobs.data_ptr(), nd))
        nat.check(nat.lib.lz_vecnorm_apply(h, vn, self.raw_o.data_ptr(), self.raw_r.data_ptr(),
                                           self.done.data_ptr(), self.obs_n.data_ptr(),
                                           self.rew_n.data_ptr(), self.dones.data_ptr(),
                                           self.tobs.data_ptr(), nd, self.tn.data_ptr()))

    def ran(self):
        return int(host(self.didx)[self.n]) != -1

    def read(self):
        d = host(self.didx)
        m = int(d[self.n])
        assert 0 <= m <= self.n, m
        order = np.argsort(d[:m], kind="stable")
        return {"obs": host(self.raw_o), "rew": host(self.raw_r), "done": host(self.done), "n_done": m,
                "didx": d[:m][order].astype(np.int64), "tobs": host(self.tobs)[:m][order],
                "obs_n": host(self.obs_n), "rew_n": host(self.rew_n), "dones": host(self.dones),
                "tobs_n": host(self.tn)[:m][order]}

    def done_per_step(self, res):
        return [int(np.count_nonzero(res["done"]))]


# ------------------------------------------------------------------ references
ORC_NAME = {"lorenz3": "l3", "lorenz4": "l4"}


class OracleRef:
    """The noise-free reference: OracleTL (independent of the GPU, its ticks explicit).
    Invariant: before any call the device's tick is tl.tick + 1 (lz_reset took tick 0)."""

    def __init__(self, orc, system, dtype, n, seed, limit):
        self.orc = orc
        self.tl = OracleTL(orc, ORC_NAME[system], np.dtype(dtype), n, seed, limit)

    def reset_all(self):
        return self.tl._reset_obs(self.tl.st)

    def _np(self, a):
        return None if a is None else host(a)

    def run(self, call):
        tl = self.tl
        if call.kind == "reset":  # the reset launch draws at its own tick and advances it by one
            tl.tick += 1
            idx = np.nonzero(call.mask_np)[0]
            fresh = self.orc.reset_draw_idx(tl.sys, tl.dt, idx, tl.seed, tl.tick)
            tl.st[idx] = fresh
            tl.steps[idx] = 0
            return {"obs_rows": tl._reset_obs(fresh)}
        if call.kind == "step":
            o, r, d, idx, term = tl.step(self._np(call.actions))
            return {"obs": o, "rew": r, "done": d, "n_done": idx.size, "didx": idx.astype(np.int64),
                    "tobs": term}
        assert call.kind == "rollout"
        t = rollout_trace(tl, self._np(call.actions))
        return {"obs": t["obs"], "rew": t["rew"], "done": t["done"], "n_done": t["didx"].size,
                "didx": t["didx"].astype(np.int64), "tobs": t["tobs"]}

    def planes(self):
        return [np.array(p) for p in self.tl.planes()]

    def close(self):
        pass


class TwinRef:
    """The device-noise reference: an eager twin handle T (same config and seed) that runs a
    spawn() of every call, eagerly, on the current stream.  Hardware v_log / v_sin / v_cos
    cannot be restated on the CPU; the eager path is pinned sample by sample in
    test_gpu_noise.py."""

    def __init__(self, env):
        self.env = self.target = env
        self.twins = {}

    def reset_all(self):
        return host(self.env.reset())

    def run(self, call):
        if call not in self.twins:
            self.twins[call] = call.spawn(self.env)
            torch.cuda.synchronize()
        tw = self.twins[call]
        tw.launch(self.target)
        return tw.read()

    def planes(self):
        return [host(self.env.get_state(p)) for p in range(self.env.info.n_planes)]

    def close(self):
        self.env.close()


class VnTwinRef(TwinRef):
    """TwinRef for PairCall: the twin handle with its own VecNormalize state."""

    def __init__(self, side):
        super().__init__(side.env)
        self.side = self.target = side

    def reset_all(self):
        return host(self.side.reset())

    def close(self):
        self.side.close()


# ------------------------------------------------------------------ the harness
class Tally:
    """Where the TimeLimit fires.  With `limit` set and every env reset together, step s
    (1-based since the reset) truncates every env iff s % limit == 0, and no other step ends
    an episode: n_done is asserted to be N on exactly those steps.  uniform=False (a masked
    reset inside the sequence staggers the episodes): only the total is kept."""

    def __init__(self, n, limit, uniform=True):
        self.n, self.limit, self.uniform, self.s, self.total = n, limit, uniform, 0, 0

    def add(self, call, res, where):
        per = call.done_per_step(res)
        assert len(per) == call.steps
        if call.steps:
            assert sum(per) == res["n_done"], (where, per, res["n_done"])
        for c in per:
            self.s += 1
            if self.uniform:
                assert c == (self.n if self.s % self.limit == 0 else 0), (where, self.s, c)
            self.total += c


def run_replay_case(g_target, g_env, st, ref, make_calls, make_eager, e0, limit, uniform=True,
                    warm=0, after_replay=None):
    """The whole case on the graph handle g_env (launch target g_target: the env itself, or
    its VnSide), bound to the side stream st (the default stream cannot be captured), against
    `ref`:

      reset | warm + e0 eager calls | capture make_calls() | 3 replays, each compared call by
      call with ref's next calls, two eager calls between replay 2 and 3 | every state
      plane | one more eager call.

    make_eager(): the Call used for the eager steps (its own buffers).  after_replay(tag, tally):
    extra comparisons after the reset, every eager call and every replay (tally.s: the steps
    taken so far).  Returns the Tally."""
    torch.cuda.synchronize()
    set_stream(g_env, st)
    tally = Tally(g_env.num_envs, limit, uniform)
    o0 = host(g_target.reset())
    w0 = ref.reset_all()
    assert o0.dtype == w0.dtype and bits_equal(o0, w0), "reset obs"
    if after_replay:
        after_replay("reset", tally)
    eager = make_eager()
    torch.cuda.synchronize()

    def eager_call(tag):
        eager.launch(g_target)
        got = eager.read()
        same(got, ref.run(eager), tag)
        tally.add(eager, got, tag)
        if after_replay:
            after_replay(tag, tally)

    for k in range(warm + e0):
        eager_call("warm-up %d" % k)
    calls = make_calls()
    assert len(calls) % 2 == 0, "a captured sequence holds an even number of calls"
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        for c in calls:
            c.launch(g_target)
    torch.cuda.synchronize()
    assert not any(c.ran() for c in calls), "captured, not run"
    for r in range(3):
        if r == 2:  # bench.py's pattern: eager calls between replays, an even number of them
            eager_call("eager 0 before replay 3")
            eager_call("eager 1 before replay 3")
        with torch.cuda.stream(st):
            gr.replay()
        torch.cuda.synchronize()
        for i, c in enumerate(calls):  # the reference's steps r * L .. r * L + L - 1
            got = c.read()
            same(got, ref.run(c), "replay %d call %d (%s)" % (r + 1, i, c.kind))
            tally.add(c, got, (r + 1, i))
        if after_replay:
            after_replay("replay %d" % (r + 1), tally)
    want = ref.planes()
    assert len(want) == g_env.info.n_planes
    for p, w in enumerate(want):
        got = host(g_env.get_state(p))
        assert got.dtype == w.dtype and bits_equal(got, w), ("plane", p)
    eager_call("eager after replay 3")  # the tick continues where the last replay left it
    return tally
