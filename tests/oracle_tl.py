"""Test helper (not a test module): the oracle env batch with gymnasium TimeLimit + SB3
DummyVecEnv auto-reset semantics, as the kernels run them (lz_body.h step_body):

  * step k after a reset uses RNG tick k + 1 (the reset launch took tick 0);
  * an env whose step counter reaches L is truncated (done bit 2), one whose own
    termination fires is terminated (bit 1: LORENZ4's reward < -1e6,
    lorenz_env_transient.py:369; PMSM's error sum > 1000, lorenz_env_try_pmsm.py:174;
    HR's |e| > 70, lorenz_env_try.py:174);
  * a done env keeps its pre-reset observation as the terminal observation and is reset
    in place from the Philox draws keyed by (seed, global env id, tick).

Drives oracle.l3_step / l4_step (Euler, the reference) or their RK4 mode
(l3_step_rk4 / l4_step_rk4), and, with process noise off, oracle.pmsm_step / hr_step in
mode DEV (the device's formulas).  What a reset keeps:

  * PMSM (lorenz_env_try_pmsm.py:59-75; lz_systems.h SysPMSM::store_reset /
    test_gpu_parity.py::test_autoreset_termination_pmsm): the six state values are redrawn
    and the episode step counter zeroes; lambda, Adam's m, v and its step counter persist.
  * HR (lorenz_env_try.py:49-79; SysHR::init / store_reset): master and slave are redrawn,
    the filter memory filtered_action zeroes, sigma is redrawn (0 with noise off).
"""
import numpy as np


class OracleTL:
    def __init__(self, orc, system, dtype, n, seed, L, steps0=None, rk4=False, gids=None,
                 alpha=0.5, params=None, add_filter=False):
        """gids: the global env ids of the n rows (a sample of a larger batch; default
        0 .. n - 1): the Philox draws are keyed by the global id, so any subset runs alone.
        alpha: PMSM's; params ({index: value} over oracle.PARAMS): PMSM's / HR's;
        add_filter: HR's."""
        self.orc, self.sys, self.dt, self.seed, self.L = orc, system, dtype, seed, L
        self.rk4 = rk4
        self.alpha, self.params, self.add_filter = alpha, params, add_filter
        self.gids = None if gids is None else np.ascontiguousarray(gids, dtype=np.int64)
        st = (orc.reset_draw(system, dtype, n, 0, seed, 0) if gids is None
              else orc.reset_draw_idx(system, dtype, self.gids, seed, 0))
        self.st = np.ascontiguousarray(st.copy())
        if system == "pmsm":    # st: the six state values; lambda / Adam in self.S
            self.S = orc.PmsmState(n)
            self.S.st = self.st
        elif system == "hr":    # st: master, slave; fa: the float32 filter memory; sigma
            self.sigma = self.st[:, 6].copy()
            self.st = np.ascontiguousarray(self.st[:, :6])
            self.fa = np.zeros((n, 2), np.float32)
        self.steps = (np.zeros(n, np.int64) if steps0 is None else steps0.astype(np.int64).copy())
        self.tick = 0

    def _reset_obs(self, fresh):
        orc = self.orc
        if self.sys == "l3":
            return orc.l3_reset_obs(fresh)
        if self.sys == "l4":
            return orc.l4_reset_obs(fresh)
        if self.sys == "pmsm":
            return orc.pmsm_reset_obs(fresh)
        return orc.hr_reset_obs(np.ascontiguousarray(fresh[:, :6]))

    def planes(self):
        """The state planes in lorenz_env.h's order, the episode step counter last."""
        cols = list(self.st.T)
        if self.sys == "pmsm":
            cols += [self.S.lam, self.S.m, self.S.v, self.S.adam_step]
        elif self.sys == "hr":
            cols += [self.sigma, self.fa[:, 0], self.fa[:, 1]]
        return cols + [self.steps.astype(np.int32)]

    def step(self, a=None):
        orc = self.orc
        self.tick += 1
        with np.errstate(all="ignore"):
            if self.sys == "l3":
                o, r = (orc.l3_step_rk4 if self.rk4 else orc.l3_step)(self.st, a)
                te = np.zeros(len(self.steps), bool)
            elif self.sys == "l4":
                o, r, te = (orc.l4_step_rk4 if self.rk4 else orc.l4_step)(self.st)
            elif self.sys == "pmsm":  # its own truncation (2000 steps) lies beyond any L used here
                o, r, te, _ = orc.pmsm_step(self.S, a, None, False, self.alpha, orc.DEV,
                                            params=self.params)
            else:
                o, r, te = orc.hr_step(self.st, self.fa, a, None, False, self.add_filter, orc.DEV,
                                       params=self.params)
        self.steps += 1
        tr = self.steps >= self.L if self.L else np.zeros(len(self.steps), bool)
        d = te.astype(np.uint8) | (tr.astype(np.uint8) << 1)
        idx = np.nonzero(d)[0]
        term = o[idx].copy()
        if idx.size:
            gi = idx if self.gids is None else self.gids[idx]
            fresh = orc.reset_draw_idx(self.sys, self.dt, gi, self.seed, self.tick)
            o[idx] = self._reset_obs(fresh)
            if self.sys == "hr":
                self.st[idx] = fresh[:, :6]
                self.sigma[idx] = fresh[:, 6]
                self.fa[idx] = 0
            else:
                self.st[idx] = fresh
            if self.sys == "pmsm":
                self.S.cur_step[idx] = 0  # lam, m, v, adam_step persist
            self.steps[idx] = 0
        return o, r, d, idx, term


def rollout_trace(ref, actions):
    """K = len(actions) steps of the OracleTL `ref` as one fused rollout reports them: a
    dict of obs [K, n, O], rew [K, n], done [K, n], the captured done list (didx: flat ids
    k * n + env in ascending order, tobs: their terminal observations) and the final state
    planes (OracleTL.planes)."""
    n = len(ref.steps)
    obs, rew, done, didx, tobs = [], [], [], [], []
    for k, a in enumerate(actions):
        o, r, d, idx, term = ref.step(a)
        obs.append(o.copy())
        rew.append(r.copy())
        done.append(d.copy())
        didx.append(k * n + idx)
        tobs.append(term)
    return {"obs": np.stack(obs), "rew": np.stack(rew), "done": np.stack(done),
            "didx": np.concatenate(didx), "tobs": np.concatenate(tobs),
            "planes": [np.array(p) for p in ref.planes()]}


def assert_same_trace(got, want, bits_equal, rew_ok=None, planes=None):
    """Two rollout_trace dicts agree bit for bit, NaN-aware: every step's obs, reward and
    done byte, the done list (ids and terminal observations) and the final state planes
    (`planes`: the plane ids to compare, default all).  rew_ok(got, want) replaces the
    reward's bit comparison where a case has a stated reason."""
    for k in range(want["obs"].shape[0]):
        assert bits_equal(got["obs"][k], want["obs"][k]), ("obs", k)
        assert (rew_ok or bits_equal)(got["rew"][k], want["rew"][k]), ("rew", k)
        assert np.array_equal(got["done"][k], want["done"][k]), ("done", k)
    assert np.array_equal(got["didx"], want["didx"]), "done list ids"
    assert bits_equal(got["tobs"], want["tobs"]), "terminal observations"
    assert len(got["planes"]) == len(want["planes"])
    for p in (range(len(want["planes"])) if planes is None else planes):
        assert got["planes"][p].dtype == want["planes"][p].dtype, ("plane dtype", p)
        assert bits_equal(got["planes"][p], want["planes"][p]), ("plane", p)
