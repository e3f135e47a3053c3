"""Test helper (not a test module): teacher-forced (env, step) pairs of the reference's
float64 trajectories, for the per-step float32 accuracy gate of BASELINE.md ("per-step
fp32 state error < 1e-5 vs CPU reference") on every system but LORENZ3 (which has its own
test, test_gpu_parity.py::test_l3_f32_teacher_forced_vs_reference).

pairs(orc, key), key in l4 / hr / t1 / t2 / tp / sc, replays the float64 oracle in mode REF
along the committed fixture (l4.npz, hr.npz, legacy.npz), asserting on the way that every
step's observation equals the fixture bit for bit (as tests/test_oracle_golden.py does; HR:
the states equal state_master / state_slave too), and returns per pair the full state
before the step, the action, the injected noise and the float64 state / obs / reward /
termination after it.  l4.npz, t2 and tp hold only observations (differences), which is why
the states come from the replay.  A pair is kept if its states before and after are finite
and |next state| < 1e6 (the filter of the LORENZ3 test).

step_f32_oracle() takes the one float32 step with the oracle (the host test);
tests/test_gpu_teacher_forced.py takes it with the kernels; measure() / assert_gates() are
the figures and the bars both are held to:

  * state: |d| / max(|s|, 1) < 1e-5 against the reference's float64 next state;
  * the non-cancelling observation components (HR's six; the m - s half of L4 / T2 / TP;
    the state half of T1 / SC) and the reward: the same measure < 1e-5 against the float64
    formula evaluated at the float32 next state itself (cast to float64) -- that separates
    the formula's error from the step's; T2 / TP rewards (-S - S**(1/3), -S - S**0.1, a pow)
    by rtol 1e-6 (the rule of test_gpu_legacy.py);
  * L4's derivative half f(m) - f(s) cancels: |d_j| / max(c_j, 1), c_j the sum of the
    absolute values of the terms of f_j(m) and f_j(s) (the four lines of l4_rhs).  The
    float32 oracle's maximum over all 12,000 pairs, measured by the host test, is
    L4_DERIV_SCALED_MAX; the kernel is held to twice that.
"""
import functools

import numpy as np

from conftest import bits_equal, golden

SYSTEMS = ("l4", "hr", "t1", "t2", "tp", "sc")
NAMES = {"l4": "lorenz4", "hr": "hr", "t1": "transient1", "t2": "transient2",
         "tp": "transient_pmsm", "sc": "singlecontrol"}
STATE_BOUND = 1e-5          # BASELINE.md north star, per step
# the fraction of the fixture's pairs the finite / < 1e6 filter must keep (T2's driven
# slave overflows by design of the fixture: 4,676 of 4,800 kept)
MIN_KEPT = {"l4": 1.0, "hr": 1.0, "t1": 1.0, "t2": 0.97, "tp": 1.0, "sc": 1.0}
# non-cancelling observation components
OBS_PLAIN = {"l4": slice(0, 4), "hr": slice(0, 6), "t1": slice(0, 3), "t2": slice(0, 4),
             "tp": slice(0, 3), "sc": slice(0, 3)}
POW_REWARD = ("t2", "tp")
# The float32 oracle's largest scaled error of L4's derivative half over the 12,000 pairs,
# as tests/test_teacher_forced_host.py measures (and asserts) it; DESIGN.md section 5.
L4_DERIV_SCALED_MAX = 1.20e-7


def _keep(before, after):
    return (np.isfinite(before).all(-1) & np.isfinite(after).all(-1)
            & (np.abs(after) < 1e6).all(-1))


def _replay_l4(orc):
    g = golden("l4")
    st = g["init"].copy()
    n, T = g["obs"].shape[:2]
    out = {k: [] for k in ("before", "after", "obs", "rew", "term")}
    with np.errstate(all="ignore"):
        for k in range(T):
            out["before"].append(st.copy())
            o, r, d = orc.l4_step(st)
            assert bits_equal(o, g["obs"][:, k]), k
            for key, v in (("after", st), ("obs", o), ("rew", r), ("term", d)):
                out[key].append(v.copy())
    P = {k: np.stack(v, 1).reshape((n * T,) + v[0].shape[1:]) for k, v in out.items()}
    P["act"] = g["actions"].reshape(n * T, 3)
    return P


def _replay_hr(orc):
    g = golden("hr")
    n, T = g["obs"].shape[:2]
    cols = {k: [] for k in ("before", "fa", "after", "obs", "rew", "term")}
    with np.errstate(all="ignore"):
        for i in range(n):
            st = g["init"][i, :6].reshape(1, 6).copy()
            fa = np.zeros((1, 2), np.float32)
            for k in range(T):
                cols["before"].append(st[0].copy())
                cols["fa"].append(fa[0].copy())
                o, r, t = orc.hr_step(st, fa, g["actions"][i, k][None], g["noise"][i, k][None],
                                      bool(g["add_noise"][i]), bool(g["add_filter"][i]), orc.REF)
                assert bits_equal(o[0].astype(np.float32), g["obs"][i, k]), (i, k)
                assert bits_equal(st[0, :3], g["state_master"][i, k]), (i, k)
                assert bits_equal(st[0, 3:], g["state_slave"][i, k]), (i, k)
                for key, v in (("after", st[0]), ("obs", o[0]), ("rew", r[0]), ("term", t[0])):
                    cols[key].append(np.copy(v))
    P = {k: np.array(v) for k, v in cols.items()}
    P["act"] = g["actions"].reshape(n * T, 2)
    P["noise"] = g["noise"].reshape(n * T, 3)
    P["sigma"] = np.repeat(g["init"][:, 6], T)
    P["add_noise"] = np.repeat(g["add_noise"].astype(bool), T)
    P["add_filter"] = np.repeat(g["add_filter"].astype(bool), T)
    return P


def _replay_legacy(orc, key):
    g = golden("legacy")
    st = np.array(g[key + "_init"], np.float64)  # a copy: stepped in place, golden() is shared
    n, T = g[key + "_obs"].shape[:2]
    out = {k: [] for k in ("before", "after", "obs", "rew", "term")}
    with np.errstate(all="ignore"):
        for k in range(T):
            out["before"].append(st.copy())
            a = None if key == "sc" else g[key + "_actions"][:, k]
            nz = g[key + "_noise"][:, k] if key in ("tp", "sc") else None
            o, r, d = orc.legacy_step(key, st, a, nz)
            assert bits_equal(o, g[key + "_obs"][:, k]), k
            for name, v in (("after", st), ("obs", o), ("rew", r), ("term", d)):
                out[name].append(v.copy())
    P = {k: np.stack(v, 1).reshape((n * T,) + v[0].shape[1:]) for k, v in out.items()}
    acts = g[key + "_actions"]
    P["act"] = acts.reshape(n * T, acts.shape[2])
    if key in ("tp", "sc"):
        P["noise"] = g[key + "_noise"].reshape(n * T, 3)
    return P


@functools.lru_cache(maxsize=None)
def pairs(orc, key):
    """The kept pairs of system `key` (computed once per session; do not modify): a dict of
    arrays with one row per pair -- before / after (float64 states), act (float32), noise
    (float64 [P, 3], TP / SC / HR), obs / rew / term after the step; HR also fa (float32
    [P, 2], the filter memory before the step), sigma, add_noise, add_filter -- plus the
    scalars total (the fixture's pairs) and kept."""
    P = _replay_l4(orc) if key == "l4" else _replay_hr(orc) if key == "hr" else _replay_legacy(orc, key)
    keep = _keep(P["before"], P["after"])
    total = keep.size
    P = {k: np.ascontiguousarray(v[keep]) for k, v in P.items()}
    for v in P.values():
        v.setflags(write=False)
    P["total"], P["kept"] = total, int(keep.sum())
    assert P["kept"] >= MIN_KEPT[key] * total, (key, P["kept"], total)
    return P


def hr_groups(P):
    """HR's pairs by (add_noise, add_filter): [(add_noise, add_filter, row indices)]."""
    out = []
    for an in (False, True):
        for af in (False, True):
            idx = np.nonzero((P["add_noise"] == an) & (P["add_filter"] == af))[0]
            if idx.size:
                out.append((an, af, idx))
    return out


def hr_filter_f32(orc, fa, act):
    """lorenz_env_try.py:85-86 in float32: (1 - alpha) * fa + alpha * action."""
    al = orc.PARAMS["hr"][11]
    f1m, fal = np.float32(1.0 - al), np.float32(al)
    return f1m * fa.astype(np.float32) + fal * act.astype(np.float32)


def step_f32_oracle(orc, key, P):
    """One float32 oracle step from the rounded `before` states (HR: mode DEV).  Returns
    after (float32 states), obs, rew, term and, for HR, fa."""
    st = np.ascontiguousarray(P["before"], np.float32)
    with np.errstate(all="ignore"):
        if key == "l4":
            o, r, t = orc.l4_step(st)
            return {"after": st, "obs": o, "rew": r, "term": t}
        if key == "hr":
            n = st.shape[0]
            fa = P["fa"].copy()
            o, r, t = np.empty((n, 6), np.float32), np.empty(n, np.float32), np.empty(n, bool)
            for an, af, idx in hr_groups(P):
                s, f = np.ascontiguousarray(st[idx]), np.ascontiguousarray(fa[idx])
                o[idx], r[idx], t[idx] = orc.hr_step(s, f, P["act"][idx],
                                                     P["noise"][idx].astype(np.float32), an, af, orc.DEV)
                st[idx], fa[idx] = s, f
            return {"after": st, "obs": o, "rew": r, "term": t, "fa": fa}
        o, r, t = orc.legacy_step(key, st, None if key == "sc" else P["act"], P.get("noise"))
        return {"after": st, "obs": o, "rew": r, "term": t}


def l4_deriv_scale(orc, st):
    """c_j of L4's derivative half at the states st [n, 8] (float64): the sum of the
    absolute values of the terms of f_j(m) and f_j(s), lorenz_env_transient.py:323-326:
      f0 = a (s1 - s0) + s3;  f1 = (c s0 - s1) - s0 s2;  f2 = s0 s1 - b s2;  f3 = (-s0) s1 - b s2"""
    a, b, c = orc.PARAMS["l4"][:3]
    tot = np.zeros((st.shape[0], 4))
    for s in (st[:, :4], st[:, 4:]):
        s0, s1, s2, s3 = (np.abs(s[:, j]) for j in range(4))
        tot[:, 0] += a * s1 + a * s0 + s3
        tot[:, 1] += c * s0 + s1 + s0 * s2
        tot[:, 2] += s0 * s1 + b * s2
        tot[:, 3] += s0 * s1 + b * s2
    return tot


def formula_f64(orc, key, P, st32, term):
    """(obs, reward) of the reference's float64 formulas at the float32 states st32 (cast
    to float64); term: the step's own termination flags (HR's reward is -2000 there)."""
    s = np.ascontiguousarray(st32, np.float64)
    with np.errstate(all="ignore"):
        if key == "l4":
            o = orc.l4_reset_obs(s)
            return o, -np.abs(o[:, :4]).sum(1)
        if key == "hr":
            p = orc.PARAMS["hr"]
            o = np.concatenate([(s[:, :3] - s[:, 3:]) / p[9], np.clip(s[:, :3] / p[10], -1.0, 1.0)], 1)
            a = P["act"].astype(np.float32)
            pen = np.float32(0.05) * (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])  # float32, :160-165
            r = -np.abs(o[:, :3]).sum(1) - pen.astype(np.float64)
            return o, np.where(term, -2000.0, r)
        o = orc.legacy_reset_obs(key, s)
        S = np.abs(o[:, OBS_PLAIN[key]]).sum(1)
        if key == "t2":
            return o, -S - S ** (1.0 / 3.0)
        if key == "tp":
            return o, -S - S ** 0.1
        return o, -S


def _rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1.0)


def measure(orc, key, P, got):
    """The figures of one float32 step `got` (after, obs, rew, term[, fa]) from P's `before`
    states: the maxima of the measures in the module docstring."""
    fo, fr = formula_f64(orc, key, P, got["after"], got["term"])
    sl = OBS_PLAIN[key]
    fig = {"pairs": P["kept"], "total": P["total"],
           "state": float(_rel(got["after"], P["after"]).max()),
           "obs": float(_rel(got["obs"][:, sl], fo[:, sl]).max()),
           "reward": float(_rel(got["rew"], fr).max()),
           "term_mismatch": int((np.asarray(got["term"], bool) != P["term"]).sum())}
    if key in POW_REWARD:
        fig["reward_rtol"] = float((np.abs(got["rew"].astype(np.float64) - fr) / np.abs(fr)).max())
    if key == "l4":
        c = l4_deriv_scale(orc, np.asarray(got["after"], np.float64))
        fig["deriv_plain"] = float(_rel(got["obs"][:, 4:], fo[:, 4:]).max())
        fig["deriv_scaled"] = float((np.abs(got["obs"][:, 4:].astype(np.float64) - fo[:, 4:])
                                     / np.maximum(c, 1.0)).max())
    if key == "hr":
        f = P["add_filter"]
        want = hr_filter_f32(orc, P["fa"][f], P["act"][f])
        fig["fa_bits_equal"] = bool(bits_equal(got["fa"][f], want))
        fig["terminations"] = int(P["term"].sum())
    return fig


def assert_gates(key, fig, deriv_factor):
    """The bars.  deriv_factor: L4's scaled derivative error may reach deriv_factor x
    L4_DERIV_SCALED_MAX (1 for the oracle that defines it, 2 for the kernel: the margin
    covers only a differently contracted fma)."""
    print("teacher-forced %s: %s" % (key, ", ".join("%s=%.3g" % (k, v) if isinstance(v, float)
                                                     else "%s=%s" % (k, v) for k, v in fig.items())))
    assert fig["pairs"] >= MIN_KEPT[key] * fig["total"], fig
    assert fig["state"] < STATE_BOUND, fig
    assert fig["obs"] < STATE_BOUND, fig
    if key in POW_REWARD:
        assert fig["reward_rtol"] <= 1e-6, fig
    else:
        assert fig["reward"] < STATE_BOUND, fig
    if key == "hr":
        assert fig["term_mismatch"] == 0 and fig["terminations"] > 0, fig
        assert fig["fa_bits_equal"], fig
    if key == "l4":
        assert fig["deriv_scaled"] <= deriv_factor * L4_DERIV_SCALED_MAX, fig
