"""The fused policy evaluation without a GPU: the evaluator's semantics (tests/eval_ref.py)
against the reference's own closed-loop traces, the episode bookkeeping on hand-built
done patterns, and the C ABI of lz_evaluate_policy_*_f32 (struct layout, column enum,
argument refusals that need no handle).  lz_create needs a device, so the refusals that
depend on the handle (float64, RK4, legacy systems, call order) are in
tests/test_gpu_eval.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eval_ref as er
from conftest import ROOT
from test_policy_f32_host import GOLD, oracle_closed_loop

HEADER = os.path.join(ROOT, "include", "lorenz_env.h")


@pytest.fixture(scope="module")
def nat():
    from gym_lorenz import _native

    return _native


# ----------------------------------------------------------------------- reference agreement
def test_eval_ref_vs_reference_traces(orc):
    """code/lorenz_pmsm/test_evaluate.py's closed loop for the eight trained policies: the
    evaluator's MAE / RMSE over steps 1000..1998 of the oracle loop against the same
    figures of the reference's own traces (gold cpu_e), at the f2 bar of 1e-4 relative."""
    gold = np.load(GOLD)
    K = 1999
    for j in range(8):
        _, _, e, _ = oracle_closed_loop(gold, j, orc, steps=K)
        o = np.zeros((K, 1, 6), np.float32)
        o[:, 0, :3] = e
        T = er.eval_ref(o, np.zeros((K, 1), np.float32), np.zeros((K, 1), np.uint8), False, skip=1000)
        got = er.pooled(T)
        ref = gold["cpu_e"][j][1000:1999].astype(np.float64)
        assert np.abs(e).max() < 100.0  # PMSM terminates past |e| = 100: no env does
        mae, rmse = np.mean(np.abs(ref)), np.sqrt(np.mean(ref ** 2))
        print("alpha=%.3f: MAE %.6f vs %.6f, RMSE %.6f vs %.6f" % (gold["alphas"][j], got["mae"], mae,
                                                                   got["rmse"], rmse))
        assert T[er.N_WIN, 0] == 999 and T[er.N_STEPS, 0] == K
        assert abs(got["mae"] - mae) <= 1e-4 * mae
        assert abs(got["rmse"] - rmse) <= 1e-4 * rmse


# ----------------------------------------------------------------------- episode bookkeeping
def _case(K=8, n=3, seed=0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(K, n, 6)).astype(np.float32)
    r = rng.normal(size=(K, n)).astype(np.float32)
    return o, r


def test_bookkeeping_autoreset_cutoff_and_tail():
    o, r = _case()
    d = np.zeros((8, 3), np.uint8)
    d[2, 0] = 2          # env 0: episodes of 3, 2 steps, then a 3-step tail
    d[4, 0] = 1
    d[1, 1] = d[3, 1] = d[5, 1] = d[7, 1] = 2   # env 1: four 2-step episodes
    # env 2: never done
    T = er.eval_ref(o, r, d, True, skip=1, max_episodes=2)
    r64 = r.astype(np.float64)
    # env 0: both episodes counted, the tail (ep = 2) is not
    assert T[er.N_EP, 0] == 2 and T[er.N_STEPS, 0] == 5 and T[er.EP_LEN_SUM, 0] == 5
    e0, e1 = r64[0, 0] + r64[1, 0] + r64[2, 0], r64[3, 0] + r64[4, 0]
    assert T[er.EP_RET_SUM, 0] == e0 + e1 and T[er.EP_RET_SQ, 0] == e0 * e0 + e1 * e1
    assert T[er.TAIL_RET, 0] == 0.0 and T[er.TAIL_LEN, 0] == 0
    assert T[er.N_WIN, 0] == 3           # t = 1, 2 of episode 0 and t = 1 of episode 1
    a = np.abs(o[:, 0, :3]).astype(np.float64)
    assert np.array_equal(T[er.ABS_SUM0:er.ABS_SUM0 + 3, 0], (a[1] + a[2]) + a[4])
    assert np.array_equal(T[er.SQ_SUM0:er.SQ_SUM0 + 3, 0], (a[1] ** 2 + a[2] ** 2) + a[4] ** 2)
    assert np.array_equal(T[er.MAX_ABS0:er.MAX_ABS0 + 3, 0], np.max(a[[1, 2, 4]], axis=0))
    assert T[er.FIRST_DONE, 0] == 2 and T[er.DONE_OR, 0] == 3 and T[er.N_DONE_STEPS, 0] == 2
    assert (T[[3, 7, 11], :] == 0).all()  # the unused fourth error dim
    # env 1: episodes 2 and 3 run uncounted but their dones are still seen
    assert T[er.N_EP, 1] == 2 and T[er.N_STEPS, 1] == 4 and T[er.N_DONE_STEPS, 1] == 4
    assert T[er.RET_SUM, 1] == ((r64[0, 1] + r64[1, 1]) + r64[2, 1]) + r64[3, 1]
    assert T[er.FIRST_DONE, 1] == 1 and T[er.DONE_OR, 1] == 2
    # env 2: one unfinished counted episode
    assert T[er.N_EP, 2] == 0 and T[er.TAIL_LEN, 2] == 8 and T[er.FIRST_DONE, 2] == -1
    tail = 0.0
    for k in range(8):
        tail += r64[k, 2]
    assert T[er.TAIL_RET, 2] == tail == T[er.RET_SUM, 2] and T[er.N_WIN, 2] == 7
    p = er.pooled(T)
    n_ep = 4
    mean = T[er.EP_RET_SUM].sum() / n_ep
    assert p["mean_reward"] == mean and p["mean_ep_length"] == (5 + 4) / 4
    assert p["std_reward"] == np.sqrt(max(T[er.EP_RET_SQ].sum() / n_ep - mean * mean, 0.0))
    # max_episodes = 0: every step counts
    T0 = er.eval_ref(o, r, d, True, skip=0, max_episodes=0)
    assert (T0[er.N_STEPS] == 8).all() and T0[er.N_EP, 1] == 4 and T0[er.TAIL_LEN, 0] == 3


def test_bookkeeping_without_autoreset():
    """Nothing restarts: t stays k, no episode is closed, the whole run is the tail."""
    o, r = _case(seed=1)
    d = np.zeros((8, 3), np.uint8)
    d[3:, 0] = 1
    T = er.eval_ref(o, r, d, False, skip=5, max_episodes=1)
    assert (T[er.N_EP] == 0).all() and (T[er.EP_RET_SUM] == 0).all()
    assert (T[er.N_STEPS] == 8).all() and (T[er.TAIL_LEN] == 8).all() and (T[er.N_WIN] == 3).all()
    assert T[er.FIRST_DONE, 0] == 3 and T[er.N_DONE_STEPS, 0] == 5 and T[er.DONE_OR, 0] == 1
    assert np.array_equal(T[er.TAIL_RET], T[er.RET_SUM])
    p = er.pooled(T)
    assert np.isnan(p["mean_reward"]) and np.isnan(p["std_reward"]) and np.isnan(p["mean_ep_length"])
    a = np.abs(o[5:, :, :3]).astype(np.float64)
    assert abs(p["mae"] - a.mean()) <= 27 * 2.0 ** -52 * a.mean()  # 27 positive summands
    assert abs(p["rmse"] - np.sqrt((a * a).mean())) <= 27 * 2.0 ** -52 * p["rmse"]


def test_nan_in_window_is_sticky():
    o, r = _case(seed=2)
    o[4, 1, 0] = np.nan
    o[2, 2, 1] = np.nan      # before the window: not seen
    T = er.eval_ref(o, r, np.zeros((8, 3), np.uint8), False, skip=3)
    assert np.isnan(T[er.ABS_SUM0, 1]) and np.isnan(T[er.SQ_SUM0, 1]) and np.isnan(T[er.MAX_ABS0, 1])
    assert np.isfinite(T[:, 0]).all() and np.isfinite(T[:, 2]).all()
    assert np.isfinite(T[[1, 2, 5, 6, 9, 10], 1]).all()
    assert np.isnan(er.pooled(T)["max_abs"]) and np.isnan(er.pooled(T)["mae"])


# ----------------------------------------------------------------------------------- ABI
def test_eval_struct_and_enum_match_header(nat, tmp_path):
    names = ["LZ_EVAL_ABS_SUM0", "LZ_EVAL_SQ_SUM0", "LZ_EVAL_MAX_ABS0", "LZ_EVAL_N_WIN", "LZ_EVAL_RET_SUM",
             "LZ_EVAL_N_STEPS", "LZ_EVAL_N_EP", "LZ_EVAL_EP_RET_SUM", "LZ_EVAL_EP_RET_SQ",
             "LZ_EVAL_EP_LEN_SUM", "LZ_EVAL_TAIL_RET", "LZ_EVAL_TAIL_LEN", "LZ_EVAL_FIRST_DONE",
             "LZ_EVAL_DONE_OR", "LZ_EVAL_N_DONE_STEPS", "LZ_EVAL_COLS", "LZ_EVAL_ABS_SUM3",
             "LZ_EVAL_SQ_SUM3", "LZ_EVAL_MAX_ABS3", "LZ_CALL_EVALUATE_POLICY_F32",
             "LZ_CALL_EVALUATE_POLICY_ATTN_F32", "LZ_CALL_EVALUATE_POLICY_ATTN_STACK_F32",
             "LZ_KERNEL_EVAL", "LZ_KERNEL_EVAL_ATTN_F32", "LZ_ABI_VERSION"]
    fields = [f for f, _ in nat.LzPolicyEvalArgs._fields_]
    c = tmp_path / "probe_eval.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "lorenz_env.h"\n'
        "int main(void){printf(\"%zu\", sizeof(lz_policy_eval_args));\n"
        + "".join('printf(" %%zu", offsetof(lz_policy_eval_args, %s));\n' % f for f in fields)
        + "".join('printf(" %%d", (int)%s);\n' % n for n in names)
        + "return 0;}\n")
    exe = tmp_path / "probe_eval"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = nat.LzPolicyEvalArgs
    want = [ctypes.sizeof(E)] + [getattr(E, f).offset for f in fields]
    assert got[:len(want)] == want
    assert fields == ["K", "flags", "blob", "obs_in", "obs_last", "obs_norm", "norm_eps", "clip_obs",
                      "act_low", "act_high", "skip", "max_episodes", "stats"]
    enum = got[len(want):]
    assert enum == [0, 4, 8, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 3, 7, 11, 10, 11, 12,
                    14, 15, 2]
    assert enum[:16] == [nat.EVAL_ABS_SUM0, nat.EVAL_SQ_SUM0, nat.EVAL_MAX_ABS0, nat.EVAL_N_WIN,
                         nat.EVAL_RET_SUM, nat.EVAL_N_STEPS, nat.EVAL_N_EP, nat.EVAL_EP_RET_SUM,
                         nat.EVAL_EP_RET_SQ, nat.EVAL_EP_LEN_SUM, nat.EVAL_TAIL_RET, nat.EVAL_TAIL_LEN,
                         nat.EVAL_FIRST_DONE, nat.EVAL_DONE_OR, nat.EVAL_N_DONE_STEPS, nat.EVAL_COLS]
    assert len(nat.EVAL_COLUMNS) == nat.EVAL_COLS == er.COLS == 24
    assert [nat.CALL_EVALUATE_POLICY_F32, nat.CALL_EVALUATE_POLICY_ATTN_F32,
            nat.CALL_EVALUATE_POLICY_ATTN_STACK_F32] == [10, 11, 12]
    assert nat.KERNELS[14] == "eval" and nat.KERNELS[15] == "eval_attn_f32"
    for name in ("n_win", "ret_sum", "ep_ret_sq", "tail_len", "n_done_steps"):  # the named views
        assert nat.EVAL_COLUMNS.index(name) == getattr(nat, "EVAL_" + name.upper())


def test_eval_null_arguments_are_refused(nat):
    """NULL handle / args never reach a dereference: LZ_ERR_INVALID with a message."""
    e = nat.LzPolicyEvalArgs()
    assert nat.lib.lz_evaluate_policy_f32(None, ctypes.byref(e)) == nat.LZ_ERR_INVALID
    assert b"NULL" in nat.lib.lz_last_error()
    assert nat.lib.lz_evaluate_policy_attn_f32(None, ctypes.byref(e)) == nat.LZ_ERR_INVALID
    assert nat.lib.lz_evaluate_policy_attn_stack_f32(None, ctypes.byref(e), 4, None, None) == nat.LZ_ERR_INVALID
    assert nat.lib.lz_evaluate_policy_f32(None, None) == nat.LZ_ERR_INVALID


def test_evaluator_is_exported():
    import gym_lorenz
    from gym_lorenz import policy

    assert gym_lorenz.FusedEvaluator is policy.FusedEvaluator
    assert gym_lorenz.EvalResult is policy.EvalResult
    assert gym_lorenz.evaluate_policy is policy.evaluate_policy
    assert policy.ERR_SCALE == er.ERR_SCALE and policy.ERR_DIMS == er.ERR_DIMS
