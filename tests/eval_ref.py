"""The evaluator's semantics (include/lorenz_env.h LZ_EVAL_*) restated in NumPy float64:
what lz_evaluate_policy_*_f32 accumulates per env, from per-step arrays.  A helper for
tests/test_eval_host.py and tests/test_gpu_eval.py, not a test."""
import numpy as np

COLS = 24
(ABS_SUM0, SQ_SUM0, MAX_ABS0) = 0, 4, 8
(N_WIN, RET_SUM, N_STEPS, N_EP, EP_RET_SUM, EP_RET_SQ, EP_LEN_SUM, TAIL_RET, TAIL_LEN, FIRST_DONE,
 DONE_OR, N_DONE_STEPS) = range(12, 24)
ERR_DIMS = {"lorenz3": 3, "lorenz4": 4, "pmsm": 3, "hr": 3}
ERR_SCALE = {"lorenz3": 1.0, "lorenz4": 1.0, "pmsm": 1.0, "hr": 50.0}


def eval_ref(o, r, d, autoreset, skip=0, max_episodes=0, err_dims=3):
    """o float32 [K, n, O]: each step's observation before any auto-reset; r float32 [K, n]
    rewards; d uint8 [K, n] done bits.  Returns the float64 [24, n] table."""
    o = np.asarray(o, np.float32)
    r = np.asarray(r, np.float32)
    d = np.asarray(d, np.uint8)
    K, n = r.shape
    T = np.zeros((COLS, n), np.float64)
    T[FIRST_DONE] = -1.0
    t = np.zeros(n, np.int64)
    ep = np.zeros(n, np.int64)
    ep_ret = np.zeros(n, np.float64)
    ep_len = np.zeros(n, np.int64)
    done_or = np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            counted = (ep < max_episodes) if max_episodes else np.ones(n, bool)
            rk = r[k].astype(np.float64)
            T[RET_SUM] = np.where(counted, T[RET_SUM] + rk, T[RET_SUM])
            T[N_STEPS] += counted
            ep_ret = np.where(counted, ep_ret + rk, ep_ret)
            ep_len += counted
            win = counted & (t >= skip)
            for j in range(err_dims):
                a = np.abs(o[k, :, j]).astype(np.float64)
                T[ABS_SUM0 + j] = np.where(win, T[ABS_SUM0 + j] + a, T[ABS_SUM0 + j])
                T[SQ_SUM0 + j] = np.where(win, T[SQ_SUM0 + j] + a * a, T[SQ_SUM0 + j])
                m = T[MAX_ABS0 + j]
                T[MAX_ABS0 + j] = np.where(win & ((a > m) | np.isnan(a)), a, m)
            T[N_WIN] += win
            t += 1
            dn = d[k] != 0
            done_or |= np.where(dn, d[k], 0).astype(np.uint8)
            T[N_DONE_STEPS] += dn
            T[FIRST_DONE] = np.where(dn & (T[FIRST_DONE] < 0), float(k), T[FIRST_DONE])
            if autoreset:
                fin = dn & counted
                T[N_EP] += fin
                T[EP_RET_SUM] = np.where(fin, T[EP_RET_SUM] + ep_ret, T[EP_RET_SUM])
                T[EP_RET_SQ] = np.where(fin, T[EP_RET_SQ] + ep_ret * ep_ret, T[EP_RET_SQ])
                T[EP_LEN_SUM] += np.where(fin, ep_len, 0)
                ep += dn
                t[dn] = 0
                ep_ret = np.where(dn, 0.0, ep_ret)
                ep_len[dn] = 0
    T[TAIL_RET] = ep_ret
    T[TAIL_LEN] = ep_len
    T[DONE_OR] = done_or
    return T


def pooled(T, err_dims=3, err_scale=1.0):
    """The pooled figures of a table (gym_lorenz.policy.EvalResult's formulas)."""
    s = T.sum(axis=1)
    n_win, ED, c = s[N_WIN], err_dims, err_scale
    nan = float("nan")
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        ab, sq = s[ABS_SUM0:ABS_SUM0 + ED], s[SQ_SUM0:SQ_SUM0 + ED]
        out["mae"] = c * ab.sum() / (ED * n_win) if n_win else nan
        out["rmse"] = c * np.sqrt(sq.sum() / (ED * n_win)) if n_win else nan
        out["mae_per_dim"] = [c * v / n_win if n_win else nan for v in ab]
        out["rmse_per_dim"] = [c * np.sqrt(v / n_win) if n_win else nan for v in sq]
        m = T[MAX_ABS0:MAX_ABS0 + ED]
        out["max_abs"] = nan if np.isnan(m).any() else c * m.max()
        n_ep = s[N_EP]
        if n_ep:
            mean = s[EP_RET_SUM] / n_ep
            out["mean_reward"] = mean
            out["std_reward"] = np.sqrt(max(s[EP_RET_SQ] / n_ep - mean * mean, 0.0))
            out["mean_ep_length"] = s[EP_LEN_SUM] / n_ep
        else:
            out["mean_reward"] = out["std_reward"] = out["mean_ep_length"] = nan
        out["mean_step_reward"] = s[RET_SUM] / s[N_STEPS] if s[N_STEPS] else nan
    return out
