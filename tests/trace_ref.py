"""The evaluation trace (include/lorenz_env.h lz_eval_trace) restated in NumPy: which steps
a traced launch records and what a row holds, given the per-step arrays of a run."""
import numpy as np

TRACE_STATE = 1
# system -> (obs_dim, action_dim, state_dim)
DIMS = {"lorenz3": (6, 3, 3), "lorenz4": (8, 3, 8), "pmsm": (6, 2, 6), "hr": (6, 2, 6)}
SYSTEM_ID = {"lorenz3": 0, "lorenz4": 1, "pmsm": 2, "hr": 3}


def recorded_steps(K, start=0, every=1):
    """The step indices k a trace records, in row order."""
    assert K >= 1 and every >= 1 and 0 <= start < K
    return np.array([k for k in range(K) if k >= start and (k - start) % every == 0], np.int64)


def shape(system, K, start=0, every=1, flags=0):
    """(T, C) of the trace buffer."""
    O, A, S = DIMS[system]
    return len(recorded_steps(K, start, every)), O + A + 2 + (S if flags & TRACE_STATE else 0)


def trace_ref(o, a, r, d, ids, start=0, every=1, state=None):
    """float32 [T, M, C] from o [K, n, O] (the observation each step emitted before any
    auto-reset), a [K, n, A] (the clipped actions), r [K, n], d [K, n] (done bits) and,
    for LZ_TRACE_STATE, state [K, n, S] (the leading state planes after each step)."""
    ks = recorded_steps(o.shape[0], start, every)
    ids = np.asarray(ids, np.int64)
    cols = [o[ks][:, ids], a[ks][:, ids], r[ks][:, ids][..., None],
            d[ks][:, ids].astype(np.float32)[..., None]]
    if state is not None:
        cols.append(state[ks][:, ids])
    return np.concatenate([np.asarray(c, np.float32) for c in cols], axis=2)
