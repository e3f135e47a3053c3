"""The evaluation trace without a GPU: lz_eval_trace_shape against tests/trace_ref.py, the
ctypes mirror of lz_eval_trace against the header, the refusals that need no handle, the
host-side id validator and the EvalTrace helpers on CPU tensors.  The traced launches
themselves are in tests/test_gpu_eval_trace.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import trace_ref as tr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lorenz_env.h")


@pytest.fixture(scope="module")
def nat():
    from gym_lorenz import _native

    return _native


@pytest.fixture(scope="module")
def pol():
    from gym_lorenz import policy

    return policy


def _shape(nat, system, K, start, every, flags):
    cfg = nat.config_init(tr.SYSTEM_ID[system])
    rows, cols = ctypes.c_int64(-7), ctypes.c_int32(-7)
    st = nat.lib.lz_eval_trace_shape(ctypes.byref(cfg), K, start, every, flags, ctypes.byref(rows),
                                     ctypes.byref(cols))
    return st, rows.value, cols.value


# ------------------------------------------------------------------------------- shape
@pytest.mark.parametrize("system", sorted(tr.DIMS))
def test_trace_shape_matches_reference(nat, pol, system):
    assert [nat.LORENZ3, nat.LORENZ4, nat.PMSM, nat.HR] == [tr.SYSTEM_ID[s] for s in
                                                           ("lorenz3", "lorenz4", "pmsm", "hr")]
    assert nat.TRACE_STATE == tr.TRACE_STATE
    seen = 0
    for K in (1, 7):
        for start in (0, 2):
            for every in (1, 3, K):
                for flags in (0, tr.TRACE_STATE):
                    st, rows, cols = _shape(nat, system, K, start, every, flags)
                    if start >= K:  # K = 1, start = 2: refused, outputs untouched
                        assert st == nat.LZ_ERR_INVALID and (rows, cols) == (-7, -7)
                        with pytest.raises(ValueError):
                            pol.trace_shape(K, start, every)
                        continue
                    assert st == nat.LZ_OK
                    assert (rows, cols) == tr.shape(system, K, start, every, flags), (K, start, every, flags)
                    assert rows == -(-(K - start) // every) == pol.trace_shape(K, start, every)
                    seen += 1
    assert seen == 18
    O, A, S = tr.DIMS[system]
    assert pol.STATE_DIMS[system] == S


def test_trace_shape_refusals(nat):
    ok = ("hr", 7, 0, 1, 0)
    assert _shape(nat, *ok)[0] == nat.LZ_OK
    for bad in (("hr", 0, 0, 1, 0), ("hr", 7, -1, 1, 0), ("hr", 7, 7, 1, 0), ("hr", 7, 0, 0, 0),
                ("hr", 7, 0, -2, 0), ("hr", 7, 0, 1, 2)):
        assert _shape(nat, *bad)[0] == nat.LZ_ERR_INVALID, bad
        assert nat.lib.lz_last_error()
    cfg = nat.config_init(nat.HR)
    rows, cols = ctypes.c_int64(), ctypes.c_int32()
    f = nat.lib.lz_eval_trace_shape
    assert f(None, 7, 0, 1, 0, ctypes.byref(rows), ctypes.byref(cols)) == nat.LZ_ERR_INVALID
    assert f(ctypes.byref(cfg), 7, 0, 1, 0, None, ctypes.byref(cols)) == nat.LZ_ERR_INVALID
    assert f(ctypes.byref(cfg), 7, 0, 1, 0, ctypes.byref(rows), None) == nat.LZ_ERR_INVALID
    cfg.system = 99
    assert f(ctypes.byref(cfg), 7, 0, 1, 0, ctypes.byref(rows), ctypes.byref(cols)) == nat.LZ_ERR_INVALID
    for legacy in (nat.T1, nat.T2, nat.TP, nat.SC):  # no fused evaluation, so no trace
        cfg = nat.config_init(legacy)
        assert f(ctypes.byref(cfg), 7, 0, 1, 0, ctypes.byref(rows), ctypes.byref(cols)) == nat.LZ_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------- ABI
def test_trace_struct_matches_header(nat, tmp_path):
    fields = [f for f, _ in nat.LzEvalTrace._fields_]
    c = tmp_path / "probe_trace.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "lorenz_env.h"\n'
        "int main(void){lz_eval_trace t;printf(\"%zu\", sizeof(lz_eval_trace));\n"
        + "".join('printf(" %%zu %%zu", offsetof(lz_eval_trace, %s), sizeof(t.%s));\n' % (f, f) for f in fields)
        + 'printf(" %d %d %zu", (int)LZ_TRACE_STATE, (int)LZ_ABI_VERSION, sizeof(lz_policy_eval_args));\n'
        + "return 0;}\n")
    exe = tmp_path / "probe_trace"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = nat.LzEvalTrace
    want = [ctypes.sizeof(E)]
    for f in fields:
        want += [getattr(E, f).offset, getattr(E, f).size]
    assert got[:len(want)] == want
    assert fields == ["ids", "count", "slot_map", "start", "every", "flags", "out", "out_capacity_bytes"]
    # additive: the flag's value, the ABI version and the untraced argument struct as they were
    assert got[len(want):] == [nat.TRACE_STATE, 2, ctypes.sizeof(nat.LzPolicyEvalArgs)]
    assert nat.lib.lz_abi_version() == 2


def test_trace_null_arguments_are_refused(nat):
    """NULL handle / args / trace never reach a dereference: LZ_ERR_INVALID with a message."""
    e, t = nat.LzPolicyEvalArgs(), nat.LzEvalTrace()
    lib = nat.lib
    assert lib.lz_evaluate_policy_f32_trace(None, ctypes.byref(e), ctypes.byref(t)) == nat.LZ_ERR_INVALID
    assert b"NULL" in lib.lz_last_error()
    assert lib.lz_evaluate_policy_attn_f32_trace(None, ctypes.byref(e), ctypes.byref(t)) == nat.LZ_ERR_INVALID
    assert lib.lz_evaluate_policy_attn_stack_f32_trace(None, ctypes.byref(e), 4, None, None,
                                                       ctypes.byref(t)) == nat.LZ_ERR_INVALID
    assert lib.lz_evaluate_policy_f32_trace(None, None, None) == nat.LZ_ERR_INVALID
    assert lib.lz_evaluate_policy_attn_f32_trace(None, None, None) == nat.LZ_ERR_INVALID
    assert lib.lz_evaluate_policy_attn_stack_f32_trace(None, None, 1, None, None, None) == nat.LZ_ERR_INVALID


# ----------------------------------------------------------------------------- id validator
def test_trace_id_validator(pol):
    v = pol.validate_trace_ids
    assert v([3, 0, 69], 70) == [3, 0, 69]
    assert v(torch.tensor([5, 1]), 70) == [5, 1]
    assert v(np.array([2, 4], np.int32), 70) == [2, 4]
    assert v(range(70), 70) == list(range(70))
    for bad in ([0, 3, 0], [-1], [70], [0, 70], [], torch.tensor([], dtype=torch.int64), [0.5],
                torch.tensor([1.0])):
        with pytest.raises(ValueError):
            v(bad, 70)


# ------------------------------------------------------------------------ EvalTrace helpers
def test_eval_trace_views_and_helpers(pol):
    rng = np.random.default_rng(0)
    K, n, start, every = 11, 5, 2, 3
    O, A, S = tr.DIMS["hr"]
    o = rng.normal(size=(K, n, O)).astype(np.float32)
    a = rng.uniform(-1, 1, size=(K, n, A)).astype(np.float32)
    r = rng.normal(size=(K, n)).astype(np.float32)
    d = rng.integers(0, 4, size=(K, n)).astype(np.uint8)
    s = rng.normal(size=(K, n, S)).astype(np.float32)
    ids = [4, 0, 2]
    buf = tr.trace_ref(o, a, r, d, ids, start, every, state=s)
    T, C = tr.shape("hr", K, start, every, tr.TRACE_STATE)
    assert buf.shape == (T, 3, C) and buf.dtype == np.float32
    t = pol.EvalTrace(torch.from_numpy(buf), "hr", O, A, True, start, every, ids)
    ks = tr.recorded_steps(K, start, every)
    assert t.steps.dtype == torch.int64 and t.steps.tolist() == ks.tolist() == [2, 5, 8]
    assert t.env_ids.dtype == torch.int64 and t.env_ids.tolist() == ids
    assert np.array_equal(t.obs.numpy(), o[ks][:, ids])
    assert np.array_equal(t.actions.numpy(), a[ks][:, ids])
    assert np.array_equal(t.rewards.numpy(), r[ks][:, ids])
    assert t.dones.dtype == torch.uint8 and np.array_equal(t.dones.numpy(), d[ks][:, ids])
    assert np.array_equal(t.state.numpy(), s[ks][:, ids])
    assert t.obs.data_ptr() == t.data.data_ptr()  # views of the launch's buffer
    # the reference's records: err_* = obs[:3] * 50, ctrl_* = action * 100, time = step * dt
    assert np.array_equal(t.errors().numpy(), o[ks][:, ids][..., :3] * np.float32(50))
    assert np.array_equal(t.controls().numpy(), a[ks][:, ids] * np.float32(100))
    assert np.array_equal(t.time(0.001).numpy(), ks.astype(np.float64) * 0.001)
    h = t.numpy()
    assert sorted(h) == ["actions", "controls", "dones", "env_ids", "errors", "obs", "rewards", "state", "steps"]
    assert np.array_equal(h["errors"], t.errors().numpy()) and np.array_equal(h["state"], s[ks][:, ids])
    # without state, another system: unscaled errors (four dims for LORENZ4) and controls
    O4, A4, _ = tr.DIMS["lorenz4"]
    o4 = rng.normal(size=(K, n, O4)).astype(np.float32)
    a4 = rng.normal(size=(K, n, A4)).astype(np.float32)
    b4 = tr.trace_ref(o4, a4, r, d, ids)
    t4 = pol.EvalTrace(torch.from_numpy(b4), "lorenz4", O4, A4, False, 0, 1, ids)
    assert t4.state is None and t4.numpy()["state"] is None and t4.steps.tolist() == list(range(K))
    assert np.array_equal(t4.errors().numpy(), o4[:, ids][..., :4])
    assert np.array_equal(t4.controls().numpy(), a4[:, ids])
    with pytest.raises(ValueError):
        pol.EvalTrace(torch.from_numpy(b4), "lorenz4", O4, A4, True, 0, 1, ids)  # C without the state


def test_eval_trace_is_exported():
    import gym_lorenz
    from gym_lorenz import policy

    assert gym_lorenz.EvalTrace is policy.EvalTrace
    assert "EvalTrace" in gym_lorenz.__all__
    assert policy.CTRL_SCALE == {"lorenz3": 1.0, "lorenz4": 1.0, "pmsm": 1.0, "hr": 100.0}
