"""The two tables between a state_dict and a launch (gym_lorenz/policy.py): _PACKERS, one
row per (family, precision) with the C packer, its blob-size function and the LZ_BLOB_* tag;
and _LAUNCH, one row per (kind, family, precision) with the entry point, laid out like
kPolicyTable in lz_api.cpp.  Host only."""
import numpy as np
import pytest

from gym_lorenz import _native as nat

FAMILIES, PRECISIONS = ("mlp", "attn", "attn_ln"), ("bf16", "fp32", "i8x4")
# the nine public packers by their table key
PUBLIC = {("mlp", "bf16"): "pack_policy", ("mlp", "fp32"): "pack_policy_f32",
          ("mlp", "i8x4"): "pack_policy_i8x4", ("attn", "bf16"): "pack_attn_policy",
          ("attn", "fp32"): "pack_attn_policy_f32", ("attn", "i8x4"): "pack_attn_policy_i8x4",
          ("attn_ln", "bf16"): "pack_attn_ln_policy", ("attn_ln", "fp32"): "pack_attn_ln_policy_f32",
          ("attn_ln", "i8x4"): "pack_attn_ln_policy_i8x4"}
# (input width, act_dim, hidden): the smallest and the largest of each family
SHAPES = {"mlp": [(1, 1, 1), (8, 4, 128)], "attn": [(1, 1, 128), (8, 4, 128)],
          "attn_ln": [(1, 1, 128), (32, 4, 128)]}


@pytest.fixture(scope="module")
def pol():
    from gym_lorenz import policy

    return policy


def _state_dict(pol, family, in_dim, act_dim, hidden):
    if family == "mlp":
        return pol.ActorCriticMlp(in_dim, act_dim, hidden=hidden, seed=3).state_dict()
    return pol.ActorCriticAttn(in_dim, act_dim, seed=3, layer_norm=family == "attn_ln").state_dict()


def test_packer_table_is_complete_and_consistent(pol):
    assert set(pol._PACKERS) == {(f, p) for f in FAMILIES for p in PRECISIONS} == set(PUBLIC)
    exported = set(nat.exported_symbols())
    packers = [row[0] for row in pol._PACKERS.values()]
    assert len(set(packers)) == len(packers) == 9 and set(packers) <= exported
    assert {row[1] for row in pol._PACKERS.values()} <= exported
    for (family, precision), (_pack_fn, _size_fn, tag) in pol._PACKERS.items():
        if precision == "bf16":
            want = nat.BLOB_UNKNOWN
            assert tag is None
        else:
            want = pol.blob_format(family != "mlp", family == "attn_ln", precision == "i8x4")
            assert tag == want != nat.BLOB_UNKNOWN
        for in_dim, act_dim, hidden in SHAPES[family]:
            sd = _state_dict(pol, family, in_dim, act_dim, hidden)
            blob = pol._pack(family, precision, sd, in_dim, act_dim)
            assert blob.dtype == np.uint8 and blob.size == getattr(nat.lib, _size_fn)()
            assert int(nat.lib.lz_policy_blob_format(blob.ctypes.data, blob.size)) == want
            assert np.array_equal(getattr(pol, PUBLIC[family, precision])(sd, in_dim, act_dim), blob)
    tags = [row[2] for row in pol._PACKERS.values() if row[2] is not None]
    assert sorted(tags) == list(range(1, 7))  # every LZ_BLOB_* format has one packer


def test_launch_table_names_the_entry_points(pol):
    rows = pol._LAUNCH
    exported = set(nat.exported_symbols())
    assert set(rows.values()) <= exported and len(set(rows.values())) == len(rows)
    by_kind = {}
    for (kind, family, precision), name in rows.items():
        assert family in FAMILIES and precision in ("bf16", "fp32")
        by_kind.setdefault(kind, set()).add(name)
    # what FusedRolloutCollector.collect can reach: six rollouts and the per-step launch ...
    assert by_kind["rollout"] | by_kind["step"] == {
        "lz_rollout_policy", "lz_rollout_policy_attn", "lz_rollout_policy_attn_stack",
        "lz_rollout_policy_f32", "lz_rollout_policy_attn_f32", "lz_rollout_policy_attn_stack_f32",
        "lz_policy_step_f32"}
    # ... and FusedEvaluator.evaluate: float32 only, plain or traced
    assert by_kind["evaluate"] == {"lz_evaluate_policy_f32", "lz_evaluate_policy_attn_f32",
                                   "lz_evaluate_policy_attn_stack_f32"}
    assert by_kind["trace"] == {name + "_trace" for name in by_kind["evaluate"]}
    assert set(by_kind) == {"rollout", "step", "evaluate", "trace"}
    for kind in ("evaluate", "trace"):
        assert {k[1:] for k in rows if k[0] == kind} == {(f, "fp32") for f in FAMILIES}
    assert {k[1:] for k in rows if k[0] == "rollout"} == {(f, p) for f in FAMILIES for p in ("bf16", "fp32")}
    # no policy entry point of the library is left out (lz_rollout_policy_f32_vn is the
    # library's own loop over the "step" row)
    policy_calls = {s for s in exported
                    if s.startswith(("lz_rollout_policy", "lz_evaluate_policy", "lz_policy_step"))}
    assert policy_calls - {"lz_rollout_policy_f32_vn"} == set(rows.values())
