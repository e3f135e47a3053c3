"""The 64-unit learner's host side (no GPU): the _hidden size functions and entry points
(lz_a2c_param_count_hidden, lz_a2c_workspace_bytes_hidden, lz_ppo_workspace_bytes_hidden,
lz_a2c_grad_hidden_f32, lz_ppo_grad_hidden_f32), the Python layout at 64 units, net_arch on
FusedA2C / FusedPPO, the packer's view of the zero-padded twin, and the reference's shipped
PPO policies as FusedPPO(net_arch=64) state."""
import ctypes

import numpy as np
import pytest
import torch

import a2c_ref
import mlp_learner_ref as ref
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol

DIMS = [(O, A) for O in range(1, 9) for A in range(1, 5)]


def test_param_count_hidden():
    cnt = nat.lib.lz_a2c_param_count_hidden
    assert cnt(6, 2, 64) == 9413 and cnt(6, 2, 128) == 35205
    for O, A in DIMS:
        assert cnt(O, A, 128) == nat.lib.lz_a2c_param_count(O, A)
        for H in (64, 128):
            assert cnt(O, A, H) == ref.param_count(O, A, H) == ref.layout(O, A, H)[1]
    for H in (0, 32, 127, 256):
        assert cnt(6, 2, H) == -1, H
    for O, A in ((0, 2), (9, 2), (6, 0), (6, 5)):
        assert cnt(O, A, 64) == -1 and cnt(O, A, 128) == -1


@pytest.mark.parametrize("kind,tail", [("a2c", 4), ("ppo", 6)])
def test_workspace_bytes_hidden(kind, tail):
    ws = getattr(nat.lib, "lz_%s_workspace_bytes_hidden" % kind)
    old = getattr(nat.lib, "lz_%s_workspace_bytes" % kind)
    for name in ("lz_%s_workspace_bytes_hidden" % kind, "lz_%s_grad_hidden_f32" % kind,
                 "lz_a2c_param_count_hidden"):
        assert hasattr(nat.lib, name) and name in nat.exported_symbols()
    slot = (9413 + tail) * 8
    assert ws(1, 6, 2, 64, 0) == slot                  # one tile, one workgroup per net
    assert ws(111, 6, 2, 64, 0) == 4 * slot            # four tiles of 32
    assert ws(5 * 1031, 6, 2, 64, 3) == 3 * slot       # the cap
    assert ws(2085, 6, 2, 64, 1) == slot
    assert ws(1 << 22, 6, 2, 64, 0) == 128 * slot      # the default grid, as at 128 units
    for O, A in DIMS:
        for n, cap in ((1, 0), (111, 0), (111, 2), (5155, 3), (1 << 20, 0)):
            assert ws(n, O, A, 128, cap) == old(n, O, A, cap)
    for H in (0, 32, 127, 256):
        assert ws(111, 6, 2, H, 0) == -1, H
    for bad in ((0, 6, 2, 0), (-5, 6, 2, 0), (10, 0, 2, 0), (10, 9, 2, 0), (10, 6, 5, 0), (10, 6, 2, -1),
                (10, 6, 2, 4097)):
        assert ws(bad[0], bad[1], bad[2], 64, bad[3]) == -1, bad


def _a2c_args(keep, hidden=64):
    """Valid-looking arguments (never dereferenced: every case below is refused first)."""
    g = nat.LzA2cGradArgs()
    fake = ctypes.c_void_p(0x1000)
    for f in ("params", "observations", "actions", "advantages", "returns", "workspace", "grad_sums"):
        setattr(g, f, fake)
    g.n_samples, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 6, 2, hidden, 0
    g.vf_coef, g.ent_coef = 0.5, 0.0
    g.workspace_bytes = nat.lib.lz_a2c_workspace_bytes_hidden(111, 6, 2, hidden, 0)
    keep.append(g)
    return g


def _ppo_args(keep, hidden=64):
    g = nat.LzPpoGradArgs()
    fake = ctypes.c_void_p(0x1000)
    for f in ("params", "observations", "actions", "advantages", "returns", "old_log_prob", "old_values",
              "indices", "workspace", "grad_sums"):
        setattr(g, f, fake)
    g.n_samples, g.n_rows, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 333, 6, 2, hidden, 0
    g.vf_coef, g.ent_coef, g.clip_range, g.clip_range_vf = 0.5, 0.0, 0.2, 0.0
    g.workspace_bytes = nat.lib.lz_ppo_workspace_bytes_hidden(111, 6, 2, hidden, 0)
    keep.append(g)
    return g


def _refusals(make, fn, nulls, invalid):
    """The old entry point's refusals, in its order, none of them needing a device."""
    keep = []
    call = lambda g: fn(ctypes.byref(g), 0, None)  # noqa: E731
    assert fn(None, 0, None) == nat.LZ_ERR_INVALID
    for f in nulls:
        g = make(keep)
        setattr(g, f, None)
        assert call(g) == nat.LZ_ERR_INVALID, f
        assert b"NULL" in nat.lib.lz_last_error()
    for f, v in invalid:
        g = make(keep)
        setattr(g, f, v)
        assert call(g) == nat.LZ_ERR_INVALID, (f, v)
    for hidden in (0, 32, 96, 127, 256):
        g = make(keep)
        g.hidden = hidden
        assert call(g) == nat.LZ_ERR_UNSUPPORTED, hidden
        assert b"hidden" in nat.lib.lz_last_error()
    # the order: bad dims and a bad max_workgroups are reported before an unsupported hidden,
    # an unsupported hidden before a short workspace
    g = make(keep)
    g.hidden, g.obs_dim = 96, 9
    assert call(g) == nat.LZ_ERR_INVALID
    g = make(keep)
    g.hidden, g.max_workgroups = 96, 4097
    assert call(g) == nat.LZ_ERR_INVALID
    g = make(keep)
    g.hidden, g.workspace_bytes = 96, 0
    assert call(g) == nat.LZ_ERR_UNSUPPORTED
    # the workspace check uses the size of the hidden asked for
    for hidden in (64, 128):
        g = make(keep, hidden)
        g.workspace_bytes -= 1
        assert call(g) == nat.LZ_ERR_INVALID, hidden
        assert b"workspace" in nat.lib.lz_last_error()
    g = make(keep, 128)
    g.workspace_bytes = make(keep, 64).workspace_bytes  # enough for 64 units, short for 128
    assert call(g) == nat.LZ_ERR_INVALID and b"workspace" in nat.lib.lz_last_error()


def test_a2c_grad_hidden_refusals_need_no_gpu():
    _refusals(_a2c_args, nat.lib.lz_a2c_grad_hidden_f32,
              ("params", "observations", "actions", "advantages", "returns", "workspace", "grad_sums"),
              (("obs_dim", 0), ("obs_dim", 9), ("act_dim", 0), ("act_dim", 5), ("n_samples", 0),
               ("n_samples", -1), ("max_workgroups", -1), ("max_workgroups", 4097)))


def test_ppo_grad_hidden_refusals_need_no_gpu():
    _refusals(_ppo_args, nat.lib.lz_ppo_grad_hidden_f32,
              ("params", "observations", "actions", "advantages", "returns", "old_log_prob", "workspace",
               "grad_sums"),
              (("obs_dim", 0), ("obs_dim", 9), ("act_dim", 0), ("act_dim", 5), ("n_samples", 0),
               ("n_rows", 0), ("clip_range", -0.1), ("clip_range", float("nan")),
               ("clip_range", float("inf")), ("clip_range_vf", float("nan")), ("max_workgroups", -1),
               ("max_workgroups", 4097)))
    keep = []
    g = _ppo_args(keep)
    g.clip_range_vf, g.old_values = 0.05, None
    assert nat.lib.lz_ppo_grad_hidden_f32(ctypes.byref(g), 0, None) == nat.LZ_ERR_INVALID
    g = _ppo_args(keep)
    g.indices, g.n_samples = None, 334
    assert nat.lib.lz_ppo_grad_hidden_f32(ctypes.byref(g), 0, None) == nat.LZ_ERR_INVALID


def test_python_layout_at_64_units_matches_the_c_count():
    for O, A in ((1, 1), (6, 2), (7, 3), (8, 4)):
        for H in (64, 128):
            lay, P = pol.a2c_param_layout(O, A, hidden=H)
            assert tuple(lay) == pol.KEYS
            assert P == nat.lib.lz_a2c_param_count_hidden(O, A, H) == ref.layout(O, A, H)[1]
            assert pol.a2c_param_shapes(O, A, hidden=H) == ref.shapes(O, A, H)
            sd = pol.ActorCriticMlp(O, A, hidden=H, seed=0).state_dict()
            o = 0
            for k in pol.KEYS:
                assert lay[k] == (o, tuple(sd[k].shape)), k
                o += sd[k].numel()
            assert o == P
        assert pol.a2c_param_layout(O, A) == pol.a2c_param_layout(O, A, hidden=128)


class _FakeCollector:
    precision = "fp32"
    frame_stack = 1
    n = 4
    device = torch.device("cpu")

    def __init__(self, O=6, A=2):
        self.O, self.A = O, A

    def set_params(self, sd):
        self.sd = sd


def _make(cls, col, sd, **kw):
    return cls(col, sd, **kw)


@pytest.mark.parametrize("cls", [pol.FusedA2C, pol.FusedPPO])
def test_net_arch_on_the_learners(cls):
    sd64, sd128 = ref.make_policy(6, 2, 0), a2c_ref.make_policy(6, 2, 0)
    for arch in (64, [64, 64], (64, 64), dict(pi=[64, 64], vf=[64, 64])):
        col = _FakeCollector()
        m = _make(cls, col, sd64, net_arch=arch)
        assert m.hidden == 64 and m.P == 9413 and m.params.numel() == 9413
        back = m.state_dict()
        assert all(torch.equal(back[k], sd64[k]) for k in pol.KEYS) and set(col.sd) == set(pol.KEYS)
        assert all(torch.equal(col.sd[k], sd64[k]) for k in pol.KEYS)
        opt = m.optimizer_state()
        for name in ("square_avg",) if cls is pol.FusedA2C else ("exp_avg", "exp_avg_sq"):
            assert set(opt[name]) == set(pol.KEYS)
            assert sum(t.numel() for t in opt[name].values()) == 9413
            assert tuple(opt[name]["mlp_extractor.policy_net.2.weight"].shape) == (64, 64)
    for arch in (128, [128, 128], dict(pi=[128, 128], vf=[128, 128])):
        m = _make(cls, _FakeCollector(), sd128, net_arch=arch)
        assert m.hidden == 128 and m.P == 35205
    # the state_dict must have the declared size
    with pytest.raises(ValueError, match="hidden=64"):
        _make(cls, _FakeCollector(), sd128, net_arch=64)
    with pytest.raises(ValueError, match="hidden=128"):
        _make(cls, _FakeCollector(), sd64, net_arch=128)
    # None is the 128-unit learner, to the letter
    with pytest.raises(ValueError, match="hidden=128"):
        _make(cls, _FakeCollector(), sd64)
    with pytest.raises(ValueError, match="hidden=128"):
        _make(cls, _FakeCollector(), sd64, net_arch=None)
    assert _make(cls, _FakeCollector(), sd128).hidden == 128
    for bad in (96, 32, 0, [64], [64, 128], [64, 64, 64], dict(pi=[64, 64], vf=[128, 128]),
                dict(pi=[64, 64]), dict(pi=[64], vf=[64]), "64", 64.0, True):
        with pytest.raises(ValueError, match="net_arch"):
            _make(cls, _FakeCollector(), sd64, net_arch=bad)


def test_wrappers_check_buffers_before_a_launch_at_64_units():
    """A CPU params tensor never reaches the library, whatever the hidden size; an
    unsupported hidden is refused with LZ_ERR_UNSUPPORTED before any buffer is looked at."""
    sd = ref.make_policy(6, 2, 0)
    obs, act, adv, ret = a2c_ref.make_batch(sd, 8, 6, 2, 0)
    flat = a2c_ref.flatten(sd)
    assert flat.numel() == 9413
    with pytest.raises(nat.LorenzEnvError):
        pol.a2c_grad(flat, obs, act, adv, ret, 6, 2, hidden=64)
    with pytest.raises(nat.LorenzEnvError):
        pol.ppo_grad(flat, obs, act, adv, ret, adv, adv, 6, 2, hidden=64)
    with pytest.raises(nat.LorenzEnvError) as e:
        pol._grad_fns("a2c", 96, 6, 2, "a2c_grad")
    assert e.value.status == nat.LZ_ERR_UNSUPPORTED and "hidden" in str(e.value)
    P, ws, fn = pol._grad_fns("ppo", 64, 6, 2, "ppo_grad")
    assert P == 9413 and ws(111, 0) == 4 * (9413 + 6) * 8


@pytest.mark.parametrize("O,A", [(6, 2), (1, 1), (8, 4)])
def test_packer_sees_the_padded_twin_as_the_same_policy(O, A):
    """What makes the zero-padded 128-unit net a twin of the 64-unit one on the forward side:
    the float32 blob is the same bytes."""
    sd64 = ref.make_policy(O, A, 3)
    sd128 = ref.pad_to_128(sd64)
    assert tuple(sd128["mlp_extractor.policy_net.2.weight"].shape) == (128, 128)
    a, b = pol.pack_policy_f32(sd64, O, A), pol.pack_policy_f32(sd128, O, A)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    # and the index map picks the 64-unit entries out of the padded flat vector
    idx = ref.unpadded_index(O, A)
    f64, f128 = a2c_ref.flatten(sd64).numpy(), a2c_ref.flatten(sd128).numpy()
    assert np.array_equal(f128[idx], f64)
    rest = np.ones(f128.size, bool)
    rest[idx] = False
    assert not f128[rest].any() and rest.sum() == f128.size - f64.size


@pytest.mark.parametrize("name,O,A", [(n, O, A) for n, _, O, A in ref.SHIPPED])
def test_shipped_reference_policies_are_accepted(name, O, A):
    """hr_sync_agent.zip (O = 6, A = 1) and lorenz_targeting_Lstm_continous_0.zip (O = 8,
    A = 3): SB3's default 64 x 64 net, which FusedPPO(net_arch=64) takes and the 128-unit
    learner refuses."""
    sd = ref.shipped_policy(name)
    assert tuple(sd["mlp_extractor.policy_net.0.weight"].shape) == (64, O)
    assert tuple(sd["mlp_extractor.value_net.2.weight"].shape) == (64, 64)
    assert tuple(sd["action_net.weight"].shape) == (A, 64) and tuple(sd["log_std"].shape) == (A,)
    assert all(sd[k].dtype == torch.float32 and bool(torch.isfinite(sd[k]).all()) for k in pol.KEYS)
    assert float(sd["mlp_extractor.policy_net.2.weight"].abs().max()) > 0
    col = _FakeCollector(O, A)
    ppo = pol.FusedPPO(col, sd, net_arch=64, n_steps=2048, batch_size=64)
    assert ppo.P == nat.lib.lz_a2c_param_count_hidden(O, A, 64) == ppo.params.numel()
    back = ppo.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in pol.KEYS)
    assert ppo.optimizer_state()["step"] == 0
    with pytest.raises(ValueError, match="hidden=128"):
        pol.FusedPPO(_FakeCollector(O, A), sd)
    blob = pol.pack_policy_f32(sd, O, A)
    assert blob.tobytes() == pol.pack_policy_f32(ref.pad_to_128(sd), O, A).tobytes()
