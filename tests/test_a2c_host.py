"""The A2C update's host side (no GPU): the reference restatement tests/a2c_ref.py is
checked against finite differences and a hand-computed RMSprop case, linear_schedule
against the reference's closure, and lz_a2c_* load, size their workspace and refuse bad
arguments with their status before any HIP call."""
import ctypes
import math

import numpy as np
import pytest
import torch

import a2c_ref as ref
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol


def test_reference_gradient_matches_central_differences():
    """a2c_ref's float64 autograd gradient against central differences of its own float64
    loss, h = 1e-6, relative error <= 1e-5, at random coordinates of every tensor.

    The difference quotient of a loss of magnitude |L| carries a rounding error of about
    eps64 |L| / h whatever the gradient is, so a relative 1e-5 can only be asked of
    coordinates with |g| >= floor = 4 eps64 |L| / (h 1e-5); smaller ones are held to the
    absolute 1e-5 floor (a wrong formula is off by the size of the gradient, not by 1e-9)."""
    O, A, B = 6, 2, 8
    sd = ref.make_policy(O, A, 3)
    batch = ref.make_batch(sd, B, O, A, 5)
    vf, ent = 0.5, 0.01
    g = ref.grad_sums(sd, batch, vf, ent)
    flat = ref.flatten(sd).to(torch.float64)
    rng = np.random.default_rng(0)
    h = 1e-6
    floor = 4 * np.finfo(np.float64).eps * abs(ref.loss64(flat, batch, O, A, vf, ent)) / (h * 1e-5)
    relative = 0
    for k, (o, shp) in ref.layout(O, A)[0].items():
        n = int(np.prod(shp))
        for i in rng.choice(n, size=min(n, 36), replace=False):
            up, dn = flat.clone(), flat.clone()
            up[o + i] += h
            dn[o + i] -= h
            fd = (ref.loss64(up, batch, O, A, vf, ent) - ref.loss64(dn, batch, O, A, vf, ent)) / (2 * h)
            scale = max(abs(g[o + i]), abs(fd))
            relative += scale >= floor
            assert abs(fd - g[o + i]) <= 1e-5 * max(scale, floor), (k, int(i), fd, g[o + i])
    assert relative >= 150  # most coordinates are checked at the relative bound itself


def test_reference_loss_sums_by_hand():
    """One sample, A = 1: log_prob, entropy and the squared error written out."""
    O, A = 3, 1
    sd = ref.make_policy(O, A, 1)
    obs = torch.tensor([[0.3, -1.2, 0.7]])
    act, adv, ret = torch.tensor([[0.4]]), torch.tensor([1.7]), torch.tensor([-0.6])
    mu, v = ref.forward(sd, obs, torch.float64)
    ls = float(sd["log_std"][0])
    logp = -(0.4000000059604645 - float(mu)) ** 2 / (2 * math.exp(ls) ** 2) - ls - 0.5 * math.log(2 * math.pi)
    pl, vl, el = ref.loss_sums(sd, (obs, act, adv, ret), torch.float64)
    assert float(pl) == pytest.approx(-float(adv[0]) * logp, rel=1e-12)
    assert float(vl) == pytest.approx((float(ret[0]) - float(v)) ** 2, rel=1e-12)
    assert float(el) == pytest.approx(-(0.5 + 0.5 * math.log(2 * math.pi) + ls), rel=1e-12)


def test_rmsprop_tf_like_two_steps_by_hand():
    """square_avg starts at ONES and eps sits inside the root."""
    lr, alpha, eps = 0.1, 0.99, 1e-5
    p0, g1, g2 = 1.0, 2.0, -3.0
    s1 = 0.99 * 1.0 + (1 - 0.99) * 4.0
    p1 = p0 - lr * g1 / math.sqrt(s1 + eps)
    s2 = 0.99 * s1 + (1 - 0.99) * 9.0
    p2 = p1 - lr * g2 / math.sqrt(s2 + eps)
    p, s = ref.rmsprop_tf_like([p0], [g1], None, lr, alpha, eps)
    assert p[0] == pytest.approx(p1, rel=1e-15) and s[0] == pytest.approx(s1, rel=1e-15)
    p, s = ref.rmsprop_tf_like(p, [g2], s, lr, alpha, eps)
    assert p[0] == pytest.approx(p2, rel=1e-15) and s[0] == pytest.approx(s2, rel=1e-15)
    # stock RMSprop (zeros, eps outside the root) would give something else
    stock = p0 - lr * g1 / (math.sqrt((1 - 0.99) * 4.0) + eps)
    assert abs(stock - p1) > 0.1
    # apply_step is the same step after the mean, the float32 rounding and the clip
    sums = np.array([8.0, -12.0, 0.0, 0.0, 0.0, 4.0])  # two params, count 4: g = (2, -3)
    pa, sa, total, coef = ref.apply_step(sums, np.float32([1.0, 1.0]), np.float32([1.0, 1.0]), lr,
                                         max_grad_norm=100.0)
    assert total == pytest.approx(math.sqrt(13.0)) and coef == 1.0
    assert pa[0] == np.float32(p1) and sa[0] == np.float32(s1)
    pa, sa, total, coef = ref.apply_step(sums, np.float32([1.0, 1.0]), np.float32([1.0, 1.0]), lr,
                                         max_grad_norm=0.5)
    assert coef == pytest.approx(0.5 / (math.sqrt(13.0) + 1e-6))
    assert sa[0] == np.float32(0.99 + 0.01 * (2.0 * coef) ** 2)


def test_linear_schedule_is_the_reference_closure():
    """code/lorenz_pmsm/train.py:187-197: max(progress_remaining * initial, 1e-5)."""
    import gym_lorenz

    f = gym_lorenz.linear_schedule(0.0005)
    for pr in (1.0, 0.75, 0.5, 0.1, 0.02, 0.01, 0.0):
        assert f(pr) == max(pr * 0.0005, 1e-5)
    assert f(0.0) == 1e-5 and f(1.0) == 0.0005
    assert gym_lorenz.FusedA2C is pol.FusedA2C


def test_flat_layout_agrees_with_keys_and_shapes():
    for O, A in ((1, 1), (6, 2), (7, 3), (8, 4)):
        lay, P = pol.a2c_param_layout(O, A)
        assert tuple(lay) == pol.KEYS
        assert P == nat.lib.lz_a2c_param_count(O, A) == ref.layout(O, A)[1]
        sd = pol.ActorCriticMlp(O, A, seed=0).state_dict()
        o = 0
        for k in pol.KEYS:
            assert lay[k] == (o, tuple(sd[k].shape)), k
            o += sd[k].numel()
        assert o == P
    assert nat.lib.lz_a2c_param_count(6, 2) == 35205
    for O, A in ((0, 2), (9, 2), (6, 0), (6, 5)):
        assert nat.lib.lz_a2c_param_count(O, A) == -1


def test_symbols_load_and_workspace_bytes():
    for name in ("lz_a2c_grad_f32", "lz_a2c_apply_f32", "lz_a2c_workspace_bytes", "lz_a2c_param_count"):
        assert hasattr(nat.lib, name) and name in nat.exported_symbols()
    ws = nat.lib.lz_a2c_workspace_bytes
    slot = (35205 + 4) * 8
    assert ws(1, 6, 2, 0) == slot                      # one tile, one workgroup per net
    assert ws(111, 6, 2, 0) == 4 * slot                # four tiles of 32
    assert ws(5 * 1031, 6, 2, 3) == 3 * slot           # the cap
    assert ws(16 * 4099, 6, 2, 0) == 128 * slot        # the default grid
    assert ws(1 << 22, 6, 2, 0) == 128 * slot
    assert ws(111, 6, 2, 2) == 2 * slot
    assert ws(111, 8, 4, 0) == 4 * (nat.lib.lz_a2c_param_count(8, 4) + 4) * 8
    for bad in ((0, 6, 2, 0), (-5, 6, 2, 0), (10, 0, 2, 0), (10, 9, 2, 0), (10, 6, 5, 0), (10, 6, 2, -1),
                (10, 6, 2, 4097)):
        assert ws(*bad) == -1, bad


def _grad_args(keep):
    """Valid-looking arguments (never dereferenced: every case below is refused first)."""
    g = nat.LzA2cGradArgs()
    fake = ctypes.c_void_p(0x1000)
    for f in ("params", "observations", "actions", "advantages", "returns", "workspace", "grad_sums"):
        setattr(g, f, fake)
    g.n_samples, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 6, 2, 128, 0
    g.vf_coef, g.ent_coef = 0.5, 0.0
    g.workspace_bytes = nat.lib.lz_a2c_workspace_bytes(111, 6, 2, 0)
    keep.append(g)
    return g


def test_grad_refusals_need_no_gpu():
    keep = []
    call = lambda g: nat.lib.lz_a2c_grad_f32(ctypes.byref(g), 0, None)  # noqa: E731
    assert nat.lib.lz_a2c_grad_f32(None, 0, None) == nat.LZ_ERR_INVALID
    for f in ("params", "observations", "actions", "advantages", "returns", "workspace", "grad_sums"):
        g = _grad_args(keep)
        setattr(g, f, None)
        assert call(g) == nat.LZ_ERR_INVALID, f
        assert b"NULL" in nat.lib.lz_last_error()
    for f, v in (("obs_dim", 0), ("obs_dim", 9), ("act_dim", 0), ("act_dim", 5), ("n_samples", 0),
                 ("n_samples", -1), ("max_workgroups", -1), ("max_workgroups", 4097)):
        g = _grad_args(keep)
        setattr(g, f, v)
        assert call(g) == nat.LZ_ERR_INVALID, (f, v)
    for hidden in (64, 127, 256, 0):
        g = _grad_args(keep)
        g.hidden = hidden
        assert call(g) == nat.LZ_ERR_UNSUPPORTED, hidden
        assert b"hidden" in nat.lib.lz_last_error()
    g = _grad_args(keep)
    g.workspace_bytes -= 1
    assert call(g) == nat.LZ_ERR_INVALID
    assert b"workspace" in nat.lib.lz_last_error()


def test_apply_refusals_need_no_gpu():
    fake = ctypes.c_void_p(0x1000)
    assert nat.lib.lz_a2c_apply_f32(None, 0, None) == nat.LZ_ERR_INVALID
    for f in ("grad_sums", "params", "square_avg", "stats"):
        a = nat.LzA2cApplyArgs()
        a.grad_sums = a.params = a.square_avg = a.stats = fake
        a.n_params = 35205
        setattr(a, f, None)
        assert nat.lib.lz_a2c_apply_f32(ctypes.byref(a), 0, None) == nat.LZ_ERR_INVALID, f
    a = nat.LzA2cApplyArgs()
    a.grad_sums = a.params = a.square_avg = a.stats = fake
    a.n_params = 0
    assert nat.lib.lz_a2c_apply_f32(ctypes.byref(a), 0, None) == nat.LZ_ERR_INVALID


def test_struct_layout_matches_header(tmp_path):
    import os
    import subprocess

    from conftest import ROOT

    c = tmp_path / "probe_a2c.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "lorenz_env.h"\n'
        "int main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(lz_a2c_grad_args),"
        " offsetof(lz_a2c_grad_args, n_samples), offsetof(lz_a2c_grad_args, max_workgroups),"
        " offsetof(lz_a2c_grad_args, vf_coef), offsetof(lz_a2c_grad_args, grad_sums),"
        " sizeof(lz_a2c_apply_args), offsetof(lz_a2c_apply_args, lr),"
        " offsetof(lz_a2c_apply_args, stats));return 0;}\n")
    exe = tmp_path / "probe_a2c"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    G, Ap = nat.LzA2cGradArgs, nat.LzA2cApplyArgs
    assert got == [ctypes.sizeof(G), G.n_samples.offset, G.max_workgroups.offset, G.vf_coef.offset,
                   G.grad_sums.offset, ctypes.sizeof(Ap), Ap.lr.offset, Ap.stats.offset]


class _FakeCollector:
    precision = None
    frame_stack = 1
    O, A, n = 6, 2, 4
    device = torch.device("cpu")

    def set_params(self, sd):
        self.sd = sd


def test_fused_a2c_refuses_what_it_does_not_implement():
    sd = ref.make_policy(6, 2, 0)
    col = _FakeCollector()
    with pytest.raises(ValueError, match="normalize_advantage"):
        pol.FusedA2C(col, sd, normalize_advantage=True)
    with pytest.raises(ValueError, match="RMSprop"):
        pol.FusedA2C(col, sd, use_rms_prop=False)
    attn = pol.ActorCriticAttn(6, 2, seed=0).state_dict()
    with pytest.raises(ValueError, match="attention"):
        pol.FusedA2C(col, attn)
    for prec in ("bf16", "i8x4"):
        col.precision = prec
        with pytest.raises(ValueError, match="float32 collector"):
            pol.FusedA2C(col, sd)
    col.precision = "fp32"
    small = pol.ActorCriticMlp(6, 2, hidden=64, seed=0).state_dict()
    with pytest.raises(ValueError, match="hidden=128"):
        pol.FusedA2C(col, small)
    # a valid construction on the host: the flat vector, the initial ones, the round trip
    a2c = pol.FusedA2C(col, sd, learning_rate=pol.linear_schedule(0.0005), n_steps=16)
    assert a2c.params.numel() == 35205 and bool((a2c.square_avg == 1).all())
    back = a2c.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in pol.KEYS) and set(col.sd) == set(pol.KEYS)
    assert set(a2c.optimizer_state()["square_avg"]) == set(pol.KEYS)
    assert a2c._lr() == 0.0005
    # every batch buffer is checked before a launch: a CPU / short buffer never reaches the library
    obs, act, adv, ret = ref.make_batch(sd, 8, 6, 2, 0)
    with pytest.raises(nat.LorenzEnvError):
        pol.a2c_grad(a2c.params, obs[:, :5].contiguous(), act, adv, ret, 6, 2)
    with pytest.raises(nat.LorenzEnvError):
        pol.a2c_grad(a2c.params, obs.double(), act, adv, ret, 6, 2)
