"""The PPO update's host side (no GPU): the reference restatement tests/ppo_ref.py is checked
against finite differences, torch.optim.Adam + clip_grad_norm_ and torch.mean / torch.std;
the test cases' construction conditions hold; lz_ppo_* / lz_adam_apply_f32 load, size their
workspace and refuse bad arguments with their status before any HIP call; FusedPPO refuses
what it does not implement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import a2c_ref
import ppo_ref as ref
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol


def test_reference_gradient_matches_central_differences():
    """ppo_ref's float64 autograd gradient against central differences of its own float64
    loss (all options on), h = 1e-6, relative error <= 1e-5 at random coordinates of every
    tensor, with test_a2c_host's floor for coordinates whose difference quotient is rounding.
    The case keeps every row 1e-4 away from a clip edge, 30 times further than h moves one."""
    case = ("fd", 37, 111, 6, 2, 0)
    c = ref.make_case(case, 3)
    O, A = 6, 2
    mb = ref.minibatch(c)
    kw = dict(normalize=True, cvf=ref.CLIP_VF, ent_coef=0.01, vf_coef=0.5)
    g = ref.grad_sums(c["sd"], mb, **kw)
    flat = a2c_ref.flatten(c["sd"]).to(torch.float64)
    rng = np.random.default_rng(0)
    h = 1e-6
    floor = 4 * np.finfo(np.float64).eps * abs(ref.loss64(flat, mb, O, A, **kw)) / (h * 1e-5)
    relative = 0
    for k, (o, shp) in a2c_ref.layout(O, A)[0].items():
        n = int(np.prod(shp))
        for i in rng.choice(n, size=min(n, 36), replace=False):
            up, dn = flat.clone(), flat.clone()
            up[o + i] += h
            dn[o + i] -= h
            fd = (ref.loss64(up, mb, O, A, **kw) - ref.loss64(dn, mb, O, A, **kw)) / (2 * h)
            scale = max(abs(g[o + i]), abs(fd))
            relative += scale >= floor
            assert abs(fd - g[o + i]) <= 1e-5 * max(scale, floor), (k, int(i), fd, g[o + i])
    assert relative >= 150
    # the clip is at work in this case: some rows are zeroed, and the value clip masks some
    zeroed, active_out, inside = ref.regimes(c)
    assert zeroed > 0 and inside > 0 and (np.abs(c["dv"]) > ref.CLIP_VF).any()


def test_adam_and_clip_are_torch_s():
    """ppo_ref.adam_step's arithmetic (before its float32 rounding) against
    torch.optim.Adam(eps=1e-5) and torch.nn.utils.clip_grad_norm_ in float64, three steps,
    clipping (0.5) and not (100)."""
    rng = np.random.default_rng(1)
    for max_norm in (0.5, 100.0):
        p0 = rng.standard_normal(50)
        w = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
        opt = torch.optim.Adam([w], lr=3e-4, eps=1e-5)
        p, m, v = p0.copy(), np.zeros(50), np.zeros(50)
        for t in (1, 2, 3):
            g = rng.standard_normal(50) * (3.0 if t == 2 else 0.3)
            w.grad = torch.tensor(g, dtype=torch.float64)
            total_t = float(torch.nn.utils.clip_grad_norm_([w], max_norm))
            opt.step()
            total = float(np.sqrt(np.sum(g * g)))
            coef = min(1.0, max_norm / (total + 1e-6))
            assert total == pytest.approx(total_t, rel=1e-14)
            assert (coef < 1.0) == (max_norm == 0.5)
            p, m, v = ref.adam64(p, g * coef, m, v, t, 3e-4)
            st = opt.state[w]
            np.testing.assert_allclose(p, w.detach().numpy(), rtol=1e-13, atol=1e-16)
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-13, atol=1e-18)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-20)
            assert int(st["step"]) == t
    # adam_step: the mean, the float32 rounding of the gradient, the clip, one rounding out
    sums = np.array([8.0, -12.0, 0, 0, 0, 4.0, 0, 0])  # two params, count 4: g = (2, -3)
    pa, ma, va, total, coef = ref.adam_step(sums, np.float32([1, 1]), np.float32([0, 0]),
                                            np.float32([0, 0]), 0, 0.1, max_grad_norm=100.0)
    assert total == pytest.approx(np.sqrt(13.0)) and coef == 1.0
    assert ma[0] == np.float32(0.2) and va[1] == np.float32(0.009)
    # step 1 of Adam moves every parameter by lr against the gradient's sign (up to eps)
    assert pa[0] == pytest.approx(0.9, abs=1e-5) and pa[1] == pytest.approx(1.1, abs=1e-5)


def test_adv_moments_are_torch_mean_and_std():
    for n, seed in ((2, 0), (111, 1), (5155, 2)):
        x = torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(torch.float32)
        mean, std = ref.adv_moments(x.numpy())
        assert mean == pytest.approx(float(x.double().mean()), rel=1e-13, abs=1e-17)
        assert std == pytest.approx(float(x.double().std()), rel=1e-13)


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[1] > 1], ids=lambda c: c[0])
def test_case_construction_conditions(case):
    """At most 2 % of the rows a case looks at are dropped for lying within 1e-4 of a clip
    edge; float32 and float64 ratios differ by far less than that margin; for O = 6, A = 2
    each regime of the clip holds at least 3 % of the minibatch."""
    for seed in ref.SEEDS:
        c = ref.make_case(case, seed)
        name, M, n_rows, O, A, _ = case
        assert c["idx"].numel() == M and len(set(c["idx"].tolist())) == M
        assert 0 <= int(c["idx"].min()) and int(c["idx"].max()) < n_rows
        assert c["dropped"] <= 0.02, (name, seed, c["dropped"], c["near_ratio"], c["near_value"])
        obs, act, adv, ret, old_lp, old_v = ref.minibatch(c)
        with torch.no_grad():
            lp32, _, _ = ref.log_prob_entropy(c["sd"], obs, act, torch.float32)
        r32 = torch.exp(lp32 - old_lp).double().numpy()
        assert np.abs(r32 - c["ratio"]).max() <= ref.MARGIN / 10
        assert np.abs(np.abs(c["ratio"] - 1) - ref.CLIP).min() >= ref.MARGIN
        assert np.abs(np.abs(c["dv"]) - ref.CLIP_VF).min() >= ref.MARGIN
        if (O, A) == (6, 2):
            shares = ref.regimes(c)
            print(name, seed, "zeroed %.3f active outside %.3f inside %.3f" % shares,
                  "value clipped %.3f" % float((np.abs(c["dv"]) > ref.CLIP_VF).mean()))
            assert min(shares) >= 0.03, (name, seed, shares)


def test_symbols_load_and_workspace_bytes():
    for name in ("lz_ppo_grad_f32", "lz_ppo_adv_moments", "lz_adam_apply_f32", "lz_ppo_workspace_bytes"):
        assert hasattr(nat.lib, name) and name in nat.exported_symbols()
    ws = nat.lib.lz_ppo_workspace_bytes
    slot = (35205 + 6) * 8
    assert ws(1, 6, 2, 0) == slot
    assert ws(111, 6, 2, 0) == 4 * slot
    assert ws(5 * 1031, 6, 2, 3) == 3 * slot
    assert ws(65536, 6, 2, 0) == 128 * slot
    assert ws(4096, 6, 2, 0) == 128 * slot
    assert ws(64, 6, 2, 0) == 2 * slot
    assert ws(111, 8, 4, 0) == 4 * (nat.lib.lz_a2c_param_count(8, 4) + 6) * 8
    for bad in ((0, 6, 2, 0), (-5, 6, 2, 0), (10, 0, 2, 0), (10, 9, 2, 0), (10, 6, 5, 0), (10, 6, 2, -1),
                (10, 6, 2, 4097)):
        assert ws(*bad) == -1, bad
    assert len(nat.PPO_STATS) == 12 and nat.PPO_STATS[:8] == nat.A2C_STATS


_GRAD_PTRS = ("params", "observations", "actions", "advantages", "returns", "old_log_prob", "workspace",
              "grad_sums")


def _grad_args(keep):
    """Valid-looking arguments (never dereferenced: every case below is refused first)."""
    g = nat.LzPpoGradArgs()
    fake = ctypes.c_void_p(0x1000)
    for f in _GRAD_PTRS + ("indices", "old_values", "adv_moments", "ctrl"):
        setattr(g, f, fake)
    g.n_samples, g.n_rows, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 333, 6, 2, 128, 0
    g.vf_coef, g.ent_coef, g.clip_range, g.clip_range_vf = 0.5, 0.0, 0.2, 0.05
    g.workspace_bytes = nat.lib.lz_ppo_workspace_bytes(111, 6, 2, 0)
    keep.append(g)
    return g


def test_grad_refusals_need_no_gpu():
    keep = []
    call = lambda g: nat.lib.lz_ppo_grad_f32(ctypes.byref(g), 0, None)  # noqa: E731
    assert nat.lib.lz_ppo_grad_f32(None, 0, None) == nat.LZ_ERR_INVALID
    for f in _GRAD_PTRS:
        g = _grad_args(keep)
        setattr(g, f, None)
        assert call(g) == nat.LZ_ERR_INVALID, f
        assert b"NULL" in nat.lib.lz_last_error()
    g = _grad_args(keep)
    g.old_values = None  # needed by the value clip
    assert call(g) == nat.LZ_ERR_INVALID and b"old_values" in nat.lib.lz_last_error()
    nan, inf = float("nan"), float("inf")
    for f, v in (("obs_dim", 0), ("obs_dim", 9), ("act_dim", 0), ("act_dim", 5), ("n_samples", 0),
                 ("n_samples", -1), ("n_rows", 0), ("max_workgroups", -1), ("max_workgroups", 4097),
                 ("clip_range", -0.1), ("clip_range", nan), ("clip_range", inf), ("clip_range_vf", nan),
                 ("clip_range_vf", inf)):
        g = _grad_args(keep)
        setattr(g, f, v)
        assert call(g) == nat.LZ_ERR_INVALID, (f, v)
    g = _grad_args(keep)
    g.indices, g.n_samples, g.n_rows = None, 111, 110  # rows 0..110 of 110 rows
    g.workspace_bytes = 1 << 30
    assert call(g) == nat.LZ_ERR_INVALID and b"n_rows" in nat.lib.lz_last_error()
    for hidden in (64, 127, 256, 0):
        g = _grad_args(keep)
        g.hidden = hidden
        assert call(g) == nat.LZ_ERR_UNSUPPORTED, hidden
        assert b"hidden" in nat.lib.lz_last_error()
    g = _grad_args(keep)
    g.workspace_bytes -= 1
    assert call(g) == nat.LZ_ERR_INVALID
    assert b"workspace" in nat.lib.lz_last_error()


def test_moments_refusals_need_no_gpu():
    fake = ctypes.c_void_p(0x1000)
    call = nat.lib.lz_ppo_adv_moments
    assert call(None, fake, 5, 10, None, fake, 0, None) == nat.LZ_ERR_INVALID
    assert call(fake, fake, 5, 10, None, None, 0, None) == nat.LZ_ERR_INVALID
    assert call(fake, fake, 0, 10, None, fake, 0, None) == nat.LZ_ERR_INVALID
    assert call(fake, fake, 5, 0, None, fake, 0, None) == nat.LZ_ERR_INVALID
    assert call(fake, None, 11, 10, None, fake, 0, None) == nat.LZ_ERR_INVALID
    assert b"n_rows" in nat.lib.lz_last_error()


def _adam_args():
    a = nat.LzAdamApplyArgs()
    fake = ctypes.c_void_p(0x1000)
    a.grad_sums = a.params = a.exp_avg = a.exp_avg_sq = a.ctrl = a.stats = fake
    a.n_params, a.lr, a.max_grad_norm, a.beta1, a.beta2, a.eps = 35205, 3e-4, 0.5, 0.9, 0.999, 1e-5
    return a


def test_adam_refusals_need_no_gpu():
    call = lambda a: nat.lib.lz_adam_apply_f32(ctypes.byref(a), 0, None)  # noqa: E731
    assert nat.lib.lz_adam_apply_f32(None, 0, None) == nat.LZ_ERR_INVALID
    for f in ("grad_sums", "params", "exp_avg", "exp_avg_sq", "ctrl", "stats"):
        a = _adam_args()
        setattr(a, f, None)
        assert call(a) == nat.LZ_ERR_INVALID, f
        assert b"NULL" in nat.lib.lz_last_error()
    for f, v in (("n_params", 0), ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", float("nan"))):
        a = _adam_args()
        setattr(a, f, v)
        assert call(a) == nat.LZ_ERR_INVALID, (f, v)


def test_struct_layout_matches_header(tmp_path):
    from conftest import ROOT

    G, Ad = nat.LzPpoGradArgs, nat.LzAdamApplyArgs
    gf = [n for n, _ in G._fields_]
    af = [n for n, _ in Ad._fields_]
    c = tmp_path / "probe_ppo.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "lorenz_env.h"\nint main(void){\n'
        + 'printf("%zu\\n", sizeof(lz_ppo_grad_args));\n'
        + "".join('printf("%%zu\\n", offsetof(lz_ppo_grad_args, %s));\n' % n for n in gf)
        + 'printf("%zu\\n", sizeof(lz_adam_apply_args));\n'
        + "".join('printf("%%zu\\n", offsetof(lz_adam_apply_args, %s));\n' % n for n in af)
        + "return 0;}\n")
    exe = tmp_path / "probe_ppo"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([ctypes.sizeof(G)] + [getattr(G, n).offset for n in gf]
            + [ctypes.sizeof(Ad)] + [getattr(Ad, n).offset for n in af])
    assert got == want


class _FakeCollector:
    precision = None
    frame_stack = 1
    O, A, n = 6, 2, 4
    device = torch.device("cpu")

    def set_params(self, sd):
        self.sd = sd


def test_fused_ppo_refuses_what_it_does_not_implement():
    import gym_lorenz

    assert gym_lorenz.FusedPPO is pol.FusedPPO
    sd = a2c_ref.make_policy(6, 2, 0)
    col = _FakeCollector()
    attn = pol.ActorCriticAttn(6, 2, seed=0).state_dict()
    with pytest.raises(ValueError, match="attention"):
        pol.FusedPPO(col, attn)
    for prec in ("bf16", "i8x4"):
        col.precision = prec
        with pytest.raises(ValueError, match="float32 collector"):
            pol.FusedPPO(col, sd)
    col.precision = "fp32"
    col.frame_stack = 4
    with pytest.raises(ValueError, match="frame_stack"):
        pol.FusedPPO(col, sd)
    col.frame_stack = 1
    small = pol.ActorCriticMlp(6, 2, hidden=64, seed=0).state_dict()
    with pytest.raises(ValueError, match="hidden=128"):
        pol.FusedPPO(col, small)
    with pytest.raises(ValueError, match="batch_size"):
        pol.FusedPPO(col, sd, batch_size=1)
    pol.FusedPPO(col, sd, batch_size=1, normalize_advantage=False)
    # FusedA2C still refuses what it refused
    with pytest.raises(ValueError, match="normalize_advantage"):
        pol.FusedA2C(col, sd, normalize_advantage=True)
    with pytest.raises(ValueError, match="RMSprop"):
        pol.FusedA2C(col, sd, use_rms_prop=False)
    # a valid construction on the host: SB3's defaults, the flat vector, Adam's zero state
    ppo = pol.FusedPPO(col, sd, learning_rate=pol.linear_schedule(3e-4), clip_range=pol.linear_schedule(0.2))
    assert (ppo.n_steps, ppo.batch_size, ppo.n_epochs, ppo.normalize_advantage) == (2048, 64, 10, True)
    assert (ppo.vf_coef, ppo.ent_coef, ppo.max_grad_norm, ppo.target_kl) == (0.5, 0.0, 0.5, None)
    assert ppo.params.numel() == 35205 and not bool(ppo.exp_avg.any()) and not bool(ppo.exp_avg_sq.any())
    back = ppo.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in pol.KEYS) and set(col.sd) == set(pol.KEYS)
    opt = ppo.optimizer_state()
    assert set(opt) == {"exp_avg", "exp_avg_sq", "step"} and opt["step"] == 0
    assert set(opt["exp_avg"]) == set(opt["exp_avg_sq"]) == set(pol.KEYS)
    assert ppo._lr() == 3e-4 and ppo._now(ppo.clip_range) == 0.2
    ppo.progress_remaining = 0.5
    assert ppo._lr() == 1.5e-4 and ppo._now(ppo.clip_range) == 0.1
    assert ppo.minibatches(130) == [(0, 64), (64, 128), (128, 130)]
    # every buffer is checked before a launch: CPU / short / mistyped buffers never reach the library
    obs, act, adv, ret, lp, v = ref.make_rows(sd, 8, 6, 2, 0)
    with pytest.raises(nat.LorenzEnvError):
        pol.ppo_grad(ppo.params, obs, act, adv, ret, lp, v, 6, 2)
    with pytest.raises(nat.LorenzEnvError):
        pol.ppo_adv_moments(adv)
    with pytest.raises(nat.LorenzEnvError):
        pol.adam_apply(torch.zeros(35211, dtype=torch.float64), ppo.params, ppo.exp_avg, ppo.exp_avg_sq,
                       ppo.ctrl, 3e-4)
    with pytest.raises(nat.LorenzEnvError, match="indices"):
        pol._check_indices(torch.zeros(4, dtype=torch.int64), 8, torch.device("cpu"), "t")
    with pytest.raises(nat.LorenzEnvError, match="indices"):
        pol._check_indices(torch.zeros(0, dtype=torch.int32), 8, torch.device("cpu"), "t")
