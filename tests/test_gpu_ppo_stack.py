"""The wide PPO gradient kernel (k_ppo_grad_h64_wide through lz_ppo_grad_wide_f32) and
FusedPPO(net_arch=64) on a frame-stacked collector (code/lorenz_filter/train.py:109-131) on
the MI355X.

(1) No tolerance: a 6-input problem embedded in 24 inputs (observation columns and W1 columns
past 6 are zero) through the wide entry point equals lz_ppo_grad_hidden_f32 at O = 6 value for
value on every shared entry and all six sums, and dW1[:, 6:] is zero -- the 18 more inputs add
exact zeros to every chain, and tiles, flushes and slots are the same.  (2) True 24-input
minibatches against torch float64 CPU autograd by the project's criterion

    err_gpu <= RATIO * max(err_t32, 2^-24),  RATIO = 2 x 24.061

per tensor, for the whole vector and for the sums -- the 64-unit PPO kernel's own bound
(tests/test_gpu_learner_h64.py), not re-derived here; counts exact; two launches bit-identical.
Measured (tools/mlp_stack_bench.py -> profiles/mlp_stack/grad_error.json): worst ratio 17.03,
the policy-loss sum at M = 2085 on one workgroup per net; the worst tensor 6.88.
(3) FusedPPO.learn end to end on the stacked HR collector equals a loop over the wrappers bit
for bit, and the collector's blob is the host pack of state_dict() afterwards."""
import numpy as np
import pytest
import torch

import a2c_ref
import mlp_learner_ref as ref
import ppo_stack_ref as ps
import gym_lorenz as gl
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LR = 3e-4
_CACHE = {}


def _case(name, seed=0, O=ps.O_WIDE):
    key = (name, seed, O)
    if key not in _CACHE:
        _CACHE[key] = ps.case(name, seed, O)
    return _CACHE[key]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", ["m111", "m2085_cap1"])
def test_embedded_six_input_problem_is_value_equal(name, normalize):
    c6 = _case(name, 0, 6)
    c24 = ps.embed(c6)
    narrow = ps.gpu(pol, DEV, c6, normalize, wide=False).cpu().numpy()
    wide = ps.gpu(pol, DEV, c24, normalize, wide=True).cpu().numpy()
    P6, P24 = ref.layout(6, 2, 64)[1], ref.layout(24, 2, 64)[1]
    assert (P6, P24) == (9413, 11717) and narrow.size == P6 + 6 and wide.size == P24 + 6
    idx = ps.embedded_index(6)
    assert ref.same_values(narrow[:P6], wide[idx]), (
        int((narrow[:P6] != wide[idx]).sum()), float(np.abs(narrow[:P6] - wide[idx]).max()))
    assert ref.same_values(narrow[P6:], wide[P24:]), (narrow[P6:], wide[P24:])
    rest = np.ones(P24, bool)
    rest[idx] = False
    assert rest.sum() == 2 * 64 * 18 and not wide[:P24][rest].any()  # dW1[:, 6:] of both nets
    assert np.abs(narrow[:P6]).max() > 0 and wide[P24 + 3] == c6["M"]
    # the wide entry point at obs_dim <= 8 launches the 64-unit kernel itself: the same bits
    again = ps.gpu(pol, DEV, c6, normalize, wide=True)
    assert np.array_equal(again.cpu().numpy().view(np.int64), narrow.view(np.int64))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", [c[0] for c in ps.CASES])
def test_wide_gradient_and_sums_match_float64_autograd(name, normalize):
    slices, P = ref.slices("ppo", ps.O_WIDE, ps.A)
    assert P == 11717 and len(slices) == 13 + 5
    for seed in ps.SEEDS:
        c = _case(name, seed)
        g64, g32 = ps.cpu(c, torch.float64, normalize), ps.cpu(c, torch.float32, normalize)
        got = ps.gpu(pol, DEV, c, normalize).cpu().numpy()
        rows = ref.accuracy_rows(got, g64, g32, slices)
        for k, (e_gpu, e_t32, ratio) in rows.items():
            print("wide %s norm=%d seed %d %s: err_gpu %.3e err_t32 %.3e ratio %.2f"
                  % (name, normalize, seed, k, e_gpu, e_t32, ratio))
        for k, (e_gpu, e_t32, ratio) in rows.items():
            assert e_gpu <= ps.RATIO * max(e_t32, a2c_ref.ERR_FLOOR), (name, seed, k, e_gpu, e_t32)
        assert got[P + 3] == c["M"] and got[P + 4] == g64[P + 4]  # the counts are exact


@pytest.mark.parametrize("name", ["m111", "m2085_cap1", "m5155_cap3"])
def test_two_wide_launches_are_bit_identical(name):
    c = _case(name)
    need = int(nat.lib.lz_ppo_workspace_bytes_wide(c["M"], 24, 2, 64, c["cap"])) // 8
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)
    a = ps.gpu(pol, DEV, c, workspace=ws).clone()
    ws.fill_(float("nan"))  # the second launch must not read what the first one left
    b = ps.gpu(pol, DEV, c, workspace=ws)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert bool(torch.isfinite(b).all())


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("params", "m", "v", "ctrl"))


def test_fused_ppo_on_the_stacked_collector_learn_equals_the_wrappers():
    """HR (add_filter, as the reference's script), 70 envs, frame_stack = 4, n_steps = 8 (560
    rows), batch_size = 64 (a ragged ninth minibatch), n_epochs = 2, two updates."""
    n, K, bs, n_epochs = 70, 8, 64, 2
    B = n * K
    env = gl.BatchedEnv("hr", n, seed=5, add_filter=True, max_episode_steps=5)
    col = pol.FusedRolloutCollector(env, None, precision="fp32", frame_stack=4)
    sd0 = ref.make_policy(24, 2, 4)
    gen = torch.Generator(device=DEV).manual_seed(123)
    twin_gen = torch.Generator(device=DEV).manual_seed(123)
    ppo = pol.FusedPPO(col, sd0, learning_rate=LR, n_steps=K, batch_size=bs, n_epochs=n_epochs, ent_coef=0.01,
                       generator=gen, net_arch=64)
    assert ppo.wide and ppo.P == 11717 and col.mlp_stack

    def blob_is_pack_of(sd):
        return np.array_equal(col.blob.cpu().numpy(), pol.pack_policy_stack_f32(sd, 24, 2))

    assert blob_is_pack_of(sd0)
    prev = {"params": ppo.params.clone(), "m": ppo.exp_avg.clone(), "v": ppo.exp_avg_sq.clone(),
            "ctrl": ppo.ctrl.clone()}
    cuts = [(lo, min(lo + bs, B)) for lo in range(0, B, bs)]
    assert len(cuts) == 9 and cuts[-1] == (512, 560)
    seen = []

    def check(model, batch, out):
        i = len(seen)
        assert batch.observations.shape == (K, n, 24) and (batch.dones != 0).any()
        s = {k: v.clone() for k, v in prev.items()}
        stats = torch.zeros((n_epochs * len(cuts), 12), dtype=torch.float64, device=DEV)
        flat = (batch.observations, batch.actions, batch.advantages, batch.returns, batch.log_probs, batch.values)
        row = 0
        for _ in range(n_epochs):
            perm = torch.randperm(B, dtype=torch.int32, device=DEV, generator=twin_gen)
            for lo, hi in cuts:
                idx = perm[lo:hi]
                mom = pol.ppo_adv_moments(batch.advantages, idx)
                sums = pol.ppo_grad(s["params"], *flat, 24, 2, idx, 0.2, None, mom, s["ctrl"], 0.5, 0.01,
                                    hidden=64, wide=True)
                pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], LR, 0.5, vf_coef=0.5, ent_coef=0.01,
                               stats=stats[row])
                row += 1
        mine = {"params": model.params, "m": model.exp_avg, "v": model.exp_avg_sq, "ctrl": model.ctrl}
        assert row == 18 and _same_bits(s, mine)
        assert s["ctrl"].tolist() == [(i + 1) * row, 0]
        assert np.array_equal(stats.cpu().numpy().view(np.int64), out["rows"].view(np.int64))
        assert np.isfinite(out["rows"]).all()
        assert out["rows"][:, 6].tolist() == ([bs] * 8 + [48]) * n_epochs
        assert out["n_updates"] == (i + 1) * n_epochs and not out["stopped"]
        assert blob_is_pack_of(model.state_dict())
        for k in prev:
            prev[k] = mine[k].clone()
        seen.append(out)

    out = ppo.learn(2 * B, callback=check)
    assert len(out) == len(seen) == 2 and ppo.num_timesteps == 2 * B
    assert not torch.equal(ppo.params.cpu(), a2c_ref.flatten(sd0))
    assert ppo.optimizer_state()["step"] == 2 * n_epochs * len(cuts)
    back = ppo.state_dict()
    assert tuple(back["mlp_extractor.policy_net.0.weight"].shape) == (64, 24)
    assert blob_is_pack_of(back) and not blob_is_pack_of(sd0)
    env.close()
