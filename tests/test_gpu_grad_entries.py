"""Two gradient entry points that accept the same net launch the same kernel form: the same
bits.  The pairs: lz_a2c_grad_hidden_f32 and lz_ppo_grad_hidden_f32 at 128 units against the
first entry points, lz_ppo_grad_wide_f32 at obs_dim 6 against lz_ppo_grad_hidden_f32 at 64
units.  33 samples (two tiles, the second ragged) on one workgroup per net, so the
grid-stride loop and the flush run; PPO gathers them from 40 rows through an index list."""
import ctypes

import pytest
import torch

import a2c_ref
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
O, A, N, ROWS = 6, 2, 33, 40


def _launch(entry, ws_name, ws_hidden, hidden, flat, rows, idx):
    """One call of `entry` through ctypes on buffers of exactly the sizes it asks for."""
    ppo = "ppo" in entry
    tail = 6 if ppo else 4
    h = (hidden,) if ws_hidden else ()
    need = int(getattr(nat.lib, ws_name)(N, O, A, *h, 1))
    assert need == (flat.numel() + tail) * 8  # one workgroup per net
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((flat.numel() + tail,), float("nan"), dtype=torch.float64, device=DEV)
    g = (nat.LzPpoGradArgs if ppo else nat.LzA2cGradArgs)()
    g.params = flat.data_ptr()
    g.observations, g.actions, g.advantages, g.returns = [t.data_ptr() for t in rows[:4]]
    g.n_samples, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = N, O, A, hidden, 1
    g.vf_coef, g.ent_coef = 0.5, 0.01
    g.workspace, g.workspace_bytes, g.grad_sums = ws.data_ptr(), need, out.data_ptr()
    if ppo:
        g.old_log_prob, g.old_values, g.indices = rows[4].data_ptr(), rows[5].data_ptr(), idx.data_ptr()
        g.n_rows, g.clip_range, g.clip_range_vf = ROWS, 0.2, 0.3
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    nat.check(getattr(nat.lib, entry)(ctypes.byref(g), 0, stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hidden,one,other", [
    (128, ("lz_a2c_grad_f32", "lz_a2c_workspace_bytes", False),
     ("lz_a2c_grad_hidden_f32", "lz_a2c_workspace_bytes_hidden", True)),
    (128, ("lz_ppo_grad_f32", "lz_ppo_workspace_bytes", False),
     ("lz_ppo_grad_hidden_f32", "lz_ppo_workspace_bytes_hidden", True)),
    (64, ("lz_ppo_grad_hidden_f32", "lz_ppo_workspace_bytes_hidden", True),
     ("lz_ppo_grad_wide_f32", "lz_ppo_workspace_bytes_wide", True)),
])
def test_entry_points_that_share_a_form_give_the_same_bits(hidden, one, other):
    ppo = "ppo" in one[0]
    n = ROWS if ppo else N
    gen = torch.Generator().manual_seed(7)
    flat = a2c_ref.flatten(pol.ActorCriticMlp(O, A, hidden=hidden, seed=3).state_dict()).to(DEV)
    assert flat.numel() == nat.lib.lz_a2c_param_count_hidden(O, A, hidden)
    # observations, actions, advantages, returns, old_log_prob, old_values
    rows = [torch.randn(shape, generator=gen).to(DEV).contiguous()
            for shape in ((n, O), (n, A), (n,), (n,), (n,), (n,))]
    idx = torch.randint(0, ROWS, (N,), generator=gen, dtype=torch.int32).to(DEV)
    a = _launch(*one, hidden, flat, rows, idx)
    b = _launch(*other, hidden, flat, rows, idx)
    P = flat.numel()
    assert bool(torch.isfinite(a).all()) and float(a[:P].abs().max()) > 0 and float(a[P + 3]) == N
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
