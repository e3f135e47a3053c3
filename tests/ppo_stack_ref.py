"""Cases of the wide PPO gradient (lz_ppo_grad_wide_f32: the 64-unit MlpPolicy on a 24-wide
frame-stacked observation, code/lorenz_filter/train.py:109-131), shared by
tests/test_gpu_ppo_stack.py and tools/mlp_stack_bench.py.  Built on tests/mlp_learner_ref.py
and tests/ppo_ref.py, which take any input width."""
import numpy as np
import torch

import a2c_ref
import mlp_learner_ref as ref
import ppo_ref
from gym_lorenz.policy import KEYS

O_WIDE, A, H = 24, 2, 64
# the project's own bound for the 64-unit PPO kernel (tests/test_gpu_learner_h64.py): not
# re-derived from the kernel under test
RATIO = 2 * 24.061
# (name, M, workgroup cap): one sample; ragged tiles; 66 tiles on ONE workgroup per net (the
# float32 accumulators are flushed after tile 64 inside the loop); a grid-stride loop with a
# ragged tail (162 tiles on 3 workgroups per net)
CASES = (("m1", 1, 0), ("m111", 111, 0), ("m2085_cap1", 2085, 1), ("m5155_cap3", 5155, 3))
SEEDS = (0, 1, 2)
W1_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.value_net.0.weight")


def case(name, seed, O=O_WIDE):
    """mlp_learner_ref.ppo_case of a CASES row at input width O."""
    _, M, cap = next(c for c in CASES if c[0] == name)
    return ref.ppo_case((name, M, O, A, cap, False), seed)


def options(M, normalize):
    """Value clipping and the entropy term on; normalisation as asked (SB3: only with more
    than one sample)."""
    return dict(normalize=bool(normalize) and M > 1, cvf=ppo_ref.CLIP_VF, ent_coef=0.01)


def cpu(c, dtype, normalize=True):
    return ppo_ref.grad_sums(c["sd"], ref.ppo_minibatch(c), dtype=dtype, **options(c["M"], normalize))


def gpu(pol, dev, c, normalize=True, wide=True, **kw):
    """ppo_adv_moments + ppo_grad on a case: wide -> lz_ppo_grad_wide_f32, else
    lz_ppo_grad_hidden_f32 (hidden = 64 either way), same inputs, same grid cap."""
    rows = [t.to(dev) for t in c["rows"]]
    idx = c["idx"].to(dev)
    opt = options(c["M"], normalize)
    mom = pol.ppo_adv_moments(rows[2], idx) if opt["normalize"] else None
    kw.setdefault("max_workgroups", c["cap"])
    return pol.ppo_grad(a2c_ref.flatten(c["sd"]).to(dev), *rows, c["O"], c["A"], idx, ppo_ref.CLIP, opt["cvf"],
                        mom, None, 0.5, opt["ent_coef"], hidden=H, wide=wide, **kw)


def embed(c, O=O_WIDE):
    """The case's problem embedded in O inputs: observation columns and W1 columns past its
    own are zero, everything else is the same object."""
    o = c["O"]
    sd = dict(c["sd"])
    for k in W1_KEYS:
        big = torch.zeros((H, O), dtype=torch.float32)
        big[:, :o] = sd[k]
        sd[k] = big.contiguous()
    obs = torch.zeros((c["n_rows"], O), dtype=torch.float32)
    obs[:, :o] = c["rows"][0]
    return dict(c, O=O, sd=sd, rows=(obs.contiguous(),) + tuple(c["rows"][1:]))


def embedded_index(o, O=O_WIDE):
    """int64 [P_o]: where entry i of the o-input flat vector sits in the O-input one."""
    lay, P = ref.layout(O, A, H)
    idx = []
    for k, shp in zip(KEYS, ref.shapes(o, A, H)):
        off, big = lay[k]
        grid = np.arange(int(np.prod(big)), dtype=np.int64).reshape(big)
        sub = grid[:shp[0], :shp[1]] if len(shp) == 2 else grid[:shp[0]]
        idx.append(off + sub.reshape(-1))
    idx = np.concatenate(idx)
    assert idx.size == ref.layout(o, A, H)[1] and np.unique(idx).size == idx.size and idx.max() < P
    return idx
