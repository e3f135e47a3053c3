"""SB3 2.7.1 ``PPO.train()`` for the float32 MlpPolicy restated in torch on the CPU: the
reference of lz_ppo_adv_moments / lz_ppo_grad_f32 / lz_adam_apply_f32 (include/lorenz_env.h).

  minibatch loss / gradient   ppo/ppo.py:205-262 with ActorCriticPolicy.evaluate_actions and
                              DiagGaussianDistribution (a2c_ref.forward), written with
                              torch.min / torch.clamp as SB3 writes them, so ties and edges
                              are torch's; autograd in float64 (or float32: what SB3 itself
                              computes) over the same float32 inputs
  advantage moments           advantages.mean() / advantages.std() (unbiased), two passes
  clip_grad_norm_ + Adam      torch.nn.utils.clip_grad_norm_ and torch.optim.Adam(betas=(0.9,
                              0.999), eps=1e-5) in NumPy float64 from the float32 state,
                              rounded once (tests/test_ppo_host.py pins it to torch itself)

SB3 is not importable here, so these formulas are restated from its source, not run
against it (parity at the SB3 layer is unpinned).
"""
import math

import numpy as np
import torch

import a2c_ref
from gym_lorenz.policy import KEYS

CLIP, CLIP_VF = 0.2, 0.05
MARGIN = 1e-4          # rows this close (float64) to a clip edge are kept out of a case
OLD_SCALE = 0.02       # the "old" policy: every tensor + OLD_SCALE * N(0, 1)

# (name, M, n_rows, O, A, workgroup cap): the shapes at which the gradient kernel can go
# wrong -- one sample; a gather with a ragged last tile; a grid-stride loop with a ragged
# tail (162 tiles on 3 workgroups per net, 54 each: one flush, after the last tile); the
# same on 2 workgroups per net (81 tiles each: the flush inside the loop after 64 tiles,
# then the last one adds into the slot); the (O, A) corners
CASES = (
    ("m1", 1, 33, 6, 2, 0),
    ("m111", 111, 333, 6, 2, 0),
    ("m5155_cap3", 5 * 1031, 16 * 4099, 6, 2, 3),
    ("m5155_cap2", 5 * 1031, 16 * 4099, 6, 2, 2),
    ("o1a1", 111, 333, 1, 1, 0),
    ("o8a4", 111, 333, 8, 4, 0),
)
SEEDS = (0, 1, 2)
# every option alone and all together: (normalize_advantage, value clipping, ent_coef)
OPTIONS = {
    "plain": (False, False, 0.0),
    "norm": (True, False, 0.0),
    "vclip": (False, True, 0.0),
    "ent": (False, False, 0.01),
    "all": (True, True, 0.01),
}
TAIL = 6


def log_prob_entropy(p, obs, act, dtype):
    """(log_prob [M], entropy per sample (scalar), v [M]) of evaluate_actions."""
    mu, v = a2c_ref.forward(p, obs, dtype)
    ls = p["log_std"].to(dtype)
    var = torch.exp(ls) ** 2
    logp = (-((act.to(dtype) - mu) ** 2) / (2 * var) - ls - math.log(math.sqrt(2 * math.pi))).sum(1)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    return logp, ent, v


def old_policy(sd, seed):
    g = torch.Generator().manual_seed(7000 + seed)
    return {k: (sd[k] + OLD_SCALE * torch.randn(sd[k].shape, generator=g)).to(torch.float32) for k in KEYS}


def make_rows(sd, n_rows, O, A, seed, scale=OLD_SCALE):
    """The flat rollout arrays (obs, act, adv, ret, old_log_prob, old_values), float32:
    a2c_ref.make_batch plus the float32 forward of the perturbed policy."""
    obs, act, adv, ret = a2c_ref.make_batch(sd, n_rows, O, A, 100 + seed)
    old = old_policy(sd, seed)
    with torch.no_grad():
        lp, _, v = log_prob_entropy(old, obs, act, torch.float32)
    return obs, act, adv, ret, lp.contiguous(), v.contiguous()


def edge_report(sd, rows, clip=CLIP, cvf=CLIP_VF):
    """float64 ratio and v - old_v of every row, and which rows lie within MARGIN of an edge."""
    obs, act, adv, ret, old_lp, old_v = rows
    with torch.no_grad():
        lp, _, v = log_prob_entropy(sd, obs, act, torch.float64)
        ratio = torch.exp(lp - old_lp.double()).numpy()
        dv = (v - old_v.double()).numpy()
    near_r = (np.abs(ratio - (1 + clip)) < MARGIN) | (np.abs(ratio - (1 - clip)) < MARGIN)
    near_v = np.abs(np.abs(dv) - cvf) < MARGIN
    return ratio, dv, near_r, near_v


def make_case(case, seed):
    """dict(sd, rows, idx [M] int32, near_ratio, near_value, dropped: shares of the rows
    looked at that lie near an edge, ratio / dv: float64, of the chosen rows).  The minibatch
    is the first M rows of a fixed permutation that are not within MARGIN of a clip edge."""
    name, M, n_rows, O, A, cap = case
    sd = a2c_ref.make_policy(O, A, seed)
    rows = make_rows(sd, n_rows, O, A, seed)
    ratio, dv, near_r, near_v = edge_report(sd, rows)
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(500 + seed)).numpy()
    ok = ~(near_r | near_v)
    if M == 1:  # the one sample is inside both clips: no tensor's gradient is all zero
        ok &= (np.abs(ratio - 1) < CLIP) & (np.abs(dv) < CLIP_VF)
    keep = perm[ok[perm]]
    assert keep.size >= M, (name, keep.size)
    idx = keep[:M]
    looked = int(np.nonzero(perm == idx[-1])[0][0]) + 1  # rows of the permutation gone through
    seen = perm[:looked]
    return dict(case=case, seed=seed, sd=sd, rows=rows, idx=torch.from_numpy(idx.astype(np.int32)),
                near_ratio=float(near_r[seen].mean()), near_value=float(near_v[seen].mean()),
                dropped=float((near_r | near_v)[seen].sum()) / looked, ratio=ratio[idx], dv=dv[idx])


def minibatch(c, idx=None):
    idx = c["idx"] if idx is None else idx
    return tuple(t[idx.long()] for t in c["rows"])


def regimes(c, normalize=True, clip=CLIP):
    """Shares of the minibatch (outside the clip and zeroed, outside and still active, inside)."""
    adv = minibatch(c)[2].double()
    if normalize and adv.numel() > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    adv, ratio = adv.numpy(), c["ratio"]
    outside = (ratio > 1 + clip) | (ratio < 1 - clip)
    zeroed = ((ratio > 1 + clip) & (adv > 0)) | ((ratio < 1 - clip) & (adv < 0))
    return float(zeroed.mean()), float((outside & ~zeroed).mean()), float((~outside).mean())


def loss_sums(p, mb, dtype, normalize=True, clip=CLIP, cvf=CLIP_VF):
    """(sum pl_i, sum (ret - v_pred)^2, sum -entropy, clipped count, sum (ratio-1) - log_ratio)
    as tensors of `dtype`; cvf None: no value clipping."""
    obs, act, adv, ret, old_lp, old_v = mb
    adv, ret, old_lp, old_v = adv.to(dtype), ret.to(dtype), old_lp.to(dtype), old_v.to(dtype)
    if normalize and adv.numel() > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    lp, ent, v = log_prob_entropy(p, obs, act, dtype)
    log_ratio = lp - old_lp
    ratio = torch.exp(log_ratio)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip))
    v_pred = v if cvf is None else old_v + torch.clamp(v - old_v, -cvf, cvf)
    with torch.no_grad():
        n_clip = (torch.abs(ratio - 1) > clip).to(dtype).sum()
        kl = ((ratio - 1) - log_ratio).sum()
    return pl.sum(), ((ret - v_pred) ** 2).sum(), -ent * obs.shape[0], n_clip, kl


def grad_sums(sd, mb, normalize=True, cvf=CLIP_VF, ent_coef=0.0, vf_coef=0.5, clip=CLIP,
              dtype=torch.float64):
    """What lz_ppo_grad_f32 writes, by autograd in `dtype`: float64 numpy [P + 6]."""
    p = {k: sd[k].detach().clone().to(dtype).requires_grad_(True) for k in KEYS}
    pl, vl, el, n_clip, kl = loss_sums(p, mb, dtype, normalize, clip, cvf)
    (pl + vf_coef * vl + ent_coef * el).backward()
    g = torch.cat([p[k].grad.reshape(-1) for k in KEYS]).to(torch.float64)
    tail = torch.stack([pl.detach(), vl.detach(), el.detach(),
                        torch.tensor(float(mb[0].shape[0]), dtype=dtype), n_clip, kl]).to(torch.float64)
    return torch.cat([g, tail]).numpy()


def loss64(flat64, mb, O, A, normalize=True, cvf=CLIP_VF, ent_coef=0.0, vf_coef=0.5, clip=CLIP):
    """The summed loss as a float64 function of the flat float64 parameter vector."""
    p = a2c_ref.unflatten(flat64, O, A)
    pl, vl, el, _, _ = loss_sums(p, mb, torch.float64, normalize, clip, cvf)
    return float(pl + vf_coef * vl + ent_coef * el)


def adv_moments(adv):
    """(mean, unbiased std) in NumPy float64, two passes."""
    x = np.asarray(adv, np.float64)
    mean = x.sum() / x.size
    d = x - mean
    return mean, math.sqrt((d * d).sum() / (x.size - 1))


def adam_step(sums, params32, m32, v32, step, lr, max_grad_norm=0.5, b1=0.9, b2=0.999, eps=1e-5):
    """lz_adam_apply_f32 in NumPy float64 from the float32 state: (params, exp_avg, exp_avg_sq)
    rounded once to float32, the gradient norm and the clip coefficient; step: the count
    before this call."""
    sums = np.asarray(sums, np.float64)
    P = sums.size - TAIL
    g = (sums[:P] / sums[P + 3]).astype(np.float32).astype(np.float64)
    total = math.sqrt(float(np.sum(g * g)))
    coef = min(1.0, max_grad_norm / (total + 1e-6))
    p, m, v = adam64(np.asarray(params32, np.float64), g * coef, np.asarray(m32, np.float64),
                     np.asarray(v32, np.float64), step + 1, lr, b1, b2, eps)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32), total, coef


def adam64(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-5):
    """torch.optim.Adam's step t (1-based) on float64 arrays."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * (g * g)
    step_size = lr / (1.0 - b1 ** t)
    p = p - step_size * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def check_slices(O, A):
    """name -> slice of the [P + 6] vector for every quantity held to the accuracy criterion:
    the 13 tensors, the whole gradient, the three loss sums and the kl sum."""
    lay, P = a2c_ref.layout(O, A)
    out = {k: slice(o, o + int(np.prod(shp))) for k, (o, shp) in lay.items()}
    out.update(all=slice(0, P), policy_sum=slice(P, P + 1), value_sum=slice(P + 1, P + 2),
               entropy_sum=slice(P + 2, P + 3), kl_sum=slice(P + 5, P + 6))
    return out, P
