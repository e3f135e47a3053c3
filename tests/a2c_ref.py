"""SB3 2.7.1 ``A2C.train()`` for the float32 MlpPolicy restated in torch on the CPU: the
reference of lz_a2c_grad_f32 / lz_a2c_apply_f32 (include/lorenz_env.h).

  forward / loss / gradient   a2c/a2c.py:134-190 with ActorCriticPolicy.evaluate_actions and
                              DiagGaussianDistribution (common/distributions.py), as torch
                              autograd in float64 (or float32: what SB3 itself computes) over
                              the same float32 inputs
  clip_grad_norm_             torch.nn.utils.clip_grad_norm_: coef = min(1, max / (total + 1e-6))
  RMSpropTFLike               common/sb2_compat/rmsprop_tf_like.py: square_avg starts at ones,
                              eps inside the root, no momentum, not centred

SB3 is not importable here, so these formulas are restated from its source, not run
against it (parity at the SB3 layer is unpinned).
"""
import math

import numpy as np
import torch

from gym_lorenz.policy import HIDDEN, KEYS, ActorCriticMlp


# (name, B, O, A, workgroup cap, saturated): the shapes at which the gradient kernel can go
# wrong -- one sample; a few 32-sample tiles with a ragged last one; a grid-stride loop with
# a ragged tail (162 tiles on 3 workgroups per net); the default grid with a ragged tail;
# every (O, A) corner (an odd O pads the last k-step); tanh' at its rounding floor
CASES = (
    ("b1", 1, 6, 2, 0, False),
    ("b111", 111, 6, 2, 0, False),
    ("b5155_cap3", 5 * 1031, 6, 2, 3, False),
    ("b65584", 16 * 4099, 6, 2, 0, False),
    ("o1a1", 111, 1, 1, 0, False),
    ("o7a3", 111, 7, 3, 0, False),
    ("o8a4", 111, 8, 4, 0, False),
    ("saturated", 111, 6, 2, 0, True),
)
SEEDS = (0, 1, 2)
# a float32 result is not expected closer to the float64 one than half an ulp: the floor of
# err_t32 in the ratio err_gpu / err_t32 (a one-element tensor's float32 value can be exact)
ERR_FLOOR = 2.0 ** -24


def case_inputs(case, seed):
    """(state_dict, batch) of a CASES row: the saturated one scales both W1 by 8."""
    _, B, O, A, _, sat = case
    sd = make_policy(O, A, seed)
    if sat:
        for k in ("mlp_extractor.policy_net.0.weight", "mlp_extractor.value_net.0.weight"):
            sd[k] = (sd[k] * 8.0).contiguous()
    return sd, make_batch(sd, B, O, A, 100 + seed, saturate=sat)


def shapes(O, A, H=HIDDEN):
    return [(H, O), (H,), (H, H), (H,)] * 2 + [(A, H), (A,), (1, H), (1,), (A,)]


def layout(O, A):
    """{key: (offset, shape)} of the flat parameter vector, and its length P."""
    out, o = {}, 0
    for k, shp in zip(KEYS, shapes(O, A)):
        out[k] = (o, shp)
        o += int(np.prod(shp))
    return out, o


def flatten(sd):
    return torch.cat([torch.as_tensor(sd[k]).detach().reshape(-1).to(torch.float32) for k in KEYS])


def unflatten(flat, O, A):
    lay, _ = layout(O, A)
    return {k: flat[o:o + int(np.prod(shp))].reshape(shp) for k, (o, shp) in lay.items()}


def make_policy(O, A, seed):
    """ActorCriticMlp(seed) with the biases and log_std moved away from their zero init
    (every one of the 13 gradients is then non-zero) -> float32 state_dict."""
    net = ActorCriticMlp(O, A, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k in KEYS:
        if k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    sd["log_std"] = -0.3 + 0.2 * torch.randn(sd["log_std"].shape, generator=g)
    return {k: sd[k].to(torch.float32).contiguous() for k in KEYS}


def make_batch(sd, B, O, A, seed, saturate=False):
    """obs ~ N(0,1) clipped to +-10, actions = mu + sigma eps, adv and ret ~ N(0,1), float32.
    saturate: observations at +-10 (the caller scales W1): 1 - h^2 at its rounding floor."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(B, O, generator=g).clamp(-10, 10)
    if saturate:
        obs = torch.where(obs >= 0, torch.tensor(10.0), torch.tensor(-10.0))
    with torch.no_grad():
        mu, _ = forward(sd, obs, torch.float32)
    act = mu + torch.exp(sd["log_std"]) * torch.randn(B, A, generator=g)
    adv = torch.randn(B, generator=g)
    ret = torch.randn(B, generator=g)
    return tuple(t.to(torch.float32).contiguous() for t in (obs, act, adv, ret))


def forward(p, obs, dtype):
    x = obs.to(dtype)
    q = {k: p[k].to(dtype) for k in KEYS}

    def net(pre, w3, b3):
        h = torch.tanh(x @ q[pre + ".0.weight"].T + q[pre + ".0.bias"])
        h = torch.tanh(h @ q[pre + ".2.weight"].T + q[pre + ".2.bias"])
        return h @ q[w3].T + q[b3]

    mu = net("mlp_extractor.policy_net", "action_net.weight", "action_net.bias")
    v = net("mlp_extractor.value_net", "value_net.weight", "value_net.bias").flatten()
    return mu, v


def loss_sums(p, batch, dtype):
    """(sum(-adv log_prob), sum((ret - v)^2), sum(-entropy)) as tensors of `dtype`."""
    obs, act, adv, ret = batch
    mu, v = forward(p, obs, dtype)
    ls = p["log_std"].to(dtype)
    var = torch.exp(ls) ** 2
    logp = (-((act.to(dtype) - mu) ** 2) / (2 * var) - ls - math.log(math.sqrt(2 * math.pi))).sum(1)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    return (-(adv.to(dtype) * logp)).sum(), ((ret.to(dtype) - v) ** 2).sum(), -ent * obs.shape[0]


def grad_sums(sd, batch, vf_coef=0.5, ent_coef=0.0, dtype=torch.float64):
    """What lz_a2c_grad_f32 writes, by autograd in `dtype`: float64 numpy [P + 4] (sums over
    the samples, not divided by B)."""
    p = {k: sd[k].detach().clone().to(dtype).requires_grad_(True) for k in KEYS}
    pl, vl, el = loss_sums(p, batch, dtype)
    (pl + vf_coef * vl + ent_coef * el).backward()
    g = torch.cat([p[k].grad.reshape(-1) for k in KEYS]).to(torch.float64)
    tail = torch.stack([pl.detach(), vl.detach(), el.detach()]).to(torch.float64)
    return torch.cat([g, tail, torch.tensor([float(batch[0].shape[0])], dtype=torch.float64)]).numpy()


def loss64(flat64, batch, O, A, vf_coef=0.5, ent_coef=0.0):
    """The summed loss as a float64 function of the flat float64 parameter vector."""
    p = unflatten(flat64, O, A)
    pl, vl, el = loss_sums(p, batch, torch.float64)
    return float(pl + vf_coef * vl + ent_coef * el)


def apply_step(sums, params32, sq32, lr, max_grad_norm=0.5, alpha=0.99, eps=1e-5):
    """lz_a2c_apply_f32 in NumPy float64 from the float32 state: (params, square_avg) rounded
    once to float32, the gradient norm and the clip coefficient."""
    sums = np.asarray(sums, np.float64)
    P = sums.size - 4
    g = (sums[:P] / sums[P + 3]).astype(np.float32).astype(np.float64)
    total = math.sqrt(float(np.sum(g * g)))
    coef = min(1.0, max_grad_norm / (total + 1e-6))
    g = g * coef
    s = alpha * np.asarray(sq32, np.float64) + (1.0 - alpha) * (g * g)
    p = np.asarray(params32, np.float64) - lr * g / np.sqrt(s + eps)
    return p.astype(np.float32), s.astype(np.float32), total, coef


def rmsprop_tf_like(p, g, sq=None, lr=7e-4, alpha=0.99, eps=1e-5):
    """One RMSpropTFLike step on float64 arrays: (p, square_avg); square_avg None = the
    initial ones."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    sq = np.ones_like(p) if sq is None else np.asarray(sq, np.float64)
    sq = alpha * sq + (1.0 - alpha) * g * g
    return p - lr * g / np.sqrt(sq + eps), sq


def rel_err(a, b):
    """||a - b|| / ||b||."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def per_tensor(vec, O, A):
    lay, _ = layout(O, A)
    return {k: np.asarray(vec)[o:o + int(np.prod(shp))] for k, (o, shp) in lay.items()}


def ulp_diff(a, b):
    """Largest distance in float32 ulps between two float32 arrays of finite values."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.max(np.abs(key(a) - key(b)))) if np.size(a) else 0
