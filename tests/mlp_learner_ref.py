"""Hidden-size-aware helpers for the 64-unit learner tests: what tests/a2c_ref.py fixes at
128 units (its layout and make_policy), the zero-padded 128-unit twin of a 64-unit net, the
shapes at which the 64-unit gradient kernels can go wrong, and the reference's two shipped
PPO policies (tests/golden/ref_ppo_policies.npz).  a2c_ref.forward / loss_sums / grad_sums /
flatten / apply_step / ulp_diff and ppo_ref's loss do not depend on the hidden size and are
used as they are.

The padded twin is exact: a padded unit has h = tanh(0) = 0 and zero outgoing weights, so
every product it enters is an exact zero, every gradient entry that touches it is exactly 0,
and adding exact zeros changes no float32 chain of the units that are there."""
import os

import numpy as np
import torch

import a2c_ref
from gym_lorenz.policy import KEYS, ActorCriticMlp

H64, H128 = 64, 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ppo_policies.npz")

# (name, B, O, A, workgroup cap, saturated): one sample; ragged tiles; a grid-stride loop with
# a ragged tail (162 tiles on 3 workgroups per net); 66 tiles on ONE workgroup per net: the
# float32 accumulators are flushed after tile 64 inside the loop and the last two tiles add
# into the slot; the (O, A) corners (an odd O pads the last k-step; O = 8 needs both passes of
# the 128-thread x fill); tanh' at its rounding floor
CASES = (
    ("b1", 1, 6, 2, 0, False),
    ("b111", 111, 6, 2, 0, False),
    ("b5155_cap3", 5 * 1031, 6, 2, 3, False),
    ("b2085_cap1", 2085, 6, 2, 1, False),
    ("o1a1", 111, 1, 1, 0, False),
    ("o7a3", 111, 7, 3, 0, False),
    ("o8a4", 111, 8, 4, 0, False),
    ("saturated", 111, 6, 2, 0, True),
)
SEEDS = (0, 1, 2)
# the shipped policies as weights on a synthetic batch: (name, B, O, A)
SHIPPED = (("hr", 111, 6, 1), ("lorenz", 111, 8, 3))
SHIPPED_OLD_SCALE = 0.002


def shapes(O, A, H):
    return a2c_ref.shapes(O, A, H)


def layout(O, A, H):
    """{key: (offset, shape)} of the flat parameter vector of an H-unit net, and its length."""
    out, o = {}, 0
    for k, shp in zip(KEYS, shapes(O, A, H)):
        out[k] = (o, shp)
        o += int(np.prod(shp))
    return out, o


def param_count(O, A, H):
    return 2 * (H * O + H + H * H + H) + A * H + A + H + 1 + A


def make_policy(O, A, seed, hidden=H64):
    """a2c_ref.make_policy for a net of `hidden` units: ActorCriticMlp(seed) with the biases
    and log_std moved off their zero init -> float32 state_dict."""
    net = ActorCriticMlp(O, A, hidden=hidden, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k in KEYS:
        if k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    sd["log_std"] = -0.3 + 0.2 * torch.randn(sd["log_std"].shape, generator=g)
    return {k: sd[k].to(torch.float32).contiguous() for k in KEYS}


def shipped_policy(name):
    """The 13 float32 tensors of a shipped reference policy ("hr": O = 6, A = 1; "lorenz":
    O = 8, A = 3)."""
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z["%s/%s" % (name, k)].copy()) for k in KEYS}


def unflatten(flat, O, A, H):
    lay, _ = layout(O, A, H)
    return {k: flat[o:o + int(np.prod(shp))].reshape(shp) for k, (o, shp) in lay.items()}


def pad_to_128(sd):
    """The 13 tensors zero-padded to 128 hidden units (log_std and the head biases as they are)."""
    H = sd["mlp_extractor.policy_net.2.weight"].shape[0]
    O = sd["mlp_extractor.policy_net.0.weight"].shape[1]
    A = sd["action_net.weight"].shape[0]
    out = {}
    for k, shp in zip(KEYS, shapes(O, A, H128)):
        src = torch.as_tensor(sd[k]).to(torch.float32)
        big = torch.zeros(shp, dtype=torch.float32)
        if src.dim() == 2:
            big[:src.shape[0], :src.shape[1]] = src
        else:
            big[:src.shape[0]] = src
        out[k] = big.contiguous()
    assert H <= H128
    return out


def unpadded_index(O, A, H=H64):
    """int64 [P_H]: where entry i of the H-unit flat vector sits in the 128-unit one."""
    lay128, P128 = layout(O, A, H128)
    idx = []
    for k, shp in zip(KEYS, shapes(O, A, H)):
        o128, shp128 = lay128[k]
        grid = np.arange(int(np.prod(shp128)), dtype=np.int64).reshape(shp128)
        sub = grid[:shp[0], :shp[1]] if len(shp) == 2 else grid[:shp[0]]
        idx.append(o128 + sub.reshape(-1))
    idx = np.concatenate(idx)
    assert idx.size == layout(O, A, H)[1] and np.unique(idx).size == idx.size and idx.max() < P128
    return idx


def case_inputs(case, seed):
    """(64-unit state_dict, batch) of a CASES row: the saturated one scales both W1 by 8."""
    _, B, O, A, _, sat = case
    sd = make_policy(O, A, seed)
    if sat:
        for k in ("mlp_extractor.policy_net.0.weight", "mlp_extractor.value_net.0.weight"):
            sd[k] = (sd[k] * 8.0).contiguous()
    return sd, a2c_ref.make_batch(sd, B, O, A, 100 + seed, saturate=sat)


def same_values(a, b):
    """Value equality of two float64 arrays with NaNs equal (only a zero's sign may differ)."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ------------------------------------------------------------------ cases shared by the GPU
# tests and tools/learner_h64_grad_error.py
def a2c_case(case, seed, sd=None):
    """dict(name, O, A, B, cap, sd, batch) of a CASES row (sd given: a shipped policy's
    weights on the row's synthetic batch)."""
    name, B, O, A, cap, sat = case
    if sd is None:
        sd, batch = case_inputs(case, seed)
    else:
        batch = a2c_ref.make_batch(sd, B, O, A, 100 + seed)
    return dict(name=name, O=O, A=A, B=B, cap=cap, sd=sd, batch=batch, seed=seed)


def ppo_case(case, seed, sd=None, M=None, old_scale=None):
    """ppo_ref.make_case for a 64-unit net on a CASES row: the flat rollout arrays of
    2 B + 32 rows (old log-probs and values from the perturbed policy), and a minibatch of M
    (default B) gathered rows of a fixed permutation that are not within ppo_ref.MARGIN of a
    clip edge.  old_scale: the perturbation that makes the old policy (default
    ppo_ref.OLD_SCALE).  dict(name, O, A, M, n_rows, cap, sd, rows, idx)."""
    import ppo_ref

    name, B, O, A, cap, sat = case
    M = B if M is None else M
    n_rows = 2 * B + 32
    if sd is None:
        sd, _ = case_inputs(case, seed)
    obs, act, adv, ret = a2c_ref.make_batch(sd, n_rows, O, A, 100 + seed, saturate=sat)
    scale = ppo_ref.OLD_SCALE if old_scale is None else old_scale
    g = torch.Generator().manual_seed(7000 + seed)  # ppo_ref.old_policy's draws
    old = {k: (sd[k] + scale * torch.randn(sd[k].shape, generator=g)).to(torch.float32) for k in KEYS}
    with torch.no_grad():
        lp, _, v = ppo_ref.log_prob_entropy(old, obs, act, torch.float32)
    rows = (obs, act, adv, ret, lp.contiguous(), v.contiguous())
    ratio, dv, near_r, near_v = ppo_ref.edge_report(sd, rows)
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(500 + seed)).numpy()
    ok = ~(near_r | near_v)
    if M == 1:  # the one sample is inside both clips: no tensor's gradient is all zero
        ok &= (np.abs(ratio - 1) < ppo_ref.CLIP) & (np.abs(dv) < ppo_ref.CLIP_VF)
    keep = perm[ok[perm]]
    assert keep.size >= M, (name, keep.size)
    idx = torch.from_numpy(keep[:M].astype(np.int32))
    return dict(name=name, O=O, A=A, M=M, n_rows=n_rows, cap=cap, sd=sd, rows=rows, idx=idx, seed=seed)


def shipped_case(kind, which, seed):
    """A shipped policy's weights on a synthetic 111-row batch (A2C) or minibatch (PPO).  The
    trained value heads reach |v| = 300 on N(0, 1) observations, so a perturbation of 0.02 moves
    v past SB3-sized value clips on 98 % of the rows and the vf net's gradient would be (nearly)
    all zero; at SHIPPED_OLD_SCALE a quarter of the rows stay inside the clip and nearly all
    inside the ratio clip."""
    name, B, O, A = next(s for s in SHIPPED if s[0] == which)
    row = ("shipped_" + name, B, O, A, 0, False)
    if kind == "a2c":
        return a2c_case(row, seed, sd=shipped_policy(name))
    return ppo_case(row, seed, sd=shipped_policy(name), old_scale=SHIPPED_OLD_SCALE)


def ppo_minibatch(c):
    return tuple(t[c["idx"].long()] for t in c["rows"])


def ppo_options(M):
    """Every option on: normalisation (SB3: only with more than one sample), value clipping,
    the entropy term."""
    import ppo_ref

    return dict(normalize=M > 1, cvf=ppo_ref.CLIP_VF, ent_coef=0.01)


def accuracy_rows(got, g64, g32, slices):
    """{slice name: (err_gpu, err_t32, ratio)} of f3u's criterion; every norm must be > 0."""
    out = {}
    for k, sl in slices.items():
        assert np.linalg.norm(g64[sl]) > 0, k  # nothing passes vacuously
        e_gpu, e_t32 = a2c_ref.rel_err(got[sl], g64[sl]), a2c_ref.rel_err(g32[sl], g64[sl])
        out[k] = (e_gpu, e_t32, e_gpu / max(e_t32, a2c_ref.ERR_FLOOR))
    return out


def slices(kind, O, A, H=H64):
    """name -> slice of the sums vector for every quantity held to the accuracy criterion:
    the 13 tensors, the whole gradient, the loss sums (PPO: and the kl sum)."""
    lay, P = layout(O, A, H)
    out = {k: slice(o, o + int(np.prod(shp))) for k, (o, shp) in lay.items()}
    out.update(all=slice(0, P), policy_sum=slice(P, P + 1), value_sum=slice(P + 1, P + 2),
               entropy_sum=slice(P + 2, P + 3))
    if kind == "ppo":
        out.update(kl_sum=slice(P + 5, P + 6))
    return out, P


def gpu_a2c(pol, dev, c, hidden=H64, rows=None, **kw):
    """a2c_grad on a case: the 64-unit net through the 64-unit kernel (hidden=64) or its
    zero-padded twin through the 128-unit kernel (hidden=128), same inputs, same grid cap."""
    sd = c["sd"] if hidden == H64 else pad_to_128(c["sd"])
    batch = c["batch"] if rows is None else tuple(t[rows].contiguous() for t in c["batch"])
    kw.setdefault("max_workgroups", c["cap"])
    return pol.a2c_grad(a2c_ref.flatten(sd).to(dev), *[t.to(dev) for t in batch], c["O"], c["A"], 0.5, 0.01,
                        hidden=hidden, **kw)


def gpu_ppo(pol, dev, c, hidden=H64, idx="case", ctrl=None, normalize=True, **kw):
    """ppo_adv_moments (more than one sample) + ppo_grad with every option on, as gpu_a2c.
    normalize=False leaves the moments out: those of a minibatch with an index outside the
    arrays are NaN by contract, and so is every gradient that uses them."""
    import ppo_ref

    sd = c["sd"] if hidden == H64 else pad_to_128(c["sd"])
    rows = [t.to(dev) for t in c["rows"]]
    idx = c["idx"].to(dev) if isinstance(idx, str) else idx
    opt = ppo_options(int(idx.numel()))
    mom = pol.ppo_adv_moments(rows[2], idx) if opt["normalize"] and normalize else None
    kw.setdefault("max_workgroups", c["cap"])
    return pol.ppo_grad(a2c_ref.flatten(sd).to(dev), *rows, c["O"], c["A"], idx, ppo_ref.CLIP, opt["cvf"], mom,
                        ctrl, 0.5, opt["ent_coef"], hidden=hidden, **kw)


def cpu_a2c(c, dtype):
    return a2c_ref.grad_sums(c["sd"], c["batch"], 0.5, 0.01, dtype=dtype)


def cpu_ppo(c, dtype):
    import ppo_ref

    return ppo_ref.grad_sums(c["sd"], ppo_minibatch(c), dtype=dtype, **ppo_options(c["M"]))


def accuracy_cases(kind):
    """[(label, builder(seed))]: every CASES row and both shipped policies."""
    make = a2c_case if kind == "a2c" else ppo_case
    out = [(row[0], (lambda seed, row=row: make(row, seed))) for row in CASES]
    out += [("shipped_" + s[0], (lambda seed, s=s: shipped_case(kind, s[0], seed))) for s in SHIPPED]
    return out
