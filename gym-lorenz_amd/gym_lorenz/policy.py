"""Policy in the loop: SB3 on-policy rollout collection fused on the GPU.

The reference trains its envs with stable-baselines3 A2C / PPO ``"MlpPolicy"``
actor-critics, ``net_arch=dict(pi=[128, 128], vf=[128, 128])`` with Tanh
(code/lorenz_pmsm/train.py:155-178: A2C, n_steps=16, VecNormalize(norm_obs=True,
norm_reward=False, clip_obs=10); code/lorenz_filter/train.py:117-127 and
code/gym_try.py:106-116: PPO, n_steps=2048, gae_lambda=0.95; code/gym_run.py:79).
SB3 then runs ``OnPolicyAlgorithm.collect_rollouts``: per step one policy forward on
the host, one ``DummyVecEnv.step`` over the envs one at a time, a RolloutBuffer add,
and finally ``RolloutBuffer.compute_returns_and_advantage``.

``FusedRolloutCollector.collect(K)`` does all K steps in ONE kernel launch
(``lz_rollout_policy_f32``): the two 6->128->128 MLPs at SB3's own precision
(float32 operands and accumulation on f32-input MFMA, a deterministic operation order
the C oracle reproduces bit for bit -- likewise code/train.py's and code/lorenz_filter/
train.py's attention actor-critics, ``lz_rollout_policy_attn_f32`` / ``_attn_stack_f32``;
``precision="bf16"`` selects the faster bf16-MFMA kernels), the Gaussian
sample (Philox), the action-space clip, the env step with
auto-reset, SB3's truncation bootstrap, and VecNormalize's observation normalisation.
With a training VecNormalize the float32 kernel follows SB3's order exactly: each
step's batch updates obs_rms before that step's observations are normalised
(``lz_rollout_policy_f32_vn``: one launch per step, the statistics update between
launches); ``vecnorm_update="rollout"`` (and the bf16 / attention kernels) keep the
statistics frozen for the K steps and update them once from the pooled moments.
``compute_returns_and_advantage`` is ``lz_gae``.  The buffers come back as
time-major device tensors in SB3's RolloutBuffer layout ([K, N, ...]).

``FusedEvaluator.evaluate(K)`` is what the reference does with a trained policy
afterwards (its ``test_evaluate.py`` scripts, SB3 ``evaluate_policy``): the same closed
loop without the value net, the bootstrap and the [K, N, *] buffers, the MAE / RMSE /
episode-return statistics kept as per-env float64 running sums on the device
(``lz_evaluate_policy_f32`` / ``_attn_f32`` / ``_attn_stack_f32``).  With ``trace=ids`` the
same launch also records those envs' per-step trajectories (``EvalTrace``: the scripts'
error / control curves and state records).

``FusedA2C.update(batch)`` is the learner's gradient step on such a batch (SB3
``A2C.train()``: ``lz_a2c_grad_f32`` + ``lz_a2c_apply_f32``) and ``FusedA2C.learn`` the loop
collect -> returns -> update of code/lorenz_pmsm/train.py:151-185, for the float32 MlpPolicy.

``ActorCriticMlp`` is a plain-torch restatement of SB3's ActorCriticPolicy for this
net_arch (same state_dict keys, same orthogonal init) -- the weight source when SB3 is
absent and the fp32 reference in the tests.  An SB3 policy's ``state_dict()`` can be
passed to ``set_params`` directly.
"""
import contextlib
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import _native as nat
from .core import check_buffer
from .registry import LEGACY_SPECS, SPECS

HIDDEN = nat.POLICY_HIDDEN

KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
        "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
        "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
        "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
        "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std")
_FIELDS = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w1", "vf_b1", "vf_w2", "vf_b2",
           "act_w", "act_b", "val_w", "val_b", "log_std")


def action_bounds(system_name):
    for spec in list(SPECS.values()) + list(LEGACY_SPECS.values()):
        if spec.system_name == system_name:
            return float(spec.act[0]), float(spec.act[1])
    raise KeyError(system_name)


class _MlpExtractor(nn.Module):
    def __init__(self, obs_dim, hidden=HIDDEN):
        super().__init__()
        self.policy_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                        nn.Linear(hidden, hidden), nn.Tanh())
        self.value_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                       nn.Linear(hidden, hidden), nn.Tanh())


class ActorCriticMlp(nn.Module):
    """SB3 ActorCriticPolicy (MlpPolicy, net_arch pi=[128,128] vf=[128,128], Tanh,
    DiagGaussian, log_std_init=0, ortho_init=True) in plain torch, fp32."""

    def __init__(self, obs_dim, act_dim, hidden=HIDDEN, log_std_init=0.0, seed=None):
        super().__init__()
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        self.mlp_extractor = _MlpExtractor(obs_dim, hidden)
        self.action_net = nn.Linear(hidden, act_dim)
        self.value_net = nn.Linear(hidden, 1)
        self.log_std = nn.Parameter(torch.ones(act_dim) * log_std_init)
        # SB3 ActorCriticPolicy._build: orthogonal init, gains sqrt(2) / 0.01 / 1, zero bias
        with torch.no_grad():
            for mod, gain in ((self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01),
                              (self.value_net, 1.0)):
                for m in mod.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain, generator=g)
                        m.bias.zero_()

    def forward(self, obs):
        """(mean actions, values) in fp32."""
        mean = self.action_net(self.mlp_extractor.policy_net(obs))
        value = self.value_net(self.mlp_extractor.value_net(obs)).flatten()
        return mean, value


class AttentionFeaturesExtractor(nn.Module):
    """code/train.py:52-95 restated in plain torch (same submodule names, so the same
    state_dict keys under ``features_extractor.``): fc1 obs->128 + ReLU, the 128 units
    as 8 tokens of 16, nn.MultiheadAttention(16, 4 heads, batch_first) self-attention,
    flatten, post_attention_fc 128->features_dim + ReLU."""

    def __init__(self, obs_dim, features_dim=64):
        super().__init__()
        self.hidden_dim, self.seq_len, self.token_dim = 128, 8, 16
        self.features_dim = features_dim
        self.fc1 = nn.Linear(obs_dim, self.hidden_dim)
        self.attention_layer = nn.MultiheadAttention(embed_dim=self.token_dim, num_heads=4,
                                                     batch_first=True)
        self.post_attention_fc = nn.Sequential(nn.Linear(self.hidden_dim, features_dim), nn.ReLU())

    def forward(self, observations):
        x = torch.relu(self.fc1(observations))
        x_seq = x.view(-1, self.seq_len, self.token_dim)
        attn_output, _ = self.attention_layer(x_seq, x_seq, x_seq)
        return self.post_attention_fc(attn_output.reshape(-1, self.hidden_dim))


class AttentionFeaturesExtractorLN(AttentionFeaturesExtractor):
    """code/lorenz_filter/train.py:54-103: the same extractor with a residual connection
    and LayerNorm(16) per token after the attention (x_seq = layer_norm(x_seq +
    attn_output)) before post_attention_fc; used there on VecFrameStack(n_stack=4)."""

    def __init__(self, obs_dim, features_dim=64):
        super().__init__(obs_dim, features_dim)
        self.layer_norm = nn.LayerNorm(self.token_dim)

    def forward(self, observations):
        x = torch.relu(self.fc1(observations))
        x_seq = x.view(-1, self.seq_len, self.token_dim)
        attn_output, _ = self.attention_layer(x_seq, x_seq, x_seq)
        x_seq = self.layer_norm(x_seq + attn_output)
        return self.post_attention_fc(x_seq.reshape(-1, self.hidden_dim))


class ActorCriticAttn(nn.Module):
    """SB3 ActorCriticPolicy as code/train.py:101-112 builds it: the shared
    AttentionFeaturesExtractor (features_dim=64), net_arch pi=[128,128] vf=[128,128]
    Tanh, DiagGaussian (log_std_init=0), SB3's orthogonal init (gain sqrt(2) for the
    extractor and the nets, 0.01 / 1 for the heads, zero biases; init_weights touches
    nn.Linear modules only, so in_proj keeps torch's xavier init)."""

    def __init__(self, obs_dim, act_dim, features_dim=64, hidden=HIDDEN, log_std_init=0.0,
                 seed=None, layer_norm=False):
        super().__init__()
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        if seed is not None:
            torch.manual_seed(seed)  # nn.MultiheadAttention's own xavier init
        ext = AttentionFeaturesExtractorLN if layer_norm else AttentionFeaturesExtractor
        self.features_extractor = ext(obs_dim, features_dim)
        self.mlp_extractor = _MlpExtractor(features_dim, hidden)
        self.action_net = nn.Linear(hidden, act_dim)
        self.value_net = nn.Linear(hidden, 1)
        self.log_std = nn.Parameter(torch.ones(act_dim) * log_std_init)
        with torch.no_grad():
            for mod, gain in ((self.features_extractor, math.sqrt(2)),
                              (self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01),
                              (self.value_net, 1.0)):
                for m in mod.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain, generator=g)
                        m.bias.zero_()

    def forward(self, obs):
        f = self.features_extractor(obs)
        mean = self.action_net(self.mlp_extractor.policy_net(f))
        value = self.value_net(self.mlp_extractor.value_net(f)).flatten()
        return mean, value


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


# 2 / ln 2 in float32: lz_policy_pack stores the two tanh layers as bf16(s * W) and
# s * b so that the kernel's tanh needs no multiply (lz_policy.hip tanh_scaled)
TANH_SCALE = np.float32(2.8853900817779268)


def reference_forward_bf16(state_dict, obs):
    """The fused kernel's arithmetic restated in torch: bf16 operands (the tanh layers'
    weights as bf16(s W) with s = 2/ln 2 folded in, the head's as bf16(W), and each
    layer's input activations rounded to bf16, round-to-nearest-even), fp32 bias and
    accumulation, tanh(acc / s).  Differs from the kernel only in fp32 summation order
    and the tanh implementation (|err| <= 2e-7).  Returns (mean, value)."""
    return _bf16_tanh_nets(state_dict, _bf(torch.as_tensor(obs, dtype=torch.float32)))


def _t(sd, k):
    return torch.as_tensor(np.asarray(_np(sd[k])), dtype=torch.float32)


def _bf16_tanh_nets(sd, feat):
    """The restated forwards' tail: the two [128, 128] Tanh nets and their heads on the
    bf16-valued features (the MlpPolicy: observations) -> (mean, value)."""
    s = torch.tensor(TANH_SCALE)

    def net(prefix, w3, b3):
        h = feat
        for layer in (".0", ".2"):
            acc = h @ _bf(s * _t(sd, prefix + layer + ".weight")).T + s * _t(sd, prefix + layer + ".bias")
            h = _bf(torch.tanh(acc / s))
        return h @ _bf(_t(sd, w3)).T + _t(sd, b3)

    mean = net("mlp_extractor.policy_net", "action_net.weight", "action_net.bias")
    value = net("mlp_extractor.value_net", "value_net.weight", "value_net.bias").flatten()
    return mean, value


# log2(e) / sqrt(head dim 4): lz_attn_policy_pack stores the Q projection pre-scaled by
# it (bf16(c W_q), c b_q) so the kernel's softmax is exp2(q.k - max)
ATTN_Q_SCALE = 1.4426950408889634 / 2.0
FE = "features_extractor."
ATTN_FE_KEYS = ("fc1.weight", "fc1.bias", "attention_layer.in_proj_weight",
                "attention_layer.in_proj_bias", "attention_layer.out_proj.weight",
                "attention_layer.out_proj.bias", "post_attention_fc.0.weight",
                "post_attention_fc.0.bias")
_ATTN_FE_FIELDS = ("fc1_w", "fc1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b",
                   "post_w", "post_b")


def is_attention_policy(state_dict):
    """True for a state_dict of code/train.py's AttentionFeaturesExtractor policy."""
    return any(k.endswith("features_extractor.fc1.weight") for k in state_dict)


def is_attention_ln_policy(state_dict):
    """True for code/lorenz_filter/train.py's residual + LayerNorm extractor."""
    return any(k.endswith("features_extractor.layer_norm.weight") for k in state_dict)


def _fe_key(state_dict, name):
    # SB3 (share_features_extractor=True) stores the shared extractor under
    # features_extractor. and aliases it as pi_features_extractor. / vf_features_extractor.
    for pre in (FE, "pi_" + FE):
        if pre + name in state_dict:
            return pre + name
    raise KeyError("policy state_dict lacks %r (expected code/train.py's "
                   "AttentionFeaturesExtractor)" % (FE + name))


def attn_folded_post(sd):
    """out_proj folded into post_attention_fc, float64 (as lz_attn_policy_pack):
    Wf [8 tokens, 64, 16] and the folded bias [64]."""
    g = {k: torch.as_tensor(np.asarray(_np(sd[_fe_key(sd, k)])), dtype=torch.float64)
         for k in ATTN_FE_KEYS[4:]}
    wo, bo = g["attention_layer.out_proj.weight"], g["attention_layer.out_proj.bias"]
    wp, bp = g["post_attention_fc.0.weight"], g["post_attention_fc.0.bias"]
    blocks = wp.view(wp.shape[0], 8, 16).permute(1, 0, 2)  # [8, 64, 16]
    wf = blocks @ wo
    bf = bp + (blocks @ bo).sum(0)
    return wf, bf


def _bf16_attn_stem(sd, obs):
    """The bf16 attention forwards up to the head outputs: bf16 obs / weights / tokens
    (RNE), fp32 accumulation and attention, the Q projection pre-scaled by ATTN_Q_SCALE
    and a base-2 softmax.  Returns the bf16-valued tokens and head outputs, [n, 8, 16]."""
    f32 = torch.float32
    x = _bf(torch.as_tensor(obs, dtype=f32))
    n = x.shape[0]
    tok = _bf(torch.relu(x @ _bf(_t(sd, _fe_key(sd, "fc1.weight"))).T + _t(sd, _fe_key(sd, "fc1.bias"))))
    tok = tok.view(n, 8, 16)
    w_in, b_in = _t(sd, _fe_key(sd, ATTN_FE_KEYS[2])), _t(sd, _fe_key(sd, ATTN_FE_KEYS[3]))
    c = torch.tensor(np.float64(ATTN_Q_SCALE))
    wq = _bf((c.double() * w_in[:16].double()).to(f32))
    bq = (c.double() * b_in[:16].double()).to(f32)
    q = tok @ wq.T + bq
    k = tok @ _bf(w_in[16:32]).T + b_in[16:32]
    v = tok @ _bf(w_in[32:48]).T + b_in[32:48]
    q, k, v = (z.view(n, 8, 4, 4).transpose(1, 2) for z in (q, k, v))  # [n, head, token, 4]
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = (p @ v) * (1.0 / p.sum(-1, keepdim=True))  # normalised after the weighted sum
    return tok, _bf(o.transpose(1, 2).reshape(n, 8, 16))


def reference_forward_attn_bf16(state_dict, obs):
    """lz_rollout_policy_attn's arithmetic restated in torch: bf16 obs / weights /
    tokens / head outputs / features (RNE), fp32 accumulation and attention, the Q
    projection pre-scaled by ATTN_Q_SCALE and a base-2 softmax, out_proj folded into
    post_attention_fc in float64, the Tanh nets as reference_forward_bf16.  Differs
    from the kernel in fp32 summation order and the exp2 / rcp / tanh implementations.
    Returns (mean, value)."""
    _, a = _bf16_attn_stem(state_dict, obs)
    wf, bfold = attn_folded_post(state_dict)
    feat = bfold.to(torch.float32) + torch.einsum("nid,ifd->nf", a, _bf(wf.to(torch.float32)))
    return _bf16_tanh_nets(state_dict, _bf(torch.relu(feat)))


def reference_forward_attn_ln_bf16(state_dict, obs):
    """lz_rollout_policy_attn_stack's arithmetic restated in torch (code/lorenz_filter/
    train.py's extractor): as reference_forward_attn_bf16 up to the head outputs, then
    out_proj (bf16 operands, fp32 accumulate), the residual with the bf16 token values,
    LayerNorm(16) in fp32 (biased variance, eps 1e-5), bf16, post_attention_fc (bf16
    operands) + ReLU, the Tanh nets.  obs: the (stacked) policy input.  Returns
    (mean, value)."""
    sd = state_dict

    def t(name):
        return _t(sd, _fe_key(sd, name))

    tok, a = _bf16_attn_stem(sd, obs)
    y = a @ _bf(t(ATTN_FE_KEYS[4])).T + t(ATTN_FE_KEYS[5])
    z = y + tok
    mu = z.mean(-1, keepdim=True)
    z = z - mu
    var = (z * z).mean(-1, keepdim=True)
    u = _bf(z * torch.rsqrt(var + 1e-5) * t("layer_norm.weight") + t("layer_norm.bias"))
    feat = _bf(torch.relu(u.reshape(-1, 128) @ _bf(t(ATTN_FE_KEYS[6])).T + t(ATTN_FE_KEYS[7])))
    return _bf16_tanh_nets(sd, feat)


def _np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().to("cpu", torch.float32).numpy()
    return np.asarray(v, np.float32)


def _mlp_policy_struct(state_dict, obs_dim, act_dim):
    arrs = []
    for key in KEYS:
        if key not in state_dict:
            raise KeyError("policy state_dict lacks %r (expected SB3 MlpPolicy with "
                           "net_arch pi=[H,H] vf=[H,H], H <= 128)" % key)
        arrs.append(np.ascontiguousarray(_np(state_dict[key]), dtype=np.float32))
    H = arrs[0].shape[0]
    shapes = [(H, obs_dim), (H,), (H, H), (H,)] * 2 + [
        (act_dim, H), (act_dim,), (1, H), (1,), (act_dim,)]
    for key, a, shp in zip(KEYS, arrs, shapes):
        if a.shape != shp:
            raise ValueError("%s has shape %s, expected %s" % (key, a.shape, shp))
    p = nat.LzMlpPolicy()
    p.obs_dim, p.act_dim = int(obs_dim), int(act_dim)
    for f, a in zip(_FIELDS, arrs):
        setattr(p, f, a.ctypes.data)
    return p, H, arrs  # arrs keep the weights alive while p points at them


def _attn_struct(state_dict, in_dim, act_dim, features_dim, ln):
    if features_dim != 64:
        raise ValueError("the fused kernel implements features_dim=64 (code/train.py:100)")
    keys = [_fe_key(state_dict, k) for k in ATTN_FE_KEYS] + list(KEYS)
    if ln:
        keys += [_fe_key(state_dict, "layer_norm.weight"), _fe_key(state_dict, "layer_norm.bias")]
    for key in KEYS:
        if key not in state_dict:
            raise KeyError("policy state_dict lacks %r" % key)
    arrs = [np.ascontiguousarray(_np(state_dict[k]), dtype=np.float32) for k in keys]
    F = features_dim
    shapes = [(HIDDEN, in_dim), (HIDDEN,), (48, 16), (48,), (16, 16), (16,), (F, HIDDEN), (F,)] + [
        (HIDDEN, F), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,)] * 2 + [
        (act_dim, HIDDEN), (act_dim,), (1, HIDDEN), (1,), (act_dim,)] + ([(16,), (16,)] if ln else [])
    for key, a, shp in zip(keys, arrs, shapes):
        if a.shape != shp:
            raise ValueError("%s has shape %s, expected %s" % (key, a.shape, shp))
    p = nat.LzAttnPolicy()
    p.obs_dim, p.act_dim = int(in_dim), int(act_dim)
    for f, a in zip(_ATTN_FE_FIELDS + _FIELDS, arrs):
        setattr(p, f, a.ctypes.data)
    if not ln:
        return p, arrs
    q = nat.LzAttnLnPolicy()
    q.attn = p
    q.ln_w, q.ln_b = arrs[-2].ctypes.data, arrs[-1].ctypes.data
    return q, arrs


# The packers, one row per (family, precision): the C pack function, the function that
# gives its blob's size, and the LZ_BLOB_* tag the blob carries (None: the bf16 blobs carry
# none).  A new policy family or precision is added here and in _LAUNCH.
_PACKERS = {
    ("mlp", "bf16"): ("lz_policy_pack_hidden", "lz_policy_blob_bytes", None),
    ("mlp", "fp32"): ("lz_policy_pack_f32", "lz_policy_f32_blob_bytes", nat.BLOB_MLP_F32),
    ("mlp", "i8x4"): ("lz_policy_pack_i8x4", "lz_policy_f32_blob_bytes", nat.BLOB_MLP_I8X4),
    ("attn", "bf16"): ("lz_attn_policy_pack", "lz_attn_policy_blob_bytes", None),
    ("attn", "fp32"): ("lz_attn_policy_pack_f32", "lz_attn_policy_f32_blob_bytes", nat.BLOB_ATTN_F32),
    ("attn", "i8x4"): ("lz_attn_policy_pack_i8x4", "lz_attn_policy_f32_blob_bytes", nat.BLOB_ATTN_I8X4),
    ("attn_ln", "bf16"): ("lz_attn_ln_policy_pack", "lz_attn_ln_policy_blob_bytes", None),
    ("attn_ln", "fp32"): ("lz_attn_ln_policy_pack_f32", "lz_attn_policy_f32_blob_bytes",
                          nat.BLOB_ATTN_LN_F32),
    ("attn_ln", "i8x4"): ("lz_attn_ln_policy_pack_i8x4", "lz_attn_policy_f32_blob_bytes",
                          nat.BLOB_ATTN_LN_I8X4),
}

# The frame-stacked MlpPolicy (code/lorenz_filter/train.py:109-131: PPO("MlpPolicy") on
# VecFrameStack(n_stack=4), SB3's default 64 x 64 nets), family "mlp_stack": its rows of the
# two tables, kept beside them -- float32 only, no traced evaluation.
STACK_HIDDEN = 64
_STACK_PACKERS = {
    ("mlp_stack", "fp32"): ("lz_policy_pack_stack_f32", "lz_policy_stack_f32_blob_bytes",
                            nat.BLOB_MLP_STACK_F32),
}


def _packer_row(family, precision):
    key = (family, precision)
    return _STACK_PACKERS[key] if key in _STACK_PACKERS else _PACKERS[key]


def _pack(family, precision, state_dict, in_dim, act_dim, features_dim=64):
    """SB3 state_dict -> the uint8 numpy blob of _PACKERS[family, precision] (host; needs
    no GPU).  in_dim: the policy's input width (the stacked one for "attn_ln" and
    "mlp_stack")."""
    pack, blob_bytes, _tag = _packer_row(family, precision)
    if family in ("mlp", "mlp_stack"):
        p, H, _keep = _mlp_policy_struct(state_dict, in_dim, act_dim)
        args = (ctypes.byref(p), H)
    else:
        p, _keep = _attn_struct(state_dict, in_dim, act_dim, features_dim, family == "attn_ln")
        args = (ctypes.byref(p),)
    blob = np.zeros(int(getattr(nat.lib, blob_bytes)()), np.uint8)
    nat.check(getattr(nat.lib, pack)(*args, blob.ctypes.data, blob.size))
    return blob


def pack_policy(state_dict, obs_dim, act_dim):
    """lz_policy_pack / lz_policy_pack_hidden: SB3 state_dict (net_arch pi=[H,H]
    vf=[H,H], H <= 128) -> uint8 numpy blob of the bf16 kernel (host; needs no GPU)."""
    return _pack("mlp", "bf16", state_dict, obs_dim, act_dim)


def pack_policy_f32(state_dict, obs_dim, act_dim):
    """lz_policy_pack_f32: SB3 state_dict (net_arch pi=[H,H] vf=[H,H], H <= 128) ->
    uint8 numpy blob of the float32 kernel (host; needs no GPU)."""
    return _pack("mlp", "fp32", state_dict, obs_dim, act_dim)


def pack_policy_stack_f32(state_dict, in_dim, act_dim):
    """lz_policy_pack_stack_f32: code/lorenz_filter/train.py:109-131's policy -- the 64-unit
    MlpPolicy on VecFrameStack observations (in_dim = the stacked observation width, up to
    24) -> uint8 numpy blob of the native 64-unit float32 kernel (host; needs no GPU)."""
    return _pack("mlp_stack", "fp32", state_dict, in_dim, act_dim)


def pack_policy_i8x4(state_dict, obs_dim, act_dim):
    """lz_policy_pack_i8x4: the float32 MlpPolicy blob with each net's layer 2 as exact
    4-digit int8 fixed-point products (precision="i8x4"; oracle orc_mlp_i8x4)."""
    return _pack("mlp", "i8x4", state_dict, obs_dim, act_dim)


def pack_attn_policy_f32(state_dict, obs_dim, act_dim, features_dim=64):
    """lz_attn_policy_pack_f32: code/train.py's attention actor-critic at SB3's float32
    precision (lz_rollout_policy_attn_f32) -> uint8 numpy blob (host; needs no GPU)."""
    return _pack("attn", "fp32", state_dict, obs_dim, act_dim, features_dim)


def pack_attn_ln_policy_f32(state_dict, in_dim, act_dim, features_dim=64):
    """lz_attn_ln_policy_pack_f32: code/lorenz_filter/train.py's residual + LayerNorm
    policy at float32 precision (in_dim = the stacked observation width)."""
    return _pack("attn_ln", "fp32", state_dict, in_dim, act_dim, features_dim)


def pack_attn_policy_i8x4(state_dict, obs_dim, act_dim, features_dim=64):
    """lz_attn_policy_pack_i8x4: code/train.py's attention actor-critic with the nets' two
    wide layers as exact 4-digit int8 fixed-point products (precision="i8x4"; the float32
    blob's size and layout otherwise) -> uint8 numpy blob (host; needs no GPU)."""
    return _pack("attn", "i8x4", state_dict, obs_dim, act_dim, features_dim)


def pack_attn_ln_policy_i8x4(state_dict, in_dim, act_dim, features_dim=64):
    """lz_attn_ln_policy_pack_i8x4: code/lorenz_filter/train.py's residual + LayerNorm
    policy, precision="i8x4" (in_dim = the stacked observation width)."""
    return _pack("attn_ln", "i8x4", state_dict, in_dim, act_dim, features_dim)


def pack_attn_policy(state_dict, obs_dim, act_dim, features_dim=64):
    """lz_attn_policy_pack: SB3 state_dict of code/train.py's attention actor-critic ->
    uint8 numpy blob (host; needs no GPU)."""
    return _pack("attn", "bf16", state_dict, obs_dim, act_dim, features_dim)


def pack_attn_ln_policy(state_dict, in_dim, act_dim, features_dim=64):
    """lz_attn_ln_policy_pack: code/lorenz_filter/train.py's policy (in_dim = the
    stacked observation width) -> uint8 numpy blob (host; needs no GPU)."""
    return _pack("attn_ln", "bf16", state_dict, in_dim, act_dim, features_dim)


@dataclass
class RolloutBatch:
    """SB3 RolloutBuffer contents, time-major device tensors."""
    observations: torch.Tensor   # [K, N, O] what the policy saw (normalised)
    actions: torch.Tensor        # [K, N, A] unclipped samples
    log_probs: torch.Tensor      # [K, N]
    values: torch.Tensor         # [K, N]
    rewards: torch.Tensor        # [K, N] (+ gamma * V(terminal obs) on truncation)
    dones: torch.Tensor          # [K, N] uint8 LZ_DONE_* bits of each step
    episode_starts: torch.Tensor  # [K, N] float32 (SB3 _last_episode_starts per step)
    last_values: torch.Tensor    # [N] V(normalised last obs)
    last_obs: torch.Tensor       # [N, O] raw
    obs_moments: torch.Tensor = None  # [1 + 2 O] float64 or None
    done_idx: torch.Tensor = None     # compact list k*N + env
    terminal_obs: torch.Tensor = None
    n_done: torch.Tensor = None
    last_stack: torch.Tensor = None   # [N, n_stack * O] VecFrameStack obs after the rollout
    advantages: torch.Tensor = None
    returns: torch.Tensor = None


def _p(t):
    return None if t is None else t.data_ptr()


def blob_format(attention, attention_ln, i8x4, mlp_stack=False):
    """The LZ_BLOB_* format a float32 / i8x4 launch reads (entry point + LZ_POLICY_I8X4)."""
    family = "attn_ln" if attention_ln else "attn" if attention else "mlp_stack" if mlp_stack else "mlp"
    return _packer_row(family, "i8x4" if i8x4 else "fp32")[2]


# The entry points, one row per (kind, family, precision), laid out like kPolicyTable in
# lz_api.cpp; precision "i8x4" runs the "fp32" row with LZ_POLICY_I8X4.  The "attn_ln" rows
# take (n_stack, stack_in, stack_out) after the arguments, the "trace" rows an lz_eval_trace
# last.  "step" is the per-step VecNormalize collect's launch (lz_rollout_policy_f32_vn is
# the library's own loop over it).
_LAUNCH = {
    ("rollout", "mlp", "bf16"): "lz_rollout_policy",
    ("rollout", "attn", "bf16"): "lz_rollout_policy_attn",
    ("rollout", "attn_ln", "bf16"): "lz_rollout_policy_attn_stack",
    ("rollout", "mlp", "fp32"): "lz_rollout_policy_f32",
    ("rollout", "attn", "fp32"): "lz_rollout_policy_attn_f32",
    ("rollout", "attn_ln", "fp32"): "lz_rollout_policy_attn_stack_f32",
    ("step", "mlp", "fp32"): "lz_policy_step_f32",
    ("evaluate", "mlp", "fp32"): "lz_evaluate_policy_f32",
    ("evaluate", "attn", "fp32"): "lz_evaluate_policy_attn_f32",
    ("evaluate", "attn_ln", "fp32"): "lz_evaluate_policy_attn_stack_f32",
    ("trace", "mlp", "fp32"): "lz_evaluate_policy_f32_trace",
    ("trace", "attn", "fp32"): "lz_evaluate_policy_attn_f32_trace",
    ("trace", "attn_ln", "fp32"): "lz_evaluate_policy_attn_stack_f32_trace",
}
# ... and family "mlp_stack"'s (see _STACK_PACKERS): (n_stack, stack_in, stack_out) as "attn_ln"
_STACK_LAUNCH = {
    ("rollout", "mlp_stack", "fp32"): "lz_stack_rollout_policy_f32",
    ("evaluate", "mlp_stack", "fp32"): "lz_stack_evaluate_policy_f32",
}


class _PolicySeam:
    """What FusedRolloutCollector and FusedEvaluator share between a state_dict and a
    launch: the policy family and the frame-stack rules, the packed and tag-checked blob,
    the carried observations / frame stack, and the call into _LAUNCH's entry point on the
    env handle's stream.  A subclass sets env, device, n, O, A, obs_rms and _what."""

    _what = "rollout"          # the noun of the refusals
    attention = attention_ln = mlp_stack = False
    f32, i8x4 = True, False    # the evaluator's stance; the collector sets its own
    blob = last_obs = last_stack = None

    @property
    def family(self):
        return ("attn_ln" if self.attention_ln else "attn" if self.attention
                else "mlp_stack" if self.mlp_stack else "mlp")

    def _init_frame_stack(self, frame_stack):
        # SB3 VecFrameStack(n_stack) between the env and the policy
        # (code/lorenz_filter/train.py:115): the stack is carried on the device
        self.frame_stack = int(frame_stack)
        if self.frame_stack not in (1, 4):
            raise ValueError("frame_stack must be 1 or 4 (the fused kernel's instantiations)")
        if self.frame_stack > 1 and self.obs_rms is not None:
            raise ValueError("the frame-stacked %s stacks raw observations (no VecNormalize)" % self._what)

    def _select(self, state_dict):
        """The family of the state_dict's keys (as FusedRolloutCollector.set_params says)."""
        self.attention = is_attention_policy(state_dict)
        self.attention_ln = is_attention_ln_policy(state_dict)
        # ... or, frame-stacked, the 64-unit MlpPolicy that script trains in fact
        # (code/lorenz_filter/train.py:109-131: its policy_kwargs are never passed on)
        w1 = state_dict.get(KEYS[0]) if not self.attention else None
        self.mlp_stack = (self.frame_stack > 1 and w1 is not None
                          and tuple(w1.shape) == (STACK_HIDDEN, self.frame_stack * self.O))
        if self.frame_stack > 1 and not (self.attention_ln or self.mlp_stack):
            raise ValueError("frame_stack > 1 runs code/lorenz_filter/train.py's policy "
                             "(the residual + LayerNorm attention extractor)")

    def _pack_params(self, state_dict, precision):
        if self.attention_ln and self.obs_rms is not None:
            raise ValueError("the LayerNorm attention %s takes raw observations" % self._what)
        in_dim = self.frame_stack * self.O if (self.attention_ln or self.mlp_stack) else self.O
        return _pack(self.family, precision, state_dict, in_dim, self.A)

    def _set_blob(self, blob):
        """Upload a packed blob; a float32 / i8x4 one only if its format tag is the one the
        launch this object makes will expect."""
        if self.f32:
            want = blob_format(self.attention, self.attention_ln, self.i8x4, self.mlp_stack)
            got = int(nat.lib.lz_policy_blob_format(blob.ctypes.data, blob.size))
            if got != want:
                raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "policy blob format %d, the launch "
                                         "expects %d" % (got, want))
        self.blob = torch.from_numpy(blob).to(self.device)

    def _start_from(self, obs):
        """The next launch starts from obs and a fresh frame stack (StackedObservations.reset:
        zeros, the first frame last)."""
        self.last_obs = obs.clone()
        self.last_stack = torch.zeros((self.n, self.frame_stack * self.O), dtype=torch.float32,
                                      device=self.device)
        self.last_stack[:, -self.O:] = obs
        return self.last_obs

    @contextlib.contextmanager
    def _on_env_stream(self):
        """The launches run on the env handle's stream: the caller's current stream (where
        the buffers were allocated and blob / last_obs written, and where the results are
        read) is ordered around them both ways.  Yields the caller's stream."""
        caller = torch.cuda.current_stream(self.device)
        es = self.env.stream
        if es != caller:
            es.wait_stream(caller)
        yield caller
        if es != caller:
            caller.wait_stream(es)

    def _launch(self, kind, args, trace=None):
        """Call _LAUNCH's entry point for this policy; returns the frame stack it wrote
        (None unless the family carries one)."""
        key = (kind, self.family, "fp32" if self.f32 else "bf16")
        fn = getattr(nat.lib, _STACK_LAUNCH[key] if key in _STACK_LAUNCH else _LAUNCH[key])
        stack_out, extra = None, ()
        if self.attention_ln or self.mlp_stack:
            stack_out = torch.empty((self.n, self.frame_stack * self.O), dtype=torch.float32,
                                    device=self.device)
            extra = (self.frame_stack, _p(self.last_stack), _p(stack_out))
        if trace is not None:
            extra += (ctypes.byref(trace),)
        nat.check(fn(self.env._h, ctypes.byref(args), *extra))
        return stack_out

    def _hand_over(self, obs_last, stack_out):
        self._keep = (self.blob, self.last_obs, self.last_stack)  # alive until consumed
        self.last_obs = obs_last
        if stack_out is not None:
            self.last_stack = stack_out


class FusedRolloutCollector(_PolicySeam):
    """OnPolicyAlgorithm.collect_rollouts over a BatchedEnv, one launch per rollout.

    backend:       gym_lorenz.core.BatchedEnv (float32, autoreset)
    state_dict:    SB3 ActorCriticPolicy / ActorCriticMlp state_dict
    obs_rms:       gym_lorenz.vec_normalize.DeviceRunningMeanStd or None
    training:      update obs_rms (VecNormalize.training)
    vecnorm_update: how a training obs_rms is updated.  "step" (the default for the
                   float32 MlpPolicy): SB3's order -- every step's batch updates obs_rms
                   before that step's observations (and the truncated steps' terminal
                   observations) are normalised (lz_rollout_policy_f32_vn: one launch
                   per step + the statistics update between).  "rollout" (opt-in; the
                   only mode of the bf16 / attention kernels): the K steps run in one
                   launch with the rollout-start statistics and one update from the K
                   steps' pooled moments afterwards -- faster, not SB3's trajectory.
    precision:     policy arithmetic: "fp32" (default; SB3's float32 forward --
                   lz_rollout_policy_f32, and for the attention actor-critics of
                   code/train.py / code/lorenz_filter/train.py lz_rollout_policy_attn_f32 /
                   _attn_stack_f32), "i8x4" (the same float32 kernels with the pi / vf
                   nets' wide layers as exact 4-digit int8 fixed-point products on the
                   int8 MFMA -- float32-level accuracy, bit-exact vs orc_attn_i8x4 /
                   orc_mlp_i8x4, not bit-equal to "fp32"; the MlpPolicy one without the
                   per-step VecNormalize collect, and for LORENZ3 / LORENZ4 / PMSM / HR)
                   or "bf16" (bf16 MFMA
                   operands, fp32 accumulation: lz_rollout_policy / _attn / _attn_stack,
                   ~2.5-5x faster, ~1e-2 off SB3).
    """

    def __init__(self, backend, state_dict=None, gamma=0.99, gae_lambda=0.95, obs_rms=None,
                 clip_obs=10.0, norm_eps=1e-8, training=True, bootstrap=True,
                 deterministic=False, capture_terminal=0, group=None, frame_stack=1,
                 precision=None, vecnorm_update=None):
        if backend.tdtype != torch.float32:
            raise ValueError("the fused policy rollout runs float32 env handles")
        self.env = backend
        self.device = backend.device
        self.n, self.O, self.A = backend.num_envs, backend.obs_dim, backend.action_dim
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.obs_rms, self.clip_obs, self.norm_eps = obs_rms, float(clip_obs), float(norm_eps)
        self.training, self.bootstrap, self.deterministic = training, bootstrap, deterministic
        self.capture_terminal = int(capture_terminal)
        self.group = group
        self.act_low, self.act_high = action_bounds(backend.system_name)
        if precision not in (None, "fp32", "bf16", "i8x4"):
            raise ValueError("precision must be 'fp32', 'i8x4' or 'bf16'")
        self.precision = precision
        if vecnorm_update not in (None, "step", "rollout"):
            raise ValueError("vecnorm_update must be 'step' or 'rollout'")
        self.vecnorm_update = vecnorm_update
        self.f32 = False  # until set_params
        self._init_frame_stack(frame_stack)
        self.last_episode_starts = torch.ones((self.n,), dtype=torch.float32, device=self.device)
        if state_dict is not None:
            self.set_params(state_dict)

    def set_params(self, state_dict):
        """Pack and upload the actor-critic weights (call after every optimizer step).
        A state_dict with code/train.py's AttentionFeaturesExtractor selects the
        attention kernel (lz_rollout_policy_attn), any other the MlpPolicy kernel."""
        self._select(state_dict)
        if self.mlp_stack and self.precision not in (None, "fp32"):
            raise ValueError("the frame-stacked MlpPolicy rollout runs precision='fp32' only")
        self.f32 = self.precision != "bf16"
        self.i8x4 = self.precision == "i8x4"
        if self.i8x4 and self.family == "mlp":
            if self.env.system_name not in ("lorenz3", "lorenz4", "pmsm", "hr"):
                raise ValueError("the i8x4 MlpPolicy runs LORENZ3 / LORENZ4 / PMSM / HR")
            if self.obs_rms is not None and self.training and self.vecnorm_update != "rollout":
                raise ValueError("precision='i8x4' with a training VecNormalize needs "
                                 "vecnorm_update='rollout' (the per-step collect is float32)")
        blob = self._pack_params(state_dict, self.precision or "fp32")
        if self.vecnorm_update == "step" and (not self.f32 or self.family != "mlp"):
            raise ValueError("vecnorm_update='step' runs the float32 MlpPolicy kernel")
        self._set_blob(blob)

    @property
    def per_step_vecnorm(self):
        """True when the collect updates obs_rms in SB3's per-step order."""
        return (self.obs_rms is not None and self.training and self.f32 and not self.attention
                and not self.attention_ln and self.vecnorm_update != "rollout")

    def _rms_update_obs(self, x):
        """VecNormalize.reset()'s obs_rms.update(obs) in the per-step kernel's moment order."""
        rms = self.obs_rms
        x = x.reshape(x.shape[0], self.O).contiguous()
        if self.group is None:
            nat.check(nat.lib.lz_rms_update_obs(rms._h, x.data_ptr(), x.shape[0], None))
            return
        mom = torch.empty((1 + 2 * self.O,), dtype=torch.float64, device=self.device)
        nat.check(nat.lib.lz_rms_update_obs(rms._h, x.data_ptr(), x.shape[0], mom.data_ptr()))
        dist.all_reduce(mom, group=self.group)
        nat.check(nat.lib.lz_rms_update(rms._h, ctypes.c_void_p(mom.data_ptr())))

    def reset(self):
        """VecEnv.reset(): fresh episodes; the next rollout starts from their obs."""
        self._start_from(self.env.reset())
        self.last_episode_starts.fill_(1.0)
        if self.obs_rms is not None and self.training:
            if self.per_step_vecnorm:
                self._rms_update_obs(self.last_obs)
            else:
                self.obs_rms.update(self.last_obs, self.group)
        return self.last_obs

    def collect(self, K):
        if self.blob is None:
            raise RuntimeError("set_params() first")
        if self.last_obs is None:
            self.reset()
        n, O, A, dev = self.n, self.O, self.A, self.device
        f32 = torch.float32
        SO = self.frame_stack * O if (self.attention_ln or self.mlp_stack) else O
        obs_buf = torch.empty((K, n, SO), dtype=f32, device=dev)
        act_buf = torch.empty((K, n, A), dtype=f32, device=dev)
        logp = torch.empty((K, n), dtype=f32, device=dev)
        val = torch.empty((K, n), dtype=f32, device=dev)
        rew = torch.empty((K, n), dtype=f32, device=dev)
        done = torch.empty((K, n), dtype=torch.uint8, device=dev)
        last_val = torch.empty((n,), dtype=f32, device=dev)
        obs_last = torch.empty((n, O), dtype=f32, device=dev)
        per_step = self.per_step_vecnorm
        want_mom = self.obs_rms is not None and self.training and not per_step
        mom = torch.empty((1 + 2 * O,), dtype=torch.float64, device=dev) if want_mom else None
        didx = tobs = ndone = None
        if self.capture_terminal:
            didx = torch.empty((self.capture_terminal,), dtype=torch.int64, device=dev)
            tobs = torch.empty((self.capture_terminal, O), dtype=f32, device=dev)
            ndone = torch.zeros((1,), dtype=torch.int32, device=dev)
        r = nat.LzPolicyRolloutArgs()
        r.K = int(K)
        r.flags = ((nat.POLICY_DETERMINISTIC if self.deterministic else 0)
                   | (nat.POLICY_BOOTSTRAP if self.bootstrap else 0)
                   | (nat.POLICY_I8X4 if self.i8x4 else 0))
        r.blob, r.obs_in, r.obs_last = _p(self.blob), _p(self.last_obs), _p(obs_last)
        r.obs_norm = _p(self.obs_rms.state) if self.obs_rms is not None and not per_step else None
        r.norm_eps, r.clip_obs, r.gamma = self.norm_eps, self.clip_obs, self.gamma
        r.act_low, r.act_high = self.act_low, self.act_high
        r.obs_buf, r.act_buf, r.logp_buf, r.val_buf = _p(obs_buf), _p(act_buf), _p(logp), _p(val)
        r.rew_buf, r.done_buf, r.last_values = _p(rew), _p(done), _p(last_val)
        r.obs_moments = _p(mom)
        r.done_idx, r.terminal_obs, r.cap, r.n_done = _p(didx), _p(tobs), self.capture_terminal, _p(ndone)
        stack_out = None
        with self._on_env_stream() as caller:
            state = ctypes.c_void_p(self.obs_rms.state.data_ptr()) if per_step else None
            if not per_step:
                stack_out = self._launch("rollout", r)
            elif self.group is None:
                nat.check(nat.lib.lz_rollout_policy_f32_vn(self.env._h, ctypes.byref(r), state))
            else:  # every step's batch moments all-reduced before its update
                step = getattr(nat.lib, _LAUNCH["step", "mlp", "fp32"])
                es = self.env.stream
                mom = torch.empty((1 + 2 * O,), dtype=torch.float64, device=dev)
                rh = self.obs_rms._h
                nat.check(nat.lib.lz_rms_set_stream(rh, ctypes.c_void_p(caller.cuda_stream)))
                for k in range(K + 1):
                    nat.check(step(self.env._h, ctypes.byref(r), k, state,
                                   ctypes.c_void_p(mom.data_ptr()) if k < K else None))
                    if k < K:
                        if es != caller:
                            caller.wait_stream(es)
                        dist.all_reduce(mom, group=self.group)
                        nat.check(nat.lib.lz_rms_update(rh, ctypes.c_void_p(mom.data_ptr())))
                        if es != caller:
                            es.wait_stream(caller)
        starts = torch.empty((K, n), dtype=f32, device=dev)
        carry = torch.empty((n,), dtype=f32, device=dev)
        nat.check(nat.lib.lz_episode_starts(n, K, _p(done), _p(self.last_episode_starts),
                                            _p(starts), _p(carry), dev.index,
                                            ctypes.c_void_p(caller.cuda_stream)))
        self.last_episode_starts = carry
        self._hand_over(obs_last, stack_out)
        if want_mom:
            if self.group is not None:
                dist.all_reduce(mom, group=self.group)
            nat.check(nat.lib.lz_rms_update(self.obs_rms._h, ctypes.c_void_p(mom.data_ptr())))
        return RolloutBatch(obs_buf, act_buf, logp, val, rew, done, starts, last_val, obs_last,
                            mom, didx, tobs, ndone, stack_out)

    def compute_returns_and_advantage(self, batch):
        """RolloutBuffer.compute_returns_and_advantage(last_values, dones) on device."""
        K, n = batch.rewards.shape
        adv = torch.empty_like(batch.rewards)
        ret = torch.empty_like(batch.rewards)
        nat.check(nat.lib.lz_gae(n, K, _p(batch.rewards), _p(batch.values), _p(batch.dones),
                                 _p(batch.last_values), self.gamma, self.gae_lambda, _p(adv), _p(ret),
                                 self.device.index,
                                 ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        batch.advantages, batch.returns = adv, ret
        return adv, ret


# ------------------------------------------------------------------------------ evaluation
# The factor the reference's evaluators multiply the error observations by before they
# take MAE / RMSE: HRSyncEnv emits e / 50 and code/test_evaluate.py:124-126,137 multiplies
# it back; the other systems' observations carry the error itself.
ERR_SCALE = {"lorenz3": 1.0, "lorenz4": 1.0, "pmsm": 1.0, "hr": 50.0}
ERR_DIMS = {"lorenz3": 3, "lorenz4": 4, "pmsm": 3, "hr": 3}
# ... and the factor they multiply the action by before they plot it as the control signal
# (code/test_evaluate.py:127-128 action * 100 for HR; the other systems' scripts keep the action)
CTRL_SCALE = {"lorenz3": 1.0, "lorenz4": 1.0, "pmsm": 1.0, "hr": 100.0}
# the leading state planes LZ_TRACE_STATE appends to a trace row (lorenz_env.h)
STATE_DIMS = {"lorenz3": 3, "lorenz4": 8, "pmsm": 6, "hr": 6}


def trace_shape(K, start=0, every=1):
    """T, the rows of a trace of K steps: step k is recorded when k >= start and
    (k - start) % every == 0.  Refuses what lz_eval_trace_shape refuses."""
    K, start, every = int(K), int(start), int(every)
    if K < 1 or every < 1 or start < 0 or start >= K:
        raise ValueError("a trace needs K >= 1, trace_every >= 1 and 0 <= trace_start < K "
                         "(K=%d, trace_start=%d, trace_every=%d)" % (K, start, every))
    return -(-(K - start) // every)


def validate_trace_ids(ids, num_envs):
    """The env ids of a trace as a list of ints: at least one, each in [0, num_envs), no
    repeats (at the C level a repeated id leaves it open which of its rows is written)."""
    if isinstance(ids, torch.Tensor):
        if ids.is_floating_point() or ids.dtype == torch.bool:
            raise ValueError("trace ids must be integers, got %s" % ids.dtype)
        ids = ids.detach().cpu().reshape(-1).tolist()
    else:
        ids = [i for i in np.asarray(ids).reshape(-1).tolist()]
        if any(not isinstance(i, int) or isinstance(i, bool) for i in ids):
            raise ValueError("trace ids must be integers")
    if not ids:
        raise ValueError("trace needs at least one env id (trace=None evaluates without a trace)")
    bad = [i for i in ids if not 0 <= i < num_envs]
    if bad:
        raise ValueError("trace ids outside [0, %d): %s" % (num_envs, bad[:8]))
    if len(set(ids)) != len(ids):
        seen, dup = set(), []
        for i in ids:
            if i in seen:
                dup.append(i)
            seen.add(i)
        raise ValueError("trace ids repeat: %s" % sorted(set(dup))[:8])
    return ids


class EvalTrace:
    """The per-step record of the traced envs of one ``FusedEvaluator.evaluate(...,
    trace=ids)`` launch: views into ``data``, the float32 [T, M, C] buffer the launch wrote
    (lorenz_env.h lz_eval_trace), row t = step ``steps[t]``, slot m = env ``env_ids[m]``.

    obs [T, M, O]      the observation each step emitted before any auto-reset
    actions [T, M, A]  the clipped action the env was stepped with (model.predict's)
    rewards [T, M]     the env reward
    dones [T, M]       uint8 LZ_DONE_* bits
    state [T, M, S]    with trace_state: the leading state planes after the step, else None
    steps [T]          int64, the step index k of each row
    env_ids [M]        int64
    """

    def __init__(self, data, system_name, obs_dim, action_dim, with_state, start, every, env_ids):
        O, A = int(obs_dim), int(action_dim)
        S = STATE_DIMS[system_name] if with_state else 0
        if data.dim() != 3 or data.shape[2] != O + A + 2 + S:
            raise ValueError("trace data must be [T, M, %d], got %s" % (O + A + 2 + S, tuple(data.shape)))
        self.data = data
        self.system_name = system_name
        self.obs = data[..., :O]
        self.actions = data[..., O:O + A]
        self.rewards = data[..., O + A]
        self.dones = data[..., O + A + 1].to(torch.uint8)
        self.state = data[..., O + A + 2:] if with_state else None
        self.start, self.every = int(start), int(every)
        self.steps = self.start + self.every * torch.arange(data.shape[0], dtype=torch.int64,
                                                            device=data.device)
        self.env_ids = torch.as_tensor(env_ids, dtype=torch.int64).to(data.device)

    def errors(self):
        """[T, M, ED] the synchronisation error as the reference records it (err_x / err_y /
        err_z = obs[:3] * 50 for HR; the other systems' observations carry it unscaled)."""
        return self.obs[..., :ERR_DIMS[self.system_name]] * ERR_SCALE[self.system_name]

    def controls(self):
        """[T, M, A] the control signal as the reference plots it (ctrl_x / ctrl_y =
        action * 100 for HR, the action itself elsewhere)."""
        return self.actions * CTRL_SCALE[self.system_name]

    def time(self, dt):
        """[T] float64: the reference's time axis, step * dt."""
        return self.steps.to(torch.float64) * float(dt)

    def numpy(self):
        """Everything on the host, one dict of NumPy arrays (errors / controls included)."""
        out = {k: getattr(self, k).cpu().numpy() for k in ("obs", "actions", "rewards", "dones", "steps",
                                                           "env_ids")}
        out["state"] = None if self.state is None else self.state.cpu().numpy()
        out["errors"] = self.errors().cpu().numpy()
        out["controls"] = self.controls().cpu().numpy()
        return out


class EvalResult:
    """What one ``FusedEvaluator.evaluate`` launch wrote: ``stats``, the float64 device
    table [EVAL_COLS, N] of lorenz_env.h's LZ_EVAL_* columns (``res.n_win``,
    ``res.ret_sum`` ... are its rows by name, ``res.columns`` all of them), and the pooled
    figures the reference's evaluators print.

    ``pooled_sums`` is the float64 device tensor [EVAL_COLS] of column sums over this
    handle's envs; a multi-rank caller all-reduces it (SUM) and passes it back through
    ``EvalResult.pool``.  The max / first-done / done-bit columns do not pool by a sum:
    ``max_abs`` is taken over the table itself.  ``trace``: the EvalTrace of a traced
    launch, else None."""

    def __init__(self, stats, system_name, trace=None):
        self.stats = stats
        self.trace = trace
        self.system_name = system_name
        self.err_dims = ERR_DIMS[system_name]
        self.err_scale = ERR_SCALE[system_name]
        self.pooled_sums = stats.sum(dim=1)
        self.columns = {name: stats[i] for i, name in enumerate(nat.EVAL_COLUMNS)}
        self._pooled = None

    def __getattr__(self, name):
        cols = self.__dict__.get("columns")
        if cols is not None and name in cols:
            return cols[name]
        raise AttributeError(name)

    def pool(self, pooled_sums=None):
        """The pooled figures as a dict of Python floats / lists (one device-to-host copy),
        from ``pooled_sums`` (default: this handle's own)."""
        s = (self.pooled_sums if pooled_sums is None else pooled_sums).cpu().numpy()
        ED, c = self.err_dims, self.err_scale
        nan = float("nan")
        n_win = s[nat.EVAL_N_WIN]
        ab = s[nat.EVAL_ABS_SUM0:nat.EVAL_ABS_SUM0 + ED]
        sq = s[nat.EVAL_SQ_SUM0:nat.EVAL_SQ_SUM0 + ED]
        out = {}
        with np.errstate(invalid="ignore", divide="ignore"):
            out["mae_per_dim"] = [float(c * v / n_win) if n_win else nan for v in ab]
            out["rmse_per_dim"] = [float(c * np.sqrt(v / n_win)) if n_win else nan for v in sq]
            out["mae"] = float(c * ab.sum() / (ED * n_win)) if n_win else nan
            out["rmse"] = float(c * np.sqrt(sq.sum() / (ED * n_win))) if n_win else nan
            n_ep = s[nat.EVAL_N_EP]
            if n_ep:
                mean = s[nat.EVAL_EP_RET_SUM] / n_ep
                out["mean_reward"] = float(mean)
                out["std_reward"] = float(np.sqrt(max(s[nat.EVAL_EP_RET_SQ] / n_ep - mean * mean, 0.0)))
                out["mean_ep_length"] = float(s[nat.EVAL_EP_LEN_SUM] / n_ep)
            else:
                out["mean_reward"] = out["std_reward"] = out["mean_ep_length"] = nan
            n_steps = s[nat.EVAL_N_STEPS]
            out["mean_step_reward"] = float(s[nat.EVAL_RET_SUM] / n_steps) if n_steps else nan
        return out

    def _get(self, key):
        if self._pooled is None:
            self._pooled = self.pool()
        return self._pooled[key]

    mae = property(lambda self: self._get("mae"))
    rmse = property(lambda self: self._get("rmse"))
    mae_per_dim = property(lambda self: self._get("mae_per_dim"))
    rmse_per_dim = property(lambda self: self._get("rmse_per_dim"))
    mean_reward = property(lambda self: self._get("mean_reward"))
    std_reward = property(lambda self: self._get("std_reward"))
    mean_ep_length = property(lambda self: self._get("mean_ep_length"))
    mean_step_reward = property(lambda self: self._get("mean_step_reward"))

    @property
    def max_abs(self):
        """Largest |error| in the window over envs and error dims (NaN if any is NaN)."""
        m = self.stats[nat.EVAL_MAX_ABS0:nat.EVAL_MAX_ABS0 + self.err_dims]
        return float(self.err_scale * m.max().item())  # torch.max propagates NaN


class FusedEvaluator(_PolicySeam):
    """The reference's evaluation loops on the device, one launch per evaluation
    (lz_evaluate_policy_f32 / _attn_f32 / _attn_stack_f32): K steps of {frozen
    VecNormalize, policy forward at SB3's float32 precision, (sample,) clip, env step}
    with per-env float64 running sums of |error|, error^2, max |error|, rewards and episode
    returns in registers -- no [K, N, *] buffer, no value net -- and one [EVAL_COLS, N]
    table at the end (code/test_evaluate.py:91-150, verify_sync.py:208-237,
    code/lorenz_filter/test_evaluate.py:94-157, code/lorenz_pmsm/test_evaluate.py:61-166).

    backend:       gym_lorenz.core.BatchedEnv, float32 (lorenz3 / lorenz4 / pmsm / hr; the
                   attention policies: lorenz3 / pmsm / hr)
    state_dict:    SB3 ActorCriticPolicy state_dict; its keys pick the kernel as
                   FusedRolloutCollector.set_params does (MlpPolicy, code/train.py's
                   attention extractor, code/lorenz_filter/train.py's LayerNorm one)
    obs_rms:       DeviceRunningMeanStd whose statistics stay frozen, or None
    deterministic: SB3 predict(deterministic=True) (default); False draws the Philox
                   normals a rollout would
    frame_stack:   1 or 4 (VecFrameStack in front of the LayerNorm attention policy, or of
                   the 64-unit MlpPolicy code/lorenz_filter/train.py:109-131 trains:
                   lz_stack_evaluate_policy_f32, untraced)
    """

    _what = "evaluation"

    def __init__(self, backend, state_dict, obs_rms=None, clip_obs=10.0, norm_eps=1e-8,
                 deterministic=True, frame_stack=1):
        if backend.tdtype != torch.float32:
            raise ValueError("the fused evaluation runs float32 env handles")
        if backend.system_name not in ERR_SCALE:
            raise ValueError("the fused evaluation runs LORENZ3 / LORENZ4 / PMSM / HR")
        self.env = backend
        self.device = backend.device
        self.n, self.O, self.A = backend.num_envs, backend.obs_dim, backend.action_dim
        self.obs_rms, self.clip_obs, self.norm_eps = obs_rms, float(clip_obs), float(norm_eps)
        self.deterministic = bool(deterministic)
        self.act_low, self.act_high = action_bounds(backend.system_name)
        self._init_frame_stack(frame_stack)
        self.set_params(state_dict)

    def set_params(self, state_dict):
        """Pack and upload the policy (float32 only: no bf16 or i8x4 evaluation); the blob's
        format tag is checked on the host against the launch this evaluator makes."""
        self._select(state_dict)
        self._set_blob(self._pack_params(state_dict, "fp32"))

    def reset(self, init=None):
        """VecEnv.reset() (init: injected initial states [N, init_dim], as lz_reset); the
        next evaluation starts from these observations and a fresh frame stack."""
        return self._start_from(self.env.reset(init=init))

    def evaluate(self, K, skip=0, max_episodes=0, trace=None, trace_every=1, trace_start=0,
                 trace_state=False, trace_out=None, trace_slot_map=None):
        """K closed-loop steps in one launch -> EvalResult.  skip: in-episode step index
        from which the error window opens (the reference's ``step >= 1000``);
        max_episodes: episodes counted per env (0: every step counts).

        trace: env ids (a sequence or tensor, no repeats) whose trajectories the launch
        records besides the table -> ``EvalResult.trace`` (EvalTrace): steps trace_start,
        trace_start + trace_every, ... whatever skip and max_episodes say; trace_state adds
        the state planes (the master and slave states).  trace_out / trace_slot_map:
        caller-owned buffers for the rows (float32, >= T * M * C elements) and the launch's
        slot map (int32 [N]); allocated here when None."""
        if trace is not None and self.mlp_stack:
            raise ValueError("the frame-stacked MlpPolicy evaluation has no traced form (trace=)")
        if self.last_obs is None:
            self.reset()
        n, O, dev = self.n, self.O, self.device
        tr = None
        if trace is not None:
            T = trace_shape(K, trace_start, trace_every)
            ids = validate_trace_ids(trace, n)
            M = len(ids)
            C = O + self.A + 2 + (STATE_DIMS[self.env.system_name] if trace_state else 0)
            if trace_out is None:
                trace_out = torch.empty((T * M * C,), dtype=torch.float32, device=dev)
            if trace_slot_map is None:
                trace_slot_map = torch.empty((n,), dtype=torch.int32, device=dev)
            ids_dev = torch.tensor(ids, dtype=torch.int64, device=dev)
            tr = nat.LzEvalTrace()
            tr.ids, tr.count = _p(ids_dev), M
            tr.slot_map = check_buffer(trace_slot_map, "trace_slot_map", torch.int32, n, dev)
            tr.start, tr.every = int(trace_start), int(trace_every)
            tr.flags = nat.TRACE_STATE if trace_state else 0
            tr.out = check_buffer(trace_out, "trace_out", torch.float32, T * M * C, dev, at_least=True)
            tr.out_capacity_bytes = trace_out.numel() * 4
        elif trace_every != 1 or trace_start != 0 or trace_state or trace_out is not None:
            raise ValueError("trace_every / trace_start / trace_state / trace_out need trace=ids")
        stats = torch.empty((nat.EVAL_COLS, n), dtype=torch.float64, device=dev)
        obs_last = torch.empty((n, O), dtype=torch.float32, device=dev)
        e = nat.LzPolicyEvalArgs()
        e.K = int(K)
        e.flags = nat.POLICY_DETERMINISTIC if self.deterministic else 0
        e.blob, e.obs_in, e.obs_last = _p(self.blob), _p(self.last_obs), _p(obs_last)
        e.obs_norm = _p(self.obs_rms.state) if self.obs_rms is not None else None
        e.norm_eps, e.clip_obs = self.norm_eps, self.clip_obs
        e.act_low, e.act_high = self.act_low, self.act_high
        e.skip, e.max_episodes = int(skip), int(max_episodes)
        e.stats = _p(stats)
        with self._on_env_stream():
            stack_out = self._launch("evaluate" if tr is None else "trace", e, trace=tr)
        self._hand_over(obs_last, stack_out)
        if tr is None:
            return EvalResult(stats, self.env.system_name)
        self._keep += (ids_dev, trace_slot_map)
        rows = EvalTrace(trace_out[:T * M * C].view(T, M, C), self.env.system_name, O, self.A,
                         trace_state, trace_start, trace_every, ids_dev)
        return EvalResult(stats, self.env.system_name, trace=rows)


def evaluate_policy(backend, state_dict, n_eval_episodes, **kw):
    """SB3 ``evaluate_policy(model, env, n_eval_episodes)`` (code/gym_run.py:95) on an
    auto-reset handle with ``max_episode_steps = L > 0``: every env runs
    ``max_episodes = ceil(n_eval_episodes / N)`` whole episodes in one launch of
    ``K = max_episodes * L`` steps; returns ``(mean_reward, std_reward)`` over the counted
    episodes, std = sqrt(max(sum(R^2)/n - mean^2, 0)).

    SB3 takes n_eval_episodes / N episodes from each of the N envs, so this is SB3's
    episode set when N divides n_eval_episodes; otherwise this raises.  (Episodes that
    terminate before L steps are counted as they end; an env that finishes its share early
    keeps stepping uncounted.)  **kw: FusedEvaluator's arguments."""
    n = backend.num_envs
    L = int(backend.config.max_episode_steps)
    if not (backend.config.flags & nat.FLAG_AUTORESET) or L <= 0:
        raise ValueError("evaluate_policy needs an auto-reset handle with max_episode_steps > 0")
    n_eval_episodes = int(n_eval_episodes)
    if n_eval_episodes < 1 or n_eval_episodes % n:
        raise ValueError("n_eval_episodes (%d) must be a positive multiple of the %d envs"
                         % (n_eval_episodes, n))
    per_env = -(-n_eval_episodes // n)
    ev = FusedEvaluator(backend, state_dict, **kw)
    ev.reset()
    res = ev.evaluate(per_env * L, skip=0, max_episodes=per_env)
    return res.mean_reward, res.std_reward


# ------------------------------------------------------------------------------ A2C update
# SB3 2.7.1 A2C.train() for the float32 MlpPolicy on the device (lz_a2c_grad_f32 +
# lz_a2c_apply_f32): the gradient step of code/lorenz_pmsm/train.py:151-185's learner.
def linear_schedule(initial_value):
    """code/lorenz_pmsm/train.py:187-197: the learning rate falls linearly with SB3's
    ``progress_remaining`` (1 -> 0) and never below 1e-5."""
    initial_value = float(initial_value)

    def schedule(progress_remaining):
        return max(progress_remaining * initial_value, 1e-5)

    return schedule


LEARNER_HIDDEN = (64, HIDDEN)  # the hidden sizes the gradient kernels are built for


def a2c_param_shapes(obs_dim, act_dim, hidden=HIDDEN):
    """The 13 tensors' shapes in KEYS order (nn.Linear layout)."""
    H = int(hidden)
    return [(H, obs_dim), (H,), (H, H), (H,)] * 2 + [(act_dim, H), (act_dim,), (1, H), (1,),
                                                      (act_dim,)]


def a2c_param_layout(obs_dim, act_dim, hidden=HIDDEN):
    """{key: (offset, shape)} of lz_a2c_grad_f32's (lz_a2c_grad_hidden_f32's) flat parameter
    vector, and its length."""
    out, o = {}, 0
    for k, shp in zip(KEYS, a2c_param_shapes(obs_dim, act_dim, hidden)):
        out[k] = (o, shp)
        o += int(np.prod(shp))
    return out, o


def _stream_ptr(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def net_arch_hidden(net_arch, who="net_arch"):
    """SB3's policy_kwargs["net_arch"] -> the hidden size of a learner: H, [H, H] or
    dict(pi=[H, H], vf=[H, H]) with H in LEARNER_HIDDEN; anything else is a ValueError."""
    arch = net_arch
    if isinstance(arch, dict):
        if set(arch) != {"pi", "vf"} or list(arch["pi"]) != list(arch["vf"]):
            raise ValueError("%s: net_arch must have equal pi and vf lists, not %r" % (who, net_arch))
        arch = list(arch["pi"])
    if isinstance(arch, (list, tuple)):
        if len(arch) != 2 or arch[0] != arch[1]:
            raise ValueError("%s: net_arch must be two equal layers, not %r" % (who, net_arch))
        arch = arch[0]
    if isinstance(arch, bool) or not isinstance(arch, (int, np.integer)) or int(arch) not in LEARNER_HIDDEN:
        raise ValueError("%s: net_arch %r is not implemented (hidden sizes %s)"
                         % (who, net_arch, " / ".join(str(h) for h in LEARNER_HIDDEN)))
    return int(arch)


def _grad_fns(kind, hidden, O, A, who, wide=False):
    """(P, workspace_bytes(n, max_workgroups), grad entry point) of _native.GRAD_ENTRIES' row
    for a hidden size: the first entry points at HIDDEN, the _hidden ones
    (lz_a2c_grad_hidden_f32, ...) otherwise; wide (PPO only): the _wide ones, the 64-unit net
    on up to 24 inputs."""
    H = int(hidden)
    if wide and kind != "ppo":
        raise nat.LorenzEnvError(nat.LZ_ERR_UNSUPPORTED, "%s: the wide gradient is PPO's" % who)
    if not wide and nat.lib.lz_a2c_param_count(O, A) < 0:
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "%s: obs_dim must be 1..8, act_dim 1..4" % who)
    row = nat.GRAD_ENTRIES[kind, "wide" if wide else "first" if H == HIDDEN else "hidden"]
    count, ws, grad = (getattr(nat.lib, name) for name in row[:3])
    h = (H,) if row[3] else ()
    P = int(count(O, A, *h))
    if P < 0:
        raise nat.LorenzEnvError(nat.LZ_ERR_UNSUPPORTED, "%s: %s" % (
            who, "the wide gradient takes obs_dim 1..24, act_dim 1..4 and hidden 64" if wide
            else "hidden must be 64 or 128"))
    return P, (lambda n, cap: int(ws(n, O, A, *h, cap))), grad


def _launch_grad(who, fns, g, n, tail, max_workgroups, workspace, out, dev):
    """The end of a2c_grad / ppo_grad: g's workspace and grad_sums [P + tail] (allocated when
    None, checked either way) for n samples, then the launch on the current stream."""
    P, ws_bytes, grad_fn = fns
    need = ws_bytes(n, int(max_workgroups))
    if need < 0:
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "%s: empty batch or bad max_workgroups" % who)
    if workspace is None:
        workspace = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    g.workspace = check_buffer(workspace, "workspace", torch.float64, need // 8, dev, at_least=True)
    g.workspace_bytes = workspace.numel() * 8
    if out is None:
        out = torch.empty((P + tail,), dtype=torch.float64, device=dev)
    g.grad_sums = check_buffer(out, "grad_sums", torch.float64, P + tail, dev)
    nat.check(grad_fn(ctypes.byref(g), dev.index, _stream_ptr(dev)))
    return out


def a2c_grad(params, observations, actions, advantages, returns, obs_dim, act_dim, vf_coef=0.5,
             ent_coef=0.0, max_workgroups=0, workspace=None, out=None, hidden=HIDDEN):
    """lz_a2c_grad_f32 (hidden=64: lz_a2c_grad_hidden_f32) on the current stream: float64
    device tensor [P + 4] of gradient sums over the samples, then sum(-adv log_prob),
    sum((ret - v)^2), sum(-entropy), the count.  Every buffer is checked (core.check_buffer)
    before the launch."""
    dev = params.device
    O, A = int(obs_dim), int(act_dim)
    if dev.type != "cuda":
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "a2c_grad: params must be a device tensor")
    fns = _grad_fns("a2c", hidden, O, A, "a2c_grad")
    B = int(advantages.numel())
    f32 = torch.float32
    g = nat.LzA2cGradArgs()
    g.params = check_buffer(params, "params", f32, fns[0], dev)
    g.observations = check_buffer(observations, "observations", f32, B * O, dev)
    g.actions = check_buffer(actions, "actions", f32, B * A, dev)
    g.advantages = check_buffer(advantages, "advantages", f32, B, dev)
    g.returns = check_buffer(returns, "returns", f32, B, dev)
    g.n_samples, g.obs_dim, g.act_dim, g.hidden = B, O, A, int(hidden)
    g.max_workgroups = int(max_workgroups)
    g.vf_coef, g.ent_coef = float(vf_coef), float(ent_coef)
    return _launch_grad("a2c_grad", fns, g, B, 4, max_workgroups, workspace, out, dev)


def a2c_apply(grad_sums, params, square_avg, lr, max_grad_norm=0.5, alpha=0.99, eps=1e-5,
              vf_coef=0.5, ent_coef=0.0, stats=None):
    """lz_a2c_apply_f32 on the current stream: clip_grad_norm_ + the RMSpropTFLike step on
    params / square_avg in place; returns the float64 device tensor stats [8]
    (_native.A2C_STATS)."""
    dev = params.device
    if dev.type != "cuda":
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "a2c_apply: params must be a device tensor")
    P = int(params.numel())
    a = nat.LzA2cApplyArgs()
    a.grad_sums = check_buffer(grad_sums, "grad_sums", torch.float64, P + 4, dev)
    a.params = check_buffer(params, "params", torch.float32, P, dev)
    a.square_avg = check_buffer(square_avg, "square_avg", torch.float32, P, dev)
    a.n_params = P
    a.lr, a.max_grad_norm, a.alpha, a.eps = float(lr), float(max_grad_norm), float(alpha), float(eps)
    a.vf_coef, a.ent_coef = float(vf_coef), float(ent_coef)
    if stats is None:
        stats = torch.empty((8,), dtype=torch.float64, device=dev)
    a.stats = check_buffer(stats, "stats", torch.float64, 8, dev)
    nat.check(nat.lib.lz_a2c_apply_f32(ctypes.byref(a), dev.index, _stream_ptr(dev)))
    return stats


class _FusedLearner:
    """What FusedA2C and FusedPPO share: the collectors they refuse, the policy as one flat
    float32 device vector in a2c_param_layout's order, the schedules, and SB3's
    OnPolicyAlgorithm.learn loop around the subclass's per-rollout step."""

    # the frame stack a learner also trains on: FusedPPO's 4 (with net_arch=64), else none
    _frame_stacks = ()

    def __init__(self, collector, state_dict, learning_rate, n_steps, net_arch=None):
        who = type(self).__name__
        # SB3's policy_kwargs["net_arch"]; None: the 128-unit net, as before the 64-unit form
        self.hidden = HIDDEN if net_arch is None else net_arch_hidden(net_arch, who)
        if is_attention_policy(state_dict) or is_attention_ln_policy(state_dict):
            raise ValueError("%s updates the MlpPolicy; the attention policies' update is "
                             "not implemented" % who)
        if collector.precision in ("bf16", "i8x4"):
            raise ValueError("%s needs a float32 collector (precision='fp32'), not %r"
                             % (who, collector.precision))
        # the frame-stacked 64-unit MlpPolicy (code/lorenz_filter/train.py:109-131): the
        # learner's input is the stacked observation, its gradient the _wide entry points'
        self.wide = (collector.frame_stack != 1 and collector.frame_stack in self._frame_stacks
                     and self.hidden == STACK_HIDDEN)
        if collector.frame_stack != 1 and not self.wide:
            raise ValueError("%s updates the MlpPolicy (frame_stack=1)" % who)
        self.collector = collector
        self.device = collector.device
        self.O, self.A = collector.frame_stack * collector.O, collector.A
        self.layout, self.P = a2c_param_layout(self.O, self.A, self.hidden)
        flat = []
        for k, (_, shp) in self.layout.items():
            if k not in state_dict:
                raise KeyError("policy state_dict lacks %r" % k)
            t = torch.as_tensor(_np(state_dict[k]))
            if tuple(t.shape) != tuple(shp):
                raise ValueError("%s has shape %s, expected %s (%s implements hidden=%d)"
                                 % (k, tuple(t.shape), shp, who, self.hidden))
            flat.append(t.reshape(-1))
        self.params = torch.cat(flat).to(self.device).contiguous()
        self.learning_rate = learning_rate
        self.n_steps = int(n_steps)
        self.num_timesteps = 0
        self.progress_remaining = 1.0
        self._ws = None

    def _now(self, v):
        """A float, or a schedule of SB3's progress_remaining, as of now."""
        return float(v(self.progress_remaining)) if callable(v) else float(v)

    def _lr(self):
        return self._now(self.learning_rate)

    def _by_key(self, vec):
        flat = vec.detach().cpu()
        return {k: flat[o:o + int(np.prod(shp))].reshape(shp).clone()
                for k, (o, shp) in self.layout.items()}

    def state_dict(self):
        """SB3 keys -> float32 CPU tensors (one device-to-host copy)."""
        return self._by_key(self.params)

    def _workspace_need(self, kind, n):
        """Entries of the workspace a gradient launch on n samples needs."""
        return _grad_fns(kind, self.hidden, self.O, self.A, type(self).__name__, self.wide)[1](n, 0) // 8

    def _workspace(self, need):
        """The gradient kernels' float64 workspace, grown to `need` entries."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((max(need, 1),), dtype=torch.float64, device=self.device)
        return self._ws

    def _step(self, batch):
        """The update on one rollout (FusedA2C.update, FusedPPO.train): returns its stats."""
        raise NotImplementedError

    def _world_size(self):
        """The ranks whose rollouts count into num_timesteps."""
        return 1

    def learn(self, total_timesteps, callback=None):
        """SB3 OnPolicyAlgorithm.learn: rollouts of n_steps x num_envs timesteps until
        total_timesteps, progress_remaining = 1 - num_timesteps / total_timesteps updated
        after each collect (what the schedules see in the update); gamma and gae_lambda are
        the collector's.  callback(self, batch, stats) runs after every update.  Returns the
        list of the updates' stats."""
        total = int(total_timesteps)
        col = self.collector
        n = col.n * self._world_size()
        out = []
        start = self.num_timesteps
        while self.num_timesteps - start < total:
            batch = col.collect(self.n_steps)
            self.num_timesteps += self.n_steps * n
            self.progress_remaining = 1.0 - float(self.num_timesteps - start) / float(total)
            col.compute_returns_and_advantage(batch)
            stats = self._step(batch)
            out.append(stats)
            if callback is not None:
                callback(self, batch, stats)
        return out


class FusedA2C(_FusedLearner):
    """SB3 A2C on a FusedRolloutCollector: ``learn`` is the loop collect(n_steps) ->
    compute_returns_and_advantage -> update, and ``update`` one A2C.train() -- the whole
    rollout as one batch, loss = -mean(adv log_prob) + vf_coef mse(returns, values) +
    ent_coef (-mean(entropy)), clip_grad_norm_(max_grad_norm), RMSpropTFLike(alpha=0.99,
    eps=rms_prop_eps) -- in two launches (lz_a2c_grad_f32, lz_a2c_apply_f32) with, when
    ``group`` is set, an all-reduce of the [P + 4] gradient sums between them.  The
    parameters live on the device as one flat float32 vector; after each step they go
    through the host packer into the collector's blob (collector.set_params).

    learning_rate: a float or a schedule of SB3's progress_remaining (linear_schedule).
    net_arch: SB3's policy_kwargs["net_arch"] -- None (the 128-unit net), or 64 / [64, 64] /
    dict(pi=[64, 64], vf=[64, 64]) for SB3's default MlpPolicy, which is what
    code/lorenz_pmsm/train.py:130-139 trains (the same forms with 128 are accepted); the
    state_dict must have that size.  Float32 MlpPolicy collectors only; normalize_advantage
    and Adam are not implemented."""

    def __init__(self, collector, state_dict, learning_rate=7e-4, n_steps=5, vf_coef=0.5,
                 ent_coef=0.0, max_grad_norm=0.5, rms_prop_eps=1e-5, group=None,
                 normalize_advantage=False, use_rms_prop=True, net_arch=None):
        if normalize_advantage:
            raise ValueError("FusedA2C: normalize_advantage is not implemented (SB3's default-off "
                             "option; the reference leaves it off)")
        if not use_rms_prop:
            raise ValueError("FusedA2C: only RMSpropTFLike (use_rms_prop=True) is implemented")
        super().__init__(collector, state_dict, learning_rate, n_steps, net_arch)
        self.square_avg = torch.ones_like(self.params)  # RMSpropTFLike starts at ones
        self.vf_coef, self.ent_coef = float(vf_coef), float(ent_coef)
        self.max_grad_norm, self.rms_prop_eps = float(max_grad_norm), float(rms_prop_eps)
        self.group = group
        self._sums = torch.empty((self.P + 4,), dtype=torch.float64, device=self.device)
        collector.set_params(self.state_dict())

    def optimizer_state(self):
        """{"square_avg": {SB3 key: float32 CPU tensor}}: RMSpropTFLike's state."""
        return {"square_avg": self._by_key(self.square_avg)}

    def update(self, batch, lr=None):
        """One gradient step on the whole RolloutBatch (advantages / returns set by
        compute_returns_and_advantage); pushes the new weights to the collector.  Returns
        the stats as a dict of Python floats (_native.A2C_STATS)."""
        if batch.advantages is None or batch.returns is None:
            raise ValueError("FusedA2C.update: compute_returns_and_advantage(batch) first")
        lr = self._lr() if lr is None else float(lr)
        B = int(batch.advantages.numel())
        ws = self._workspace(self._workspace_need("a2c", B))
        a2c_grad(self.params, batch.observations, batch.actions, batch.advantages, batch.returns,
                 self.O, self.A, self.vf_coef, self.ent_coef, workspace=ws, out=self._sums,
                 hidden=self.hidden)
        if self.group is not None:
            dist.all_reduce(self._sums, group=self.group)
        stats = a2c_apply(self._sums, self.params, self.square_avg, lr, self.max_grad_norm, 0.99,
                          self.rms_prop_eps, self.vf_coef, self.ent_coef)
        self.collector.set_params(self.state_dict())
        return dict(zip(nat.A2C_STATS, stats.cpu().tolist()))

    def _step(self, batch):
        return self.update(batch)

    def _world_size(self):
        return dist.get_world_size(self.group) if self.group is not None else 1


# ------------------------------------------------------------------------------ PPO update
# SB3 2.7.1 PPO.train() for the float32 MlpPolicy on the device (lz_ppo_adv_moments +
# lz_ppo_grad_f32 + lz_adam_apply_f32 per minibatch): the update of code/train.py:97-129's,
# code/lorenz_filter/train.py's and code/gym_run.py:83's learners.
def _check_indices(indices, n_rows, dev, who):
    """(pointer or None, M) of a minibatch's row list: int32, on the device, contiguous,
    at least one entry (its values are checked by the kernels, on the device)."""
    if indices is None:
        return None, n_rows
    M = int(indices.numel()) if isinstance(indices, torch.Tensor) else 0
    if M < 1:
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "%s: indices must be a non-empty tensor" % who)
    return check_buffer(indices, "indices", torch.int32, M, dev), M


def ppo_adv_moments(advantages, indices=None, out=None):
    """lz_ppo_adv_moments on the current stream: float64 device tensor [2] = (mean, unbiased
    std) of advantages[indices] (indices None: of all of them), in float64."""
    dev = advantages.device
    if dev.type != "cuda":
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "ppo_adv_moments: advantages must be a device tensor")
    n_rows = int(advantages.numel())
    adv = check_buffer(advantages, "advantages", torch.float32, n_rows, dev)
    idx, M = _check_indices(indices, n_rows, dev, "ppo_adv_moments")
    if out is None:
        out = torch.empty((2,), dtype=torch.float64, device=dev)
    o = check_buffer(out, "adv_moments", torch.float64, 2, dev)
    nat.check(nat.lib.lz_ppo_adv_moments(adv, idx, M, n_rows, None, o, dev.index, _stream_ptr(dev)))
    return out


def ppo_grad(params, observations, actions, advantages, returns, old_log_prob, old_values, obs_dim,
             act_dim, indices=None, clip_range=0.2, clip_range_vf=None, adv_moments=None, ctrl=None,
             vf_coef=0.5, ent_coef=0.0, max_workgroups=0, workspace=None, out=None, hidden=HIDDEN,
             wide=False):
    """lz_ppo_grad_f32 (hidden=64: lz_ppo_grad_hidden_f32; wide: lz_ppo_grad_wide_f32, obs_dim up
    to 24 at hidden=64) on the current stream over the rows `indices` (int32 device tensor
    [M]; None: every row) of the flat rollout arrays: float64 device tensor [P + 6] of the
    gradient sums, then sum(policy loss terms), sum((ret - v_pred)^2), sum(-entropy), M,
    the clipped count and sum((ratio - 1) - log_ratio).  adv_moments: ppo_adv_moments'
    output (None: no normalisation); clip_range_vf None or <= 0: no value clipping
    (old_values may then be None); ctrl: the int64 [2] control block of adam_apply.  Every
    buffer is checked (core.check_buffer) before the launch."""
    dev = params.device
    O, A = int(obs_dim), int(act_dim)
    if dev.type != "cuda":
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "ppo_grad: params must be a device tensor")
    fns = _grad_fns("ppo", hidden, O, A, "ppo_grad", wide)
    n_rows = int(advantages.numel())
    cvf = 0.0 if clip_range_vf is None else float(clip_range_vf)
    f32 = torch.float32
    g = nat.LzPpoGradArgs()
    g.params = check_buffer(params, "params", f32, fns[0], dev)
    g.observations = check_buffer(observations, "observations", f32, n_rows * O, dev)
    g.actions = check_buffer(actions, "actions", f32, n_rows * A, dev)
    g.advantages = check_buffer(advantages, "advantages", f32, n_rows, dev)
    g.returns = check_buffer(returns, "returns", f32, n_rows, dev)
    g.old_log_prob = check_buffer(old_log_prob, "old_log_prob", f32, n_rows, dev)
    g.old_values = check_buffer(old_values, "old_values", f32, n_rows, dev, required=cvf > 0.0)
    g.indices, M = _check_indices(indices, n_rows, dev, "ppo_grad")
    g.n_samples, g.n_rows, g.obs_dim, g.act_dim, g.hidden = M, n_rows, O, A, int(hidden)
    g.max_workgroups = int(max_workgroups)
    g.vf_coef, g.ent_coef = float(vf_coef), float(ent_coef)
    g.clip_range, g.clip_range_vf = float(clip_range), cvf
    g.adv_moments = check_buffer(adv_moments, "adv_moments", torch.float64, 2, dev, required=False)
    g.ctrl = check_buffer(ctrl, "ctrl", torch.int64, 2, dev, required=False)
    return _launch_grad("ppo_grad", fns, g, M, 6, max_workgroups, workspace, out, dev)


def adam_apply(grad_sums, params, exp_avg, exp_avg_sq, ctrl, lr, max_grad_norm=0.5, betas=(0.9, 0.999),
               eps=1e-5, vf_coef=0.5, ent_coef=0.0, target_kl=None, stats=None):
    """lz_adam_apply_f32 on the current stream: the target_kl stop, clip_grad_norm_ and
    torch.optim.Adam's step on params / exp_avg / exp_avg_sq in place, the step count and
    the stop flag in ctrl (int64 device tensor [2] = step, stopped); returns the float64
    device tensor stats [12] (_native.PPO_STATS)."""
    dev = params.device
    if dev.type != "cuda":
        raise nat.LorenzEnvError(nat.LZ_ERR_INVALID, "adam_apply: params must be a device tensor")
    P = int(params.numel())
    a = nat.LzAdamApplyArgs()
    a.grad_sums = check_buffer(grad_sums, "grad_sums", torch.float64, P + 6, dev)
    a.params = check_buffer(params, "params", torch.float32, P, dev)
    a.exp_avg = check_buffer(exp_avg, "exp_avg", torch.float32, P, dev)
    a.exp_avg_sq = check_buffer(exp_avg_sq, "exp_avg_sq", torch.float32, P, dev)
    a.ctrl = check_buffer(ctrl, "ctrl", torch.int64, 2, dev)
    a.n_params = P
    a.lr, a.max_grad_norm, a.eps = float(lr), float(max_grad_norm), float(eps)
    a.beta1, a.beta2 = float(betas[0]), float(betas[1])
    a.vf_coef, a.ent_coef = float(vf_coef), float(ent_coef)
    a.target_kl = 0.0 if target_kl is None else float(target_kl)
    if stats is None:
        stats = torch.empty((len(nat.PPO_STATS),), dtype=torch.float64, device=dev)
    a.stats = check_buffer(stats, "stats", torch.float64, len(nat.PPO_STATS), dev)
    nat.check(nat.lib.lz_adam_apply_f32(ctypes.byref(a), dev.index, _stream_ptr(dev)))
    return stats


class FusedPPO(_FusedLearner):
    """SB3 PPO on a FusedRolloutCollector: ``learn`` is the loop collect(n_steps) ->
    compute_returns_and_advantage -> train, and ``train`` one PPO.train(): n_epochs
    permutations of the rollout's rows cut into minibatches of batch_size, each one
    lz_ppo_adv_moments + lz_ppo_grad_f32 + lz_adam_apply_f32 on the device with no host
    round trip (the Adam step count and the target_kl stop flag live on the device); the
    per-minibatch stats come to the host once, and the new weights go through the host
    packer into the collector's blob once, after the last minibatch.

    learning_rate, clip_range (and clip_range_vf): a float or a schedule of SB3's
    progress_remaining (linear_schedule).  generator: the torch.Generator (on the
    collector's device) the permutations are drawn from.  net_arch: as FusedA2C's (64 is
    what code/train.py:106-118 and code/lorenz_filter/train.py:117-129 train, and the size of
    the reference's shipped PPO policies).  Float32 MlpPolicy collectors only -- with
    net_arch=64 also the frame-stacked one (frame_stack=4: code/lorenz_filter/train.py:109-131's
    PPO("MlpPolicy") on VecFrameStack(n_stack=4)), through lz_ppo_grad_wide_f32 on the
    stacked observations."""

    _frame_stacks = (4,)

    def __init__(self, collector, state_dict, learning_rate=3e-4, n_steps=2048, batch_size=64,
                 n_epochs=10, clip_range=0.2, clip_range_vf=None, normalize_advantage=True,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, target_kl=None, generator=None,
                 net_arch=None):
        if int(batch_size) < 1 or int(n_epochs) < 1 or int(n_steps) < 1:
            raise ValueError("FusedPPO: n_steps, batch_size and n_epochs must be >= 1")
        if normalize_advantage and int(batch_size) < 2:
            raise ValueError("FusedPPO: batch_size must be > 1 with normalize_advantage "
                             "(SB3 asserts it)")
        super().__init__(collector, state_dict, learning_rate, n_steps, net_arch)
        dev = self.device
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.ctrl = torch.zeros((2,), dtype=torch.int64, device=dev)  # Adam's step, stopped
        self.clip_range, self.clip_range_vf = clip_range, clip_range_vf
        self.batch_size, self.n_epochs = int(batch_size), int(n_epochs)
        self.normalize_advantage = bool(normalize_advantage)
        self.vf_coef, self.ent_coef = float(vf_coef), float(ent_coef)
        self.max_grad_norm = float(max_grad_norm)
        self.target_kl = None if target_kl is None else float(target_kl)
        self.generator = generator
        self.n_updates = 0
        self._sums = torch.empty((self.P + 6,), dtype=torch.float64, device=dev)
        self._mom = torch.empty((2,), dtype=torch.float64, device=dev)
        self._perm = self._stats = None
        collector.set_params(self.state_dict())

    def optimizer_state(self):
        """{"exp_avg": {SB3 key: float32 CPU tensor}, "exp_avg_sq": {...}, "step": int}:
        torch.optim.Adam's state."""
        return {"exp_avg": self._by_key(self.exp_avg), "exp_avg_sq": self._by_key(self.exp_avg_sq),
                "step": int(self.ctrl[0].item())}

    def minibatches(self, B):
        """[(first, last)] positions of a permutation of B rows that form each minibatch
        (RolloutBuffer.get: the last one may be shorter)."""
        return [(s, min(s + self.batch_size, B)) for s in range(0, B, self.batch_size)]

    def train(self, batch, lr=None, clip_range=None):
        """One PPO.train() on the RolloutBatch (advantages / returns set by
        compute_returns_and_advantage); pushes the new weights to the collector.  Returns
        {"rows": float64 array [n_epochs * n_minibatches, 12] (_native.PPO_STATS per
        minibatch), SB3's logged means over the minibatches whose loss was computed
        (policy_gradient_loss, value_loss, entropy_loss, clip_fraction, approx_kl), loss (the
        last one computed), learning_rate, clip_range, stopped, n_updates}."""
        if batch.advantages is None or batch.returns is None:
            raise ValueError("FusedPPO.train: compute_returns_and_advantage(batch) first")
        lr = self._lr() if lr is None else float(lr)
        clip = self._now(self.clip_range) if clip_range is None else float(clip_range)
        cvf = None if self.clip_range_vf is None else self._now(self.clip_range_vf)
        dev = self.device
        B = int(batch.advantages.numel())
        cuts = self.minibatches(B)
        self._workspace(self._workspace_need("ppo", min(self.batch_size, B)))
        if self._perm is None or self._perm.numel() != B:
            self._perm = torch.empty((B,), dtype=torch.int32, device=dev)
        rows = self.n_epochs * len(cuts)
        if self._stats is None or self._stats.shape[0] != rows:
            self._stats = torch.empty((rows, len(nat.PPO_STATS)), dtype=torch.float64, device=dev)
        self.ctrl[1:].zero_()  # SB3's continue_training = True (a fill: capturable)
        i = 0
        for _ in range(self.n_epochs):
            torch.randperm(B, dtype=torch.int32, device=dev, generator=self.generator, out=self._perm)
            for lo, hi in cuts:
                self.minibatch_step(batch, self._perm[lo:hi], lr, clip, cvf, self._stats[i])
                i += 1
        out = self._stats.cpu().numpy()
        self.collector.set_params(self.state_dict())
        self.n_updates += self.n_epochs
        col = nat.PPO_STATS.index
        done = out[~np.isnan(out[:, col("n_samples")])]  # after a stop the rows hold no losses
        mean = (lambda name: float(done[:, col(name)].mean())) if len(done) else (lambda name: float("nan"))
        return {"rows": out, "policy_gradient_loss": mean("policy_loss"), "value_loss": mean("value_loss"),
                "entropy_loss": mean("entropy_loss"), "clip_fraction": mean("clip_fraction"),
                "approx_kl": mean("approx_kl"), "loss": float(done[-1, col("loss")]) if len(done) else float("nan"),
                "learning_rate": lr, "clip_range": clip, "stopped": bool(out[-1, col("stopped")] != 0),
                "n_updates": self.n_updates}

    def minibatch_step(self, batch, indices, lr, clip_range, clip_range_vf, stats_row):
        """moments -> grad -> apply for the minibatch of rows `indices`; nothing leaves the
        device, and after a train() of the same batch_size nothing is allocated (the three
        launches capture into a graph)."""
        M = int(indices.numel())
        mom = None
        if self.normalize_advantage and M > 1:  # SB3: len(advantages) > 1
            mom = ppo_adv_moments(batch.advantages, indices, out=self._mom)
        ppo_grad(self.params, batch.observations, batch.actions, batch.advantages, batch.returns,
                 batch.log_probs, batch.values, self.O, self.A, indices, clip_range, clip_range_vf, mom,
                 self.ctrl, self.vf_coef, self.ent_coef, workspace=self._ws, out=self._sums,
                 hidden=self.hidden, wide=self.wide)
        adam_apply(self._sums, self.params, self.exp_avg, self.exp_avg_sq, self.ctrl, lr,
                   self.max_grad_norm, (0.9, 0.999), 1e-5, self.vf_coef, self.ent_coef, self.target_kl,
                   stats=stats_row)

    def _step(self, batch):
        return self.train(batch)
