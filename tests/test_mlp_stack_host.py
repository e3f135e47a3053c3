"""The frame-stacked 64-unit MlpPolicy on the host (code/lorenz_filter/train.py:109-131:
PPO("MlpPolicy") on VecFrameStack(n_stack=4), SB3's default 64 x 64 Tanh nets on a 24-wide
stacked observation): the packer lz_policy_pack_stack_f32 and its blob (format tag 7), the
policy seam's family "mlp_stack", the three lz_ppo_*_wide functions and FusedPPO's
construction on a frame-stacked collector.  No GPU: no compute call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol

# lz_internal.h kStk*: byte offsets of the blob
W1, W2, B1, B2, HW, HB = 0, 6144, 22528, 22784, 23040, 24064
TAG, NET = HB + 48, HB + 64
LOGSTD, TANH = 2 * NET, 2 * NET + 64
BYTES = TANH + 73 * 32
F32_TANH = 2 * 73024 + 64  # lz_internal.h kF32Tanh: the same table in the 128-unit float32 blob

NEW_SYMBOLS = ("lz_policy_pack_stack_f32", "lz_policy_stack_f32_blob_bytes", "lz_stack_rollout_policy_f32",
               "lz_stack_evaluate_policy_f32", "lz_ppo_param_count_wide", "lz_ppo_workspace_bytes_wide",
               "lz_ppo_grad_wide_f32")


def _sd(in_dim, act_dim, hidden=64, seed=3):
    net = pol.ActorCriticMlp(in_dim, act_dim, hidden=hidden, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _row(g, h):
    return (g & 3) + 8 * (g >> 2) + 4 * h


def test_symbols_and_constants():
    header = open(ROOT + "/include/lorenz_env.h").read()
    for name in NEW_SYMBOLS:
        assert hasattr(nat.lib, name) and name in nat.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for text in ("LZ_BLOB_MLP_STACK_F32 = 7", "LZ_CALL_ROLLOUT_POLICY_STACK_F32 = 13",
                 "LZ_CALL_EVALUATE_POLICY_STACK_F32 = 14", "LZ_KERNEL_POLICY_STACK_F32 = 16",
                 "LZ_KERNEL_EVAL_STACK_F32 = 17"):
        assert text in header, text
    assert header.count("code/lorenz_filter/train.py:109-131") >= 4
    assert "code/lorenz_filter/test_evaluate.py:94-157" in header
    assert (nat.BLOB_MLP_STACK_F32, nat.CALL_ROLLOUT_POLICY_STACK_F32, nat.CALL_EVALUATE_POLICY_STACK_F32) == (7, 13, 14)
    assert nat.KERNELS[16] == "policy_stack_f32" and nat.KERNELS[17] == "eval_stack_f32"
    assert nat.lib.lz_policy_stack_f32_blob_bytes() == BYTES == 50656
    assert nat.lib.lz_abi_version() == 2
    # the new family's rows sit beside the two pinned tables, not in them
    assert ("mlp_stack", "fp32") not in pol._PACKERS and set(pol._STACK_PACKERS) == {("mlp_stack", "fp32")}
    assert pol._STACK_PACKERS["mlp_stack", "fp32"] == ("lz_policy_pack_stack_f32", "lz_policy_stack_f32_blob_bytes", 7)
    assert pol._STACK_LAUNCH == {("rollout", "mlp_stack", "fp32"): "lz_stack_rollout_policy_f32",
                                 ("evaluate", "mlp_stack", "fp32"): "lz_stack_evaluate_policy_f32"}
    assert not set(pol._STACK_LAUNCH) & set(pol._LAUNCH)
    assert pol.blob_format(False, False, False, mlp_stack=True) == 7
    assert pol.blob_format(False, False, False) == nat.BLOB_MLP_F32


def _struct(sd, in_dim, act_dim):
    return pol._mlp_policy_struct(sd, in_dim, act_dim)


def test_packer_refusals_in_order():
    pack = nat.lib.lz_policy_pack_stack_f32
    err = lambda: nat.lib.lz_last_error()  # noqa: E731
    blob = np.zeros(BYTES, np.uint8)
    sd = _sd(24, 2)
    p, H, keep = _struct(sd, 24, 2)
    assert H == 64
    ok = lambda: pack(ctypes.byref(p), 64, blob.ctypes.data, blob.size)  # noqa: E731
    assert ok() == nat.LZ_OK
    # 1. the policy, 2. hidden, 3. dims, 4. pointers, 5. the blob -- lz_policy_pack_hidden's order
    assert pack(None, 0, None, 0) == nat.LZ_ERR_INVALID and b"policy is NULL" in err()
    p.obs_dim, p.pi_w1 = 25, None
    for hidden in (0, 129, -1):
        assert pack(ctypes.byref(p), hidden, None, 0) == nat.LZ_ERR_UNSUPPORTED and b"1..128" in err()
    for hidden in (128, 32, 63, 65, 1):
        assert pack(ctypes.byref(p), hidden, None, 0) == nat.LZ_ERR_UNSUPPORTED and b"64-unit" in err()
    for o, a in ((25, 2), (0, 2), (24, 0), (24, 5), (32, 2)):
        p.obs_dim, p.act_dim = o, a
        assert pack(ctypes.byref(p), 64, None, 0) == nat.LZ_ERR_UNSUPPORTED and b"1..24" in err(), (o, a)
    p.obs_dim, p.act_dim = 24, 2
    assert pack(ctypes.byref(p), 64, None, 0) == nat.LZ_ERR_INVALID and b"weight pointer" in err()
    for f in pol._FIELDS:
        q, _, keep2 = _struct(sd, 24, 2)
        setattr(q, f, None)
        assert pack(ctypes.byref(q), 64, blob.ctypes.data, blob.size) == nat.LZ_ERR_INVALID, f
        assert b"weight pointer" in err()
    p, _, keep = _struct(sd, 24, 2)
    assert pack(ctypes.byref(p), 64, None, BYTES) == nat.LZ_ERR_INVALID and b"NULL" in err()
    assert pack(ctypes.byref(p), 64, blob.ctypes.data, BYTES - 1) == nat.LZ_ERR_INVALID and b"capacity" in err()
    assert ok() == nat.LZ_OK
    # the Python packer: the same refusals as exceptions
    with pytest.raises(nat.LorenzEnvError):
        pol.pack_policy_stack_f32(_sd(25, 2), 25, 2)
    with pytest.raises(nat.LorenzEnvError):
        pol.pack_policy_stack_f32(_sd(24, 2, hidden=128), 24, 2)
    # the 128-unit packers still refuse a 24-wide input (tests/test_policy_host.py pins obs_dim > 8)
    with pytest.raises(nat.LorenzEnvError):
        pol.pack_policy_f32(sd, 24, 2)


def test_tag_is_seven_and_one_flipped_byte_is_not():
    fmt = nat.lib.lz_policy_blob_format
    blob = pol.pack_policy_stack_f32(_sd(24, 2), 24, 2)
    assert blob.dtype == np.uint8 and blob.size == BYTES
    assert fmt(blob.ctypes.data, blob.size) == 7
    tag = np.frombuffer(blob[TAG:TAG + 16].tobytes(), np.uint32)
    assert list(tag) == [0x42505A4C, 7, 7 ^ 0xFFFFFFFF, 0x42505A4C ^ 7]
    assert fmt(blob.ctypes.data, blob.size - 1) == nat.BLOB_UNKNOWN  # too small to be one
    for off in range(TAG, TAG + 16):
        bad = blob.copy()
        bad[off] ^= 1
        assert fmt(bad.ctypes.data, bad.size) == nat.BLOB_UNKNOWN, off
    # the other families' blobs are not taken for this one, nor this one for theirs
    sd8 = _sd(6, 2)
    for other in (pol.pack_policy_f32(sd8, 6, 2), pol.pack_policy_i8x4(sd8, 6, 2)):
        assert fmt(other.ctypes.data, other.size) in (nat.BLOB_MLP_F32, nat.BLOB_MLP_I8X4)
        assert fmt(other.ctypes.data, BYTES) == nat.BLOB_UNKNOWN
    big = np.zeros(300000, np.uint8)
    big[:BYTES] = blob
    assert fmt(big.ctypes.data, big.size) == 7


@pytest.mark.parametrize("in_dim,act_dim", [(24, 2), (24, 3), (1, 1), (23, 4), (6, 2)])
def test_blob_reproduces_every_weight(in_dim, act_dim):
    sd = _sd(in_dim, act_dim, seed=5 + in_dim)
    blob = pol.pack_policy_stack_f32(sd, in_dim, act_dim)
    f = np.frombuffer(blob.tobytes(), np.float32)
    used = np.zeros(BYTES // 4, bool)

    def at(byte_off, idx):
        used[byte_off // 4 + idx] = True
        return f[byte_off // 4 + idx]

    K = pol.KEYS
    nets = [(0, [sd[K[i]].numpy() for i in (0, 1, 2, 3)], sd[K[8]].numpy(), sd[K[9]].numpy(), act_dim),
            (NET, [sd[K[i]].numpy() for i in (4, 5, 6, 7)], sd[K[10]].numpy(), sd[K[11]].numpy(), 1)]
    for base, (w1, b1, w2, b2), w3, b3, rows in nets:
        for lane in range(64):
            r, h = lane & 31, lane >> 5
            for t in range(2):
                for s in range(12):  # layer 1: k-step s = input 2s + h, zero past the input width
                    k = 2 * s + h
                    want = w1[32 * t + r, k] if k < in_dim else 0.0
                    assert at(base + W1, (t * 64 + lane) * 12 + s) == want
                for q in range(32):  # layer 2: k-step q = unit 32 (q >> 4) + row(q & 15, h)
                    got = at(base + W2, ((t * 8 + q // 4) * 64 + lane) * 4 + q % 4)
                    assert got == w2[32 * t + r, 32 * (q >> 4) + _row(q & 15, h)]
        for t in range(2):
            for h in range(2):
                for g in range(16):
                    u = 32 * t + _row(g, h)
                    assert at(base + B1, (2 * t + h) * 16 + g) == b1[u]
                    assert at(base + B2, (2 * t + h) * 16 + g) == b2[u]
                    for j in range(4):
                        assert at(base + HW, (j * 2 + h) * 32 + t * 16 + g) == (w3[j, u] if j < rows else 0.0)
        for j in range(4):
            assert at(base + HB, j) == (b3[j] if j < rows else 0.0)
    # every unit of both layers was met exactly once per map: the maps are permutations
    assert sorted(_row(g, h) for g in range(16) for h in range(2)) == list(range(32))
    # pack_gauss's 16 Normal constants: log_std, exp, 2 exp^2, log exp -- and bit for bit what
    # the float32 MlpPolicy's packer writes for the same log_std
    ls = sd["log_std"].numpy()
    sc = np.exp(ls.astype(np.float64))
    want = np.zeros(16)
    want[0:act_dim], want[4:4 + act_dim] = ls, sc
    want[8:8 + act_dim], want[12:12 + act_dim] = 2.0 * sc * sc, ls
    got = np.array([at(LOGSTD, j) for j in range(16)])
    assert np.array_equal(got[:4], want[:4].astype(np.float32)) and np.allclose(got, want, rtol=1e-6, atol=1e-7)
    small = _sd(6, act_dim)
    small["log_std"] = sd["log_std"]
    ref = pol.pack_policy_f32(small, 6, act_dim)
    assert np.array_equal(blob[LOGSTD:LOGSTD + 64], ref[F32_TANH - 64:F32_TANH])
    # the tanh table: the float32 MlpPolicy blob's, byte for byte
    assert np.array_equal(blob[TANH:], ref[F32_TANH:F32_TANH + 73 * 32])
    used[TANH // 4:] = True
    used[TAG // 4:TAG // 4 + 4] = True
    assert not f[~used].view(np.uint32).any()  # nothing else is written


class _Seam(pol._PolicySeam):
    def __init__(self, frame_stack, O=6, A=2, obs_rms=None):
        self.O, self.A, self.obs_rms = O, A, obs_rms
        self._init_frame_stack(frame_stack)


def test_seam_selects_the_family_and_keeps_its_refusals():
    s = _Seam(4)
    s._select(_sd(24, 2))
    assert s.mlp_stack and s.family == "mlp_stack" and not (s.attention or s.attention_ln)
    blob = s._pack_params(_sd(24, 2), "fp32")
    assert blob.size == BYTES and nat.lib.lz_policy_blob_format(blob.ctypes.data, blob.size) == 7
    assert np.array_equal(blob, pol.pack_policy_stack_f32(_sd(24, 2), 24, 2))
    # every other frame-stacked MlpPolicy keeps the refusal it had
    for sd in (_sd(24, 2, hidden=128), _sd(6, 2), _sd(6, 2, hidden=128), _sd(24, 2, hidden=32)):
        with pytest.raises(ValueError, match="LayerNorm attention extractor"):
            _Seam(4)._select(sd)
    with pytest.raises(ValueError, match="LayerNorm attention extractor"):
        _Seam(4)._select(pol.ActorCriticAttn(6, 2, seed=0).state_dict())
    ln = _Seam(4)
    ln._select(pol.ActorCriticAttn(24, 2, seed=0, layer_norm=True).state_dict())
    assert ln.attention_ln and not ln.mlp_stack and ln.family == "attn_ln"
    one = _Seam(1)
    one._select(_sd(6, 2))
    assert one.family == "mlp" and not one.mlp_stack
    with pytest.raises(ValueError, match="no VecNormalize"):
        _Seam(4, obs_rms=object())
    with pytest.raises(ValueError, match="frame_stack must be 1 or 4"):
        _Seam(2)
    # the collector: fp32 only
    col = pol.FusedRolloutCollector.__new__(pol.FusedRolloutCollector)
    col.O, col.A, col.obs_rms, col.frame_stack, col.vecnorm_update = 6, 2, None, 4, None
    for prec in ("bf16", "i8x4"):
        col.precision = prec
        with pytest.raises(ValueError, match="precision='fp32' only"):
            col.set_params(_sd(24, 2))
    # the evaluator: no traced form
    ev = pol.FusedEvaluator.__new__(pol.FusedEvaluator)
    ev.mlp_stack = True
    with pytest.raises(ValueError, match="no traced form"):
        ev.evaluate(4, trace=[0])


def test_wide_functions_values_and_refusals():
    count, ws = nat.lib.lz_ppo_param_count_wide, nat.lib.lz_ppo_workspace_bytes_wide
    P = 2 * (64 * 24 + 64 + 64 * 64 + 64) + 2 * 64 + 2 + 64 + 1 + 2
    assert count(24, 2, 64) == P == 11717
    for O, A in ((1, 1), (6, 2), (8, 4), (9, 2), (24, 4)):
        assert count(O, A, 64) == 2 * (64 * O + 64 + 64 * 64 + 64) + A * 64 + A + 64 + 1 + A
    assert count(6, 2, 64) == nat.lib.lz_a2c_param_count_hidden(6, 2, 64)
    for bad in ((0, 2, 64), (25, 2, 64), (24, 0, 64), (24, 5, 64), (24, 2, 128), (24, 2, 32), (6, 2, 128)):
        assert count(*bad) == -1, bad
    slot = (P + 6) * 8
    assert ws(1, 24, 2, 64, 0) == slot
    assert ws(111, 24, 2, 64, 0) == 4 * slot
    assert ws(5155, 24, 2, 64, 3) == 3 * slot
    assert ws(65536, 24, 2, 64, 0) == 128 * slot
    assert ws(64, 6, 2, 64, 0) == nat.lib.lz_ppo_workspace_bytes_hidden(64, 6, 2, 64, 0)
    for bad in ((0, 24, 2, 64, 0), (10, 0, 2, 64, 0), (10, 25, 2, 64, 0), (10, 24, 5, 64, 0),
                (10, 24, 2, 128, 0), (10, 24, 2, 64, -1), (10, 24, 2, 64, 4097)):
        assert ws(*bad) == -1, bad
    # the _hidden entry points keep refusing a wide input
    assert nat.lib.lz_a2c_param_count_hidden(9, 2, 64) == -1
    assert nat.lib.lz_ppo_workspace_bytes_hidden(10, 9, 2, 64, 0) == -1


_PTRS = ("params", "observations", "actions", "advantages", "returns", "old_log_prob", "workspace", "grad_sums")


def _grad_args(keep):
    """Valid-looking arguments (never dereferenced: every case below is refused first)."""
    g = nat.LzPpoGradArgs()
    fake = ctypes.c_void_p(0x1000)
    for f in _PTRS + ("indices", "old_values", "adv_moments", "ctrl"):
        setattr(g, f, fake)
    g.n_samples, g.n_rows, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 333, 24, 2, 64, 0
    g.vf_coef, g.ent_coef, g.clip_range, g.clip_range_vf = 0.5, 0.0, 0.2, 0.05
    g.workspace_bytes = nat.lib.lz_ppo_workspace_bytes_wide(111, 24, 2, 64, 0)
    keep.append(g)
    return g


def test_wide_grad_refusals_need_no_gpu():
    keep = []
    call = lambda g: nat.lib.lz_ppo_grad_wide_f32(ctypes.byref(g), 0, None)  # noqa: E731
    err = lambda: nat.lib.lz_last_error()  # noqa: E731
    assert nat.lib.lz_ppo_grad_wide_f32(None, 0, None) == nat.LZ_ERR_INVALID
    for f in _PTRS:
        g = _grad_args(keep)
        setattr(g, f, None)
        assert call(g) == nat.LZ_ERR_INVALID and b"NULL" in err(), f
    g = _grad_args(keep)
    g.old_values = None
    assert call(g) == nat.LZ_ERR_INVALID and b"old_values" in err()
    for f, v in (("obs_dim", 0), ("obs_dim", 25), ("act_dim", 0), ("act_dim", 5), ("n_samples", 0),
                 ("n_rows", 0), ("max_workgroups", -1), ("max_workgroups", 4097), ("clip_range", -0.1),
                 ("clip_range", float("nan")), ("clip_range_vf", float("inf"))):
        g = _grad_args(keep)
        setattr(g, f, v)
        assert call(g) == nat.LZ_ERR_INVALID, (f, v)
    g = _grad_args(keep)
    g.obs_dim = 25
    assert call(g) == nat.LZ_ERR_INVALID and b"1..24" in err()
    # hidden after the dims (and the rest of the argument checks), as lz_ppo_grad_hidden_f32
    for hidden in (128, 32, 0):
        g = _grad_args(keep)
        g.hidden = hidden
        assert call(g) == nat.LZ_ERR_UNSUPPORTED and b"hidden must be 64" in err(), hidden
        g.obs_dim = 25
        assert call(g) == nat.LZ_ERR_INVALID and b"1..24" in err()
    g = _grad_args(keep)
    g.workspace_bytes -= 1
    assert call(g) == nat.LZ_ERR_INVALID and b"lz_ppo_workspace_bytes_wide" in err()
    # lz_ppo_grad_hidden_f32 keeps refusing obs_dim 9 where it did
    g = _grad_args(keep)
    g.obs_dim = 9
    assert nat.lib.lz_ppo_grad_hidden_f32(ctypes.byref(g), 0, None) == nat.LZ_ERR_INVALID
    assert b"1..8" in err()


class _FakeCollector:
    precision = None
    frame_stack = 4
    O, A, n = 6, 2, 4
    device = torch.device("cpu")

    def set_params(self, sd):
        self.sd = sd


def test_fused_ppo_on_a_frame_stacked_collector():
    col = _FakeCollector()
    sd = _sd(24, 2, seed=9)
    ppo = pol.FusedPPO(col, sd, net_arch=64)
    assert ppo.wide and ppo.hidden == 64 and (ppo.O, ppo.A) == (24, 2)
    assert ppo.P == ppo.params.numel() == 11717 == nat.lib.lz_ppo_param_count_wide(24, 2, 64)
    assert ppo._sums.numel() == 11717 + 6
    assert ppo._workspace_need("ppo", 64) == 2 * (11717 + 6)
    back = ppo.state_dict()
    assert set(back) == set(pol.KEYS)
    for k in pol.KEYS:
        assert back[k].dtype == torch.float32 and torch.equal(back[k], sd[k]), k
        assert torch.equal(col.sd[k], sd[k])  # what the collector was given to pack
    assert tuple(back[pol.KEYS[0]].shape) == (64, 24)
    # ... and what it packs is the stacked blob
    assert np.array_equal(pol.pack_policy_stack_f32(col.sd, 24, 2), pol.pack_policy_stack_f32(sd, 24, 2))
    # every other combination keeps its refusal (tests/test_ppo_host.py:269-271 pins the first two)
    for arch in (None, 128):
        with pytest.raises(ValueError, match="frame_stack"):
            pol.FusedPPO(col, sd, net_arch=arch)
    with pytest.raises(ValueError, match="frame_stack"):
        pol.FusedA2C(col, sd, net_arch=64)
    with pytest.raises(ValueError, match="hidden=64"):
        pol.FusedPPO(col, _sd(6, 2), net_arch=64)  # an unstacked layer 1 on a stacked collector
    col.frame_stack = 1
    flat = pol.FusedPPO(col, _sd(6, 2), net_arch=64)
    assert not flat.wide and flat.O == 6 and flat.P == nat.lib.lz_a2c_param_count_hidden(6, 2, 64)
