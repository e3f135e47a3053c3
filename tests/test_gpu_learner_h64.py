"""The 64-unit gradient kernels (k_a2c_grad_h64, k_ppo_grad_h64 through
lz_a2c_grad_hidden_f32 / lz_ppo_grad_hidden_f32) and FusedA2C / FusedPPO(net_arch=64) on the
MI355X.

Two independent pins.  (1) The padded twin, with no tolerance: the 64-unit launch equals the
128-unit launch on the zero-padded net, value for value, at the 64-unit entries and in the
tail, and the padded entries of the 128-unit result are exactly 0 -- a padded unit adds exact
zeros to every chain, and tiles, flushes and slots are the same.  (2) torch float64 CPU
autograd of the 64-unit net, by the criterion of test_gpu_a2c / test_gpu_ppo,

    err_gpu <= RATIO * max(err_t32, 2^-24)

per tensor (all 13, each with ||g64|| > 0), for the whole vector and for the loss sums, with
RATIO twice the worst ratio measured over every case below, both shipped reference policies
and three seeds (tools/learner_h64_grad_error.py -> profiles/learner_h64/grad_error.json).
A2C: 11.025, the layer-1 bias of the vf net at B = 2085 on one workgroup per net, a sequential
float32 sum over 2048 samples where torch sums pairwise.  PPO: 24.061, the kl sum of the
shipped Lorenz policy (seed 2), sum((ratio - 1) - log_ratio) for an old policy 0.002 away
(every term the small difference of two float32 numbers near 0); the next one is 8.12.  The
whole-vector ratio is below 1.3 everywhere."""
import numpy as np
import pytest
import torch

import a2c_ref
import mlp_learner_ref as ref
import ppo_ref
import gym_lorenz as gl
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol
from gym_lorenz.vec_normalize import DeviceRunningMeanStd

pytestmark = pytest.mark.gpu

RATIO = {"a2c": 2 * 11.025, "ppo": 2 * 24.061}  # grad_error.json: worst_ratio_a2c, worst_ratio_ppo
DEV = torch.device("cuda", 0)
LR = 3e-4
NAMES = [c[0] for c in ref.CASES]
_CACHE = {}


def _case(kind, label, **kw):
    """A case (seed 0) with its two CPU references, built once and left unchanged."""
    key = (kind, label) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        if label.startswith("shipped_"):
            c = ref.shipped_case(kind, label[len("shipped_"):], 0)
        else:
            row = next(r for r in ref.CASES if r[0] == label)
            c = (ref.a2c_case if kind == "a2c" else ref.ppo_case)(row, 0, **kw)
        cpu = ref.cpu_a2c if kind == "a2c" else ref.cpu_ppo
        c["g64"], c["g32"] = cpu(c, torch.float64), cpu(c, torch.float32)
        _CACHE[key] = c
    return _CACHE[key]


def _gpu(kind, c, hidden=64, **kw):
    return (ref.gpu_a2c if kind == "a2c" else ref.gpu_ppo)(pol, DEV, c, hidden, **kw)


def _check_twin(kind, c, got64, got128):
    """got64 == got128 at the 64-unit entries and in the tail; the padded entries are 0."""
    O, A = c["O"], c["A"]
    idx = ref.unpadded_index(O, A)
    P64, P128 = ref.layout(O, A, 64)[1], ref.layout(O, A, 128)[1]
    tail = 4 if kind == "a2c" else 6
    assert got64.size == P64 + tail and got128.size == P128 + tail
    assert ref.same_values(got64[:P64], got128[idx]), (
        c["name"], int((got64[:P64] != got128[idx]).sum()), float(np.abs(got64[:P64] - got128[idx]).max()))
    assert ref.same_values(got64[P64:], got128[P128:]), (got64[P64:], got128[P128:])
    rest = np.ones(P128, bool)
    rest[idx] = False
    assert not got128[:P128][rest].any()
    assert np.abs(got64[:P64]).max() > 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_padded_twin_is_value_equal(kind, name):
    c = _case(kind, name)
    _check_twin(kind, c, _gpu(kind, c).cpu().numpy(), _gpu(kind, c, 128).cpu().numpy())


@pytest.mark.parametrize("M", [70, 64])
def test_padded_twin_ppo_minibatch_sizes(M):
    """A ragged 70-row and the reference's 64-row minibatch, gathered from the 254 rows."""
    c = _case("ppo", "b111", M=M)
    got = _gpu("ppo", c).cpu().numpy()
    assert got[-3] == M
    _check_twin("ppo", c, got, _gpu("ppo", c, 128).cpu().numpy())


def test_padded_twin_ppo_with_an_out_of_range_index():
    """One index past the arrays (value clipping and the entropy term on; no normalisation,
    whose moments would be NaN by contract): the three loss sums are NaN in both forms (NaNs
    compare equal), the gradient is finite and still the twin's."""
    c = _case("ppo", "b111")
    idx = c["idx"].clone()
    idx[70] = c["n_rows"]
    idx = idx.to(DEV)
    got = _gpu("ppo", c, idx=idx, normalize=False).cpu().numpy()
    P = got.size - 6
    assert np.isnan(got[P:P + 3]).all() and np.isfinite(got[:P]).all() and got[P + 3] == c["M"]
    _check_twin("ppo", c, got, _gpu("ppo", c, 128, idx=idx, normalize=False).cpu().numpy())
    again = _gpu("ppo", c).cpu().numpy()
    assert np.isfinite(again).all()


def test_hidden_128_through_the_hidden_entry_points_is_the_old_launch():
    """lz_*_grad_hidden_f32 at hidden = 128 launches the same kernels: the same bits."""
    import ctypes

    c = _case("a2c", "b111")
    sd = ref.pad_to_128(c["sd"])
    flat = a2c_ref.flatten(sd).to(DEV)
    batch = [t.to(DEV) for t in c["batch"]]
    old = pol.a2c_grad(flat, *batch, 6, 2, 0.5, 0.01)
    P = flat.numel()
    need = int(nat.lib.lz_a2c_workspace_bytes_hidden(111, 6, 2, 128, 0))
    ws = torch.empty((need // 8,), dtype=torch.float64, device=DEV)
    out = torch.empty((P + 4,), dtype=torch.float64, device=DEV)
    g = nat.LzA2cGradArgs()
    g.params, g.observations, g.actions, g.advantages, g.returns = [t.data_ptr() for t in [flat] + batch]
    g.n_samples, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, 6, 2, 128, 0
    g.vf_coef, g.ent_coef = 0.5, 0.01
    g.workspace, g.workspace_bytes, g.grad_sums = ws.data_ptr(), need, out.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    nat.check(nat.lib.lz_a2c_grad_hidden_f32(ctypes.byref(g), 0, stream))
    torch.cuda.synchronize()
    assert torch.equal(old.view(torch.int64), out.view(torch.int64))


def _check_accuracy(kind, c, got, what):
    slices, P = ref.slices(kind, c["O"], c["A"])
    assert len(slices) == 13 + (4 if kind == "a2c" else 5)
    for k, (e_gpu, e_t32, ratio) in ref.accuracy_rows(got, c["g64"], c["g32"], slices).items():
        print("%s %s %s %s: err_gpu %.3e err_t32 %.3e ratio %.2f" % (what, kind, c["name"], k, e_gpu, e_t32, ratio))
        assert e_gpu <= RATIO[kind] * max(e_t32, a2c_ref.ERR_FLOOR), (what, k, e_gpu, e_t32)
    assert got[P + 3] == (c["B"] if kind == "a2c" else c["M"])
    if kind == "ppo":
        assert got[P + 4] == c["g64"][P + 4]  # the clipped count


@pytest.mark.parametrize("name", NAMES + ["shipped_hr", "shipped_lorenz"])
@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_gradient_and_sums_match_float64_autograd(kind, name):
    c = _case(kind, name)
    _check_accuracy(kind, c, _gpu(kind, c).cpu().numpy(), "grad")


@pytest.mark.parametrize("name", ["b111", "b5155_cap3", "b2085_cap1"])
@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_two_launches_are_bit_identical(kind, name):
    c = _case(kind, name)
    n = c["B"] if kind == "a2c" else c["M"]
    fn = getattr(nat.lib, "lz_%s_workspace_bytes_hidden" % kind)
    need = int(fn(n, c["O"], c["A"], 64, c["cap"])) // 8
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)
    a = _gpu(kind, c, workspace=ws).clone()
    ws.fill_(float("nan"))  # the second launch must not read what the first one left
    b = _gpu(kind, c, workspace=ws)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert bool(torch.isfinite(b).all())


@pytest.mark.parametrize("name", ["b111", "b5155_cap3"])
def test_half_batches_add_up(name):
    """What the all-reduce relies on: the sums of two half batches, added in float64, are the
    whole batch's sums within the accuracy bound."""
    c = _case("a2c", name)
    B = c["B"]
    cut = B // 2 + 3  # both halves ragged
    lo = _gpu("a2c", c, rows=slice(0, cut)).cpu().numpy()
    hi = _gpu("a2c", c, rows=slice(cut, B)).cpu().numpy()
    assert lo[-1] == cut and hi[-1] == B - cut
    _check_accuracy("a2c", c, lo + hi, "halves")


def test_lanes_past_the_last_sample_add_nothing():
    """A batch of 33 (one full tile and one lane of the next) given as the leading rows of the
    111-row buffers: the 31 idle lanes of the second tile must not read the rows behind them
    as samples, nor add their biases' share."""
    c = _case("a2c", "b111")
    O, A = c["O"], c["A"]
    flat = a2c_ref.flatten(c["sd"]).to(DEV)
    obs, act, adv, ret = [t.to(DEV) for t in c["batch"]]
    small = pol.a2c_grad(flat, obs[:33], act[:33], adv[:33], ret[:33], O, A, 0.5, 0.01, hidden=64).cpu().numpy()
    batch = tuple(t[:33].contiguous() for t in c["batch"])
    g64 = a2c_ref.grad_sums(c["sd"], batch, 0.5, 0.01)
    g32 = a2c_ref.grad_sums(c["sd"], batch, 0.5, 0.01, dtype=torch.float32)
    P = g64.size - 4
    assert small[P + 3] == 33
    assert a2c_ref.rel_err(small[:P], g64[:P]) <= RATIO["a2c"] * max(a2c_ref.rel_err(g32[:P], g64[:P]),
                                                                     a2c_ref.ERR_FLOOR)
    # and it is exactly the launch on buffers that end after row 33
    alone = pol.a2c_grad(flat, *[t.to(DEV) for t in batch], O, A, 0.5, 0.01, hidden=64).cpu().numpy()
    assert np.array_equal(small.view(np.int64), alone.view(np.int64))


@pytest.mark.parametrize("max_grad_norm,adv_scale", [(0.5, 50.0), (100.0, 1.0)])
def test_a2c_apply_on_9413_params_is_the_float64_step_within_one_ulp(max_grad_norm, adv_scale):
    c = _case("a2c", "b111")
    O, A, B = c["O"], c["A"], c["B"]
    obs, act, adv, ret = [t.to(DEV) for t in c["batch"]]
    adv = (adv * adv_scale).contiguous()
    params = a2c_ref.flatten(c["sd"]).to(DEV)
    assert params.numel() == 9413
    sq = torch.ones_like(params)
    lr = 7e-4
    for step in range(2):
        sums = pol.a2c_grad(params, obs, act, adv, ret, O, A, 0.5, 0.01, hidden=64)
        p0, s0 = params.cpu().numpy(), sq.cpu().numpy()
        stats = pol.a2c_apply(sums, params, sq, lr, max_grad_norm, 0.99, 1e-5, 0.5, 0.01).cpu().numpy()
        h = sums.cpu().numpy()
        p_ref, s_ref, total, coef = a2c_ref.apply_step(h, p0, s0, lr, max_grad_norm)
        assert (coef < 1.0) == (max_grad_norm == 0.5), (total, coef)
        assert a2c_ref.ulp_diff(params.cpu().numpy(), p_ref) <= 1, step
        assert a2c_ref.ulp_diff(sq.cpu().numpy(), s_ref) <= 1, step
        assert not np.array_equal(params.cpu().numpy(), p0)
        P = h.size - 4
        pl, vl, el = h[P] / B, h[P + 1] / B, h[P + 2] / B
        np.testing.assert_allclose(stats, [pl, vl, el, pl + 0.01 * el + 0.5 * vl, total, coef, B, lr], rtol=1e-12)
    assert float(sq.min()) < 1.0  # it moved


def _state(c):
    flat = a2c_ref.flatten(c["sd"]).to(DEV)
    P = flat.numel()
    return dict(params=flat, m=torch.zeros((P,), device=DEV), v=torch.zeros((P,), device=DEV),
                ctrl=torch.zeros((2,), dtype=torch.int64, device=DEV))


def _snapshot(s):
    return {k: s[k].clone() for k in ("params", "m", "v", "ctrl")}


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("params", "m", "v", "ctrl"))


@pytest.mark.parametrize("max_grad_norm,adv_scale", [(0.5, 50.0), (100.0, 1.0)])
def test_adam_apply_on_9413_params_is_the_float64_step_within_one_ulp(max_grad_norm, adv_scale):
    c = _case("ppo", "b111")
    O, A, M = c["O"], c["A"], c["M"]
    rows = [t.to(DEV) for t in c["rows"]]
    rows[2] = (rows[2] * adv_scale).contiguous()
    idx = c["idx"].to(DEV)
    s = _state(c)
    assert s["params"].numel() == 9413
    vf, ent = 0.5, 0.01
    for step in range(2):
        sums = pol.ppo_grad(s["params"], *rows, O, A, idx, ppo_ref.CLIP, ppo_ref.CLIP_VF, None, s["ctrl"], vf, ent,
                            hidden=64)
        p0, m0, v0 = (s[k].cpu().numpy() for k in ("params", "m", "v"))
        stats = pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], LR, max_grad_norm, vf_coef=vf,
                               ent_coef=ent).cpu().numpy()
        h = sums.cpu().numpy()
        p_ref, m_ref, v_ref, total, coef = ppo_ref.adam_step(h, p0, m0, v0, step, LR, max_grad_norm)
        assert (coef < 1.0) == (max_grad_norm == 0.5), (total, coef)
        assert a2c_ref.ulp_diff(s["params"].cpu().numpy(), p_ref) <= 1, step
        assert a2c_ref.ulp_diff(s["m"].cpu().numpy(), m_ref) <= 1, step
        assert a2c_ref.ulp_diff(s["v"].cpu().numpy(), v_ref) <= 1, step
        assert not np.array_equal(s["params"].cpu().numpy(), p0)
        P = h.size - 6
        pl, vl, el = h[P] / M, h[P + 1] / M, h[P + 2] / M
        want = [pl, vl, el, pl + ent * el + vf * vl, total, coef, M, LR, h[P + 4] / M, h[P + 5] / M, step + 1, 0]
        np.testing.assert_allclose(stats, want, rtol=1e-12)
    assert s["ctrl"].tolist() == [2, 0]


def test_target_kl_stops_on_the_device():
    """As test_gpu_ppo's: two minibatches of 100 of the 254 rows, the second one's
    old_log_prob moved so that 1.5 target_kl sits between the two approx_kl with a factor of
    two of room on both sides (asserted on the CPU reference).  Step 1 is taken; minibatch 2
    and a third call change nothing and say `stopped`; after the flag is cleared the next call
    steps."""
    c = _case("ppo", "b111")
    O, A, n_rows = c["O"], c["A"], c["n_rows"]
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(11)).to(torch.int32)
    mb = [perm[:100].contiguous(), perm[100:200].contiguous()]
    rows_cpu = list(c["rows"])
    old_lp = rows_cpu[4].clone()
    old_lp[mb[1].long()] += 0.8 * torch.randn(100, generator=torch.Generator().manual_seed(12))
    rows_cpu[4] = old_lp
    kw = dict(normalize=True, cvf=ppo_ref.CLIP_VF, ent_coef=0.0)
    take = lambda i: tuple(t[mb[i].long()] for t in rows_cpu)  # noqa: E731
    g1 = ppo_ref.grad_sums(c["sd"], take(0), **kw)
    P = g1.size - 6
    p0 = a2c_ref.flatten(c["sd"]).numpy()
    p1 = ppo_ref.adam_step(g1, p0, np.zeros(P, np.float32), np.zeros(P, np.float32), 0, LR)[0]
    g2 = ppo_ref.grad_sums(ref.unflatten(torch.from_numpy(p1), O, A, 64), take(1), **kw)
    kl1, kl2 = g1[P + 5] / 100, g2[P + 5] / 100
    thr = float(np.sqrt(kl1 * kl2))
    assert 0 < 2 * kl1 <= thr <= kl2 / 2, (kl1, kl2)
    target_kl = thr / 1.5

    rows = [t.to(DEV) for t in rows_cpu]
    idx = [m.to(DEV) for m in mb]
    s = _state(c)
    stats = torch.zeros((4, 12), dtype=torch.float64, device=DEV)

    def step(i, row):
        mom = pol.ppo_adv_moments(rows[2], idx[i])
        sums = pol.ppo_grad(s["params"], *rows, O, A, idx[i], ppo_ref.CLIP, ppo_ref.CLIP_VF, mom, s["ctrl"],
                            hidden=64)
        pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], LR, target_kl=target_kl, stats=stats[row])

    before = _snapshot(s)
    step(0, 0)
    after1 = _snapshot(s)
    assert not torch.equal(after1["params"], before["params"]) and after1["ctrl"].tolist() == [1, 0]
    step(1, 1)  # approx_kl > 1.5 target_kl: sets the flag, steps nothing
    after2 = _snapshot(s)
    assert after2["ctrl"].tolist() == [1, 1]
    after2["ctrl"][1] = 0
    assert _same_bits(after1, after2)
    step(0, 2)  # the flag is set: a no-op whatever the minibatch
    assert s["ctrl"].tolist() == [1, 1]
    s["ctrl"][1] = 0
    assert _same_bits(after1, _snapshot(s))
    step(0, 3)  # the flag cleared: steps again
    assert s["ctrl"].tolist() == [2, 0] and not torch.equal(s["params"], after1["params"])
    st = stats.cpu().numpy()
    col = nat.PPO_STATS.index
    assert st[:, col("stopped")].tolist() == [0, 1, 1, 0] and st[:, col("step")].tolist() == [1, 1, 1, 2]
    assert st[0, col("approx_kl")] == pytest.approx(kl1, rel=1e-3) and st[0, col("approx_kl")] <= thr / 2
    assert st[1, col("approx_kl")] == pytest.approx(kl2, rel=1e-2) and st[1, col("approx_kl")] >= 2 * thr
    assert np.isfinite(st[1, :4]).all() and np.isnan(st[1, col("grad_norm")])
    assert np.isnan(st[2, :7]).all() and st[2, col("lr")] == LR


def test_out_of_range_indices_are_not_read():
    """Index -1, n_rows and the int32 extremes, the row arrays being interior views of larger
    tensors (so that even an unguarded read would stay inside owned memory), without
    normalisation as in test_gpu_ppo: the three loss sums are NaN, the gradient is finite, the
    moments are NaN; a call with valid indices afterwards is what it was before."""
    c = _case("ppo", "b111")
    M, n_rows = c["M"], c["n_rows"]
    pad = 64
    inside = []
    for t in c["rows"]:
        big = torch.full((n_rows + 2 * pad,) + tuple(t.shape[1:]), 3.0, dtype=t.dtype, device=DEV)
        big[pad:pad + n_rows] = t.to(DEV)
        inside.append(big[pad:pad + n_rows])
    assert all(r.is_contiguous() and r.data_ptr() != r.untyped_storage().data_ptr() for r in inside)
    cc = dict(c, rows=tuple(inside))
    good = _gpu("ppo", cc, normalize=False).clone()
    P = good.numel() - 6
    for bad_value, where in ((-1, 5), (n_rows, 70), (2 ** 31 - 1, 110), (-2 ** 31, 0)):
        idx = c["idx"].clone().to(DEV)
        idx[where] = bad_value
        got = _gpu("ppo", cc, idx=idx, normalize=False).cpu().numpy()
        assert np.isnan(got[P:P + 3]).all(), (bad_value, got[P:])
        assert np.isfinite(got[:P]).all() and got[P + 3] == M
        assert np.isnan(pol.ppo_adv_moments(inside[2], idx).cpu().numpy()).all()
    again = _gpu("ppo", cc, normalize=False)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(again.view(torch.int64), good.view(torch.int64))
    assert torch.equal(good.view(torch.int64), _gpu("ppo", c, normalize=False).view(torch.int64))


def _replay_equals_eager(make_state, step, keys):
    a, b = make_state(), make_state()
    for _ in range(3):
        step(a)
    step(b)
    torch.cuda.synchronize()
    after_one = b["params"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        step(b)
    torch.cuda.synchronize()
    assert torch.equal(b["params"], after_one)  # captured, not run
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert not torch.equal(b["params"], after_one)


def test_captured_a2c_step_replays_equal_eager_calls():
    """grad + apply captured after one eager call and replayed twice == three eager calls."""
    c = _case("a2c", "b111")
    O, A, B = c["O"], c["A"], c["B"]
    batch = [t.to(DEV) for t in c["batch"]]
    P = int(nat.lib.lz_a2c_param_count_hidden(O, A, 64))
    need = int(nat.lib.lz_a2c_workspace_bytes_hidden(B, O, A, 64, 0)) // 8

    def state():
        return dict(params=a2c_ref.flatten(c["sd"]).to(DEV), sq=torch.ones((P,), device=DEV),
                    ws=torch.empty((need,), dtype=torch.float64, device=DEV),
                    sums=torch.empty((P + 4,), dtype=torch.float64, device=DEV),
                    stats=torch.empty((8,), dtype=torch.float64, device=DEV))

    def step(s):
        pol.a2c_grad(s["params"], *batch, O, A, 0.5, 0.0, workspace=s["ws"], out=s["sums"], hidden=64)
        pol.a2c_apply(s["sums"], s["params"], s["sq"], 7e-4, 0.5, stats=s["stats"])

    _replay_equals_eager(state, step, ("params", "sq", "sums", "stats"))


def test_captured_ppo_step_replays_equal_eager_calls():
    """moments + grad + apply on the 111-row minibatch, as the A2C one."""
    c = _case("ppo", "b111")
    O, A, M = c["O"], c["A"], c["M"]
    rows = [t.to(DEV) for t in c["rows"]]
    idx = c["idx"].to(DEV)
    need = int(nat.lib.lz_ppo_workspace_bytes_hidden(M, O, A, 64, 0)) // 8

    def state():
        s = _state(c)
        P = s["params"].numel()
        s.update(ws=torch.empty((need,), dtype=torch.float64, device=DEV),
                 sums=torch.empty((P + 6,), dtype=torch.float64, device=DEV),
                 mom=torch.empty((2,), dtype=torch.float64, device=DEV),
                 stats=torch.zeros((12,), dtype=torch.float64, device=DEV))
        return s

    def step(s):
        pol.ppo_adv_moments(rows[2], idx, out=s["mom"])
        pol.ppo_grad(s["params"], *rows, O, A, idx, ppo_ref.CLIP, ppo_ref.CLIP_VF, s["mom"], s["ctrl"], 0.5, 0.01,
                     workspace=s["ws"], out=s["sums"], hidden=64)
        pol.adam_apply(s["sums"], s["params"], s["m"], s["v"], s["ctrl"], LR, 0.5, vf_coef=0.5, ent_coef=0.01,
                       stats=s["stats"])

    _replay_equals_eager(state, step, ("params", "m", "v", "ctrl", "sums", "stats"))


def _collector_runs(sd, col, n):
    """The collector's blob is the packer's image of `sd`."""
    twin = gl.BatchedEnv("pmsm", n, seed=9)
    fresh = pol.FusedRolloutCollector(twin, sd, deterministic=True, precision="fp32")
    same = torch.equal(fresh.blob, col.blob)
    twin.close()
    return same


def test_fused_a2c_net_arch_64_learn_equals_the_wrappers():
    """PMSM, 96 envs, n_steps = 5, VecNormalize on, three updates through
    FusedA2C(net_arch=64).learn: each one is a2c_grad(hidden=64) + a2c_apply on its batch from
    the parameters before it, bit for bit; afterwards the collector carries the weights."""
    n, K = 96, 5
    env = gl.BatchedEnv("pmsm", n, seed=5)
    rms = DeviceRunningMeanStd(6, env.device)
    col = pol.FusedRolloutCollector(env, None, obs_rms=rms, training=True, precision="fp32")
    sd0 = ref.make_policy(6, 2, 4)
    sched = pol.linear_schedule(0.0005)
    a2c = pol.FusedA2C(col, sd0, learning_rate=sched, n_steps=K, net_arch=64)
    assert a2c.P == 9413 and _collector_runs(sd0, col, n)
    prev = {"p": a2c.params.clone(), "s": a2c.square_avg.clone()}
    seen = []

    def check(model, batch, stats):
        i = len(seen)
        lr = sched(1.0 - (i + 1) / 3.0)
        p, s = prev["p"].clone(), prev["s"].clone()
        sums = pol.a2c_grad(p, batch.observations, batch.actions, batch.advantages, batch.returns, 6, 2, 0.5, 0.0,
                            hidden=64)
        st = pol.a2c_apply(sums, p, s, lr, 0.5, 0.99, 1e-5, 0.5, 0.0).cpu().tolist()
        assert torch.equal(p.view(torch.int32), model.params.view(torch.int32))
        assert torch.equal(s.view(torch.int32), model.square_avg.view(torch.int32))
        assert torch.equal(sums.view(torch.int64), model._sums.view(torch.int64))
        assert stats == dict(zip(nat.A2C_STATS, st))
        assert all(np.isfinite(v) for v in stats.values())
        assert stats["n_samples"] == K * n and stats["lr"] == pytest.approx(lr, rel=1e-15)
        prev["p"], prev["s"] = model.params.clone(), model.square_avg.clone()
        seen.append(stats)

    out = a2c.learn(3 * K * n, callback=check)
    assert len(out) == len(seen) == 3 and a2c.num_timesteps == 3 * K * n
    assert not torch.equal(a2c.params.cpu(), a2c_ref.flatten(sd0))
    back = a2c.state_dict()
    assert tuple(back["mlp_extractor.policy_net.2.weight"].shape) == (64, 64)
    assert _collector_runs(back, col, n)
    env.close()


def test_fused_ppo_net_arch_64_learn_equals_the_wrappers():
    """PMSM, 96 envs, n_steps = 8 (768 rows), batch_size = 64, n_epochs = 2, two updates
    through FusedPPO(net_arch=64).learn with a seeded device generator: a loop over the
    wrappers with hidden=64, on each update's batch, from the state before it, with the
    randperm draws of an equally seeded generator, gives the same bits."""
    n, K, bs, n_epochs = 96, 8, 64, 2
    B = n * K
    env = gl.BatchedEnv("pmsm", n, seed=5)
    rms = DeviceRunningMeanStd(6, env.device)
    col = pol.FusedRolloutCollector(env, None, obs_rms=rms, training=True, precision="fp32")
    sd0 = ref.make_policy(6, 2, 4)
    gen = torch.Generator(device=DEV).manual_seed(123)
    twin_gen = torch.Generator(device=DEV).manual_seed(123)
    ppo = pol.FusedPPO(col, sd0, learning_rate=LR, n_steps=K, batch_size=bs, n_epochs=n_epochs, ent_coef=0.01,
                       generator=gen, net_arch=[64, 64])
    assert ppo.P == 9413 and _collector_runs(sd0, col, n)
    prev = {"params": ppo.params.clone(), "m": ppo.exp_avg.clone(), "v": ppo.exp_avg_sq.clone(),
            "ctrl": ppo.ctrl.clone()}
    seen = []

    def check(model, batch, out):
        i = len(seen)
        s = {k: v.clone() for k, v in prev.items()}
        stats = torch.zeros((n_epochs * (B // bs), 12), dtype=torch.float64, device=DEV)
        flat = (batch.observations, batch.actions, batch.advantages, batch.returns, batch.log_probs, batch.values)
        row = 0
        for _ in range(n_epochs):
            perm = torch.randperm(B, dtype=torch.int32, device=DEV, generator=twin_gen)
            for lo in range(0, B, bs):
                idx = perm[lo:lo + bs]
                mom = pol.ppo_adv_moments(batch.advantages, idx)
                sums = pol.ppo_grad(s["params"], *flat, 6, 2, idx, 0.2, None, mom, s["ctrl"], 0.5, 0.01, hidden=64)
                pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], LR, 0.5, vf_coef=0.5, ent_coef=0.01,
                               stats=stats[row])
                row += 1
        mine = {"params": model.params, "m": model.exp_avg, "v": model.exp_avg_sq, "ctrl": model.ctrl}
        assert row == 24 and _same_bits(s, mine)
        assert s["ctrl"].tolist() == [(i + 1) * row, 0]
        assert np.array_equal(stats.cpu().numpy().view(np.int64), out["rows"].view(np.int64))
        assert np.isfinite(out["rows"]).all() and (out["rows"][:, 6] == bs).all()
        assert out["n_updates"] == (i + 1) * n_epochs and not out["stopped"]
        assert all(np.isfinite(out[k]) for k in ("policy_gradient_loss", "value_loss", "entropy_loss",
                                                 "clip_fraction", "approx_kl", "loss"))
        for k in prev:
            prev[k] = mine[k].clone()
        seen.append(out)

    out = ppo.learn(2 * B, callback=check)
    assert len(out) == len(seen) == 2 and ppo.num_timesteps == 2 * B
    assert not torch.equal(ppo.params.cpu(), a2c_ref.flatten(sd0))
    assert ppo.optimizer_state()["step"] == 2 * n_epochs * (B // bs)
    assert _collector_runs(ppo.state_dict(), col, n)
    env.close()
