"""lz_a2c_grad_f32 / lz_a2c_apply_f32 and FusedA2C on the MI355X against tests/a2c_ref.py
(torch float64 CPU autograd, clip_grad_norm_ and RMSpropTFLike restated from SB3 2.7.1).

Gradient accuracy is measured against what SB3 itself would have computed: with g64 the
float64 gradient, err_gpu = ||g_gpu - g64|| / ||g64|| and err_t32 the same for torch's
float32 CPU autograd on the same inputs, per tensor (all 13, each with ||g64|| > 0), for the
whole vector and for the three loss sums, the bound is

    err_gpu <= RATIO_BOUND * max(err_t32, 2^-24)

RATIO_BOUND is twice the worst ratio measured over every shape below and three seeds
(tools/a2c_grad_error.py -> profiles/a2c/grad_error.json: 6.58, the layer-2 bias of the pi
net at B = 5155 on 3 workgroups per net, a sequential float32 sum over 1728 samples where
torch sums pairwise; the whole-vector ratio is below 1.7 everywhere).  2^-24 is half a
float32 ulp: a one-element tensor's float32 value can be exact by luck."""
import numpy as np
import pytest
import torch

import a2c_ref as ref
import gym_lorenz as gl
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol
from gym_lorenz.vec_normalize import DeviceRunningMeanStd

pytestmark = pytest.mark.gpu

RATIO_BOUND = 2 * 6.576
DEV = torch.device("cuda", 0)
_CACHE = {}


def _case(name):
    """Inputs and the two CPU references of a CASES row (seed 0), computed once."""
    if name not in _CACHE:
        case = next(c for c in ref.CASES if c[0] == name)
        sd, batch = ref.case_inputs(case, 0)
        _CACHE[name] = dict(case=case, sd=sd, batch=batch, g64=ref.grad_sums(sd, batch),
                            g32=ref.grad_sums(sd, batch, dtype=torch.float32))
    return _CACHE[name]


def _gpu_grad(c, rows=None, **kw):
    _, B, O, A, cap, _ = c["case"]
    batch = c["batch"] if rows is None else tuple(t[rows].contiguous() for t in c["batch"])
    kw.setdefault("max_workgroups", cap)
    return pol.a2c_grad(ref.flatten(c["sd"]).to(DEV), *[t.to(DEV) for t in batch], O, A, 0.5, 0.0, **kw)


def _check_accuracy(got, c, what):
    _, B, O, A, _, _ = c["case"]
    g64, g32 = c["g64"], c["g32"]
    P = g64.size - 4
    lay = ref.layout(O, A)[0]
    slices = {k: slice(o, o + int(np.prod(shp))) for k, (o, shp) in lay.items()}
    slices.update(all=slice(0, P), policy_sum=slice(P, P + 1), value_sum=slice(P + 1, P + 2),
                  entropy_sum=slice(P + 2, P + 3))
    assert len(slices) == 13 + 4
    for k, sl in slices.items():
        assert np.linalg.norm(g64[sl]) > 0, k  # nothing passes vacuously
        e_gpu, e_t32 = ref.rel_err(got[sl], g64[sl]), ref.rel_err(g32[sl], g64[sl])
        print("%s %s %s: err_gpu %.3e err_t32 %.3e ratio %.2f" % (what, c["case"][0], k, e_gpu, e_t32,
                                                                  e_gpu / max(e_t32, ref.ERR_FLOOR)))
        assert e_gpu <= RATIO_BOUND * max(e_t32, ref.ERR_FLOOR), (what, k, e_gpu, e_t32)
    assert got[P + 3] == B


@pytest.mark.parametrize("name", [c[0] for c in ref.CASES])
def test_gradient_and_loss_sums_match_float64_autograd(name):
    c = _case(name)
    _check_accuracy(_gpu_grad(c).cpu().numpy(), c, "grad")


@pytest.mark.parametrize("name", ["b111", "b5155_cap3", "b65584"])
def test_two_launches_are_bit_identical(name):
    c = _case(name)
    _, B, O, A, cap, _ = c["case"]
    need = int(nat.lib.lz_a2c_workspace_bytes(B, O, A, cap)) // 8
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)
    a = _gpu_grad(c, workspace=ws).clone()
    ws.fill_(float("nan"))  # the second launch must not read what the first one left
    b = _gpu_grad(c, workspace=ws)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("name", ["b111", "b5155_cap3"])
def test_half_batches_add_up(name):
    """What the all-reduce relies on: the sums of two half batches, added in float64, are
    the whole batch's sums within the accuracy bound."""
    c = _case(name)
    B = c["case"][1]
    cut = B // 2 + 3  # both halves ragged
    lo = _gpu_grad(c, rows=slice(0, cut)).cpu().numpy()
    hi = _gpu_grad(c, rows=slice(cut, B)).cpu().numpy()
    assert lo[-1] == cut and hi[-1] == B - cut
    _check_accuracy(lo + hi, c, "halves")


def test_lanes_past_the_last_sample_add_nothing():
    """A batch of 33 (one full tile and one lane of the next) given as the leading rows of
    the 111-row buffers: the 31 idle lanes of the second tile must not read the rows behind
    them as samples, nor add their biases' share."""
    c = _case("b111")
    _, B, O, A, _, _ = c["case"]
    flat = ref.flatten(c["sd"]).to(DEV)
    obs, act, adv, ret = [t.to(DEV) for t in c["batch"]]
    small = pol.a2c_grad(flat, obs[:33].contiguous(), act[:33].contiguous(), adv[:33].contiguous(),
                         ret[:33].contiguous(), O, A)
    sd, batch = c["sd"], tuple(t[:33].contiguous() for t in c["batch"])
    g64 = ref.grad_sums(sd, batch)
    P = g64.size - 4
    assert small[P + 3].item() == 33
    assert ref.rel_err(small.cpu().numpy()[:P], g64[:P]) <= RATIO_BOUND * max(
        ref.rel_err(ref.grad_sums(sd, batch, dtype=torch.float32)[:P], g64[:P]), ref.ERR_FLOOR)


@pytest.mark.parametrize("max_grad_norm,adv_scale", [(0.5, 50.0), (100.0, 1.0)])
def test_apply_is_the_float64_step_within_one_ulp(max_grad_norm, adv_scale):
    """Two consecutive updates (square_avg leaves its initial ones) fed the GPU's own sums:
    params and square_avg within 1 float32 ulp of a2c_ref's float64 step rounded once."""
    c = _case("b111")
    _, B, O, A, _, _ = c["case"]
    obs, act, adv, ret = [t.to(DEV) for t in c["batch"]]
    adv = (adv * adv_scale).contiguous()
    params = ref.flatten(c["sd"]).to(DEV)
    sq = torch.ones_like(params)
    lr = 7e-4
    for step in range(2):
        sums = pol.a2c_grad(params, obs, act, adv, ret, O, A, 0.5, 0.01)
        p0, s0 = params.cpu().numpy(), sq.cpu().numpy()
        stats = pol.a2c_apply(sums, params, sq, lr, max_grad_norm, 0.99, 1e-5, 0.5, 0.01).cpu().numpy()
        h = sums.cpu().numpy()
        p_ref, s_ref, total, coef = ref.apply_step(h, p0, s0, lr, max_grad_norm)
        assert (coef < 1.0) == (max_grad_norm == 0.5), (total, coef)
        assert ref.ulp_diff(params.cpu().numpy(), p_ref) <= 1, step
        assert ref.ulp_diff(sq.cpu().numpy(), s_ref) <= 1, step
        assert not np.array_equal(params.cpu().numpy(), p0)
        P = h.size - 4
        pl, vl, el = h[P] / B, h[P + 1] / B, h[P + 2] / B
        want = [pl, vl, el, pl + 0.01 * el + 0.5 * vl, total, coef, B, lr]
        np.testing.assert_allclose(stats, want, rtol=1e-12)
    assert float(sq.min()) < 1.0  # it moved


def test_captured_graph_replays_equal_eager_calls():
    """grad + apply captured after one eager call and replayed twice == three eager calls."""
    c = _case("b111")
    _, B, O, A, _, _ = c["case"]
    batch = [t.to(DEV) for t in c["batch"]]
    P = int(nat.lib.lz_a2c_param_count(O, A))
    need = int(nat.lib.lz_a2c_workspace_bytes(B, O, A, 0)) // 8

    def state():
        return dict(params=ref.flatten(c["sd"]).to(DEV), sq=torch.ones((P,), device=DEV),
                    ws=torch.empty((need,), dtype=torch.float64, device=DEV),
                    sums=torch.empty((P + 4,), dtype=torch.float64, device=DEV),
                    stats=torch.empty((8,), dtype=torch.float64, device=DEV))

    def step(s):
        pol.a2c_grad(s["params"], *batch, O, A, 0.5, 0.0, workspace=s["ws"], out=s["sums"])
        pol.a2c_apply(s["sums"], s["params"], s["sq"], 7e-4, 0.5, stats=s["stats"])

    a, b = state(), state()
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
    for k in ("params", "sq", "sums", "stats"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_learn_end_to_end_pmsm():
    """PMSM, 64 envs, n_steps = 16, VecNormalize on, three updates through FusedA2C.learn.
    Each update is checked on its own batch from the GPU's previous parameters (the chaotic
    env would amplify rounding across updates): the gradient sums within the accuracy bound of
    the float64 autograd, the step within 1 ulp of a2c_ref's on those sums.  Then the weights
    reached the collector's blob: a fresh deterministic collector packed from
    a2c.state_dict() acts bit for bit as one running the trained collector's blob."""
    n, K = 64, 16
    env = gl.BatchedEnv("pmsm", n, seed=5)
    rms = DeviceRunningMeanStd(6, env.device)
    col = pol.FusedRolloutCollector(env, None, obs_rms=rms, training=True, precision="fp32")
    sd0 = ref.make_policy(6, 2, 4)
    sched = pol.linear_schedule(0.0005)
    a2c = pol.FusedA2C(col, sd0, learning_rate=sched, n_steps=K, max_grad_norm=0.5)
    prev = {"p": a2c.params.clone(), "s": a2c.square_avg.clone()}
    seen = []

    def check(model, batch, stats):
        i = len(seen)
        p0, s0 = prev["p"].cpu(), prev["s"].cpu().numpy()
        sd = ref.unflatten(p0, 6, 2)
        b = (batch.observations.reshape(K * n, 6).cpu(), batch.actions.reshape(K * n, 2).cpu(),
             batch.advantages.reshape(-1).cpu(), batch.returns.reshape(-1).cpu())
        c = dict(case=("e2e%d" % i, K * n, 6, 2, 0, False), sd=sd, batch=b, g64=ref.grad_sums(sd, b),
                 g32=ref.grad_sums(sd, b, dtype=torch.float32))
        sums = model._sums.cpu().numpy()
        _check_accuracy(sums, c, "learn")
        lr = sched(1.0 - (i + 1) / 3.0)
        assert stats["lr"] == pytest.approx(lr, rel=1e-15) and stats["n_samples"] == K * n
        p_ref, s_ref, total, coef = ref.apply_step(sums, p0.numpy(), s0, lr, 0.5)
        assert ref.ulp_diff(model.params.cpu().numpy(), p_ref) <= 1
        assert ref.ulp_diff(model.square_avg.cpu().numpy(), s_ref) <= 1
        assert stats["grad_norm"] == pytest.approx(total, rel=1e-12)
        prev["p"], prev["s"] = model.params.clone(), model.square_avg.clone()
        seen.append(stats)

    out = a2c.learn(3 * K * n, callback=check)
    assert len(out) == len(seen) == 3 and a2c.num_timesteps == 3 * K * n
    assert not torch.equal(a2c.params.cpu(), ref.flatten(sd0))
    # the trained weights are what the collector now runs
    acts = []
    for use_trained_blob in (False, True):
        twin = gl.BatchedEnv("pmsm", n, seed=9)
        fresh = pol.FusedRolloutCollector(twin, a2c.state_dict(), deterministic=True, precision="fp32")
        if use_trained_blob:
            fresh.blob = col.blob
        else:
            assert torch.equal(fresh.blob, col.blob)
        fresh.reset()
        acts.append(fresh.collect(4).actions.cpu().numpy())
        twin.close()
    assert np.array_equal(acts[0].view(np.int32), acts[1].view(np.int32)) and np.abs(acts[0]).max() > 0
    env.close()
