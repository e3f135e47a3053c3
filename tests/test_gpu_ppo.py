"""lz_ppo_adv_moments / lz_ppo_grad_f32 / lz_adam_apply_f32 and FusedPPO on the MI355X against
tests/ppo_ref.py (torch float64 CPU autograd of SB3 2.7.1's PPO loss, clip_grad_norm_ and
torch.optim.Adam restated).

Gradient accuracy is measured as for A2C (tests/test_gpu_a2c.py): with g64 the float64
gradient, err_gpu = ||g_gpu - g64|| / ||g64|| and err_t32 the same for torch's float32 CPU
autograd on the same inputs, per tensor (all 13, each with ||g64|| > 0), for the whole
vector, for the three loss sums and for the kl sum, the bound is

    err_gpu <= RATIO_BOUND * max(err_t32, 2^-24)

RATIO_BOUND is twice the worst ratio measured over every shape of ppo_ref.CASES, every option
set and three seeds (tools/ppo_grad_error.py -> profiles/ppo/grad_error.json: 19.33, the
policy-loss sum of 5,155 normalised advantages, a sum of 36.9 over terms of size 1 in which
err_gpu is 1.15e-6 -- the other two seeds' err_t32 are 1.1e-6 and 1.2e-6 -- and this seed's
err_t32 happens to be 3.6e-8; the worst tensor ratio is 5.47, a layer-2 bias as for A2C, and
the whole-vector ratio is below 1.5 everywhere but the one-sample case, 3.27).  The count and
the clipped count are integers and must be exact.  The cases keep every row 1e-4 away from a
clip edge (float32 and float64 ratios differ by 3e-6 at most), so both precisions clip the
same rows."""
import numpy as np
import pytest
import torch

import a2c_ref
import gym_lorenz as gl
import ppo_ref as ref
from gym_lorenz import _native as nat
from gym_lorenz import policy as pol
from gym_lorenz.vec_normalize import DeviceRunningMeanStd

pytestmark = pytest.mark.gpu

RATIO_BOUND = 2 * 19.326
DEV = torch.device("cuda", 0)
_CACHE = {}
LR = 3e-4


def _case(name):
    """A CASES row (seed 0) with its arrays on the device, built once."""
    if name not in _CACHE:
        c = ref.make_case(next(k for k in ref.CASES if k[0] == name), 0)
        c["dev_rows"] = [t.to(DEV) for t in c["rows"]]
        c["dev_idx"] = c["idx"].to(DEV)
        c["flat"] = a2c_ref.flatten(c["sd"]).to(DEV)
        c["cpu"] = {}
        _CACHE[name] = c
    return _CACHE[name]


def _cpu(c, opt):
    """(g64, g32) of an option set, computed once."""
    if opt not in c["cpu"]:
        normalize, vclip, ent = ref.OPTIONS[opt]
        kw = dict(normalize=normalize, cvf=ref.CLIP_VF if vclip else None, ent_coef=ent)
        mb = ref.minibatch(c)
        c["cpu"][opt] = (ref.grad_sums(c["sd"], mb, **kw), ref.grad_sums(c["sd"], mb, dtype=torch.float32, **kw))
    return c["cpu"][opt]


def _gpu(c, opt, idx="case", params=None, rows=None, ctrl=None, **kw):
    """moments (when the option normalises and M > 1) + grad on the case's rows."""
    _, M, n_rows, O, A, cap = c["case"]
    normalize, vclip, ent = ref.OPTIONS[opt]
    rows = c["dev_rows"] if rows is None else rows
    idx = c["dev_idx"] if isinstance(idx, str) else idx
    m = rows[2].numel() if idx is None else idx.numel()
    mom = pol.ppo_adv_moments(rows[2], idx) if normalize and m > 1 else None
    kw.setdefault("max_workgroups", cap)
    return pol.ppo_grad(c["flat"] if params is None else params, *rows, O, A, idx, ref.CLIP,
                        ref.CLIP_VF if vclip else None, mom, ctrl, 0.5, ent, **kw)


def _check_accuracy(got, g64, g32, O, A, M, what, skip=()):
    slices, P = ref.check_slices(O, A)
    assert len(slices) == 13 + 5
    for k, sl in slices.items():
        if k in skip:
            continue
        assert np.linalg.norm(g64[sl]) > 0, k  # nothing passes vacuously
        e_gpu, e_t32 = a2c_ref.rel_err(got[sl], g64[sl]), a2c_ref.rel_err(g32[sl], g64[sl])
        print("%s %s: err_gpu %.3e err_t32 %.3e ratio %.2f" % (what, k, e_gpu, e_t32,
                                                               e_gpu / max(e_t32, a2c_ref.ERR_FLOOR)))
        assert e_gpu <= RATIO_BOUND * max(e_t32, a2c_ref.ERR_FLOOR), (what, k, e_gpu, e_t32)
    assert got[P + 3] == M


@pytest.mark.parametrize("name", [c[0] for c in ref.CASES])
def test_gradient_and_sums_match_float64_autograd(name):
    """Every option on (the one-sample case: no normalisation, as SB3's len(advantages) > 1)."""
    c = _case(name)
    _, M, _, O, A, _ = c["case"]
    g64, g32 = _cpu(c, "all")
    got = _gpu(c, "all").cpu().numpy()
    _check_accuracy(got, g64, g32, O, A, M, "all " + name)
    P = got.size - 6
    assert got[P + 4] == g64[P + 4]  # the clipped count


@pytest.mark.parametrize("opt", list(ref.OPTIONS))
def test_each_option_alone_and_all_together(opt):
    c = _case("m111")
    _, M, _, O, A, _ = c["case"]
    g64, g32 = _cpu(c, opt)
    got = _gpu(c, opt).cpu().numpy()
    _check_accuracy(got, g64, g32, O, A, M, opt)
    P = got.size - 6
    assert got[P + 4] == g64[P + 4] and 0 < got[P + 4] < M
    if opt != "plain":  # the option changes the result: it is not ignored
        plain = _gpu(c, "plain").cpu().numpy()
        assert not np.array_equal(plain[:P], got[:P])


def test_null_indices_are_the_first_rows():
    """indices = NULL on the first M rows equals an explicit arange(M) into the larger
    arrays, bit for bit."""
    c = _case("m111")
    M = 111
    head = [t[:M].contiguous() for t in c["dev_rows"]]
    a = _gpu(c, "all", idx=None, rows=head)
    b = _gpu(c, "all", idx=torch.arange(M, dtype=torch.int32, device=DEV))
    assert a[-3].item() == M
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("name", ["m111", "m5155_cap3", "m5155_cap2"])
def test_two_launches_are_bit_identical(name):
    c = _case(name)
    _, M, _, O, A, cap = c["case"]
    need = int(nat.lib.lz_ppo_workspace_bytes(M, O, A, cap)) // 8
    ws = torch.zeros((need,), dtype=torch.float64, device=DEV)
    a = _gpu(c, "all", workspace=ws).clone()
    ws.fill_(float("nan"))  # the second launch must not read what the first one left
    b = _gpu(c, "all", workspace=ws)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert bool(torch.isfinite(b).all())


@pytest.mark.parametrize("name", ["m111", "m5155_cap3"])
def test_adv_moments(name):
    """Within 2 float64 ulps of NumPy's two-pass mean and unbiased std; the same bits twice."""
    c = _case(name)
    adv = c["dev_rows"][2]
    a = pol.ppo_adv_moments(adv, c["dev_idx"]).clone()
    b = pol.ppo_adv_moments(adv, c["dev_idx"])
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    mean, std = ref.adv_moments(c["rows"][2][c["idx"].long()].numpy())
    got = a.cpu().numpy()
    print(name, "mean", got[0], mean, "std", got[1], std)
    assert abs(got[0] - mean) <= 2 * np.spacing(abs(mean))
    assert abs(got[1] - std) <= 2 * np.spacing(std)
    # all rows, no index list
    whole = pol.ppo_adv_moments(adv).cpu().numpy()
    mean, std = ref.adv_moments(c["rows"][2].numpy())
    assert abs(whole[0] - mean) <= 2 * np.spacing(abs(mean)) and abs(whole[1] - std) <= 2 * np.spacing(std)


def _state(c):
    P = c["flat"].numel()
    return dict(params=c["flat"].clone(), m=torch.zeros((P,), device=DEV), v=torch.zeros((P,), device=DEV),
                ctrl=torch.zeros((2,), dtype=torch.int64, device=DEV))


def _snapshot(s):
    return {k: s[k].clone() for k in ("params", "m", "v", "ctrl")}


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("params", "m", "v", "ctrl"))


@pytest.mark.parametrize("max_grad_norm,adv_scale", [(0.5, 50.0), (100.0, 1.0)])
def test_adam_is_the_float64_step_within_one_ulp(max_grad_norm, adv_scale):
    """Three consecutive steps fed the GPU's own sums (value clipping and the entropy term on,
    no normalisation so that the scale of the advantages decides whether the norm clips):
    params and both moments within 1 float32 ulp of ppo_ref's float64 step rounded once, the
    step count on the device, the stats row the sums over the count."""
    c = _case("m111")
    _, M, _, O, A, _ = c["case"]
    rows = list(c["dev_rows"])
    rows[2] = (rows[2] * adv_scale).contiguous()
    s = _state(c)
    vf, ent = 0.5, 0.01
    for step in range(3):
        sums = pol.ppo_grad(s["params"], *rows, O, A, c["dev_idx"], ref.CLIP, ref.CLIP_VF, None, s["ctrl"],
                            vf, ent)
        p0, m0, v0 = (s[k].cpu().numpy() for k in ("params", "m", "v"))
        stats = pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], LR, max_grad_norm, vf_coef=vf,
                               ent_coef=ent).cpu().numpy()
        h = sums.cpu().numpy()
        p_ref, m_ref, v_ref, total, coef = ref.adam_step(h, p0, m0, v0, step, LR, max_grad_norm)
        assert (coef < 1.0) == (max_grad_norm == 0.5), (total, coef)
        assert a2c_ref.ulp_diff(s["params"].cpu().numpy(), p_ref) <= 1, step
        assert a2c_ref.ulp_diff(s["m"].cpu().numpy(), m_ref) <= 1, step
        assert a2c_ref.ulp_diff(s["v"].cpu().numpy(), v_ref) <= 1, step
        assert not np.array_equal(s["params"].cpu().numpy(), p0)
        P = h.size - 6
        pl, vl, el = h[P] / M, h[P + 1] / M, h[P + 2] / M
        want = [pl, vl, el, pl + ent * el + vf * vl, total, coef, M, LR, h[P + 4] / M, h[P + 5] / M, step + 1, 0]
        np.testing.assert_allclose(stats, want, rtol=1e-12)
    assert s["ctrl"].tolist() == [3, 0]


def test_target_kl_stops_on_the_device():
    """Two minibatches of the 333 rows; the second one's old_log_prob is moved so that its
    approx_kl is more than four times the first one's, and 1.5 target_kl sits between them
    with a factor of two of room on both sides (asserted on the CPU reference, minibatch 2
    evaluated at the reference's parameters after step 1).  Step 1 is taken; minibatch 2 and a
    third call change nothing and say `stopped`; after the flag is cleared the next call steps."""
    c = _case("m111")
    _, _, n_rows, O, A, _ = c["case"]
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(11)).to(torch.int32)
    mb = [perm[:160].contiguous(), perm[160:320].contiguous()]
    rows_cpu = list(c["rows"])
    old_lp = rows_cpu[4].clone()
    shift = 0.8 * torch.randn(160, generator=torch.Generator().manual_seed(12))
    old_lp[mb[1].long()] += shift
    rows_cpu[4] = old_lp
    cc = dict(c, rows=tuple(rows_cpu))
    kw = dict(normalize=True, cvf=ref.CLIP_VF, ent_coef=0.0)
    g1 = ref.grad_sums(c["sd"], ref.minibatch(cc, mb[0]), **kw)
    P = g1.size - 6
    p0 = a2c_ref.flatten(c["sd"]).numpy()
    p1, _, _, _, _ = ref.adam_step(g1, p0, np.zeros(P, np.float32), np.zeros(P, np.float32), 0, LR)
    g2 = ref.grad_sums(a2c_ref.unflatten(torch.from_numpy(p1), O, A), ref.minibatch(cc, mb[1]), **kw)
    kl1, kl2 = g1[P + 5] / 160, g2[P + 5] / 160
    thr = float(np.sqrt(kl1 * kl2))
    assert 0 < 2 * kl1 <= thr <= kl2 / 2, (kl1, kl2)
    target_kl = thr / 1.5

    rows = [t.to(DEV) for t in rows_cpu]
    idx = [m.to(DEV) for m in mb]
    s = _state(c)
    stats = torch.zeros((4, 12), dtype=torch.float64, device=DEV)

    def step(i, row):
        mom = pol.ppo_adv_moments(rows[2], idx[i])
        sums = pol.ppo_grad(s["params"], *rows, O, A, idx[i], ref.CLIP, ref.CLIP_VF, mom, s["ctrl"])
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
    """Index -1 and index n_rows, the row arrays being interior views of larger tensors (so
    that even an unguarded read would stay inside owned memory): the three loss sums are NaN,
    the gradient is finite, the moments are NaN; a call with valid indices afterwards is what
    it was before."""
    c = _case("m111")
    _, M, n_rows, O, A, _ = c["case"]
    pad = 64
    rows = []
    for t in c["dev_rows"]:
        big = torch.full((n_rows + 2 * pad,) + tuple(t.shape[1:]), 3.0, dtype=t.dtype, device=DEV)
        big[pad:pad + n_rows] = t
        rows.append(big[pad:pad + n_rows])
    assert all(r.is_contiguous() and r.data_ptr() != r.untyped_storage().data_ptr() for r in rows)
    good = _gpu(c, "vclip", rows=rows).clone()
    P = good.numel() - 6
    for bad_value, where in ((-1, 5), (n_rows, 70), (2 ** 31 - 1, 110), (-2 ** 31, 0)):
        idx = c["dev_idx"].clone()
        idx[where] = bad_value
        got = _gpu(c, "vclip", idx=idx, rows=rows).cpu().numpy()
        assert np.isnan(got[P:P + 3]).all(), (bad_value, got[P:])
        assert np.isfinite(got[:P]).all() and got[P + 3] == M
        assert np.isnan(pol.ppo_adv_moments(rows[2], idx).cpu().numpy()).all()
    again = _gpu(c, "vclip", rows=rows)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(again.view(torch.int64), good.view(torch.int64))
    assert torch.equal(good.view(torch.int64), _gpu(c, "vclip").view(torch.int64))


def test_captured_graph_replays_equal_eager_epochs():
    """One epoch -- three minibatches of moments + grad + apply over the 333 rows -- captured
    after one eager epoch and replayed twice == three eager epochs, bit for bit, in params,
    both moments, the step count and the stats rows."""
    c = _case("m111")
    _, _, n_rows, O, A, _ = c["case"]
    rows = c["dev_rows"]
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(21)).to(torch.int32).to(DEV)
    mbs = [perm[i * 111:(i + 1) * 111] for i in range(3)]
    P = c["flat"].numel()
    need = int(nat.lib.lz_ppo_workspace_bytes(111, O, A, 0)) // 8

    def state():
        s = _state(c)
        s.update(ws=torch.empty((need,), dtype=torch.float64, device=DEV),
                 sums=torch.empty((P + 6,), dtype=torch.float64, device=DEV),
                 mom=torch.empty((2,), dtype=torch.float64, device=DEV),
                 stats=torch.zeros((3, 12), dtype=torch.float64, device=DEV))
        return s

    def epoch(s):
        for i, idx in enumerate(mbs):
            pol.ppo_adv_moments(rows[2], idx, out=s["mom"])
            pol.ppo_grad(s["params"], *rows, O, A, idx, ref.CLIP, ref.CLIP_VF, s["mom"], s["ctrl"], 0.5, 0.01,
                         workspace=s["ws"], out=s["sums"])
            pol.adam_apply(s["sums"], s["params"], s["m"], s["v"], s["ctrl"], LR, 0.5, vf_coef=0.5,
                           ent_coef=0.01, stats=s["stats"][i])

    a, b = state(), state()
    for _ in range(3):
        epoch(a)
    epoch(b)
    torch.cuda.synchronize()
    after_one = b["params"].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        epoch(b)
    torch.cuda.synchronize()
    assert torch.equal(b["params"], after_one) and b["ctrl"].tolist() == [3, 0]  # captured, not run
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert a["ctrl"].tolist() == b["ctrl"].tolist() == [9, 0]
    for k in ("params", "m", "v", "sums", "stats"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert a["stats"][:, 10].tolist() == [7, 8, 9]


def test_learn_end_to_end_pmsm():
    """PMSM, 64 envs, n_steps = 16, VecNormalize on, batch_size = 256, n_epochs = 2, two
    updates through FusedPPO.learn with a seeded device generator.  The kernels are
    deterministic, so a loop over the functional wrappers -- on each update's batch, from the
    parameters before it, with the randperm draws of an equally seeded generator -- reproduces
    FusedPPO's params, moments, step count and stats rows bit for bit.  The first minibatch of
    each update is held to the accuracy criterion against float64 autograd, for the 13
    tensors, the whole vector, the value and the entropy sums.  (Its parameters are the
    rollout's, so ratio = 1 up to float32 rounding: sum(-adv_n ratio) with sum(adv_n) = 0 and
    sum((ratio - 1) - log_ratio) are then the rounding residue of the float32 inputs in
    float64 too -- a question about their conditioning, not about the kernel, and the cases
    above hold both sums to the criterion where they mean something.)  Then the weights
    reached the collector's blob, as test_gpu_a2c checks for A2C."""
    n, K, bs, n_epochs = 64, 16, 256, 2
    B = n * K
    env = gl.BatchedEnv("pmsm", n, seed=5)
    rms = DeviceRunningMeanStd(6, env.device)
    col = pol.FusedRolloutCollector(env, None, obs_rms=rms, training=True, precision="fp32")
    sd0 = a2c_ref.make_policy(6, 2, 4)
    sched = pol.linear_schedule(LR)
    gen = torch.Generator(device=DEV).manual_seed(123)
    twin_gen = torch.Generator(device=DEV).manual_seed(123)
    ppo = pol.FusedPPO(col, sd0, learning_rate=sched, n_steps=K, batch_size=bs, n_epochs=n_epochs,
                       ent_coef=0.01, generator=gen)
    prev = {"params": ppo.params.clone(), "m": ppo.exp_avg.clone(), "v": ppo.exp_avg_sq.clone(),
            "ctrl": ppo.ctrl.clone()}
    seen = []

    def check(model, batch, out):
        i = len(seen)
        lr = sched(1.0 - (i + 1) / 2.0)
        assert out["learning_rate"] == lr and out["clip_range"] == 0.2 and not out["stopped"]
        s = {k: v.clone() for k, v in prev.items()}
        stats = torch.zeros((n_epochs * (B // bs), 12), dtype=torch.float64, device=DEV)
        flat = (batch.observations, batch.actions, batch.advantages, batch.returns, batch.log_probs, batch.values)
        row, first = 0, None
        for _ in range(n_epochs):
            perm = torch.randperm(B, dtype=torch.int32, device=DEV, generator=twin_gen)
            for lo in range(0, B, bs):
                idx = perm[lo:lo + bs]
                mom = pol.ppo_adv_moments(batch.advantages, idx)
                sums = pol.ppo_grad(s["params"], *flat, 6, 2, idx, 0.2, None, mom, s["ctrl"], 0.5, 0.01)
                if first is None:
                    first = (idx.cpu(), sums.cpu().numpy())
                pol.adam_apply(sums, s["params"], s["m"], s["v"], s["ctrl"], lr, 0.5, vf_coef=0.5,
                               ent_coef=0.01, stats=stats[row])
                row += 1
        mine = {"params": model.params, "m": model.exp_avg, "v": model.exp_avg_sq, "ctrl": model.ctrl}
        assert _same_bits(s, mine)
        assert s["ctrl"].tolist() == [(i + 1) * row, 0]
        assert np.array_equal(stats.cpu().numpy().view(np.int64), out["rows"].view(np.int64))
        assert out["n_updates"] == (i + 1) * n_epochs
        assert out["approx_kl"] == pytest.approx(out["rows"][:, 9].mean(), rel=1e-15)
        # the first minibatch against float64 autograd
        idx, sums = first
        sd = a2c_ref.unflatten(prev["params"].cpu(), 6, 2)
        rows_cpu = tuple(t.reshape((B,) + tuple(t.shape[2:])).cpu() for t in flat)
        mb = tuple(t[idx.long()] for t in rows_cpu)
        kw = dict(normalize=True, cvf=None, ent_coef=0.01)
        _check_accuracy(sums, ref.grad_sums(sd, mb, **kw), ref.grad_sums(sd, mb, dtype=torch.float32, **kw),
                        6, 2, bs, "learn %d" % i, skip=("policy_sum", "kl_sum"))
        assert sums[-2] == 0  # ratio = 1 up to rounding: nothing clipped
        for k in prev:
            prev[k] = mine[k].clone()
        seen.append(out)

    out = ppo.learn(2 * B, callback=check)
    assert len(out) == len(seen) == 2 and ppo.num_timesteps == 2 * B
    assert not torch.equal(ppo.params.cpu(), a2c_ref.flatten(sd0))
    assert ppo.optimizer_state()["step"] == 2 * n_epochs * (B // bs)
    # the trained weights are what the collector now runs
    acts = []
    for use_trained_blob in (False, True):
        twin = gl.BatchedEnv("pmsm", n, seed=9)
        fresh = pol.FusedRolloutCollector(twin, ppo.state_dict(), deterministic=True, precision="fp32")
        if use_trained_blob:
            fresh.blob = col.blob
        else:
            assert torch.equal(fresh.blob, col.blob)
        fresh.reset()
        acts.append(fresh.collect(4).actions.cpu().numpy())
        twin.close()
    assert np.array_equal(acts[0].view(np.int32), acts[1].view(np.int32)) and np.abs(acts[0]).max() > 0
    env.close()
