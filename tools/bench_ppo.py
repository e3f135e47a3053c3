"""One PPO update -- FusedPPO.train(): n_epochs x minibatches of lz_ppo_adv_moments +
lz_ppo_grad_f32 + lz_adam_apply_f32, the stats copied to the host once, the weights repacked
into the collector once -- against the only other route to it: ActorCriticMlp in torch
float32 on the device, SB3's loss in torch ops, backward(), clip_grad_norm_ and
torch.optim.Adam(eps=1e-5), over permutations drawn the same way.  (The torch arm does not
repack its weights for a collector; the fused arms do.)  Same synthetic PMSM-shaped rollout
(O = 6, A = 2; old log-probs and values are the initial policy's own), the arms alternating
in one process after a warm-up, HIP-event times around a whole update, at least 1 s per arm.

  32,768 envs x 16 steps (B = 524,288), n_epochs = 4, batch_size 65,536   (32 minibatches)
  the same rollout,                                   batch_size  4,096   (512 minibatches)

Arms: fused (eager: three launches per minibatch from Python), fused_graph (the update's
launches captured once with torch.cuda.graph and replayed; the permutations are drawn into
the captured buffers before each replay), autograd.  Per arm: the median per update, the
spread (max - min) / median, samples/s (B x n_epochs per update); for the fused arms the
fraction of the 157.3 TFLOP/s f32 MFMA peak in useful FLOP.  fused_beats_autograd (per fused
arm): the fused median is below the autograd median by more than the two spreads (max - min)
together.  Writes profiles/ppo/bench.json (--out elsewhere) and prints it.  Needs the MI355X.
--quick shrinks the shapes (a smoke run of the tool, not a measurement)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-lorenz_amd"))
import torch  # noqa: E402

import gym_lorenz as gl  # noqa: E402
from gym_lorenz import policy as pol  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_ppo: no HIP device visible (the update kernels need an MI355X)")
QUICK = "--quick" in sys.argv
PEAK_F32_MFMA = 157.3e12
O, A, H = 6, 2, pol.HIDDEN
VF_COEF, ENT_COEF, MAX_NORM, LR, CLIP = 0.5, 0.0, 0.5, 3e-4, 0.2


def useful_flop_per_sample():
    macs = (O * H + H * H + A * H) + (O * H + H * H + H)
    return 3 * 2 * macs


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def summary(ts, samples):
    med = statistics.median(ts)
    return {"reps": len(ts), "min_s": min(ts), "median_s": med, "max_s": max(ts),
            "spread": (max(ts) - min(ts)) / med, "samples_per_s": samples / med}


def case(K, N, batch_size, n_epochs):
    B = K * N
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    net = pol.ActorCriticMlp(O, A, seed=1).to(dev)
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    half_log_2pi = 0.9189385332046727
    obs = torch.randn(B, O, generator=g, device=dev).clamp(-10, 10)
    with torch.no_grad():
        mu, val = net(obs)
        ls = net.log_std.detach()
        act = mu + torch.exp(ls) * torch.randn(B, A, generator=g, device=dev)
        logp = (-((act - mu) ** 2) / (2 * torch.exp(ls) ** 2) - ls - half_log_2pi).sum(1)
    adv = torch.randn(B, generator=g, device=dev)
    ret = torch.randn(B, generator=g, device=dev)
    batch = pol.RolloutBatch(obs.reshape(K, N, O), act.reshape(K, N, A), logp.reshape(K, N).contiguous(),
                             val.reshape(K, N).contiguous(), None, None, None, None, None,
                             advantages=adv.reshape(K, N), returns=ret.reshape(K, N))

    # arms one and two: FusedPPO on a float32 collector of N PMSM envs
    env = gl.BatchedEnv("pmsm", N, seed=3)
    col = pol.FusedRolloutCollector(env, None, precision="fp32")
    gen = torch.Generator(device=dev).manual_seed(11)
    ppo = pol.FusedPPO(col, sd0, learning_rate=LR, n_steps=K, batch_size=batch_size, n_epochs=n_epochs,
                       clip_range=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF, max_grad_norm=MAX_NORM,
                       generator=gen)
    cuts = ppo.minibatches(B)

    def fused():
        ppo.train(batch)

    fused()  # sizes the workspace and the stats table the captured update writes
    perms = torch.empty((n_epochs, B), dtype=torch.int32, device=dev)
    stats = torch.empty((n_epochs * len(cuts), 12), dtype=torch.float64, device=dev)

    def update_on_device():
        ppo.ctrl[1:].zero_()
        i = 0
        for e in range(n_epochs):
            for lo, hi in cuts:
                ppo.minibatch_step(batch, perms[e, lo:hi], LR, CLIP, None, stats[i])
                i += 1

    for e in range(n_epochs):
        torch.randperm(B, dtype=torch.int32, device=dev, generator=gen, out=perms[e])
    update_on_device()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        update_on_device()
    torch.cuda.synchronize()

    def fused_graph():
        for e in range(n_epochs):
            torch.randperm(B, dtype=torch.int32, device=dev, generator=gen, out=perms[e])
        graph.replay()
        stats.cpu()
        col.set_params(ppo.state_dict())

    # arm three: torch autograd, clip_grad_norm_, torch.optim.Adam
    ps = list(net.parameters())
    opt = torch.optim.Adam(ps, lr=LR, eps=1e-5)
    gen_t = torch.Generator(device=dev).manual_seed(11)

    def autograd():
        for _ in range(n_epochs):
            perm = torch.randperm(B, device=dev, generator=gen_t)
            for lo, hi in cuts:
                idx = perm[lo:hi]
                a_mb = adv[idx]
                a_mb = (a_mb - a_mb.mean()) / (a_mb.std() + 1e-8)
                mean, v = net(obs[idx])
                ls = net.log_std
                lp = (-((act[idx] - mean) ** 2) / (2 * torch.exp(ls) ** 2) - ls - half_log_2pi).sum(1)
                ent = (0.5 + half_log_2pi + ls).sum()
                ratio = torch.exp(lp - logp[idx])
                pl = -torch.min(a_mb * ratio, a_mb * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
                loss = pl + VF_COEF * torch.nn.functional.mse_loss(ret[idx], v.flatten()) + ENT_COEF * -ent
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
                opt.step()

    arms = {"fused": fused, "fused_graph": fused_graph, "autograd": autograd}
    for f in arms.values():  # warm-up
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    while min(sum(v) for v in ts.values()) < (0.05 if QUICK else 1.0) or len(ts["fused"]) < 3:
        for name, f in arms.items():  # alternating
            ts[name].append(timed(f))
    per_update = B * n_epochs
    out = {"K": K, "envs": N, "samples": B, "batch_size": batch_size, "n_epochs": n_epochs,
           "minibatches_per_update": n_epochs * len(cuts), "obs_dim": O, "act_dim": A,
           "useful_flop_per_sample": useful_flop_per_sample()}
    spread = {}
    for name in arms:
        out[name] = summary(ts[name], per_update)
        spread[name] = out[name]["max_s"] - out[name]["min_s"]
    for name in ("fused", "fused_graph"):
        out[name]["fraction_of_f32_mfma_peak"] = (useful_flop_per_sample() * per_update
                                                  / out[name]["median_s"] / PEAK_F32_MFMA)
        out[name]["ratio_over_autograd"] = out[name]["median_s"] / out["autograd"]["median_s"]
        out[name]["fused_beats_autograd"] = (out["autograd"]["median_s"] - out[name]["median_s"]
                                             > spread[name] + spread["autograd"])
    env.close()
    return out


def main():
    shapes = ([(16, 1024, 4096, 2), (16, 1024, 512, 2)] if QUICK
              else [(16, 32768, 65536, 4), (16, 32768, 4096, 4)])
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "device": torch.cuda.get_device_name(0), "quick": QUICK, "peak_f32_mfma_flops": PEAK_F32_MFMA,
           "cases": [case(*s) for s in shapes]}
    path = os.path.join(ROOT, "profiles", "ppo", "bench.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    if not QUICK or "--out" in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
