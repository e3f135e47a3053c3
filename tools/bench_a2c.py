"""One A2C update, lz_a2c_grad_f32 + lz_a2c_apply_f32, against the only other route to it:
ActorCriticMlp in torch float32 on the device with autograd, clip_grad_norm_ and
RMSpropTFLike restated in torch ops.  Same synthetic PMSM-shaped batch (O = 6, A = 2, the
generator of tests/a2c_ref.py's fixtures), the two arms alternating in one process after a
warm-up, HIP-event times, at least 1 s per arm.

  K = 16, N = 262,144   (B = 4,194,304)
  K = 16, N =  32,768   (B =   524,288)

Per arm: the median per update, the spread (max - min) / median, samples/s; for the fused
arm the fraction of the 157.3 TFLOP/s f32 MFMA peak in useful FLOP (forward + backward of
the two nets = 3 x 2 x the nets' multiply-adds per sample).  fused_beats_autograd: the
fused median is below the autograd median by more than the two spreads (max - min)
together.  Writes profiles/a2c/bench.json (--out elsewhere) and prints it.  Needs the
MI355X.  --quick shrinks the batches (a smoke run of the tool, not a measurement)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-lorenz_amd"))
import torch  # noqa: E402

from gym_lorenz import policy as pol  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_a2c: no HIP device visible (the update kernels need an MI355X)")
QUICK = "--quick" in sys.argv
PEAK_F32_MFMA = 157.3e12
O, A, H = 6, 2, pol.HIDDEN
VF_COEF, ENT_COEF, MAX_NORM, ALPHA, EPS, LR = 0.5, 0.0, 0.5, 0.99, 1e-5, 7e-4


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


def summary(ts, B):
    med = statistics.median(ts)
    return {"reps": len(ts), "min_s": min(ts), "median_s": med, "max_s": max(ts),
            "spread": (max(ts) - min(ts)) / med, "samples_per_s": B / med}


def case(K, N):
    B = K * N
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    net = pol.ActorCriticMlp(O, A, seed=1).to(dev)
    obs = torch.randn(B, O, generator=g, device=dev).clamp(-10, 10)
    with torch.no_grad():
        mu, _ = net(obs)
    act = mu + torch.exp(net.log_std.detach()) * torch.randn(B, A, generator=g, device=dev)
    adv = torch.randn(B, generator=g, device=dev)
    ret = torch.randn(B, generator=g, device=dev)

    # arm one: the fused update
    sd = net.state_dict()
    params = torch.cat([sd[k].detach().reshape(-1) for k in pol.KEYS]).contiguous()
    sq = torch.ones_like(params)
    P = params.numel()
    ws = torch.empty((int(pol.nat.lib.lz_a2c_workspace_bytes(B, O, A, 0)) // 8,), dtype=torch.float64,
                     device=dev)
    sums = torch.empty((P + 4,), dtype=torch.float64, device=dev)
    stats = torch.empty((8,), dtype=torch.float64, device=dev)

    def fused():
        pol.a2c_grad(params, obs, act, adv, ret, O, A, VF_COEF, ENT_COEF, workspace=ws, out=sums)
        pol.a2c_apply(sums, params, sq, LR, MAX_NORM, ALPHA, EPS, VF_COEF, ENT_COEF, stats=stats)

    # arm two: torch autograd, clip_grad_norm_, RMSpropTFLike in torch ops
    ps = list(net.parameters())
    sq_t = [torch.ones_like(p) for p in ps]
    half_log_2pi = 0.9189385332046727

    def autograd():
        for p in ps:
            p.grad = None
        mean, v = net(obs)
        ls = net.log_std
        logp = (-((act - mean) ** 2) / (2 * torch.exp(ls) ** 2) - ls - half_log_2pi).sum(1)
        ent = (0.5 + half_log_2pi + ls).sum()
        loss = -(adv * logp).mean() + VF_COEF * torch.nn.functional.mse_loss(ret, v) + ENT_COEF * -ent
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        with torch.no_grad():
            for p, s in zip(ps, sq_t):
                s.mul_(ALPHA).addcmul_(p.grad, p.grad, value=1 - ALPHA)
                p.addcdiv_(p.grad, (s + EPS).sqrt_(), value=-LR)

    arms = {"fused": fused, "autograd": autograd}
    for f in arms.values():  # warm-up
        f()
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    while min(sum(v) for v in ts.values()) < (0.05 if QUICK else 1.0) or len(ts["fused"]) < 5:
        for name, f in arms.items():  # alternating
            ts[name].append(timed(f))
    out = {"K": K, "envs": N, "samples": B, "obs_dim": O, "act_dim": A,
           "useful_flop_per_sample": useful_flop_per_sample()}
    for name in arms:
        out[name] = summary(ts[name], B)
    out["fused"]["fraction_of_f32_mfma_peak"] = (useful_flop_per_sample() * B / out["fused"]["median_s"]
                                                 / PEAK_F32_MFMA)
    out["ratio_fused_over_autograd"] = out["fused"]["median_s"] / out["autograd"]["median_s"]
    spreads = sum(out[k]["max_s"] - out[k]["min_s"] for k in arms)
    out["fused_beats_autograd"] = out["autograd"]["median_s"] - out["fused"]["median_s"] > spreads
    return out


def main():
    shapes = [(16, 4096), (16, 1024)] if QUICK else [(16, 262144), (16, 32768)]
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "device": torch.cuda.get_device_name(0), "quick": QUICK, "peak_f32_mfma_flops": PEAK_F32_MFMA,
           "cases": [case(K, N) for K, N in shapes]}
    path = os.path.join(ROOT, "profiles", "a2c", "bench.json")
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
