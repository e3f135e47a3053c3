"""One update of a 64 x 64 MlpPolicy on the device, two ways: `native`, the 64-unit gradient
kernels (lz_a2c_grad_hidden_f32 / lz_ppo_grad_hidden_f32 at hidden = 64), against `padded`,
the same net zero-padded to 128 units through the 128-unit kernels -- exact (the padded units
add zeros) and, before the 64-unit form, the only on-device way to take this step.  Both arms
run the same launches on the same synthetic PMSM-shaped rollout (O = 6, A = 2): an A2C update
is grad + apply on the whole batch; a PPO update is n_epochs x minibatches of moments + grad +
apply over fixed permutations, captured once per arm with torch.cuda.graph and replayed (what
is timed is the device's work, not Python's launch path, which is the same in both arms).

  A2C   524,288 and 4,194,304 rows
  PPO   524,288 rows x 4 epochs, batch_size 65,536 and 4,096
  PPO   2,048 rows x 10 epochs, batch_size 64 (the reference's n_steps / batch_size / n_epochs)

The arms alternate in one process after a warm-up, HIP-event times around a whole update, at
least 1 s per arm.  Per arm: min / median / max per update and the spread; per shape
native_over_padded (the ratio of the medians) and native_beats_padded: the native median is
below the padded median by more than the two arms' (max - min) together.  Writes
profiles/learner_h64/bench.json (--out elsewhere) and prints it.  Needs the MI355X.  --quick
shrinks the shapes (a smoke run of the tool, not a measurement)."""
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
    sys.exit("bench_learner_h64: no HIP device visible (the update kernels need an MI355X)")
QUICK = "--quick" in sys.argv
O, A = 6, 2
LR, CLIP = 3e-4, 0.2
DEV = torch.device("cuda", 0)


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


def flat_params(hidden):
    """The 64-unit net of seed 1 as the flat vector of a `hidden`-unit net (128: zero-padded)."""
    sd = pol.ActorCriticMlp(O, A, hidden=64, seed=1).state_dict()
    flat = []
    for k, shp in zip(pol.KEYS, pol.a2c_param_shapes(O, A, hidden)):
        big = torch.zeros(shp)
        src = sd[k].detach()
        if src.dim() == 2:
            big[:src.shape[0], :src.shape[1]] = src
        else:
            big[:src.shape[0]] = src
        flat.append(big.reshape(-1))
    return torch.cat(flat).to(DEV).contiguous()


def rollout(B):
    g = torch.Generator(device=DEV).manual_seed(7)
    net = pol.ActorCriticMlp(O, A, hidden=64, seed=1).to(DEV)
    obs = torch.randn(B, O, generator=g, device=DEV).clamp(-10, 10)
    with torch.no_grad():
        mu, val = net(obs)
        ls = net.log_std.detach()
        act = mu + torch.exp(ls) * torch.randn(B, A, generator=g, device=DEV)
        logp = (-((act - mu) ** 2) / (2 * torch.exp(ls) ** 2) - ls - 0.9189385332046727).sum(1)
    adv = torch.randn(B, generator=g, device=DEV)
    ret = torch.randn(B, generator=g, device=DEV)
    return [t.contiguous() for t in (obs, act, adv, ret, logp, val.flatten())]


def race(arms, samples):
    for f in arms.values():  # warm-up
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    while min(sum(v) for v in ts.values()) < (0.05 if QUICK else 1.0) or len(ts["native"]) < 5:
        for name, f in arms.items():  # alternating
            ts[name].append(timed(f))
    out = {name: summary(ts[name], samples) for name in arms}
    gap = sum(out[n]["max_s"] - out[n]["min_s"] for n in arms)
    out["native_over_padded"] = out["native"]["median_s"] / out["padded"]["median_s"]
    out["native_beats_padded"] = out["padded"]["median_s"] - out["native"]["median_s"] > gap
    return out


def a2c_case(B):
    obs, act, adv, ret, _, _ = rollout(B)
    arms = {}
    for name, H in (("native", 64), ("padded", 128)):
        params = flat_params(H)
        P = params.numel()
        _, ws_bytes, _ = pol._grad_fns("a2c", H, O, A, "bench")
        s = dict(params=params, sq=torch.ones_like(params),
                 ws=torch.empty((ws_bytes(B, 0) // 8,), dtype=torch.float64, device=DEV),
                 sums=torch.empty((P + 4,), dtype=torch.float64, device=DEV),
                 stats=torch.empty((8,), dtype=torch.float64, device=DEV))

        def update(s=s, H=H):
            pol.a2c_grad(s["params"], obs, act, adv, ret, O, A, 0.5, 0.0, workspace=s["ws"], out=s["sums"],
                         hidden=H)
            pol.a2c_apply(s["sums"], s["params"], s["sq"], 7e-4, 0.5, stats=s["stats"])

        arms[name] = update
    out = {"algo": "a2c", "samples": B, "launches": "eager: grad + apply"}
    out.update(race(arms, B))
    return out


def ppo_case(B, batch_size, n_epochs):
    rows = rollout(B)
    g = torch.Generator(device=DEV).manual_seed(11)
    perms = torch.stack([torch.randperm(B, dtype=torch.int32, device=DEV, generator=g) for _ in range(n_epochs)])
    cuts = [(lo, min(lo + batch_size, B)) for lo in range(0, B, batch_size)]
    arms, keep = {}, []
    for name, H in (("native", 64), ("padded", 128)):
        params = flat_params(H)
        P = params.numel()
        _, ws_bytes, _ = pol._grad_fns("ppo", H, O, A, "bench")
        s = dict(params=params, m=torch.zeros_like(params), v=torch.zeros_like(params),
                 ctrl=torch.zeros((2,), dtype=torch.int64, device=DEV),
                 ws=torch.empty((ws_bytes(min(batch_size, B), 0) // 8,), dtype=torch.float64, device=DEV),
                 sums=torch.empty((P + 6,), dtype=torch.float64, device=DEV),
                 mom=torch.empty((2,), dtype=torch.float64, device=DEV),
                 stats=torch.empty((n_epochs * len(cuts), 12), dtype=torch.float64, device=DEV))

        def update(s=s, H=H):
            i = 0
            for e in range(n_epochs):
                for lo, hi in cuts:
                    idx = perms[e, lo:hi]
                    pol.ppo_adv_moments(rows[2], idx, out=s["mom"])
                    pol.ppo_grad(s["params"], *rows, O, A, idx, CLIP, None, s["mom"], s["ctrl"], 0.5, 0.0,
                                 workspace=s["ws"], out=s["sums"], hidden=H)
                    pol.adam_apply(s["sums"], s["params"], s["m"], s["v"], s["ctrl"], LR, 0.5, stats=s["stats"][i])
                    i += 1

        update()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            update()
        torch.cuda.synchronize()
        keep.append((s, graph))
        arms[name] = graph.replay
    out = {"algo": "ppo", "samples": B, "batch_size": batch_size, "n_epochs": n_epochs,
           "minibatches_per_update": n_epochs * len(cuts),
           "launches": "one captured graph per update: moments + grad + apply per minibatch"}
    out.update(race(arms, B * n_epochs))
    return out


def main():
    if QUICK:
        cases = [a2c_case(1 << 14), ppo_case(1 << 14, 4096, 2), ppo_case(512, 64, 2)]
    else:
        cases = [a2c_case(1 << 19), a2c_case(1 << 22), ppo_case(1 << 19, 65536, 4), ppo_case(1 << 19, 4096, 4),
                 ppo_case(2048, 64, 10)]
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "device": torch.cuda.get_device_name(0), "quick": QUICK, "obs_dim": O, "act_dim": A,
           "arms": {"native": "64-unit kernels on the 64 x 64 net (P = 9,413)",
                    "padded": "128-unit kernels on the zero-padded net (P = 35,205)"},
           "cases": cases}
    path = os.path.join(ROOT, "profiles", "learner_h64", "bench.json")
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
