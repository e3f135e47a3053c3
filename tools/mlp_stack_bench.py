"""The record of the frame-stacked 64-unit MlpPolicy (code/lorenz_filter/train.py:109-131) under
profiles/mlp_stack/: measured, no bar.

  grad_error.json  the wide PPO gradient kernel (lz_ppo_grad_wide_f32 at obs_dim 24) against
                   torch float64 CPU autograd at every tests/ppo_stack_ref.py case, advantage
                   normalisation on and off, three seeds: err_gpu, err_t32 and the ratio
                   err_gpu / max(err_t32, 2^-24) per tensor, whole vector and sums
  bench.json       (a) one collect of HR (add_filter) 32,768 envs x 2048 steps on
                   VecFrameStack(4): the stacked MlpPolicy next to the LayerNorm attention
                   policy, alternating in one process, device events around collect();
                   (b) one PPO minibatch gradient at M = 4,096: k_ppo_grad_h64_wide (24
                   inputs) next to k_ppo_grad_h64 (6 inputs), alternating; medians

  python tools/mlp_stack_bench.py [--out profiles/mlp_stack] [--rounds 5] [--skip-collect]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gym-lorenz_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def grad_error(pol, dev):
    import a2c_ref
    import mlp_learner_ref as ref
    import ppo_stack_ref as ps

    slices, P = ref.slices("ppo", ps.O_WIDE, ps.A)
    runs = []
    for name, M, cap in ps.CASES:
        for normalize in (True, False):
            for seed in ps.SEEDS:
                c = ps.case(name, seed)
                g64, g32 = ps.cpu(c, torch.float64, normalize), ps.cpu(c, torch.float32, normalize)
                got = ps.gpu(pol, dev, c, normalize).cpu().numpy()
                assert got[P + 3] == M and got[P + 4] == g64[P + 4], (name, got[P:], g64[P:])
                rows = {k: {"err_gpu": e, "err_t32": t, "ratio": r}
                        for k, (e, t, r) in ref.accuracy_rows(got, g64, g32, slices).items()}
                worst = max(rows, key=lambda k: rows[k]["ratio"])
                keep = [k for k in rows if k == "all" or k.endswith("_sum")] + [worst]
                runs.append({"case": name, "M": M, "cap": cap, "normalize": normalize, "seed": seed,
                             "worst_ratio": rows[worst]["ratio"], "worst": worst,
                             "rows": {k: rows[k] for k in dict.fromkeys(keep)}})
                print("%-11s norm=%d seed %d all ratio %.2f worst %s %.2f" % (
                    name, normalize, seed, rows["all"]["ratio"], worst, rows[worst]["ratio"]), flush=True)
    per = {}
    for r in runs:
        per[r["case"]] = max(per.get(r["case"], 0.0), r["worst_ratio"])
    sums = {}
    for r in runs:
        for k, v in r["rows"].items():
            if k == "all" or k.endswith("_sum"):
                sums[k] = max(sums.get(k, 0.0), v["ratio"])
    return {"reference": "torch float64 CPU autograd (tests/ppo_ref.py), O = 24, A = 2, hidden 64",
            "err_floor": a2c_ref.ERR_FLOOR, "bound": ps.RATIO, "worst_ratio": max(per.values()),
            "worst_ratio_per_case": per, "worst_ratio_whole_vector_and_sums": sums, "runs": runs}


def collect_bench(gl, pol, rounds):
    import mlp_learner_ref as ref

    n, K = 32768, 2048
    out = {"shape": "hr add_filter %d envs x %d steps, frame_stack 4, fp32, bootstrap on" % (n, K)}
    cols = {}
    for name, sd in (("mlp_stack", ref.make_policy(24, 2, 3)),
                     ("attn_ln", pol.ActorCriticAttn(24, 2, seed=3, layer_norm=True).state_dict())):
        env = gl.BatchedEnv("hr", n, seed=4, add_filter=True)
        col = pol.FusedRolloutCollector(env, sd, frame_stack=4, precision="fp32")
        col.reset()
        col.collect(K)  # warm-up at the timed shape
        torch.cuda.synchronize()
        cols[name] = col
    times = {k: [] for k in cols}
    for _ in range(rounds):
        for name, col in cols.items():
            times[name].append(timed(lambda: col.collect(K)))
    for name, t in times.items():
        med = statistics.median(t)
        out[name] = {"collect_s": t, "median_s": med, "env_steps_per_s": n * K / med}
    out["mlp_stack_over_attn_ln"] = out["attn_ln"]["median_s"] / out["mlp_stack"]["median_s"]
    return out


def grad_bench(pol, dev, rounds):
    import a2c_ref
    import mlp_learner_ref as ref

    M = 4096
    out = {"M": M, "calls_per_round": 50}
    cases = {}
    for name, O, wide in (("k_ppo_grad_h64_wide_O24", 24, True), ("k_ppo_grad_h64_O6", 6, False)):
        c = ref.ppo_case(("m4096", M, O, 2, 0, False), 0)
        rows = [t.to(dev) for t in c["rows"]]
        idx = c["idx"].to(dev)
        params = a2c_ref.flatten(c["sd"]).to(dev)
        mom = pol.ppo_adv_moments(rows[2], idx)
        P = params.numel()
        ws = torch.empty((128 * (P + 6),), dtype=torch.float64, device=dev)
        sums = torch.empty((P + 6,), dtype=torch.float64, device=dev)
        fn = (lambda rows=rows, idx=idx, params=params, mom=mom, ws=ws, sums=sums, O=O, wide=wide:
              pol.ppo_grad(params, *rows, O, 2, idx, 0.2, 0.2, mom, None, 0.5, 0.01, workspace=ws, out=sums,
                           hidden=64, wide=wide))
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        cases[name] = fn
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(lambda: [fn() for _ in range(50)]) / 50)
    for name, t in times.items():
        out[name] = {"per_call_s": t, "median_us": statistics.median(t) * 1e6}
    out["note"] = "grad + reduce launches per call, host enqueue included (device events around 50 calls)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_stack"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    import gym_lorenz as gl
    from gym_lorenz import policy as pol

    assert torch.cuda.is_available(), "needs the MI355X: nothing here is measured on a CPU"
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    ge = grad_error(pol, dev)
    runs = ge.pop("runs")
    with open(os.path.join(args.out, "grad_error.json"), "w") as f:  # one run per line
        f.write(json.dumps(ge, indent=1)[:-2] + ',\n "runs": [\n  ')
        f.write(",\n  ".join(json.dumps(r) for r in runs) + "\n ]\n}\n")
    print("worst ratio %.3f (bound %.3f)" % (ge["worst_ratio"], ge["bound"]))
    bench = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
             "ppo_minibatch": grad_bench(pol, dev, args.rounds)}
    if not args.skip_collect:
        bench["collect"] = collect_bench(gl, pol, args.rounds)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        json.dump(bench, f, indent=1)
        f.write("\n")
    print(json.dumps(bench, indent=1))


if __name__ == "__main__":
    main()
