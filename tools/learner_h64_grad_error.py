"""Accuracy table of the 64-unit gradient kernels (lz_a2c_grad_hidden_f32 and
lz_ppo_grad_hidden_f32 at hidden = 64): at every shape of tests/mlp_learner_ref.CASES and on
the reference's two shipped PPO policies (as weights on a synthetic batch), three seeds each,
err_gpu = ||g_gpu - g64|| / ||g64|| and err_t32 (torch float32 CPU autograd of the 64-unit net,
what SB3 would compute) against its float64 autograd -- per tensor, for the whole vector and
for the loss sums (PPO: every option on, and the kl sum) -- and the ratio
err_gpu / max(err_t32, 2^-24).  tests/test_gpu_learner_h64.py's bounds are twice the worst
ratio recorded here, per algorithm.  The sibling of tools/a2c_grad_error.py and
tools/ppo_grad_error.py.

  python tools/learner_h64_grad_error.py [--out profiles/learner_h64/grad_error.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gym-lorenz_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def measure(kind, label, c, ref, pol, dev):
    gpu, cpu = (ref.gpu_a2c, ref.cpu_a2c) if kind == "a2c" else (ref.gpu_ppo, ref.cpu_ppo)
    g64, g32 = cpu(c, torch.float64), cpu(c, torch.float32)
    got = gpu(pol, dev, c).cpu().numpy()
    slices, P = ref.slices(kind, c["O"], c["A"])
    rows = {k: {"err_gpu": e, "err_t32": t, "ratio": r}
            for k, (e, t, r) in ref.accuracy_rows(got, g64, g32, slices).items()}
    n = c["B"] if kind == "a2c" else c["M"]
    assert got[P + 3] == n, (label, got[P:])
    if kind == "ppo":
        assert got[P + 4] == g64[P + 4], (label, got[P:], g64[P:])
    tensors = [k for k in rows if k != "all" and not k.endswith("_sum")]
    worst_tensor = max(tensors, key=lambda k: rows[k]["ratio"])
    keep = [k for k in rows if k == "all" or k.endswith("_sum")] + [worst_tensor]
    return {"kind": kind, "case": label, "n": n, "O": c["O"], "A": c["A"], "cap": c["cap"], "seed": c["seed"],
            "worst_ratio": max(v["ratio"] for v in rows.values()), "worst_tensor": worst_tensor,
            "rows": {k: rows[k] for k in keep}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learner_h64", "grad_error.json"))
    args = ap.parse_args()
    import a2c_ref
    import mlp_learner_ref as ref
    from gym_lorenz import policy as pol

    dev = torch.device("cuda", 0)
    runs = []
    for kind in ("a2c", "ppo"):
        for label, build in ref.accuracy_cases(kind):
            for seed in ref.SEEDS:
                r = measure(kind, label, build(seed), ref, pol, dev)
                runs.append(r)
                w = max(r["rows"].items(), key=lambda kv: kv[1]["ratio"])
                print("%s %-14s seed %d all: gpu %.3e t32 %.3e ratio %.2f   worst %s ratio %.2f"
                      % (kind, label, seed, r["rows"]["all"]["err_gpu"], r["rows"]["all"]["err_t32"],
                         r["rows"]["all"]["ratio"], w[0], w[1]["ratio"]), flush=True)
    out = {"reference": "torch float64 CPU autograd of the 64-unit net (tests/a2c_ref.py, tests/ppo_ref.py)",
           "err_floor": a2c_ref.ERR_FLOOR, "hidden": 64}
    for kind in ("a2c", "ppo"):
        per = {}
        for r in runs:
            if r["kind"] == kind:
                per[r["case"]] = max(per.get(r["case"], 0.0), r["worst_ratio"])
        out["worst_ratio_per_case_" + kind] = per
        out["worst_ratio_" + kind] = max(per.values())
    out["worst_ratio"] = max(out["worst_ratio_a2c"], out["worst_ratio_ppo"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:  # one run per line
        f.write(json.dumps(out, indent=1)[:-2] + ',\n "runs": [\n  ')
        f.write(",\n  ".join(json.dumps(r) for r in runs) + "\n ]\n}\n")
    print("worst ratio a2c %.3f ppo %.3f -> %s" % (out["worst_ratio_a2c"], out["worst_ratio_ppo"], args.out))


if __name__ == "__main__":
    main()
