"""Accuracy table of lz_a2c_grad_f32: at every shape of tests/a2c_ref.CASES and three seeds,
err_gpu = ||g_gpu - g64|| / ||g64|| and err_t32 (torch float32 CPU autograd, what SB3 would
compute) against the float64 autograd of tests/a2c_ref.py -- per tensor, for the whole
vector and for the three loss sums -- and the ratio err_gpu / max(err_t32, 2^-24).
tests/test_gpu_a2c.py's bound is twice the worst ratio recorded here.

  python tools/a2c_grad_error.py [--out profiles/a2c/grad_error.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gym-lorenz_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def measure(case, seed, ref, pol, dev):
    name, B, O, A, cap, _ = case
    sd, batch = ref.case_inputs(case, seed)
    g64 = ref.grad_sums(sd, batch, dtype=torch.float64)
    g32 = ref.grad_sums(sd, batch, dtype=torch.float32)
    flat = ref.flatten(sd).to(dev)
    gpu = pol.a2c_grad(flat, *[t.to(dev) for t in batch], O, A, 0.5, 0.0,
                       max_workgroups=cap).cpu().numpy()
    P = gpu.size - 4
    rows = {}
    parts = dict(ref.per_tensor(g64[:P], O, A))
    for k in list(parts) + ["all", "policy_sum", "value_sum", "entropy_sum"]:
        if k == "all":
            sl = slice(0, P)
        elif k.endswith("_sum"):
            i = P + ("policy_sum", "value_sum", "entropy_sum").index(k)
            sl = slice(i, i + 1)
        else:
            o, shp = ref.layout(O, A)[0][k]
            sl = slice(o, o + int(np.prod(shp)))
        e_gpu, e_t32 = ref.rel_err(gpu[sl], g64[sl]), ref.rel_err(g32[sl], g64[sl])
        rows[k] = {"norm64": float(np.linalg.norm(g64[sl])), "err_gpu": e_gpu, "err_t32": e_t32,
                   "ratio": e_gpu / max(e_t32, ref.ERR_FLOOR)}
    assert gpu[P + 3] == B
    return {"case": name, "B": B, "O": O, "A": A, "cap": cap, "seed": seed, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2c", "grad_error.json"))
    args = ap.parse_args()
    import a2c_ref as ref
    from gym_lorenz import policy as pol

    dev = torch.device("cuda", 0)
    runs = [measure(c, s, ref, pol, dev) for c in ref.CASES for s in ref.SEEDS]
    worst = {}
    for r in runs:
        w = max(r["rows"].items(), key=lambda kv: kv[1]["ratio"])
        worst[r["case"]] = max(worst.get(r["case"], 0.0), w[1]["ratio"])
        print("%-12s seed %d  all: gpu %.3e t32 %.3e ratio %.2f   worst tensor %s ratio %.2f"
              % (r["case"], r["seed"], r["rows"]["all"]["err_gpu"], r["rows"]["all"]["err_t32"],
                 r["rows"]["all"]["ratio"], w[0], w[1]["ratio"]), flush=True)
    out = {"reference": "tests/a2c_ref.py float64 autograd", "err_floor": ref.ERR_FLOOR,
           "worst_ratio_per_case": worst, "worst_ratio": max(worst.values()), "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("worst ratio %.3f -> %s" % (out["worst_ratio"], args.out))


if __name__ == "__main__":
    main()
