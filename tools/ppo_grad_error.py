"""Accuracy table of lz_ppo_grad_f32: at every shape of tests/ppo_ref.CASES, three seeds and
every option set of ppo_ref.OPTIONS (the (O, A) corners and the one-sample case: all options
together only), err_gpu = ||g_gpu - g64|| / ||g64|| and err_t32 (torch float32 CPU autograd,
what SB3 would compute) against the float64 autograd of tests/ppo_ref.py -- per tensor, for
the whole vector, for the three loss sums and the kl sum -- and the ratio
err_gpu / max(err_t32, 2^-24).  tests/test_gpu_ppo.py's bound is twice the worst ratio
recorded here.  The file keeps, per run and on one line, the whole vector, the four sums and
the tensor with the worst ratio (every quantity is measured and enters worst_ratio).

  python tools/ppo_grad_error.py [--out profiles/ppo/grad_error.json]
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


def gpu_sums(c, opt, ref, pol, dev, **kw):
    """lz_ppo_grad_f32 (after lz_ppo_adv_moments when the option normalises) on a case."""
    name, M, n_rows, O, A, cap = c["case"]
    normalize, vclip, ent = ref.OPTIONS[opt]
    rows = [t.to(dev) for t in c["rows"]]
    idx = c["idx"].to(dev)
    mom = pol.ppo_adv_moments(rows[2], idx) if normalize and M > 1 else None
    kw.setdefault("max_workgroups", cap)
    return pol.ppo_grad(ref.a2c_ref.flatten(c["sd"]).to(dev), *rows, O, A, idx, ref.CLIP,
                        ref.CLIP_VF if vclip else None, mom, None, 0.5, ent, **kw)


def cpu_sums(c, opt, ref, dtype):
    normalize, vclip, ent = ref.OPTIONS[opt]
    return ref.grad_sums(c["sd"], ref.minibatch(c), normalize, ref.CLIP_VF if vclip else None, ent,
                         dtype=dtype)


def measure(c, opt, ref, pol, dev):
    name, M, n_rows, O, A, cap = c["case"]
    g64, g32 = cpu_sums(c, opt, ref, torch.float64), cpu_sums(c, opt, ref, torch.float32)
    gpu = gpu_sums(c, opt, ref, pol, dev).cpu().numpy()
    slices, P = ref.check_slices(O, A)
    rows = {}
    for k, sl in slices.items():
        e_gpu, e_t32 = ref.a2c_ref.rel_err(gpu[sl], g64[sl]), ref.a2c_ref.rel_err(g32[sl], g64[sl])
        rows[k] = {"norm64": float(np.linalg.norm(g64[sl])), "err_gpu": e_gpu, "err_t32": e_t32,
                   "ratio": e_gpu / max(e_t32, ref.a2c_ref.ERR_FLOOR)}
    assert gpu[P + 3] == M and gpu[P + 4] == g64[P + 4], (name, opt, gpu[P + 3:], g64[P + 3:])
    tensors = [k for k in rows if k != "all" and not k.endswith("_sum")]
    worst_tensor = max(tensors, key=lambda k: rows[k]["ratio"])
    keep = ["all", "policy_sum", "value_sum", "entropy_sum", "kl_sum", worst_tensor]
    return {"case": name, "M": M, "n_rows": n_rows, "O": O, "A": A, "cap": cap, "seed": c["seed"],
            "options": opt, "worst_ratio": max(v["ratio"] for v in rows.values()),
            "worst_tensor": worst_tensor, "rows": {k: rows[k] for k in keep}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo", "grad_error.json"))
    args = ap.parse_args()
    import ppo_ref as ref
    from gym_lorenz import policy as pol

    dev = torch.device("cuda", 0)
    runs = []
    for case in ref.CASES:
        for seed in ref.SEEDS:
            c = ref.make_case(case, seed)
            opts = list(ref.OPTIONS) if case[0] in ("m111", "m5155_cap3") else ["all"]
            for opt in opts:
                r = measure(c, opt, ref, pol, dev)
                runs.append(r)
                w = max(r["rows"].items(), key=lambda kv: kv[1]["ratio"])  # (the kept rows hold the worst)
                print("%-12s seed %d %-5s all: gpu %.3e t32 %.3e ratio %.2f   worst %s ratio %.2f"
                      % (r["case"], seed, opt, r["rows"]["all"]["err_gpu"], r["rows"]["all"]["err_t32"],
                         r["rows"]["all"]["ratio"], w[0], w[1]["ratio"]), flush=True)
    worst = {}
    for r in runs:
        worst[r["case"]] = max(worst.get(r["case"], 0.0), r["worst_ratio"])
    out = {"reference": "tests/ppo_ref.py float64 autograd", "err_floor": ref.a2c_ref.ERR_FLOOR,
           "worst_ratio_per_case": worst, "worst_ratio": max(worst.values())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:  # one run per line
        f.write(json.dumps(out, indent=1)[:-2] + ',\n "runs": [\n  ')
        f.write(",\n  ".join(json.dumps(r) for r in runs) + "\n ]\n}\n")
    print("worst ratio %.3f -> %s" % (out["worst_ratio"], args.out))


if __name__ == "__main__":
    main()
