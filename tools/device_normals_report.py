#!/usr/bin/env python3
"""Record how close the device's normals come to their Philox prescription: the worst
err / tol of every GPU case of tests/test_gpu_noise.py::test_device_noise_step and
tests/test_gpu_policy_sampling.py (the cases' own runners, so tests/device_normals.py's
tolerance), and the HR float64 case's largest recovered error in units of z -- there the
rounding terms are near 1e-12, so that figure is the hardware transcendentals' error itself.

    python tools/device_normals_report.py [--out profiles/device_normals/worst.json]

One GPU run: each group of cases runs in a fresh child process under its own timeout, and
nothing more is started after a group that failed or timed out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (("process_noise", 300), ("action_samples", 420), ("ticks", 180), ("shards", 180))  # (name, seconds)


def run_group(name):
    for p in (ROOT, os.path.join(ROOT, "gym-lorenz_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import gym_lorenz as gl
    import oracle as orc
    from gym_lorenz import policy as pol

    orc.lib()
    out = {}
    if name == "process_noise":
        import test_gpu_noise as tn

        for case in tn.STEP_CASES:
            r = tn.run_step_case(gl, orc, case)
            out[tn.step_case_id(case)] = r["worst"]
            if case[0] == "hr" and case[1] == "float64":
                out["hr_float64_largest_error_in_z"] = r["z_err"]
        return out
    import test_gpu_policy_sampling as ts

    if name == "action_samples":
        for case in ts.FAMILY_CASES:
            out[ts.family_case_id(case)] = ts.run_family_case(gl, pol, orc, case)
    elif name == "ticks":
        for kind in (ts.F32_MLP, ts.F32_STEP):
            out[kind] = ts.run_ticks_case(gl, pol, orc, kind)
    else:
        for gid0, seed in [(0, ts.SEED)] + ts.SHARDS:
            out["offset_%d_seed_%d" % (gid0, seed)] = ts.run_shard_case(gl, pol, orc, gid0, seed)[0]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_normals", "worst.json"))
    ap.add_argument("--group", help=argparse.SUPPRESS)   # the child's
    ap.add_argument("--json", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.group:
        with open(args.json, "w") as f:
            json.dump(run_group(args.group), f)
        return 0
    report = {"figure": "worst |recovered - prescribed| / tolerance per case (tests/device_normals.py); "
                        "<= 1 passes",
              "hardware_term": "HW(z) = 1e-3 / 3 + 1e-5 |z|, times the sample's std"}
    with tempfile.TemporaryDirectory() as tmp:
        for name, seconds in GROUPS:
            path = os.path.join(tmp, name + ".json")
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", name, "--json", path],
                                    timeout=seconds).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("device_normals_report: group %s ended with %d; nothing more is started" % (name, rc))
                return rc
            with open(path) as f:
                report[name] = json.load(f)
            print("%s: %s" % (name, json.dumps(report[name])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
