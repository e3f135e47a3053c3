"""Host cost of one eager lz_step call: 50,000 back-to-back calls on a 256-env LORENZ3
handle with one synchronisation at the end, five repeats, microseconds per call.  At 256
envs the kernel is far shorter than the call, so the time is the host's: validation, the
launch, and whatever an entry point does before it (the stream query of a
capture guard was weighed with this and left out).

    python tools/host_call.py                       one process, prints one JSON line
    LZ_LIB_AB=<other .so> python tools/host_call.py the same against another build
    python tools/host_call.py merge OUT.json parent=P1.json,P2.json branch=B1.json,B2.json [note=TEXT]
        the record of an interleaved parent / branch comparison (profiles/graph_replay/):
        every repeat of both, the branch's median and the parent's own min - max
"""
import ctypes
import json
import os
import statistics
import sys
import time

CALLS, REPEATS, ENVS = 50000, 5, 256


def measure():
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-lorenz_amd"))
    import gym_lorenz as gl
    from gym_lorenz import _native as nat

    env = gl.BatchedEnv("lorenz3", ENVS, seed=1)
    stream = torch.cuda.Stream(env.device)  # a non-NULL stream, as a capturable handle has
    nat.check(nat.lib.lz_set_stream(env._h, ctypes.c_void_p(stream.cuda_stream)))
    acts = torch.zeros((ENVS, env.action_dim), device=env.device)
    args = env.step_args(acts, env.obs, env.rew, env.done, env.done_idx, env.term_obs)
    torch.cuda.synchronize()
    env.reset()
    step, h = nat.lib.lz_step, env._h
    us = []
    for rep in range(REPEATS + 1):  # the first repeat warms up and is dropped
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            step(h, *args)
        torch.cuda.synchronize()
        if rep:
            us.append((time.perf_counter() - t0) / CALLS * 1e6)
    nat.check(nat.lib.lz_step(h, *args))  # the status of one call: nothing above failed silently
    env.close()
    return {"library": os.path.basename(os.path.dirname(nat.LIB_PATH)) + "/" + os.path.basename(nat.LIB_PATH),
            "calls": CALLS, "envs": ENVS, "us_per_call": us}


def merge(out, groups):
    note = groups.pop("note", None)
    rec = {"what": "eager lz_step host call, %d calls + one sync, %d-env LORENZ3, us per call; processes "
                   "alternated parent / branch" % (CALLS, ENVS)}
    if note:
        rec["note"] = note[0]
    for name, files in groups.items():
        runs = [json.load(open(f))["us_per_call"] for f in files]
        flat = [x for r in runs for x in r]
        rec[name] = {"runs": runs, "median": statistics.median(flat), "min": min(flat), "max": max(flat)}
    b, p = rec["branch"]["median"], rec["parent"]
    rec["branch_median_inside_parent_min_max"] = p["min"] <= b <= p["max"]
    rec["branch_median_not_above_parent_max"] = b <= p["max"]
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in rec if k.startswith("branch_median")}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "merge":
        merge(sys.argv[2], {k: v.split(",") for k, v in (a.split("=") for a in sys.argv[3:])})
    else:
        print(json.dumps(measure()))
