"""FusedEvaluator.evaluate(K) against the only other path to the same figures,
FusedRolloutCollector(deterministic=True, bootstrap=False).collect(K) (which materialises
the [K, N, *] buffers and runs the value net): same handle size, same policy, HIP-event
times after a warm-up, the two arms alternating in one process, at least 1 s per arm.

  PMSM  MlpPolicy   32,768 x 2048
  HR    attention   32,768 x 2048
  HR    attention  262,144 x 5000   evaluator only (the collector's buffer bytes recorded)

Writes profiles/eval/bench_eval.json and prints it.  Needs the MI355X: there is no fallback.
--quick shrinks K (smoke run of the tool itself, not a measurement).

--trace M: the trace arm instead.  The two 32,768 x 2048 shapes with three arms alternating
in one process -- the untraced evaluator, evaluate(K, trace=M env ids, stride 1) and the
collector (the only other route to those trajectories) -- into profiles/eval_trace/
bench.json.  traced_beats_collector: the traced launch's median is below the collector's by
more than the two arms' spreads (max - min) together."""
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
    sys.exit("bench_eval: no HIP device visible (the evaluation kernels need an MI355X)")
QUICK = "--quick" in sys.argv


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def collector_bytes(n, K, O, A):
    """Bytes of the [K, N, *] buffers collect(K) allocates: observations, actions, log-probs,
    values, rewards, episode starts (float32) and dones (uint8)."""
    return K * n * (4 * (O + A + 4) + 1)


def policy_of(kind, O, A):
    net = pol.ActorCriticAttn(O, A, seed=1) if kind == "attention" else pol.ActorCriticMlp(O, A, seed=1)
    return net.state_dict()


def summary(ts):
    return {"reps": len(ts), "min_s": min(ts), "median_s": statistics.median(ts), "max_s": max(ts),
            "spread": (max(ts) - min(ts)) / statistics.median(ts)}


def ab_trace(system, kind, n, K, M):
    envs = [gl.BatchedEnv(system, n, seed=3) for _ in range(3)]
    O, A = envs[0].obs_dim, envs[0].action_dim
    sd = policy_of(kind, O, A)
    ev, evt = pol.FusedEvaluator(envs[0], sd), pol.FusedEvaluator(envs[1], sd)
    col = pol.FusedRolloutCollector(envs[2], sd, deterministic=True, bootstrap=False, precision="fp32")
    for x in (ev, evt, col):
        x.reset()
    ids = [(i * n) // M for i in range(M)]  # spread over the tiles
    arms = {"untraced": lambda: ev.evaluate(K), "traced": lambda: evt.evaluate(K, trace=ids),
            "collector": lambda: col.collect(K)}
    for f in arms.values():  # warm-up
        f()
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    while min(sum(v) for v in ts.values()) < (0.05 if QUICK else 1.0) or len(ts["traced"]) < 5:
        for name, f in arms.items():  # alternating
            ts[name].append(timed(f))
    out = {"system": system, "policy": kind, "envs": n, "K": K, "trace_envs": M, "trace_every": 1,
           "trace_bytes": K * M * (O + A + 2) * 4, "collector_buffer_bytes": collector_bytes(n, K, O, A)}
    for name in arms:
        out[name] = summary(ts[name])
    med = {k: out[k]["median_s"] for k in arms}
    out["ratio_traced_over_untraced"] = med["traced"] / med["untraced"]
    out["ratio_traced_over_collector"] = med["traced"] / med["collector"]
    spreads = sum(out[k]["max_s"] - out[k]["min_s"] for k in ("traced", "collector"))
    out["traced_beats_collector"] = med["collector"] - med["traced"] > spreads
    for e in envs:
        e.close()
    return out


def ab(system, kind, n, K):
    env_e = gl.BatchedEnv(system, n, seed=3)
    env_c = gl.BatchedEnv(system, n, seed=3)
    O, A = env_e.obs_dim, env_e.action_dim
    sd = policy_of(kind, O, A)
    ev = pol.FusedEvaluator(env_e, sd)
    col = pol.FusedRolloutCollector(env_c, sd, deterministic=True, bootstrap=False, precision="fp32")
    ev.reset()
    col.reset()
    arms = {"evaluator": lambda: ev.evaluate(K), "collector": lambda: col.collect(K)}
    for f in arms.values():  # warm-up
        f()
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    while min(sum(v) for v in ts.values()) < (0.05 if QUICK else 1.0) or len(ts["evaluator"]) < 5:
        for name, f in arms.items():  # alternating A / B
            ts[name].append(timed(f))
    out = {"system": system, "policy": kind, "envs": n, "K": K,
           "evaluator": summary(ts["evaluator"]), "collector": summary(ts["collector"]),
           "collector_buffer_bytes": collector_bytes(n, K, O, A)}
    out["ratio_evaluator_over_collector"] = out["evaluator"]["median_s"] / out["collector"]["median_s"]
    out["evaluator_env_steps_per_s"] = n * K / out["evaluator"]["median_s"]
    out["collector_env_steps_per_s"] = n * K / out["collector"]["median_s"]
    env_e.close()
    env_c.close()
    return out


def evaluator_only(system, kind, n, K):
    env = gl.BatchedEnv(system, n, seed=3)
    O, A = env.obs_dim, env.action_dim
    ev = pol.FusedEvaluator(env, policy_of(kind, O, A))
    ev.reset()
    ev.evaluate(16)  # warm-up
    torch.cuda.synchronize()
    ts = [timed(lambda: ev.evaluate(K, skip=1000)) for _ in range(2)]
    env.close()
    return {"system": system, "policy": kind, "envs": n, "K": K, "evaluator": summary(ts),
            "evaluator_env_steps_per_s": n * K / statistics.median(ts),
            "stats_table_bytes": 24 * 8 * n, "collector_buffer_bytes": collector_bytes(n, K, O, A)}


def main_trace(M):
    K = 64 if QUICK else 2048
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "device": torch.cuda.get_device_name(0), "quick": QUICK,
           "cases": [ab_trace("pmsm", "mlp", 32768, K, M), ab_trace("hr", "attention", 32768, K, M)]}
    if not QUICK:
        out = os.path.join(ROOT, "profiles", "eval_trace")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


def main():
    if "--trace" in sys.argv:
        return main_trace(int(sys.argv[sys.argv.index("--trace") + 1]))
    K = 64 if QUICK else 2048
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "device": torch.cuda.get_device_name(0), "quick": QUICK,
           "cases": [ab("pmsm", "mlp", 32768, K), ab("hr", "attention", 32768, K),
                     evaluator_only("hr", "attention", 262144, 200 if QUICK else 5000)]}
    if not QUICK:  # a smoke run of the tool does not replace the measurement
        out = os.path.join(ROOT, "profiles", "eval")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "bench_eval.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
