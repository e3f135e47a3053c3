"""FusedEvaluator.evaluate(K) against the only other path to the same figures,
FusedRolloutCollector(deterministic=True, bootstrap=False).collect(K) (which materialises
the [K, N, *] buffers and runs the value net): same handle size, same policy, HIP-event
times after a warm-up, the two arms alternating in one process, at least 1 s per arm.

  PMSM  MlpPolicy   32,768 x 2048
  HR    attention   32,768 x 2048
  HR    attention  262,144 x 5000   evaluator only (the collector's buffer bytes recorded)

Writes profiles/eval/bench_eval.json and prints it.  Needs the MI355X: there is no fallback.
--quick shrinks K (smoke run of the tool itself, not a measurement)."""
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


def main():
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
