"""The policy host path of two checkouts compared on the CPU: the packed blobs, the packers'
refusals, the restated bf16 forwards and the cost of set_params.  Each checkout (built:
make -C gym-lorenz_amd) is loaded in processes of its own.

  python tools/pack_paths_check.py run <parent tree> <out dir>   (the branch: this tree)
      -> blob_equality.json, refusals.json, forward_equality.json, set_params_time.json;
         exit status 1 if any blob, refusal or forward output differs
  python tools/pack_paths_check.py time <parent tree> <out dir>  set_params_time.json alone
  python tools/pack_paths_check.py dump <tree> <what: blobs|refusals|forwards|time>
      one JSON object on stdout (what `run` starts)
"""
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

MLP_SHAPES = [(1, 1, 1), (3, 1, 64), (6, 2, 127), (8, 4, 128)]   # (O, A, H)
ATTN_SHAPES = [(1, 1), (6, 2), (8, 4)]                           # (O, A)
LN_SHAPES = [(i, a) for i in (1, 24, 32) for a in (1, 4)]        # (in_dim, A)
PRECISIONS = {"bf16": "", "fp32": "_f32", "i8x4": "_i8x4"}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def state_dict(pol, family, in_dim, act_dim, hidden=128, seed=0, log_std=0.0):
    """SB3 keys -> float32 arrays drawn from a seeded numpy.random.RandomState."""
    rs = np.random.RandomState(seed)
    H, F = hidden, 64
    sd = {}
    if family != "mlp":
        fe = [(128, in_dim), (128,), (48, 16), (48,), (16, 16), (16,), (F, 128), (F,)]
        for k, shp in zip(pol.ATTN_FE_KEYS, fe):
            sd[pol.FE + k] = (rs.standard_normal(shp) * 0.3).astype(np.float32)
        if family == "attn_ln":
            sd[pol.FE + "layer_norm.weight"] = (1 + 0.1 * rs.standard_normal(16)).astype(np.float32)
            sd[pol.FE + "layer_norm.bias"] = (0.1 * rs.standard_normal(16)).astype(np.float32)
    first = in_dim if family == "mlp" else F
    shapes = [(H, first), (H,), (H, H), (H,)] * 2 + [(act_dim, H), (act_dim,), (1, H), (1,)]
    for k, shp in zip(pol.KEYS, shapes):
        sd[k] = (rs.standard_normal(shp) * 0.3).astype(np.float32)
    sd["log_std"] = np.full((act_dim,), log_std, np.float32)
    return sd


def _packer(pol, family, precision):
    stem = {"mlp": "pack_policy", "attn": "pack_attn_policy", "attn_ln": "pack_attn_ln_policy"}[family]
    return getattr(pol, stem + PRECISIONS[precision])


def dump_blobs(pol, nat):
    out = {}
    for precision in PRECISIONS:
        for O, A, H in MLP_SHAPES:
            sd = state_dict(pol, "mlp", O, A, H, seed=O + H)
            out["mlp/%s/O%d_A%d_H%d" % (precision, O, A, H)] = _sha(_packer(pol, "mlp", precision)(sd, O, A))
        for family, shapes in (("attn", ATTN_SHAPES), ("attn_ln", LN_SHAPES)):
            for I, A in shapes:
                sd = state_dict(pol, family, I, A, seed=I + A)
                out["%s/%s/I%d_A%d" % (family, precision, I, A)] = _sha(_packer(pol, family, precision)(sd, I, A))
        for family, I in (("mlp", 6), ("attn", 6), ("attn_ln", 24)):  # a non-zero log_std
            sd = state_dict(pol, family, I, 2, seed=9, log_std=-0.7)
            sd["log_std"][1] = 0.4
            out["%s/%s/log_std" % (family, precision)] = _sha(_packer(pol, family, precision)(sd, I, 2))
    return out


# the ten C packers: family, takes `hidden`, blob-size function, widest input, arrays checked finite
C_PACKERS = {
    "lz_policy_pack": ("mlp", False, "lz_policy_blob_bytes", 8, ()),
    "lz_policy_pack_hidden": ("mlp", True, "lz_policy_blob_bytes", 8, ()),
    "lz_policy_pack_f32": ("mlp", True, "lz_policy_f32_blob_bytes", 8, ()),
    "lz_policy_pack_i8x4": ("mlp", True, "lz_policy_f32_blob_bytes", 8, ("pi_w2", "vf_w2")),
    "lz_attn_policy_pack": ("attn", False, "lz_attn_policy_blob_bytes", 8, ()),
    "lz_attn_policy_pack_f32": ("attn", False, "lz_attn_policy_f32_blob_bytes", 8, ()),
    "lz_attn_policy_pack_i8x4": ("attn", False, "lz_attn_policy_f32_blob_bytes", 8,
                                 ("pi_w1", "vf_w1", "post_w", "pi_w2", "vf_w2")),
    "lz_attn_ln_policy_pack": ("attn_ln", False, "lz_attn_ln_policy_blob_bytes", 32, ()),
    "lz_attn_ln_policy_pack_f32": ("attn_ln", False, "lz_attn_policy_f32_blob_bytes", 32, ()),
    "lz_attn_ln_policy_pack_i8x4": ("attn_ln", False, "lz_attn_policy_f32_blob_bytes", 32,
                                    ("pi_w1", "vf_w1", "post_w", "pi_w2", "vf_w2")),
}


def dump_refusals(pol, nat):
    """{case: [status, lz_last_error]} of every bad call (and the good one) of every packer."""
    out = {}
    for name, (family, takes_hidden, size_fn, max_in, finite) in C_PACKERS.items():
        fn = getattr(nat.lib, name)
        size = int(getattr(nat.lib, size_fn)())
        I = 6 if max_in == 8 else 24
        for hidden in ((128, 64) if takes_hidden else (128,)):
            sd = state_dict(pol, family, I, 2, hidden, seed=5)
            if family == "mlp":
                p, _H, arrs = pol._mlp_policy_struct(sd, I, 2)
                inner, fields = p, list(pol._FIELDS)
            else:
                p, arrs = pol._attn_struct(sd, I, 2, 64, family == "attn_ln")
                inner = p.attn if family == "attn_ln" else p
                fields = list(pol._ATTN_FE_FIELDS + pol._FIELDS)
            by_field = dict(zip(fields, arrs))
            blob = np.zeros(size, np.uint8)

            def call(tag, null_struct=False, null_blob=False, cap=size, hid=hidden):
                args = [None if null_struct else ctypes.byref(p)] + ([hid] if takes_hidden else [])
                st = int(fn(*args, None if null_blob else blob.ctypes.data, cap))
                msg = nat.lib.lz_last_error().decode(errors="replace") if st else ""
                out["%s/h%d/%s" % (name, hidden, tag)] = [st, msg]

            def with_field(obj, field, value, tag, **kw):
                old = getattr(obj, field)
                setattr(obj, field, value)
                call(tag, **kw)
                setattr(obj, field, old)

            call("ok")
            call("null_struct", null_struct=True)
            call("null_blob", null_blob=True)
            call("cap_short", cap=size - 1)
            for field, vals in (("obs_dim", (0, max_in + 1)), ("act_dim", (0, 5))):
                for v in vals:
                    with_field(inner, field, v, "%s_%d" % (field, v))
            if takes_hidden:
                call("hidden_0", hid=0)
                call("hidden_129", hid=129)
            for field in fields:
                with_field(inner, field, None, "null_" + field)
            if family == "attn_ln":
                with_field(p, "ln_w", None, "null_ln_w")
                with_field(p, "ln_b", None, "null_ln_b")
            for field in finite:
                for bad in ("nan", "inf"):
                    a = by_field[field]
                    old = a.flat[a.size - 1]
                    a.flat[a.size - 1] = float(bad)
                    call("%s_%s" % (bad, field))
                    a.flat[a.size - 1] = old
            with_field(inner, "obs_dim", 0, "null_blob+bad_dims", null_blob=True)
            with_field(inner, "vf_w2", None, "cap_short+null_weight", cap=size - 1)
            call("ok_again")
    return out


def dump_forwards(pol, nat):
    import torch

    out = {}
    for family, I, fwd in (("mlp", 6, pol.reference_forward_bf16), ("attn", 6, pol.reference_forward_attn_bf16),
                           ("attn_ln", 24, pol.reference_forward_attn_ln_bf16)):
        sd = state_dict(pol, family, I, 2, seed=11, log_std=-0.3)
        for n in (1, 7, 64):
            x = np.random.RandomState(n).standard_normal((n, I)).astype(np.float32) * 2.0
            mean, value = fwd(sd, x)
            assert mean.dtype == value.dtype == torch.float32 and mean.shape == (n, 2) and value.shape == (n,)
            assert bool(torch.isfinite(mean).all() and torch.isfinite(value).all())
            # equal digests of finite float32 tensors: torch.equal holds (and -0.0 is told from 0.0)
            out["%s/n%d" % (family, n)] = {"mean": _sha(mean.numpy()), "value": _sha(value.numpy())}
    return out


def dump_time(pol, nat, calls=200):
    """Median seconds of FusedRolloutCollector.set_params at fp32, on the CPU (no upload)."""
    out = {}
    for family, O, stack in (("mlp", 6, 1), ("attn", 6, 1), ("attn_ln", 6, 4)):
        class Env:
            num_envs, obs_dim, action_dim, system_name, device = 4, O, 2, "pmsm", "cpu"

        col = pol.FusedRolloutCollector.__new__(pol.FusedRolloutCollector)
        col.env, col.precision, col.frame_stack, col.obs_rms = Env, "fp32", stack, None
        col.vecnorm_update, col.O, col.A, col.device, col.training = None, O, 2, "cpu", True
        import torch

        sd = {k: torch.from_numpy(v) for k, v in state_dict(pol, family, O * stack, 2, seed=2).items()}
        for _ in range(calls):  # warm-up: allocator, caches, clocks
            col.set_params(sd)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            col.set_params(sd)
            ts.append(time.perf_counter() - t0)
        out[family] = statistics.median(ts)
    return out


def _child(tree, what):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "dump", tree, what],
                         capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-3000:])
        raise SystemExit(out.returncode)
    return json.loads(out.stdout.splitlines()[-1])


def run(parent, out_dir):
    branch = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(out_dir, exist_ok=True)
    bad = 0
    for what, fname in (("blobs", "blob_equality.json"), ("refusals", "refusals.json"),
                        ("forwards", "forward_equality.json")):
        a, b = _child(parent, what), _child(branch, what)
        differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        bad += len(differ)
        with open(os.path.join(out_dir, fname), "w") as f:
            json.dump({"cases": len(set(a) | set(b)),
                       "differ": {k: {"parent": a.get(k), "branch": b.get(k)} for k in differ},
                       "equal": {k: v for k, v in a.items() if k not in differ}}, f, indent=1, sort_keys=True)
        print("%s: %d cases, %d differ" % (what, len(a), len(differ)))
    run_time(parent, out_dir)
    return 1 if bad else 0


def run_time(parent, out_dir):
    branch = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(out_dir, exist_ok=True)
    runs = [(tag, _child(tree, "time")) for tag, tree in (("parent_1", parent), ("branch_1", branch),
                                                          ("parent_2", parent), ("branch_2", branch))]
    res = {"unit": "seconds, median of 200 set_params calls (fp32, CPU, no upload)", "runs": dict(runs)}
    res["verdict"] = {}
    for fam in runs[0][1]:
        p1, b1, p2, b2 = (r[fam] for _, r in runs)
        spread = abs(p1 - p2)
        res["verdict"][fam] = {"parent_median": statistics.median([p1, p2]), "parent_spread": spread,
                               "branch": b1, "branch_repeat": b2,
                               "branch_within_spread": b1 <= statistics.median([p1, p2]) + spread}
    with open(os.path.join(out_dir, "set_params_time.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res["verdict"]))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        sys.exit(run(os.path.abspath(sys.argv[2]), sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "time":
        sys.exit(run_time(os.path.abspath(sys.argv[2]), sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        sys.path.insert(0, os.path.join(os.path.abspath(sys.argv[2]), "gym-lorenz_amd"))
        from gym_lorenz import _native as nat
        from gym_lorenz import policy as pol

        fn = {"blobs": dump_blobs, "refusals": dump_refusals, "forwards": dump_forwards, "time": dump_time}
        print(json.dumps(fn[sys.argv[3]](pol, nat)))
        return
    sys.exit(__doc__)


if __name__ == "__main__":
    main()
