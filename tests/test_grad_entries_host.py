"""The five gradient entry points' refusals, the eight size functions and the Python binder,
as recorded from the library before their host code was folded into one form table and one
rule per entry point (csrc/lz_grad_common.h): tests/golden/grad_refusals.json holds, per
entry point and case, the status and the lz_last_error() text after its "<entry point>: ";
per size function, the sha256 of its values over a grid that crosses every limit (43,680
values in all, nearly all of them -1: the digest keeps the file readable) with how many are
not -1 and the largest; and what policy._grad_fns returns or raises.  The test replays all of
it against the built library and asks for equal statuses, equal message bytes and equal
sizes.  No GPU, and no HIP call: every case's workspace is one byte short of what
its own arguments need, so arguments that pass every other check are refused at the
workspace, the last check before hipSetDevice (a failed hipSetDevice would leave its error
behind for the next HIP user of the process).  That a workspace of exactly the size asked for
is taken is what tests/test_gpu_grad_entries.py launches with.

`python tests/test_grad_entries_host.py` (with the package and tests/ on sys.path) rewrites
the golden file from the library it finds; it was run once, on the parent's build."""
import ctypes
import hashlib
import json
import math
import os
import struct

from gym_lorenz import _native as nat
from gym_lorenz import policy as pol

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_refusals.json")
NO_DEVICE = -1  # never reached: were a refusal missing, hipSetDevice would fail and nothing launch

A2C_BUFFERS = ("params", "observations", "actions", "advantages", "returns", "workspace", "grad_sums")
PPO_BUFFERS = A2C_BUFFERS + ("old_log_prob", "old_values", "indices")

# entry point -> (argument struct, its workspace function, takes hidden, the accepted (obs_dim, hidden))
ENTRIES = {
    "lz_a2c_grad_f32": (nat.LzA2cGradArgs, "lz_a2c_workspace_bytes", False, (6, 128)),
    "lz_a2c_grad_hidden_f32": (nat.LzA2cGradArgs, "lz_a2c_workspace_bytes_hidden", True, (6, 64)),
    "lz_ppo_grad_f32": (nat.LzPpoGradArgs, "lz_ppo_workspace_bytes", False, (6, 128)),
    "lz_ppo_grad_hidden_f32": (nat.LzPpoGradArgs, "lz_ppo_workspace_bytes_hidden", True, (6, 64)),
    "lz_ppo_grad_wide_f32": (nat.LzPpoGradArgs, "lz_ppo_workspace_bytes_wide", True, (24, 64)),
}


def cases(ppo):
    """[(name, {field: value})]: what each case changes in the accepted block."""
    out = [("accepted but for the workspace", {})]
    out += [("NULL " + f, {f: None}) for f in (PPO_BUFFERS if ppo else A2C_BUFFERS)]
    out += [("obs_dim %d" % v, {"obs_dim": v}) for v in (0, 9, 24, 25)]
    out += [("act_dim %d" % v, {"act_dim": v}) for v in (0, 5)]
    out += [("n_samples 0", {"n_samples": 0})]
    if ppo:
        out += [("n_rows 0", {"n_rows": 0}),
                ("n_samples > n_rows without indices", {"indices": None, "n_samples": 334}),
                ("clip_range -1", {"clip_range": -1.0}), ("clip_range inf", {"clip_range": math.inf}),
                ("clip_range nan", {"clip_range": math.nan}),
                ("clip_range_vf nan", {"clip_range_vf": math.nan}),
                ("clip_range_vf inf", {"clip_range_vf": math.inf}),
                ("clip_range_vf > 0 with NULL old_values", {"clip_range_vf": 0.05, "old_values": None})]
    out += [("max_workgroups %d" % v, {"max_workgroups": v}) for v in (-1, 4097)]
    out += [("hidden %d" % v, {"hidden": v}) for v in (0, 32, 64, 96, 128, 256)]
    out += [("workspace 0", {"workspace_bytes": 0})]
    # two faults at once: which one is reported fixes the order of the checks
    out += [("obs_dim 25 and hidden 96", {"obs_dim": 25, "hidden": 96}),
            ("act_dim 5 and hidden 96", {"act_dim": 5, "hidden": 96}),
            ("max_workgroups 4097 and hidden 96", {"max_workgroups": 4097, "hidden": 96}),
            ("hidden 96 and workspace 0", {"hidden": 96, "workspace_bytes": 0}),
            ("n_samples 0 and max_workgroups 4097", {"n_samples": 0, "max_workgroups": 4097}),
            ("NULL params and obs_dim 0", {"params": None, "obs_dim": 0})]
    if ppo:
        out += [("n_rows 0 and max_workgroups 4097", {"n_rows": 0, "max_workgroups": 4097}),
                ("NULL old_values with clip_range_vf > 0 and obs_dim 0",
                 {"clip_range_vf": 0.05, "old_values": None, "obs_dim": 0}),
                ("clip_range nan and max_workgroups -1", {"clip_range": math.nan, "max_workgroups": -1})]
    return out


def _need(entry, g):
    """What the entry point's workspace function asks for g's arguments (-1: it refuses them)."""
    _, ws_name, takes_hidden, _ = ENTRIES[entry]
    h = (g.hidden,) if takes_hidden else ()
    return getattr(nat.lib, ws_name)(g.n_samples, g.obs_dim, g.act_dim, *h, g.max_workgroups)


def accepted_block(entry, obs_dim, hidden):
    """Arguments the entry point accepts but for a workspace one byte short: 111 samples (of
    333 rows), act_dim 2; the pointers are never dereferenced."""
    struct = ENTRIES[entry][0]
    ppo = struct is nat.LzPpoGradArgs
    g = struct()
    for f in (PPO_BUFFERS if ppo else A2C_BUFFERS):
        setattr(g, f, ctypes.c_void_p(0x1000))
    g.n_samples, g.obs_dim, g.act_dim, g.hidden, g.max_workgroups = 111, obs_dim, 2, hidden, 0
    g.vf_coef, g.ent_coef = 0.5, 0.0
    if ppo:
        g.n_rows, g.clip_range, g.clip_range_vf = 333, 0.2, 0.0
    need = _need(entry, g)
    assert need > 0, (entry, obs_dim, hidden)
    g.workspace_bytes = need - 1
    return g


def refusals(entry):
    """[[case, status, lz_last_error() after "<entry>: "]] of one entry point."""
    struct, _, _, (obs_dim, hidden) = ENTRIES[entry]
    fn = getattr(nat.lib, entry)

    def row(case, status):
        text = nat.lib.lz_last_error().decode()
        assert text.startswith(entry + ": "), (entry, case, text)  # the whole text: prefix + record
        return [case, status, text[len(entry) + 2:]]

    out = [row("NULL args", fn(None, NO_DEVICE, None))]
    for name, change in cases(struct is nat.LzPpoGradArgs):
        g = accepted_block(entry, obs_dim, hidden)
        for f, v in change.items():
            setattr(g, f, v)
        need = _need(entry, g)  # of the changed arguments, where they are still accepted
        if need > 0 and "workspace_bytes" not in change:
            g.workspace_bytes = need - 1
        assert g.workspace_bytes < need or need < 0
        out.append(row(name, fn(ctypes.byref(g), NO_DEVICE, None)))
    return out


GRID = {"obs_dim": list(range(26)), "act_dim": [0, 1, 4, 5], "hidden": [0, 64, 96, 128],
        "n": [0, 1, 32, 33, 5000], "cap": [-1, 0, 1, 128, 4096, 4097]}
COUNTS = {"lz_a2c_param_count": False, "lz_a2c_param_count_hidden": True, "lz_ppo_param_count_wide": True}
WORKSPACES = {"lz_a2c_workspace_bytes": False, "lz_a2c_workspace_bytes_hidden": True,
              "lz_ppo_workspace_bytes": False, "lz_ppo_workspace_bytes_hidden": True,
              "lz_ppo_workspace_bytes_wide": True}


def sizes():
    """{function: its values over GRID, obs_dim outermost; a function without `hidden` skips that axis}."""
    return {name: _digest(values) for name, values in _size_values().items()}


def _digest(values):
    """[how many values, how many are not -1, the largest, sha256 of them as little-endian int64]."""
    assert all(v == -1 or v > 0 for v in values)
    return [len(values), sum(v > 0 for v in values), max(values),
            hashlib.sha256(struct.pack("<%dq" % len(values), *values)).hexdigest()]


def _size_values():
    out = {}
    for name, takes_hidden in COUNTS.items():
        fn = getattr(nat.lib, name)
        out[name] = [fn(O, A, *h) for O in GRID["obs_dim"] for A in GRID["act_dim"]
                     for h in ([(H,) for H in GRID["hidden"]] if takes_hidden else [()])]
    for name, takes_hidden in WORKSPACES.items():
        fn = getattr(nat.lib, name)
        out[name] = [fn(n, O, A, *h, cap) for O in GRID["obs_dim"] for A in GRID["act_dim"]
                     for h in ([(H,) for H in GRID["hidden"]] if takes_hidden else [()])
                     for n in GRID["n"] for cap in GRID["cap"]]
    return out


def binder():
    """policy._grad_fns over (kind, hidden, wide, (O, A)): [key, P, workspace_bytes(111, 0), the
    entry point's name], or [key, exception type, status, message]."""
    out = []
    for kind in ("a2c", "ppo"):
        for hidden in (64, 128, 96):
            for wide in (False, True):
                for O, A in ((6, 2), (9, 2), (24, 2), (25, 2)):
                    key = "%s hidden %d wide %d obs %d act %d" % (kind, hidden, wide, O, A)
                    try:
                        P, ws, fn = pol._grad_fns(kind, hidden, O, A, "who", wide)
                        out.append([key, P, ws(111, 0), fn.__name__])
                    except Exception as e:  # noqa: BLE001 -- the type is part of the record
                        out.append([key, type(e).__name__, getattr(e, "status", None), str(e)])
    return out


def record():
    return {"refusals": {entry: refusals(entry) for entry in ENTRIES}, "grid": GRID, "sizes": sizes(),
            "binder": binder()}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_refusal_is_the_recorded_one():
    gold = _golden()["refusals"]
    assert set(gold) == set(ENTRIES)
    for entry in ENTRIES:
        got = refusals(entry)
        # every case of this module is in the file, in this order
        assert [r[0] for r in got] == [r[0] for r in gold[entry]], entry
        for g, want in zip(got, gold[entry]):
            assert g == want, (entry, g, want)
            assert want[1] in (nat.LZ_ERR_INVALID, nat.LZ_ERR_UNSUPPORTED)


def test_the_recorded_order_of_the_refusals():
    """What the file must say for the order to be the documented one (so a wrong recording
    could not pin a wrong order): dims before hidden, max_workgroups before hidden, hidden
    before the workspace, n_rows before max_workgroups, hidden alone LZ_ERR_UNSUPPORTED."""
    for entry, rows in _golden()["refusals"].items():
        for case, status, what in rows:
            if case == "NULL args":
                assert (status, what) == (nat.LZ_ERR_INVALID, "NULL args")
            elif case in ("obs_dim 25 and hidden 96", "act_dim 5 and hidden 96"):
                assert status == nat.LZ_ERR_INVALID and what.startswith("obs_dim must be 1.."), (entry, case)
            elif case == "max_workgroups 4097 and hidden 96":
                assert (status, what) == (nat.LZ_ERR_INVALID, "max_workgroups must be 0..4096")
            elif case in ("hidden 96 and workspace 0", "hidden 96", "hidden 0", "hidden 32", "hidden 256"):
                assert status == nat.LZ_ERR_UNSUPPORTED and what.startswith("hidden must be "), (entry, case)
            elif case == "n_rows 0 and max_workgroups 4097":
                assert (status, what) == (nat.LZ_ERR_INVALID, "n_rows < 1")
            elif case == "n_samples 0 and max_workgroups 4097":
                assert (status, what) == (nat.LZ_ERR_INVALID, "n_samples < 1")
            elif case.startswith("NULL old_values with clip_range_vf > 0 and"):
                assert (status, what) == (nat.LZ_ERR_INVALID, "NULL old_values with clip_range_vf > 0")
            elif case == "NULL params and obs_dim 0":
                assert (status, what) == (nat.LZ_ERR_INVALID, "NULL buffer")
            elif case in ("workspace 0", "accepted but for the workspace"):
                assert status == nat.LZ_ERR_INVALID and what == "workspace smaller than " + ENTRIES[entry][1]


def test_the_size_functions_are_the_recorded_ones():
    gold = _golden()
    assert gold["grid"] == GRID
    got = sizes()
    assert set(got) == set(gold["sizes"]) == set(COUNTS) | set(WORKSPACES)
    for name, digest in got.items():
        assert digest == gold["sizes"][name], name
        assert 0 < digest[1] < digest[0], name


def test_the_binder_is_the_recorded_one():
    gold = _golden()["binder"]
    got = binder()
    assert len(got) == len(gold) == 2 * 3 * 2 * 4
    for g, want in zip(got, gold):
        assert g == want, (g, want)
    kinds = {r[1] for r in gold if isinstance(r[1], str)}
    assert kinds == {"LorenzEnvError"}
    assert {r[3] for r in gold if not isinstance(r[1], str)} == set(ENTRIES)


def _dump(rec):
    """The record as JSON, one case per line."""
    def rows(v):
        return "[\n" + ",\n".join("    " + json.dumps(r) for r in v) + "\n  ]"

    parts = ['"refusals": {\n' + ",\n".join('  %s: %s' % (json.dumps(k), rows(v))
                                             for k, v in rec["refusals"].items()) + "\n}",
             '"grid": ' + json.dumps(rec["grid"]),
             '"sizes": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v))
                                          for k, v in rec["sizes"].items()) + "\n}",
             '"binder": ' + rows(rec["binder"])]
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    text = _dump(record())
    assert json.loads(text) == json.loads(json.dumps(record()))
    with open(GOLDEN, "w") as f:
        f.write(text)
    print("wrote %s: %d bytes" % (GOLDEN, len(text)))
