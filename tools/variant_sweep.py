"""Every launch of tests/test_gpu_variant_bits.py, once each, as a plain script: the
tuning-variant selectors (lz_config.reserved[0]; table in DESIGN.md) and the family-only
launches they are compared against, in a fixed order.  Run under a kernel trace, the
ordered kernel names show which instantiation the launcher picked for every bit:

  rocprofv3 --kernel-trace -d out -o run --output-format csv -- python tools/variant_sweep.py
  LZ_LIB_AB=<other .so> rocprofv3 --kernel-trace ... -- python tools/variant_sweep.py
  python tools/variant_sweep.py --names out/**/run_kernel_trace.csv     # the names, in start order

Two builds whose launchers agree give the same list (profiles/rollout_ring/).  Prints one
line per launch: the call, system, N, TimeLimit, variant and the reported launch shape.
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-lorenz_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import gym_lorenz as gl
    import test_gpu_variant_bits as t

    def go(run, call, system, n, tl, variant):
        shape, _ = run(gl, system, n, tl, variant)
        print("%s %s n=%d tl=%d variant=%d %s" % (call, system, n, tl, variant, shape["kernel"]), flush=True)

    seen = set()
    for n in t.ROLLOUT_SIZES:
        for system, tl, family, selector in t.ROLLOUT_CASES:
            for variant in (family, family | selector):
                if (system, n, tl, variant) not in seen:
                    seen.add((system, n, tl, variant))
                    go(t.run_rollout, "rollout", system, n, tl, variant)
    for system in sorted(t.SYSTEMS):
        for v in (0,) + t.STEP_V:
            go(t.run_steps, "step", system, 1031, 3, v)
        for v in (t.E4, t.E4 | (1 << 22)):
            go(t.run_steps, "step", system, 1613, 3, v)


def names(path):
    """The env kernels of a rocprofv3 kernel-trace csv, in start order (torch's own kernels --
    copies, fills, sorts -- are left out: only lz:: kernels are the launcher's choice)."""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        if "lz::" in r["Kernel_Name"] or "N2lz" in r["Kernel_Name"]:
            print(r["Kernel_Name"])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--names"]:
        names(sys.argv[2])
    else:
        main()
