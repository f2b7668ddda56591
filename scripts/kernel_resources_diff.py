"""Side-by-side register / scratch / LDS figures of the kernels two builds of a library have in common:

    python scripts/kernel_resources_diff.py before.so after.so [--md]

Exit status 1 if a kernel of `before` is missing from `after` or any of its figures differs (the check that a change
left the existing kernels' code objects alone); kernels only `after` has are listed as new.
"""
import sys

from kernel_resources import kernels

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def table(lib):
    return {r["name"]: r for r in kernels(lib)}


def main(argv):
    md = "--md" in argv
    before, after = [a for a in argv if not a.startswith("--")][:2]
    a, b = table(before), table(after)
    bad = 0
    rows = []
    for name, ra in sorted(a.items(), key=lambda kv: kv[1]["kernel"]):
        rb = b.get(name)
        fa = tuple(ra.get(k, 0) for k in KEYS)
        fb = tuple(rb.get(k, 0) for k in KEYS) if rb else None
        same = fa == fb
        bad += 0 if same else 1
        rows.append((ra["kernel"], fa, fb, same))
    new = [(r["kernel"], tuple(r.get(k, 0) for k in KEYS)) for n, r in sorted(b.items(), key=lambda kv: kv[1]["kernel"]) if n not in a]
    fmt = (lambda k, x, y, s: f"| `{k}` | {' / '.join(map(str, x))} | {' / '.join(map(str, y)) if y else 'missing'} | {'=' if s else 'DIFFERS'} |") \
        if md else (lambda k, x, y, s: f"{k:90s} {x} {y} {'=' if s else 'DIFFERS'}")
    print("(" + " / ".join(KEYS) + ")")
    for r in rows:
        print(fmt(*r))
    for k, f in new:
        print(f"| `{k}` | new | {' / '.join(map(str, f))} | |" if md else f"{k:90s} new {f}")
    print(f"{len(rows)} kernels in common, {bad} differ, {len(new)} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
