#!/usr/bin/env python3
"""tools/kstats_compare.py ROUNDS PARENT1.csv NEW1.csv PARENT2.csv NEW2.csv [KERNEL-PREFIX ...]: the table of profiles/r23_lazy_policy_kernel_stats.txt from four
`*_kernel_stats.csv` files of tools/kstats_plies.sh (runs in the order parent, new, parent, new).  Per kernel: the average us per launch of every run, the parent's mean
and spread (max - min), bound = mean + spread, and where the new runs lie; then the sum of all kernels per search round (ROUNDS = search rounds of a run, warm-up ply
included) and the sum of the kernels named by the prefixes (default: the three kernels of the base evaluations)."""
import csv
import sys

BASE = ("k_trunk<15, false, true, true, true>", "k_fc0_x3<2, false>", "k_facc_reduce")


def load(path):
    out = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].replace("void omok::", "").replace("omok::", "").split("(")[0]  # (without the parameter list: a changed signature is still the same kernel)
        calls, t = out.get(name, (0, 0.0))
        out[name] = (calls + int(r["Calls"]), t + float(r["TotalDurationNs"]) / 1e3)
    return out


def main(argv):
    rounds = int(argv[1])
    runs = [load(p) for p in argv[2:6]]
    prefixes = tuple(argv[6:]) or BASE
    par, new = (runs[0], runs[2]), (runs[1], runs[3])
    total = sum(t for _, t in runs[0].values())
    names = sorted(set().union(*runs), key=lambda k: -runs[0].get(k, (0, 0.0))[1])
    for k in names:
        share = runs[0].get(k, (0, 0.0))[1] / total
        if share < 0.004 and not k.startswith(prefixes) and not k.startswith("k_group"):
            continue
        if not all(k in r for r in runs):
            print(f"  {k[:44]:44s}  not launched in every run: calls " + " ".join(str(r.get(k, (0, 0.0))[0]) for r in runs) + "  average us "
                  + " ".join(f"{r[k][1] / r[k][0]:.2f}" if k in r else "-" for r in runs))
            continue
        a = [r[k][1] / r[k][0] for r in par]
        b = [r[k][1] / r[k][0] for r in new]
        mean, spread = sum(a) / 2, max(a) - min(a)
        where = "both new below both parent" if max(b) < min(a) else "both new above both parent" if min(b) > max(a) else "within"
        if where == "both new above both parent" and max(b) <= mean + spread:
            where += " (inside the bound)"
        print(f"  {k[:44]:44s}  calls {runs[0][k][0]:5d}  parent {a[0]:8.2f} {a[1]:8.2f} (mean {mean:8.2f}, spread {spread:5.2f})  new {b[0]:8.2f} {b[1]:8.2f} (mean {sum(b) / 2:8.2f})  "
              f"bound {mean + spread:8.2f} us  {where}  growth {sum(b) / 2 - mean:+.2f}")
    for label, pick in (("base kernels " + " + ".join(p.split("<")[0] for p in prefixes), lambda k: k.startswith(prefixes)), ("all kernels", lambda k: True)):
        s = [sum(t for k, (_, t) in r.items() if pick(k)) / rounds for r in runs]
        a, b = (s[0], s[2]), (s[1], s[3])
        where = "both new below both parent" if max(b) < min(a) else "both new above both parent" if min(b) > max(a) else "not separated"
        print(f"  {label}, us per search round ({rounds} rounds): parent {a[0]:.1f} {a[1]:.1f}  new {b[0]:.1f} {b[1]:.1f}   means {sum(a) / 2:.1f} -> {sum(b) / 2:.1f}: "
              f"{sum(b) / 2 - sum(a) / 2:+.1f}; the parent's spread {max(a) - min(a):.1f}; {where}")


if __name__ == "__main__":
    if len(sys.argv) < 6:
        sys.exit(__doc__)
    main(sys.argv)
