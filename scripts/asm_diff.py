#!/usr/bin/env python3
"""asm_diff.py A B: two dumps of scripts/asm_count.sh compared kernel by kernel (no GPU needed).

One row per kernel: identical / DIFFERS (its stripped disassembly and descriptor), and the resources of A
-- and of B behind them where they are not the same; then whatever belongs to no kernel (each unit's
rest*.s), symbol by symbol: a device function or a table must be the same wherever a unit has a copy of it.
The exit status is 0 when nothing differs."""
import filecmp, glob, os, re, subprocess, sys

a, b = sys.argv[1:3]


def table(d):
    return dict(line.rstrip("\n").split(" ", 1) for line in open(os.path.join(d, "resources.txt")))


ra, rb = table(a), table(b)
fa, fb = (sorted(os.listdir(os.path.join(d, "kernels"))) for d in (a, b))
names = sorted(ra)
plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
different = 0
for f in sorted(set(fa) ^ set(fb)):
    print("only in one of them:", f)
    different += 1
by_file = {f[:180]: f for f in fa}
for name, shown in zip(names, plain):
    f = by_file.get(name[:180] if len(name) > 200 else name + ".s"[:0] or name)
    f = f if f is not None else by_file.get((name + ".s")[:180])
    same = (f in fb) and filecmp.cmp(os.path.join(a, "kernels", f), os.path.join(b, "kernels", f), shallow=False)
    different += 0 if same else 1
    shown = shown.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0]
    if len(shown) > 60:
        shown = shown[:57] + "..."
    row = "%-60s %s  %s" % (shown, "identical" if same else "DIFFERS  ", ra[name])
    if rb.get(name) != ra[name]:
        row += "  ->  " + str(rb.get(name))
    print(row)


def symbols(d):
    """{symbol: {its text: the units that hold it so}} over the units' rest*.s: a device function that was not
    inlined with its .size and .set lines, or a table with its data.  (Each unit that needs one has its copy.)"""
    found = {}
    for f in sorted(glob.glob(os.path.join(d, "rest*.s"))):
        unit = os.path.basename(f)[len("rest."):-len(".s")] or "-"
        name, text = None, []
        for line in list(open(f)) + ["\n"]:
            if name and (not line.strip() or re.match(r"\s+\.(section|type|text)\b", line)):
                found.setdefault(name, {}).setdefault("".join(text), []).append(unit)
                name = None
            m = re.match(r"([^\s.]\S*):", line)
            if m and name is None:
                name, text = m.group(1), []
            if name:
                text.append(line)
    return found


sa, sb = symbols(a), symbols(b)
rest = 0
for name in sorted(set(sa) | set(sb)):
    ta, tb = sa.get(name, {}), sb.get(name, {})
    same = (len(ta) == 1) and (set(ta) == set(tb))
    rest += 0 if same else 1
    shown = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    # the units of B that hold it; where it differs, which of them hold it as A has it
    where = ", ".join("+".join(u) + ("" if same else " (as in A)" if t in ta else " (not as in A)") for t, u in tb.items())
    print("%-60s %s  %s" % (shown[:57] + "..." if len(shown) > 60 else shown, "identical" if same else "DIFFERS  ",
                            where or "in A only"))
print("outside the kernels (rest*.s): %d symbols, %d differ" % (len(set(sa) | set(sb)), rest))
print("%d kernels, %d differ" % (len(names), different))
sys.exit(0 if (different == 0 and rest == 0) else 1)
