#!/usr/bin/env python3
"""asm_diff.py A B: two dumps of scripts/asm_count.sh compared kernel by kernel (no GPU needed).

One row per kernel: identical / DIFFERS (its stripped disassembly and descriptor), and the resources of A
-- and of B behind them where they are not the same; then whatever belongs to no kernel (rest.s).
The exit status is 0 when nothing differs."""
import filecmp, os, subprocess, sys

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
rest = filecmp.cmp(os.path.join(a, "rest.s"), os.path.join(b, "rest.s"), shallow=False)
print("outside the kernels (rest.s):", "identical" if rest else "DIFFERS")
print("%d kernels, %d differ" % (len(names), different))
sys.exit(0 if (different == 0 and rest) else 1)
