#!/bin/bash
# asm_count.sh [OUT]: every kernel of the device layer as a file of its own, beside the resource
# table (cross-compiles; no GPU needed).  The units are the Makefile's DEV_SRC, compiled side by side.
#   OUT/<unit>.s          the device-side assembly of one unit (device.s, points.s, ...)
#   OUT/kernels/<name>.s  one kernel: its code and its .amdhsa_kernel descriptor, with what
#                         legitimately differs between two builds of the same code stripped
#                         (.file, .ident, .loc, the __hip_cuid_<hash> symbol, comments, and the
#                         function's ordinal in the file that its local labels carry: .LBB<n>_)
#   OUT/rest.<unit>.s     everything else of a unit, stripped the same way: device functions that were
#                         not inlined, constant tables, LDS symbols (not the metadata notes, which
#                         repeat the descriptors in the order the kernels were instantiated in)
#   OUT/resources.txt     VGPRs, AGPRs, SGPRs, scratch, occupancy, LDS and the instruction mix
# RENAME="old=new old2=new2": symbol prefixes replaced in every line before the split (device functions
# and constant tables that moved to another namespace keep their code and change their mangled names:
# the kernels that call them then differ from the older build in those names alone).
# SRC=<file> compiles that one file alone with this tree's headers: a unit, or another copy of the
# device layer (the parent's device.hip, say, from before it was split or after).  Two builds are
# then compared with
#   scripts/asm_diff.py A B          (or: diff -rq A/kernels B/kernels; diff A/resources.txt B/resources.txt)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/asm}
CSRC=$ROOT/turtle_amd/csrc
UNITS=${SRC:-$(sed -n 's/^DEV_SRC *:= *//p' "$CSRC/Makefile" | tr ' ' '\n' | sed "s|^|$CSRC/|")}
mkdir -p "$OUT"
rm -rf "$OUT/kernels" "$OUT"/rest*.s
mkdir "$OUT/kernels"
stems=()
pids=()
for src in $UNITS; do
    stem=$(basename "${src%.*}")
    stems+=("$stem")
    /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 \
        -I"$ROOT/include" -I"$CSRC" -S --cuda-device-only "$src" -o "$OUT/$stem.s" \
        -Rpass-analysis=kernel-resource-usage 2> "$OUT/remarks.$stem.txt" &
    pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
python3 - "$OUT" "${stems[@]}" <<'EOF'
import hashlib, os, re, sys
out, stems = sys.argv[1], sys.argv[2:]
rename = [p.split('=', 1) for p in os.environ.get('RENAME', '').split()]
strip = re.compile(r'^\s*(;|\.file\b|\.ident\b|\.loc\b)|__hip_cuid_')
kernels, order = {}, []
symbol = re.compile(r'_Z\w+')
ordinal = re.compile(r'\.L(BB|JTI|func_begin|func_end)\d+')
for stem in stems:
    cur, desc, rest, meta = None, None, [], False
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', open(f'{out}/{stem}.s').read(), re.M))
    for line in open(f'{out}/{stem}.s'):
        if strip.search(line):
            continue
        if '"' not in line:  # (a comment starts at a ';' -- but not inside a string's quotes)
            line = line.split(';')[0].rstrip() + '\n'
        line = ordinal.sub(r'.L\1', line)
        for old, new in rename:
            line = line.replace(old, new)
        m = re.match(r'^(\S+):', line)
        if m and m.group(1) in names and cur is None:
            cur = m.group(1); kernels.setdefault(cur, []); order.append(cur)
        if cur:
            kernels[cur].append(line)
            if line.startswith('.Lfunc_end'):
                cur = None
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', line)
        if m:
            desc = m.group(1)
        if desc:
            kernels.setdefault(desc, []).append(line)
            if '.end_amdhsa_kernel' in line:
                desc = None
            continue
        # a kernel's own directives (.section, .globl, .type, .size, .set <kernel>.num_vgpr ...) go with
        # it: kernels come out in the order they were instantiated in, which is not the code's business
        m = symbol.search(line)
        if m and m.group(0) in names:
            kernels.setdefault(m.group(0), []).append(line)
        elif '.amdgpu_metadata' in line:
            meta = not meta
        elif not meta:
            rest.append(line)
    open(f'{out}/rest.{stem}.s', 'w').writelines(rest)
for k, lines in kernels.items():
    # (hipCUB's kernels have names longer than a file's may be)
    short = k if len(k) <= 200 else k[:180] + '_' + hashlib.sha1(k.encode()).hexdigest()[:12]
    open(f'{out}/kernels/{short}.s', 'w').writelines(lines)

res, name = {}, None
keys = {'VGPRs': 'vgpr', 'AGPRs': 'agpr', 'TotalSGPRs': 'sgpr', 'ScratchSize [bytes/lane]': 'scratch',
        'Occupancy [waves/SIMD]': 'occ', 'LDS Size [bytes/block]': 'lds'}
for line in (l for stem in stems for l in open(f'{out}/remarks.{stem}.txt')):
    m = re.search(r'remark: (.*?)\s*\[-Rpass', line)
    if not m:
        continue
    k, _, v = m.group(1).strip().partition(':')
    if k.strip() == 'Function Name':
        name = v.strip(); res[name] = {}
    elif name and k.strip() in keys:
        res[name][keys[k.strip()]] = v.strip()
def count(lines, pat):
    r = re.compile(pat)
    return sum(1 for l in lines if r.match(l))
with open(f'{out}/resources.txt', 'w') as f:
    for k in sorted(order):
        body = kernels[k][:next(i for i, l in enumerate(kernels[k]) if l.startswith('.Lfunc_end'))]
        row = ' '.join(f'{a}={b}' for a, b in res.get(k, {}).items())
        mix = {'total': r'^\s+[a-z]', 'f64': r'^\s+v_[a-z_0-9]+_f64', 'valu': r'^\s+v_', 'salu': r'^\s+s_',
               'vmem': r'^\s+(global|flat|buffer)_'}
        f.write(f'{k} {row} ' + ' '.join(f'{a}={count(body, b)}' for a, b in mix.items()) + '\n')
print(f'{len(order)} kernels -> {out}/kernels, {out}/resources.txt')
EOF
grep -E "${KERNELS:-k_(trace|step)}" "$OUT/resources.txt" || true
