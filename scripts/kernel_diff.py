#!/usr/bin/env python3
"""Compare device code function by function: scripts/kernel_diff.py <parent.s> <head.s> [<head2.s> ...]

The inputs are device assembly files, `hipcc <the Makefile's flags> -S --cuda-device-only file.hip -o file.s`.  Every
function of the parent must be defined exactly once in the head files taken together, with the same instructions and,
for a kernel, the same `.amdhsa_kernel` descriptor block (registers, LDS, scratch).  Assembler comments are dropped and
the numbers that depend on a function's position in its file (.LBB<f>_<n>, .LJTI<f>_<n>, .Lfunc_*<f>, .Ltmp<n>) are
normalised, so code that only moved between files compares equal.  Text only: nothing here knows an instruction.
Prints one line per function and exits non-zero unless every line says SAME.
"""
import re
import sys

TYPE = re.compile(r'\s*\.type\s+(\S+),@function')
FUNC_END = re.compile(r'\.Lfunc_end\d+:')
PER_FUNC = re.compile(r'\.(LBB|LJTI|LCPI|Lfunc_begin|Lfunc_end)\d+')
TMP = re.compile(r'\.Ltmp\d+')


def functions(path):
    """{mangled name: [(code lines, descriptor lines), ...]} of one assembly file."""
    out, name, code, desc, pending, in_desc = {}, None, None, None, set(), False
    for raw in open(path):
        m = TYPE.match(raw)
        if m:
            pending.add(m.group(1))
        line = raw.split(';', 1)[0].rstrip()
        if name is None:
            if line.endswith(':') and line[:-1] in pending:
                name, code, desc, tmp = line[:-1], [], [], {}
            continue
        if FUNC_END.match(line):
            out.setdefault(name, []).append((code, desc))
            name = None
            continue
        if not line.strip():
            continue
        line = PER_FUNC.sub(lambda m: '.' + m.group(1), line)
        line = TMP.sub(lambda m: '.Ltmp%d' % tmp.setdefault(m.group(0), len(tmp)), line)
        in_desc = in_desc or line.strip().startswith('.amdhsa_kernel')
        (desc if in_desc else code).append(line)
        in_desc = in_desc and line.strip() != '.end_amdhsa_kernel'
    return out


def first_diff(a, b):
    for i in range(max(len(a), len(b))):
        x, y = a[i] if i < len(a) else '<end>', b[i] if i < len(b) else '<end>'
        if x != y:
            return 'line %d:\n    parent: %s\n    head  : %s' % (i + 1, x.strip(), y.strip())
    return ''


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    parent, head = functions(argv[1]), {}
    for path in argv[2:]:
        for name, bodies in functions(path).items():
            head.setdefault(name, []).extend((path, b) for b in bodies)
    bad = 0
    for name in sorted(set(parent) | set(head)):
        kind = 'kernel  ' if any(d for _, d in parent.get(name, [])) or any(b[1] for _, b in head.get(name, [])) else 'function'
        verdict, detail = 'SAME', ''
        if name not in parent:
            verdict, detail = 'EXTRA', 'not in the parent; defined in ' + ', '.join(p for p, _ in head[name])
        elif len(parent[name]) != 1:
            verdict, detail = 'TWICE', 'in the parent'
        elif name not in head:
            verdict = 'MISSING'
        elif len(head[name]) != 1:
            verdict, detail = 'TWICE', 'defined in ' + ', '.join(p for p, _ in head[name])
        else:
            (pc, pd), (hc, hd) = parent[name][0], head[name][0][1]
            detail = first_diff(pc, hc) or (first_diff(pd, hd) and 'descriptor ' + first_diff(pd, hd))
            verdict = 'DIFF' if detail else 'SAME'
        bad += verdict != 'SAME'
        print('%-7s %s %s' % (verdict, kind, name))
        if detail:
            print('  ' + detail)
    kernels = sum(1 for n in parent if parent[n][0][1])
    print('%d functions (%d kernels) in the parent, %d not SAME' % (len(parent), kernels, bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
