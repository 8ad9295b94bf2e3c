#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of device assembly files, kernel by kernel (no GPU needed).

    make -C kafka_assignment_optimizer_amd/csrc device-asm                 # writes build/*.s, here and in a checkout of the other commit
    tools/compare_kernel_asm.py --old OLD/build/*.s --new NEW/build/*.s

A kernel is the text from its label to the end of its function: the instructions and the .amdhsa_* descriptor (registers, scratch, LDS).
Comments, blank lines, .file / .ident lines and the __hip_cuid_* symbol are ignored, and the function number in local labels (.LBB12_3 ->
.LBB_3) is dropped, so a kernel may move between translation units.  A kernel of an unnamed namespace that several files define (a
shared header) is compared per file.  Exit status 0 iff both sides hold the same kernel names and every
kernel compares equal.

A template that gains a defaulted parameter renames its old instantiations; --rename REGEX REPLACEMENT (repeatable) rewrites the text of
the NEW side first, so that they are compared under the names they had."""
import argparse
import os
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
LOCAL = re.compile(r"\.L(BB|func_end|func_begin|post_getpc|JTI|CPI|tmp)(\d+)")


def kernels(paths, renames=()):
    found = []
    for path in paths:
        text = open(path).read()
        for pattern, repl in renames:
            text = re.sub(pattern, repl, text)
        lines = text.split("\n")
        names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
        name, body = None, []
        for line in lines:
            m = LABEL.match(line)
            if m and m.group(1) in names:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            text = line.split(";")[0].rstrip()
            if text.strip() and not re.match(r"\s*\.(file|ident)\b", text) and "__hip_cuid_" not in text:
                body.append(LOCAL.sub(lambda g: ".L" + g.group(1), text))
            if re.match(r"\.Lfunc_end\d+:", line):
                found.append((name, os.path.basename(path), body))
                name = None
    count = {}
    for name, _, _ in found:
        count[name] = count.get(name, 0) + 1
    out = {}
    for name, base, body in found:
        key = name if count[name] == 1 else name + " in " + base
        assert key not in out, "kernel defined twice: " + key
        out[key] = body
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"), help="rewrite the NEW side's text before comparing")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new, a.rename)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("ONLY IN %s: %s" % ("OLD" if name in old else "NEW", name)); bad += 1
        elif old[name] != new[name]:
            n = sum(1 for x, y in zip(old[name], new[name]) if x != y) + abs(len(old[name]) - len(new[name]))
            print("DIFFERS (%d of %d lines): %s" % (n, len(old[name]), name)); bad += 1
    print("%d kernels before, %d after, %d identical" % (len(old), len(new), len(set(old) & set(new)) - sum(1 for k in set(old) & set(new) if old[k] != new[k])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
