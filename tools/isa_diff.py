#!/usr/bin/env python3
"""Compare two gfx950 device assembly listings of the library kernel by kernel (CPU only).

    hipcc <Makefile HIPFLAGS> -DLG_BUILD_ID='"x"' --cuda-device-only -S lg_api.hip -o a.s     (same for b.s)
    tools/isa_diff.py a.s b.s [--alias REGEX=REPLACEMENT ...]

Kernels are matched by their demangled name (up to the parameter list).  --alias rewrites those names in both builds before matching:
a kernel template that gained a trailing parameter is compared with what it was by
    --alias 'lg_preprocess(_bwd)?<(\w+, \w+), false>=lg_preprocess\1<\2>' --alias 'lg_camera_bwd<(\w+), false>=lg_camera_bwd<\1>'

Compares instruction TEXT only (labels renumbered in order of appearance, directives and comments dropped): which kernels
differ, their instruction counts, and both builds' register / LDS / scratch figures from the code-object metadata.
"""
import re
import subprocess
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def parse(path):
    text = open(path).read()
    kernels, meta, cur, labels = {}, {}, None, {}
    for line in text.split("amdhsa.kernels:")[0].splitlines():
        m = re.match(r"(\w+):", line)
        if m and not line.startswith(".L"):
            cur, labels = kernels.setdefault(m.group(1), []), {}
            continue
        if line.lstrip().startswith(".end_amdhsa_kernel") or re.match(r"\s*\.(section|text)", line):
            cur = None
        ins = line.split(";")[0].strip()
        if cur is None or not ins or ins.startswith(".") and not ins.startswith(".L"):
            continue
        ins = re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), ins)
        cur.append(" ".join(ins.split()))
    for block in text.split("amdhsa.kernels:")[1].split("  - .agpr_count:")[1:]:
        vals = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)", block, re.M))
        meta[vals[".name"]] = [vals.get(f, "?") for f in FIELDS]
    return {k: v for k, v in kernels.items() if k in meta}, meta


def by_pretty_name(kernels, meta, aliases):
    """Both tables keyed by the demangled name without its parameter list, after the aliases."""
    names = sorted(kernels)
    demangled = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout.splitlines()
    key = {}
    for n, d in zip(names, demangled):
        d = d.split("(")[0]
        for pat, repl in aliases:
            d = re.sub(pat, repl, d)
        assert d not in key.values(), "two kernels share the name " + d
        key[n] = d
    return {key[n]: v for n, v in kernels.items()}, {key[n]: meta[n] for n in kernels}


def main(a, b, *rest):
    aliases = [tuple(r.split("=", 1)) for flag, r in zip(rest[::2], rest[1::2]) if flag == "--alias"]
    assert len(rest) == 2 * len(aliases), "usage: isa_diff.py a.s b.s [--alias REGEX=REPLACEMENT ...]"
    (ka, ma), (kb, mb) = by_pretty_name(*parse(a), aliases), by_pretty_name(*parse(b), aliases)
    names = sorted(set(ka) | set(kb))
    pretty = {n: n for n in names}
    differ = [n for n in names if ka.get(n) != kb.get(n)]
    count = lambda k, n: sum(not i.endswith(":") for i in k[n]) if n in k else "-"      # label definitions are not instructions
    print("%d kernels, %d instruction-identical, %d differ" % (len(names), len(names) - len(differ), len(differ)))
    for n in differ:
        print("DIFFERS  %5s -> %5s instructions  %s" % (count(ka, n), count(kb, n), pretty[n].split("(")[0]))
    print("\nvgpr / sgpr / lds / scratch  (a | b)")
    for n in names:
        fa, fb = ma.get(n, ["-"] * 4), mb.get(n, ["-"] * 4)
        print("%s %-19s | %-19s %s" % (" " if fa == fb else "*", " ".join(fa), " ".join(fb), pretty[n].split("(")[0]))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
