#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly files (hipcc --cuda-device-only -S), no GPU needed.

    tools/isa_diff.py before.s after.s [--show N] [--kernel SUBSTRING] [--rename OLD=NEW ...]

For every kernel: is the instruction stream identical (comments and directives stripped; the function number
in .LBB<function>_<block> labels dropped)?
For those that are not: next_free_vgpr / accum_offset / scratch / LDS of the kernel descriptor and static counts of
the instructions that matter (v_mfma, ds_read, ds_write, buffer_load, buffer_store, s_barrier, s_waitcnt, scratch_),
one row per file.  --show N prints the first N differing lines of each such kernel.  Exit status 1 if any kernel differs.
--rename OLD=NEW (repeatable) replaces OLD by NEW in the demangled names of `before` first, to pair kernels across a rename
("gram_k_kernel<=gram_kernel<"); kernels are then matched by demangled name.
Two compiles of one source differ only in the __hip_cuid_* symbol, so a whole-file cmp says nothing; this does.
"""
import argparse
import collections
import difflib
import re
import subprocess

META = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
OPS = ("v_mfma", "ds_read", "ds_write", "buffer_load", "buffer_store", "s_barrier", "s_waitcnt", "scratch_")


def parse(path):
    """-> {kernel: [instruction lines]}, {kernel: {descriptor field: value}}"""
    bodies, meta, cur, desc = {}, {}, None, None
    for line in open(path):
        if cur is None:
            m = re.match(r"^(\w+):", line)
            if m and not m.group(1).startswith(".L"):
                cur, body = m.group(1), []
                continue
        else:
            if line.startswith(".Lfunc_end"):
                bodies[cur], cur = body, None
                continue
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") or re.match(r"^\.LBB\d+_\d+:", s):
                body.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", s)))
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            desc = meta.setdefault(m.group(1), {})
        m = re.match(r"^\s*\.amdhsa_(\w+) (\S+)", line)
        if m and desc is not None and m.group(1) in META:
            desc[m.group(1)] = m.group(2)
    return {k: v for k, v in bodies.items() if k in meta}, meta


def counts(body):
    c = collections.Counter()
    for s in body:
        for op in OPS:
            if s.startswith(op):
                c[op] += 1
    return c


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def row(tag, meta, body):
    c = counts(body)
    return "  %s  vgpr %-4s accum %-4s scratch %-4s lds %-6s | %s | %d instructions" % (
        tag, meta.get("next_free_vgpr"), meta.get("accum_offset"), meta.get("private_segment_fixed_size"),
        meta.get("group_segment_fixed_size"), "  ".join("%s %d" % (op, c[op]) for op in OPS), len(body))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines per kernel")
    ap.add_argument("--kernel", default="", metavar="SUBSTRING", help="only kernels whose demangled name contains this")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="rename in the demangled names of `before`")
    args = ap.parse_args()
    (ba, ma), (bb, mb) = parse(args.before), parse(args.after)
    if args.rename:         # match by demangled name, `before` renamed
        def rekey(d, dem, ren):
            out = {}
            for k, v in d.items():
                name = dem[k]
                for r in ren:
                    old, new = r.split("=", 1)
                    name = name.replace(old, new)
                out[name] = v
            return out
        da, db = demangle(sorted(ba)), demangle(sorted(bb))
        ba, ma, bb, mb = rekey(ba, da, args.rename), rekey(ma, da, args.rename), rekey(bb, db, []), rekey(mb, db, [])
        ma, mb = {k: ma[k] for k in ba}, {k: mb[k] for k in bb}
        names = {k: k for k in set(ba) | set(bb)}
    else:
        names = demangle(sorted(set(ba) | set(bb)))
    same = differ = 0
    for k in sorted((k for k in names if args.kernel in names[k]), key=names.get):
        if k not in ba or k not in bb:
            print("ONLY IN %s: %s" % ("before" if k in ba else "after", names[k]))
            differ += 1
        elif ba[k] == bb[k] and ma[k] == mb[k]:
            same += 1
        else:
            differ += 1
            print("DIFF %s" % names[k])
            print(row("before", ma[k], ba[k]))
            print(row("after ", mb[k], bb[k]))
            if args.show:
                d = [l for l in difflib.unified_diff(ba[k], bb[k], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
                print("\n".join("    " + l for l in d[:args.show]))
    print("%d kernels identical, %d differ" % (same, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    raise SystemExit(main())
