#!/usr/bin/env python3
"""Compare the instruction streams of kernels in two gfx950 assembly files (hipcc -S --cuda-device-only).

    scripts/asm_kernel_diff.py before.s after.s k_loop_filter3_b [k_other ...]
    scripts/asm_kernel_diff.py before.s after.s k_search2ILb1ELi1E=k_search2E   # a kernel whose symbol changed: before=after
    scripts/asm_kernel_diff.py --all before.s after.s            # every kernel of both files, by its full symbol
    scripts/asm_kernel_diff.py --loop one.s k_loop_filter3_b      # static size of the kernel's largest loop

A kernel is named by a fragment of its symbol that must match exactly one kernel of each file (--all needs no names: it pairs
the kernels by their mangled symbols, template instantiations included, and fails if the two files' sets differ).  Its stream is what lies
between its entry label and its s_endpgm-terminated end, without comments, directives and blank lines; labels and mangled
symbols are renamed in order of first appearance, so streams that differ only in names compare equal.  A kernel named by fragments
is held to its kernel descriptor as well (the .amdhsa_ directives: registers, LDS, scratch and the rest).  Prints one line per
kernel (instruction counts, identical or not) and a unified diff of the streams that differ; exit status 1 if any does."""
import difflib
import re
import sys


def streams(path):
    """{kernel symbol: [normalised instruction or label line]}"""
    text = open(path).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for k in kernels:
        m = re.search(r"^" + re.escape(k) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        names = {}

        def rename(mm, names=names):
            return names.setdefault(mm.group(0), "L%d" % len(names) if mm.group(0).startswith(".L") else "SYM%d" % len(names))

        lines = []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue
            lines.append(re.sub(r"\.LBB\d+_\d+|_Z\w+", rename, " ".join(ln.split())))
        out[k] = lines
    return out


def descriptors(path):
    """{kernel symbol: [its .amdhsa_ directives]}"""
    return {m.group(1): m.group(2).split("\n") for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", open(path).read(), re.M | re.S)}


def figures(desc):
    """VGPRs, SGPRs, LDS and scratch bytes of a descriptor, for the report"""
    d = dict(ln.split()[:2] for ln in desc if ln.strip())
    return "vgpr %s sgpr %s lds %s scratch %s" % tuple(d[".amdhsa_" + k] for k in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"))


def pick(ks, frag):
    hit = [k for k in ks if re.search(re.escape(frag) + r"(?![a-z0-9_])", k)]   # (a mangled name goes on with an upper-case letter)
    if len(hit) != 1:
        sys.exit("%r matches %s" % (frag, hit or "nothing"))
    return hit[0]


def instructions(lines):
    return [ln for ln in lines if not ln.endswith(":")]


def largest_loop(lines):
    """(first, last) line index of the largest span from a label to the last backward branch to it"""
    at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    best = (0, 0)
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(L\d+)$", ln)
        if m and at.get(m.group(1), i) < i and i - at[m.group(1)] > best[1] - best[0]:
            best = (at[m.group(1)], i)
    return best


def report(name, b, a):
    """one line for a pair of streams, and their diff if they differ; 1 if they do"""
    same = b == a
    print("%-28s %5d -> %5d instructions  %s" % (name, len(instructions(b)), len(instructions(a)), "identical" if same else "DIFFERENT"))
    if not same:
        sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(b, a, "before " + name, "after " + name, lineterm="", n=2))
    return 0 if same else 1


def main(argv):
    if argv and argv[0] == "--all":
        before, after = streams(argv[1]), streams(argv[2])
        differ = 0
        for k in sorted(set(before) | set(after)):
            if k in before and k in after:
                differ |= report(k, before[k], after[k])
            else:
                differ = 1
                print("%-28s only in %s" % (k, argv[1] if k in before else argv[2]))
        print("%d kernels in %s, %d in %s: %s" % (len(before), argv[1], len(after), argv[2], "DIFFERENT" if differ else "all identical"))
        return differ
    if argv and argv[0] == "--loop":
        s = streams(argv[1])
        for frag in argv[2:]:
            k = pick(s, frag)
            a, b = largest_loop(s[k])
            print("%s: largest loop %d instructions (of %d)" % (k, len(instructions(s[k][a:b + 1])), len(instructions(s[k]))))
        return 0
    before, after = streams(argv[0]), streams(argv[1])
    dbefore, dafter = descriptors(argv[0]), descriptors(argv[1])
    differ = 0
    for frag in argv[2:]:
        fb, fa = frag.split("=") if "=" in frag else (frag, frag)
        kb, ka = pick(before, fb), pick(after, fa)
        differ |= report(frag, before[kb], after[ka])
        same = dbefore[kb] == dafter[ka]
        print("    %s -> %s  descriptor %s" % (figures(dbefore[kb]), figures(dafter[ka]), "identical" if same else "DIFFERENT"))
        differ |= not same
    return differ


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
