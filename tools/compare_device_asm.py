#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files of the same source file, before and after a change that is meant to
leave the generated code alone (the recipe of profiles/r10, r12, r13 and r14 *_isa_identity.txt). Make the two files with the
Makefile's flags plus `--cuda-device-only -S`, once per flag set (with and without -DSPMV_AMD_LAB), at the parent and at the head:
   hipcc <CXXFLAGS> --cuda-device-only -S csrc/spmv_kernels.hip -o spmv_kernels.s
   python tools/compare_device_asm.py parent/spmv_kernels.s head/spmv_kernels.s [--diff]
A kernel's section is everything from its `.section .text.<kernel>` line to the next kernel's: instructions, labels, .set lines
and the .amdhsa_kernel block (register counts, LDS and scratch sizes). Comment lines, .file, .ident and the per-TU hash symbol are
dropped and the function ordinal in local labels is masked. One line per section:
   identical        the filtered text is the same
   registers-only   the same sequence of mnemonics and labels and the same .amdhsa_* block; only register numbers differ
   different        anything else: the two lengths, and whether the .amdhsa_* block is the same (--diff adds the unified diff)
Exit status 1 if a section is different or exists in one file only."""
import difflib
import re
import sys

DROP = re.compile(r"^\s*(;|\.(file|ident)\b)|__hip_cuid_")
REGISTER = re.compile(r"\b[vsa](\d+|\[\d+:\d+\])")


def sections(path):
    """{kernel: filtered lines}, in file order."""
    out, name = {}, None
    for line in open(path):
        if DROP.search(line):
            continue
        line = re.sub(r"[ \t]*;.*$", "", line.rstrip("\n"))
        line = re.sub(r"\.LBB[0-9]+_", ".LBB#_", line)
        line = re.sub(r"\.Lfunc_(begin|end)[0-9]+", r".Lfunc_\1#", line)
        words = line.split()
        if words and words[0] in (".section", ".text", ".amdgpu_metadata"):
            target = words[1].split(",")[0] if len(words) > 1 else ""
            if target.startswith(".text."):
                name = target[len(".text."):]
            elif target not in (".rodata", ".AMDGPU.csdata"):  # the descriptor and the resource notes belong to the kernel before them
                name = None
        if name is not None and line.strip():
            out.setdefault(name, []).append(line)
    return out


def descriptor(lines):
    return [l.split() for l in lines if l.lstrip().startswith(".amdhsa_")]


def classify(a, b):
    """'identical', 'registers-only' or 'different' for two filtered sections."""
    if a == b:
        return "identical"
    if descriptor(a) == descriptor(b) and [REGISTER.sub("R", l) for l in a] == [REGISTER.sub("R", l) for l in b]:
        return "registers-only"
    return "different"


def main(argv):
    show_diff = "--diff" in argv
    paths = [p for p in argv if p != "--diff"]
    if len(paths) != 2:
        sys.exit(__doc__)
    a, b = sections(paths[0]), sections(paths[1])
    bad = False
    for name in list(a) + [n for n in b if n not in a]:
        if name not in a or name not in b:
            print(f"{'only-in-first' if name in a else 'only-in-second':15s} {len(a.get(name) or b[name]):6d}         {name}")
            bad = True
            continue
        kind = classify(a[name], b[name])
        note = ""
        if kind == "different":
            bad = True
            note = "  .amdhsa block " + ("same" if descriptor(a[name]) == descriptor(b[name]) else "DIFFERS")
        print(f"{kind:15s} {len(a[name]):6d} {len(b[name]):6d}  {name}{note}")
        if kind == "different" and show_diff:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[name], b[name], "first", "second", lineterm="", n=2))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
