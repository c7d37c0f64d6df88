#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.  No GPU needed.

    python tools/isa_diff.py OLD_TREE NEW_TREE [--map OLD=NEW ...] [file.hip ...]

Every csrc/*.hip of both trees (or only the files named) is compiled device-only to assembly with the Makefile's CXXFLAGS.  Kernels are
paired BY NAME — the demangled name without return type and parameter list, `pmt::` dropped: `batch_horizon_dyn_kernel<16>` — so a kernel
may move within its file; one that was renamed, or became an instantiation of a template, is paired through `--map OLD=NEW`
(`--map 'batch_horizon_dyn_expand_kernel=dynamics_expand_kernel<false>'`).  The __hip_cuid_<hash> symbol, every kernel's mangled name
(KERNEL_ in its own text), the function index in local labels (.LBB<k>_<n>, .Lfunc_end<k>) and the linkage and text-section directives
around a kernel (they change when a kernel becomes a template or gets another neighbour) are normalised; what is left is compared as text:
the body, the kernel descriptor, the resource summary and the metadata entry (registers, LDS, scratch, argument layout) of each kernel,
and the rest of the file.  Prints `identical` or the number of differing lines per kernel, and for a differing kernel its resource counts
in both trees; exit status 1 on any difference.
"""
import difflib
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = pathlib.Path("parametron.jl_amd") / "csrc"
# the metadata fields a differing kernel is reported with
COUNTS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def cxxflags(tree):
    mk = (tree / CSRC / "Makefile").read_text()
    def var(name):
        m = re.search(rf"^{name} \?= (.*)$", mk, re.M)
        if not m:
            sys.exit(f"{tree / CSRC / 'Makefile'}: no line '{name} ?= ...'")
        return m.group(1)
    return var("HIPCC"), var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


def assembly(tree, name, tmp):
    hipcc, flags = cxxflags(tree)
    out = pathlib.Path(tmp) / (name + ".s")
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", name, "-o", str(out)], cwd=tree / CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(f"{tree / CSRC / name} does not compile:\n{r.stderr}")
    return out.read_text()


def short_names(tree, mangled):
    """mangled kernel names -> `name<template arguments>`: demangled, without return type, parameter list and the pmt:: namespace"""
    if not mangled:
        return []
    filt = pathlib.Path(cxxflags(tree)[0]).resolve().parent.parent / "llvm" / "bin" / "llvm-cxxfilt"
    filt = str(filt) if filt.exists() else (shutil.which("llvm-cxxfilt") or shutil.which("c++filt"))
    if not filt:
        return list(mangled)
    out = subprocess.run([filt, *mangled], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    names = []
    for d in out:
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):                              # the parameter list opens at the first '(' outside template arguments
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0 and not d.startswith("(anonymous namespace)", i):
                cut = i
                break
        head = d[:cut]
        depth = 0
        for i in range(len(head) - 1, -1, -1):                  # a template's return type stands in front of the name
            depth += (head[i] == ">") - (head[i] == "<")
            if head[i] == " " and depth == 0:
                head = head[i + 1:]
                break
        names.append(head.replace("pmt::", ""))
    return names


def split_kernels(tree, text):
    """-> {short kernel name: lines, "(file scope)": everything else}"""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_HASH", text)
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    names = [n for n in re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M) if n in kernels]
    # the name without its _Z prefix also occurs inside the names of a kernel's static __shared__ arrays (_ZZ<name>E3lds)
    for i in sorted(range(len(names)), key=lambda i: -len(names[i])):
        text = text.replace(names[i], f"KERNEL{i}_").replace(names[i][2:], f"KERNEL{i}_")
    buckets, cur, meta = {-1: []}, -1, False
    for line in text.splitlines():
        if ".amdgpu_metadata" in line:
            meta, cur = not meta, -1
        elif meta and re.match(r"  - \.|amdhsa\.", line):       # a metadata entry: its kernel is named further down, file it then
            cur = ("meta", len(buckets))
        elif not meta and re.match(r"\s*(\.text$|\.section\s|\.p2alignl\s|\.fill\s)", line):
            if ".AMDGPU.gpr_maximums" in line:
                cur = -1                                        # behind the file's last function
            continue                                            # which section comes next, and the padding of .text: not device code
        elif not meta and re.match(r"\s*\.(protected|globl|weak|hidden)\s", line):
            m = re.search(r"KERNEL(\d+)_", line)
            cur = int(m.group(1)) if m else -1
            if m:
                continue                                        # a kernel's linkage: a template's differs
        buckets.setdefault(cur, []).append(line)
    for key in [k for k in buckets if isinstance(k, tuple)]:
        m = re.search(r"\.name:\s+KERNEL(\d+)_", "\n".join(buckets[key]))
        buckets.setdefault(int(m.group(1)) if m else -1, []).extend(buckets.pop(key))
    out = {"(file scope)": buckets.pop(-1)}
    for i, short in enumerate(short_names(tree, names)):
        lines = "\n".join(buckets.get(i, []))
        lines = re.sub(rf"KERNEL{i}_", "KERNEL_", lines)
        lines = re.sub(r"(\.L[A-Za-z_]*?)\d+_(\d+)", r"\1_\2", lines)       # .LBB<function>_<block>
        lines = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", lines)                    # ... and in the loop comments
        lines = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", lines)
        out[short] = lines.splitlines()
    return out


def counts(lines):
    found = {}
    for line in lines:
        m = re.match(r"\s*(\.\w+):\s+(\d+)\s*$", line)
        if m and m.group(1) in COUNTS:
            found[m.group(1)] = m.group(2)
    return " ".join(f"{k[1:]}={found.get(k, '?')}" for k in COUNTS)


def main():
    args, renamed = sys.argv[1:], {}
    while "--map" in args:
        i = args.index("--map")
        if i + 1 >= len(args) or "=" not in args[i + 1]:
            sys.exit("--map takes OLD=NEW")
        o, n = args[i + 1].split("=", 1)
        renamed[o] = n
        del args[i:i + 2]
    if len(args) < 2:
        sys.exit(__doc__)
    old, new = pathlib.Path(args[0]).resolve(), pathlib.Path(args[1]).resolve()
    files = args[2:] or sorted({p.name for t in (old, new) for p in (t / CSRC).glob("*.hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for f in files:
            if not ((old / CSRC / f).exists() and (new / CSRC / f).exists()):
                print(f"{f}: only in one tree")
                bad += 1
                continue
            a, b = split_kernels(old, assembly(old, f, ta)), split_kernels(new, assembly(new, f, tb))
            pairs = [(k, renamed[k] if k in renamed and k not in b else k) for k in a]
            pairs += [(None, k) for k in b if k not in {kb for _, kb in pairs}]
            for ka, kb in pairs:
                if ka is None or kb not in b:
                    print(f"{f}: {kb}: only in the {'new' if ka is None else 'old'} tree")
                    bad += 1
                    continue
                la, lb = a[ka], b[kb]
                ndiff = sum(1 for d in difflib.ndiff(la, lb) if d[0] in "+-") if la != lb else 0
                label = ka if ka == kb else f"{ka} -> {kb}"
                print(f"{f}: {label}: " + (f"{ndiff} differing lines" if ndiff else "identical"))
                if ndiff and ka != "(file scope)":
                    print(f"{f}:     old {counts(la)}\n{f}:     new {counts(lb)}")
                bad += 1 if ndiff else 0
    print("ALL IDENTICAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
