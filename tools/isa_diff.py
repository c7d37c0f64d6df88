#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.  No GPU needed.

    python tools/isa_diff.py OLD_TREE NEW_TREE [file.hip ...]

Every csrc/*.hip of both trees (or only the files named) is compiled device-only to assembly with the Makefile's CXXFLAGS.  The
__hip_cuid_<hash> symbol and every kernel's mangled name (replaced by KERNEL<i> in order of definition, so a kernel may lose a template
parameter) are normalised; what is left is compared as text: the body, the kernel descriptor and the metadata entry (registers, LDS,
scratch, argument layout) of each kernel, and the rest of the file.  Prints `identical` or the number of differing lines per kernel;
exit status 1 on any difference.
"""
import difflib
import pathlib
import re
import subprocess
import sys
import tempfile

CSRC = pathlib.Path("parametron.jl_amd") / "csrc"


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


def split_kernels(text):
    """-> (demangled-free names in order of definition, {bucket: lines}); bucket i = kernel i, -1 = everything else"""
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
        elif not meta and re.match(r"\s*\.(protected|globl|weak)\s", line):
            m = re.search(r"KERNEL(\d+)_", line)
            cur = int(m.group(1)) if m else -1
        buckets.setdefault(cur, []).append(line)
    for key in [k for k in buckets if isinstance(k, tuple)]:
        m = re.search(r"\.name:\s+KERNEL(\d+)_", "\n".join(buckets[key]))
        buckets.setdefault(int(m.group(1)) if m else -1, []).extend(buckets.pop(key))
    return names, buckets


def main():
    old, new = pathlib.Path(sys.argv[1]).resolve(), pathlib.Path(sys.argv[2]).resolve()
    files = sys.argv[3:] or sorted({p.name for t in (old, new) for p in (t / CSRC).glob("*.hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for f in files:
            if not ((old / CSRC / f).exists() and (new / CSRC / f).exists()):
                print(f"{f}: only in one tree")
                bad += 1
                continue
            (na, a), (nb, b) = split_kernels(assembly(old, f, ta)), split_kernels(assembly(new, f, tb))
            if len(na) != len(nb):
                print(f"{f}: {len(na)} kernels against {len(nb)}")
                bad += 1
            for k in sorted(set(a) | set(b)):
                la, lb = a.get(k, []), b.get(k, [])
                ndiff = sum(1 for d in difflib.ndiff(la, lb) if d[0] in "+-") if la != lb else 0
                label = "(file scope)" if k < 0 else (na[k] if k < len(na) else nb[k])
                if k >= 0 and k < len(na) and k < len(nb) and na[k] != nb[k]:
                    label += " -> " + nb[k]
                print(f"{f}: {label}: " + (f"{ndiff} differing lines" if ndiff else "identical"))
                bad += 1 if ndiff else 0
    print("ALL IDENTICAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
