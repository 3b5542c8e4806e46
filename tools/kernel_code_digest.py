#!/usr/bin/env python3
"""One line per gfx950 kernel of the given .hip files: name, registers, LDS, scratch and a digest of its instructions.

    python tools/kernel_code_digest.py graphaudio_amd/csrc/ga_conv.hip graphaudio_amd/csrc/ga_biquad.hip > after.txt

Every file is compiled for the device alone with the FLAGS of graphaudio_amd/csrc/Makefile (no GPU needed).  The kernel
metadata (llvm-readelf --notes) gives .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size; the
digest is the SHA-256 of the kernel's disassembly (llvm-objdump -d) with the address column removed, so a kernel that moved
inside its object, or into another file, keeps its line.  Lines are sorted by mangled name: `diff` of the outputs of two
trees says whether a refactor left the device code alone.  With --dump DIR the disassembly of every kernel is also written to
DIR/<name>.s, to diff a kernel whose digest changed.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphaudio_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def makefile_flags(arch):
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^FLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels_of(path, arch, tmp):
    obj = os.path.join(tmp, os.path.basename(path) + ".o")
    run(os.path.join(ROCM, "bin", "hipcc"), *makefile_flags(arch), "-I", CSRC, "--offload-device-only", "--no-gpu-bundle-output",
        "-c", path, "-o", obj)
    meta = {}
    for block in re.split(r"^  - (?=\.)", run(os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "--notes", obj), flags=re.M)[1:]:
        field = dict(re.findall(r"^    (\.\w+):\s+(\S+)$", block, re.M))   # the kernel's own keys: an argument's sit deeper
        meta[field[".name"]] = [field[k] for k in KEYS]
    # a symbol's size ends its code: what the assembler pads with up to the next symbol, or to the section's end, is not the kernel's
    size = {m[1]: int(m[0]) for m in re.findall(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$",
                                                run(os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "-s", obj), re.M)}
    text = {}
    name, end = None, 0
    for line in run(os.path.join(ROCM, "llvm", "bin", "llvm-objdump"), "-d", obj).splitlines():
        head = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        addr = re.search(r"// ([0-9A-F]+):", line)
        if head:
            name, end = head.group(2), int(head.group(1), 16) + size.get(head.group(2), 0)
            text[name] = []
        elif name and addr and int(addr.group(1), 16) < end:
            text[name].append(line.strip().replace(addr.group(0), "//"))
    return {k: (v, "\n".join(text[k]) + "\n") for k, v in meta.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--dump", metavar="DIR", help="also write every kernel's disassembly to DIR/<name>.s")
    args = ap.parse_args()
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for path in args.files:
            for name, entry in kernels_of(path, args.arch, tmp).items():
                if name in found:
                    sys.exit("kernel defined twice: " + name)
                found[name] = entry
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    print("# name vgpr sgpr lds scratch sha256(instructions)")
    for name in sorted(found):
        numbers, code = found[name]
        print(name, *numbers, hashlib.sha256(code.encode()).hexdigest())
        if args.dump:
            # (mangled names of templates can exceed a file name's length: the digest of the name stands in for the rest)
            stem = name if len(name) < 200 else name[:160] + "." + hashlib.sha256(name.encode()).hexdigest()[:16]
            with open(os.path.join(args.dump, stem + ".s"), "w") as f:
                f.write(code)


if __name__ == "__main__":
    main()
