"""Is the device code of the working tree that of another revision, kernel by kernel?

Exports <git-rev> with `git archive` into a temporary directory, compiles its translation units and the
working tree's to gfx950 assembly (the units and flags of __graft_entry__.UNITS, tools/isa_check.py's
compile_asm) and compares every kernel's instructions and register counts.  The compiler's per-compile
random symbol `__hip_cuid_<hex>` and the function numbers in local labels are masked.  CPU only; the proof a refactor of the kernels owes.
--mask-kernarg also masks where a kernel's arguments lie, for a change that only adds or removes fields of an argument
struct: the immediate offsets of the scalar loads from the kernel-argument pointer (s[0:1] at entry, or a copy of it) and
of the additions to it that form the address of the implicit arguments, and .amdhsa_kernarg_size.

Usage: python tools/asm_same.py <git-rev> [--mask-kernarg] [--defines -DRH_PROF ...]   (exit status 1 if a kernel differs)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check as I  # noqa: E402

CSRC = os.path.relpath(I.G.CSRC, I.ROOT)


def device_code(csrc, defines, mask_kernarg=False):
    """{kernel: (instruction lines, (VGPRs, spilled VGPRs))} of the tree whose sources are in `csrc`."""
    path = I.compile_asm(defines, csrc)
    with open(path) as fh:
        text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", fh.read())
    # local labels (and the comments that name them) carry the function's number within its unit (BB<f>_<n>), which follows the order in
    # which the host code first names the kernels' instantiations: not an instruction, masked too
    lines = re.sub(r"\bBB\d+_", "BB_", text.replace(".LBB", "BB")).split("\n")
    os.unlink(path)
    res = I.resources(lines)
    return {k: (masked_kernarg(body) if mask_kernarg else body, res.get(k)) for k, body in I.kernels(lines).items()}


def masked_kernarg(body):
    """The kernel's lines with the offsets into its argument segment masked (--mask-kernarg)."""
    text = re.sub(r"(\.amdhsa_kernarg_size\s+)\d+", r"\1<kernarg>", "\n".join(body))
    lo = ["0"] + re.findall(r"\bs_mov_b64\s+s\[(\d+):\d+\],\s+s\[0:1\]", text)   # low SGPR of the pointer and of its copies
    for r in lo:
        text = re.sub(r"(\bs_load_dword\w*\s+\S+\s+s\[%s:\d+\],\s+)0x[0-9a-f]+" % r, r"\1<kernarg>", text)
        text = re.sub(r"(\bs_add_u32\s+s\d+,\s+s%s,\s+)0x[0-9a-f]+" % r, r"\1<kernarg>", text)
    return text.split("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("--mask-kernarg", action="store_true", help="mask the kernel-argument offsets and size")
    ap.add_argument("--defines", nargs=argparse.REMAINDER, default=[], help="extra compiler flags, e.g. -DRH_PROF")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", I.ROOT, "archive", args.rev], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
        old = device_code(os.path.join(tmp, CSRC), args.defines, args.mask_kernarg)
    new = device_code(I.G.CSRC, args.defines, args.mask_kernarg)
    differ = sorted(k for k in old.keys() | new.keys() if old.get(k) != new.get(k))
    for k in differ:
        print("differs:" if k in old and k in new else "only in %s:" % (args.rev if k in old else "the working tree"), I.demangle(k))
    print(f"{len(new)} kernels, {len(differ)} differing from {args.rev}" + (" with " + " ".join(args.defines) if args.defines else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
