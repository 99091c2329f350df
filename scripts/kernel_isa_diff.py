#!/usr/bin/env python3
"""kernel_isa_diff.py REV [--rename OLD=NEW ...] — is the device code of every kernel the same as at commit REV?

Builds the gfx950 device assembly of wgatools_amd/csrc/wga_capi.cpp twice, for the working tree and for REV (taken with
`git archive` into a temporary directory), with build_hip's flags plus --cuda-device-only -S, cuts both files into kernels
(entry label to .Lfunc_end, plus the kernel's .amdhsa_kernel ... .end_amdhsa_kernel block: registers, LDS, scratch), strips
`;` comments and the function number inside local labels, and compares the texts kernel by kernel.

--rename OLD=NEW (repeatable): the kernel called OLD at REV is called NEW in the working tree (each a symbol of the assembly,
or a part of a name that only one kernel on its side has); it is compared after OLD is replaced by NEW throughout its text.  Of
a kernel whose text differs, the line counts and the descriptor's registers, LDS and scratch are printed for both sides.

It compares text only, looks for no particular instruction and runs nothing on a GPU.  For a pull request that only moves
source between files it stands in for a per-kernel timing: the same instructions under the same launch geometry.

Exit status 0: the same kernel names on both sides and no kernel differs.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall"]   # build_hip's (wgatools_amd/build.py)
SRC = os.path.join("wgatools_amd", "csrc", "wga_capi.cpp")


def device_asm(tree, out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc] + FLAGS + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(tree, SRC), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        sys.exit("hipcc failed on " + tree)
    with open(out) as f:
        return f.read()


def normalise(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def kernels(asm):
    """name -> normalised text of the kernel's code and of its descriptor block"""
    lines = asm.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {n: [] for n in names}
    cur = None
    for l in lines:
        m = re.match(r"(\S+):", l)
        if cur is None and m and m.group(1) in out:          # the entry label
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
        if cur is not None:
            n = normalise(l)
            if n.strip():
                out[cur].append(n)
            if re.match(r"\.Lfunc_end\d+:", l) or l.strip() == ".end_amdhsa_kernel":
                cur = None
    return {n: "\n".join(t) for n, t in out.items()}


def unique(part, names, side):
    hit = [part] if part in names else [n for n in names if part in n]
    if len(hit) != 1:
        sys.exit("--rename: %r names %d kernels %s" % (part, len(hit), side))
    return hit[0]


def resources(text):
    """the descriptor's registers, LDS and scratch, and the number of lines"""
    keys = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
            ".amdhsa_private_segment_fixed_size")
    got = dict(l.split()[:2] for l in text.split("\n") if l.split() and l.split()[0] in keys)
    return "  ".join("%s %s" % (k[len(".amdhsa_"):], got.get(k, "?")) for k in keys) + "  lines %d" % (text.count("\n") + 1)


def main():
    argv, renames = [], []
    args = iter(sys.argv[1:])
    for a in args:
        if a == "--rename":
            renames.append(next(args, "").split("=", 1))
        else:
            argv.append(a)
    if len(argv) != 1 or any(len(r) != 2 for r in renames):
        sys.exit(__doc__)
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", argv[0]], check=True, stdout=subprocess.PIPE,
                         text=True).stdout.strip()
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, stdout=subprocess.PIPE,
                          text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "wgatools_amd/csrc", "include"], check=True,
                           stdout=subprocess.PIPE, text=True).stdout.strip() != ""
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "rev")
        os.makedirs(old_tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "wgatools_amd/csrc", "include"], check=True,
                             stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
        old = kernels(device_asm(old_tree, os.path.join(tmp, "rev.s")))
        new = kernels(device_asm(ROOT, os.path.join(tmp, "tree.s")))
    for a, b in renames:
        a, b = unique(a, old, "at the reference"), unique(b, new, "in the working tree")
        old[b] = old.pop(a).replace(a, b)
        print("renamed       %s -> %s" % (a, b))
    print("reference     %s" % rev)
    print("working tree  %s%s" % (head, " + uncommitted changes" if dirty else ""))
    print("kernels       %d in the reference, %d in the working tree" % (len(old), len(new)))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    for title, names in (("only in the reference", only_old), ("only in the working tree", only_new),
                         ("text differs", differ)):
        print("%-24s %d" % (title + ":", len(names)))
        for n in names:
            print("    " + n)
            if names is differ:
                print("        reference     " + resources(old[n]))
                print("        working tree  " + resources(new[n]))
    ok = not (only_old or only_new or differ)
    print("verdict       %s" % ("device code unchanged" if ok else "DEVICE CODE DIFFERS"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
