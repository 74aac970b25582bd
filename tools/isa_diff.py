#!/usr/bin/env python3
"""Development tool: do two source trees compile to the same device code, kernel by kernel?

    python tools/isa_diff.py                       # HEAD~1 against the working tree
    python tools/isa_diff.py --old-rev v1 --rename blend_backward_kernelILi0E=blend_backward_kernelI

Every .hip translation unit of gaussianeditor_amd/csrc is compiled to gfx950 assembly (--cuda-device-only -S) with the
command `make -n` prints for that unit in its own tree, so the flags are the Makefile's.  The assembly is split per
function symbol (a kernel's .amdhsa_ descriptor with it); comments, other directives and blank lines are dropped,
basic-block label numbers (.LBB<n>_) are normalised, and the --rename pairs are applied to the old tree's symbols and text
(a template parameter that went away changes the mangled name and nothing else).  Prints identical / different /
only-in-old / only-in-new per unit; the exit status is non-zero on any "different" or "only-in-new".  Needs hipcc and no
GPU; about 25 s per unit.
"""
import argparse, concurrent.futures, os, re, shlex, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "gaussianeditor_amd/csrc"


def unit_commands(tree):
    """{unit: argv} from the Makefile's own compile lines, '-c X.hip -o X.o' taken off."""
    base = os.path.join(tree, CSRC)  # (units in subdirectories too, named by their path: loss/gsr_loss)
    objs = sorted(os.path.relpath(os.path.join(d, f), base)[:-4] + ".o" for d, _, fs in os.walk(base) for f in fs if f.endswith(".hip"))
    out = subprocess.run(["make", "-n", "-B", "-C", base] + objs, check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r"^(.*\S)\s+-c ([\w/]+)\.hip -o \2\.o\s*$", line)
        if m:
            cmds[m.group(2)] = shlex.split(m.group(1))
    return cmds


def functions(asm, renames):
    """{symbol: [instruction lines, then the .amdhsa_ descriptor lines of a kernel]} of one assembly file."""
    out, name, body = {}, None, []
    for line in asm.splitlines():
        for old, new in renames:
            line = line.replace(old, new)
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name is not None:
            text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            # dropped: directives (.p2align ...) other than the kernel descriptor's (.amdhsa_: registers, LDS, scratch); kept: labels (.LBB_3:)
            if text and (text.startswith(".amdhsa_") or not re.match(r"\.[a-z_0-9]+(\s|$)", text)):
                body.append(text)
    return out


def compile_unit(tree, unit, argv, renames, workdir):
    asm = os.path.join(workdir, unit.replace("/", "_") + ".s")
    subprocess.run(argv + ["-w", "--cuda-device-only", "-S", unit + ".hip", "-o", asm], check=True, cwd=os.path.join(tree, CSRC))
    with open(asm) as f:
        return functions(f.read(), renames)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--old", help="old source tree (default: --old-rev unpacked under a temporary directory)")
    ap.add_argument("--old-rev", default="HEAD~1", help="git revision of the old tree (default HEAD~1)")
    ap.add_argument("--new", default=ROOT, help="new source tree (default: the working tree)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="mangled-name fragment that changed")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = args.old
        if old is None:
            old = os.path.join(tmp, "old")
            os.mkdir(old)
            tar = subprocess.run(["git", "-C", ROOT, "archive", args.old_rev, CSRC, "include"], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        sides = []
        for label, tree, ren in (("old", old, renames), ("new", args.new, [])):
            os.mkdir(os.path.join(tmp, "asm_" + label))
            sides.append((tree, unit_commands(tree), ren, os.path.join(tmp, "asm_" + label)))
        units = sorted(set(sides[0][1]) | set(sides[1][1]))
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            jobs = {(i, u): pool.submit(compile_unit, tree, u, cmds[u], ren, work)
                    for i, (tree, cmds, ren, work) in enumerate(sides) for u in units if u in cmds}
            for u in units:
                a = jobs[0, u].result() if (0, u) in jobs else {}
                b = jobs[1, u].result() if (1, u) in jobs else {}
                different = sorted(k for k in a if k in b and a[k] != b[k])
                gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
                same = len(set(a) & set(b)) - len(different)
                print(f"{u}.hip: {same} identical, {len(different)} different, {len(gone)} only-in-old, {len(new)} only-in-new")
                for tag, names in (("different", different), ("only-in-old", gone), ("only-in-new", new)):
                    for k in names:
                        print(f"  {tag}: {k}")
                bad += len(different) + len(new)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
