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

--commutative adds a class between identical and different: kernels that differ ONLY in the order of the two source
operands of the integer opcodes in COMMUTATIVE (a helper that takes a pointer where the text indexed an array makes the
compiler state `v_and_b32 v1, v79, v78` as `v1, v78, v79`; in the SDWA encoding a source moves together with its
src<n>_sel).  Everything else still has to match line for line: the
number of lines, every opcode, every destination register, every other instruction and the .amdhsa_ descriptor.  Such
kernels are printed as "commutative" and do not count towards the exit status.  No floating-point opcode is in the set.
"""
import argparse, concurrent.futures, os, re, shlex, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "gaussianeditor_amd/csrc"


# two-source integer opcodes whose result does not depend on the order of the sources
COMMUTATIVE = ("v_and_b32", "v_or_b32", "v_xor_b32", "v_add_u32", "s_and_b32", "s_and_b64", "s_or_b32", "s_or_b64", "s_xor_b32",
               "s_xor_b64", "s_add_u32")
_COMMUTATIVE_RE = re.compile(r"^((?:%s)(?:_e32|_e64)?)\s+([^,\s]+),\s*([^,\s]+),\s*([^,\s]+)$" % "|".join(COMMUTATIVE))
# the same opcodes in their SDWA encoding: every source carries its sub-dword selector with it
_COMMUTATIVE_SDWA_RE = re.compile(r"^((?:%s)_sdwa)\s+([^,\s]+),\s*([^,\s]+),\s*([^,\s]+)((?:\s+dst_\w+:\w+)*)"
                                  r"\s+src0_sel:(\w+)\s+src1_sel:(\w+)$" % "|".join(COMMUTATIVE))


def sort_commutative(body):
    """The lines of one function with the two sources of every plain COMMUTATIVE instruction in sorted order."""
    out = []
    for text in body:
        m = _COMMUTATIVE_RE.match(text)  # (an instruction with a source modifier, a third operand or another suffix stays as it is)
        if m:
            text = "%s %s, %s, %s" % ((m.group(1), m.group(2)) + tuple(sorted(m.group(3, 4))))
        m = _COMMUTATIVE_SDWA_RE.match(text)
        if m:
            (a, sa), (b, sb) = sorted([(m.group(3), m.group(6)), (m.group(4), m.group(7))])
            text = "%s %s, %s, %s%s src0_sel:%s src1_sel:%s" % (m.group(1), m.group(2), a, b, m.group(5), sa, sb)
        out.append(text)
    return out


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
    ap.add_argument("--commutative", action="store_true", help="report kernels that differ only in the source order of COMMUTATIVE opcodes apart")
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
                swapped = [k for k in different if args.commutative and sort_commutative(a[k]) == sort_commutative(b[k])]
                different = [k for k in different if k not in swapped]
                gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
                same = len(set(a) & set(b)) - len(different) - len(swapped)
                print(f"{u}.hip: {same} identical, " + (f"{len(swapped)} commutative, " if args.commutative else "")
                      + f"{len(different)} different, {len(gone)} only-in-old, {len(new)} only-in-new")
                for tag, names in (("commutative", swapped), ("different", different), ("only-in-old", gone), ("only-in-new", new)):
                    for k in names:
                        print(f"  {tag}: {k}")
                bad += len(different) + len(new)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
