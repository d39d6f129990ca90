"""Compare two device-assembly dumps of one translation unit kernel by kernel -- the check of a change that must not touch the
machine code (a refactor of the host side, a move of kernel sources between files).

    hipcc $(python -c "from epipolar_transformers_amd import build; print(' '.join(build.flags()))") \\
          --offload-device-only -S -o before.s epipolar_transformers_amd/csrc/et_forward_tile.hip     # at the old commit
    ... the same at the new commit -> after.s ...
    python scripts/dev/compare_kernel_asm.py before.s after.s [--show NAME_SUBSTRING]

A kernel's text is everything from its symbol label to its .end_amdhsa_kernel (instructions, then the .amdhsa_* resource
block), keyed by the mangled name.  Normalised: the function's ordinal in local labels (.LBB12_3 -> .LBB_3, .Lfunc_end12) -- the
kernel's position in the module, which changes when kernels are instantiated in another order -- and the assembler comments
(from ';' on: they repeat those ordinals and are padded to the label's width); the labels of long branches (.Lpost_getpc7),
which are numbered through the module, are renumbered from 0 in every kernel.
(Two compiles of the same source differ in the __hip_cuid_* symbol only, which belongs to no kernel.)
Exit status 0 when both dumps hold the same kernels with identical text.
"""
import difflib
import re
import sys

_LABEL = re.compile(r"\.L(BB|func_begin|func_end)\d+")


def kernels(path):
    """mangled name -> (instruction lines, .amdhsa_* lines)"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l and l[0] not in " \t.;" and l.split(":")[0] in set(names)}
    out = {}
    for name in names:
        i = start[name]
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        body = [l for l in (_LABEL.sub(r".L\1", l.split(";")[0]).rstrip() for l in lines[i:j]) if l]
        ids = {}
        body = [re.sub(r"\.Lpost_getpc\d+", lambda m: ".Lpost_getpc_%d" % ids.setdefault(m.group(0), len(ids)), l) for l in body]
        a = next(k for k, l in enumerate(body) if l.strip().startswith(".amdhsa_kernel"))
        out[name] = (body[:a], body[a:])
    return out


def main(argv):
    show = argv[argv.index("--show") + 1] if "--show" in argv else None
    before, after = kernels(argv[1]), kernels(argv[2])
    only = sorted(set(before) ^ set(after))
    for name in only:
        print("only in %s: %s" % ("before" if name in before else "after", name))
    same_text = same_res = 0
    common = sorted(set(before) & set(after))
    for name in common:
        t, r = before[name][0] == after[name][0], before[name][1] == after[name][1]
        same_text += t
        same_res += r
        if not (t and r):
            print("DIFFERS (%s): %s" % (", ".join(w for w, ok in (("instructions", t), ("resources", r)) if not ok), name))
        if show and show in name and not (t and r):
            for which in (0, 1):
                sys.stdout.write("\n".join(difflib.unified_diff(before[name][which], after[name][which], "before", "after", lineterm="", n=2)) + "\n")
    print("%d kernels before, %d after, %d in both: %d with identical instructions, %d with identical .amdhsa_* resources"
          % (len(before), len(after), len(common), same_text, same_res))
    return 0 if not only and same_text == same_res == len(common) == len(before) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
