"""Compare the kernels of two builds by their device assembly:  python scripts/isa_diff.py OLD NEW [-v] [--map OLDSYM=NEWSYM ...]

OLD and NEW are .s files from `hipcc -S --cuda-device-only` (with the Makefile's flags), or directories of them; a kernel may move
between files.  Kernel symbols are paired by name.  A body is the text from the symbol's label to its .Lfunc_end, without assembler
comments and with the function's own basic-block label numbers (.LBB<function>_<block>) reduced to the block number, so that a kernel
that merely moved to another place or file compares equal.  Section directives (.text, .section ...) are left out as well: a kernel
that became a template moves to a COMDAT section of its own.  Such a kernel also has another symbol: --map OLDSYM=NEWSYM (the mangled
names, as printed for a symbol that is on one side only) reads OLDSYM in OLD as NEWSYM.  Per symbol: identical, differs (both
instruction counts), or only on one side; -v also prints a unified diff of the bodies that differ.  Exit status 1 unless every
symbol is on both sides and identical."""
import difflib
import os
import re
import subprocess
import sys


def kernels(path, rename=()):
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".s")) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        text = open(f).read()
        for a, b in rename:
            text = re.sub(r"(?<![\w$.])%s(?![\w$])" % re.escape(a), lambda m: b, text)
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
            m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
            if m is None:
                sys.exit("%s: no body found for kernel %s" % (f, name))
            body = m.group(1)
            lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).strip() for l in body.split("\n")]
            out[name] = [l for l in lines if l and not re.match(r"\.(text|section)\b", l)]
    return out


def n_instr(body):
    return sum(1 for l in body if not l.endswith(":") and not l.startswith("."))


def demangled(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    verbose = "-v" in argv
    rename = [tuple(argv[i + 1].split("=", 1)) for i, a in enumerate(argv) if a == "--map"]
    paths = [a for i, a in enumerate(argv) if a not in ("-v", "--map") and (i == 0 or argv[i - 1] != "--map")]
    if len(paths) != 2 or any(len(r) != 2 for r in rename):
        sys.exit(__doc__)
    old, new = kernels(paths[0], rename), kernels(paths[1])
    names = sorted(set(old) | set(new))
    pretty = demangled(names)
    count = {"identical": 0, "differs": 0, "only old": 0, "only new": 0}
    for n in names:
        if n not in new or n not in old:
            verdict = "only old" if n in old else "only new"
            note = "  [%s]" % n
        elif old[n] == new[n]:
            verdict, note = "identical", "  (%d instructions)" % n_instr(old[n])
        else:
            verdict, note = "differs", "  (%d -> %d instructions)" % (n_instr(old[n]), n_instr(new[n]))
        count[verdict] += 1
        print("%-9s %s%s" % (verdict, pretty[n], note))
        if verbose and verdict == "differs":
            print("\n".join(difflib.unified_diff(old[n], new[n], "old", "new", lineterm="", n=2)))
    print("%d symbols old, %d new: " % (len(old), len(new)) + ", ".join("%d %s" % (v, k) for k, v in count.items()))
    return 0 if count["identical"] == len(names) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
