#!/usr/bin/env python3
"""Did a source change move the machine code?  Compares two device-only assembly listings kernel by kernel.

  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result -Iinclude -Ikaldi-aslp_amd/csrc \\
        -Ikaldi-aslp_amd/nnet -Ikaldi-aslp_amd/util -Ikaldi-aslp_amd/parallel --cuda-device-only -S kaldi-aslp_amd/csrc/FILE.hip -o NEW.s
  (the Makefile's CXXFLAGS + --cuda-device-only -S; OLD.s the same from a checkout of the commit before)
  devtools/kernel_text_cmp.py OLD.s NEW.s [--rename 'regex=>repl' ...]

Kernels are paired by demangled name (c++filt; mangled where there is none) after the renames, which are applied in order to the names of
both files.  Per kernel: `name  text same|DIFF  descriptor same|DIFF`, text = the instructions from the kernel's label to its descriptor,
descriptor = the whole .amdhsa_kernel block (registers, scratch, LDS, ...).  Only symbol names, .L labels and the block names in loop comments are normalised.  The last line
counts; exit status 1 on any DIFF or unpaired kernel.  Reads text, needs no GPU."""
import argparse
import re
import shutil
import subprocess
import sys


def kernels(path):
    """mangled name -> (text lines, descriptor lines), in file order"""
    lines = open(path).read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        label = max(j for j in range(i) if lines[j].startswith(name + ":"))
        stop = next(j for j in range(label, i) if lines[j].startswith("\t.section"))
        # (.LBB12_3 -> .LBB_3; the same block named in a comment, "in Loop: Header=BB12_3", carries the function's number too: a kernel
        # added in front of this one moves it, and with one more digit in it the blanks that align the comment behind a label)
        norm = lambda s: re.sub(r"[ \t]+;", " ;", re.sub(r"\bBB\d+(_\d+)\b", r"BB\1", re.sub(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b", r".L\1\2", s.replace(name, "SELF"))))
        out[name] = ([norm(s) for s in lines[label:stop]], [norm(s) for s in lines[i:end + 1]])
    return out


def display_names(names, renames):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    shown = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n") if filt and names else list(names)
    shown = [re.sub(r"\(.*$", "", s.replace("void ", "", 1).replace("(anonymous namespace)::", "")) for s in shown[:len(names)]]   # the argument list says nothing here
    for pat, repl in renames:
        shown = [re.sub(pat, repl, s) for s in shown]
    return dict(zip(shown, names))


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=>REPL")
    args = ap.parse_args(argv)
    paths, renames = [args.old, args.new], [tuple(r.split("=>", 1)) for r in args.rename]
    if any(len(r) != 2 for r in renames):
        ap.error("--rename takes 'regex=>repl'")
    old, new = kernels(paths[0]), kernels(paths[1])
    old_by, new_by = display_names(list(old), renames), display_names(list(new), renames)
    bad = 0
    for shown in sorted(set(old_by) | set(new_by)):
        if shown not in old_by or shown not in new_by:
            print("%s  only in %s" % (shown, paths[0] if shown in old_by else paths[1]))
            bad += 1
            continue
        (ta, da), (tb, db) = old[old_by[shown]], new[new_by[shown]]
        print("%s  text %s  descriptor %s" % (shown, "same" if ta == tb else "DIFF", "same" if da == db else "DIFF"))
        bad += ta != tb or da != db
    bad += len(old_by) != len(old) or len(new_by) != len(new)   # two kernels renamed onto one name
    print("%d kernels in %s, %d in %s, %d differ or are unpaired" % (len(old), paths[0], len(new), paths[1], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
