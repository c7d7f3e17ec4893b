#!/usr/bin/env python3
"""Compare the device code of two builds function by function.

    hipcc $(CXXFLAGS) -c FILE.hip -o DIR/FILE.o -save-temps=obj     # leaves DIR/FILE-hip-amdgcn-amd-amdhsa-gfx950.s
    scripts/compare_device_asm.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

Every function of the old files is looked up by its symbol in the new files (code may have moved between translation
units).  Two functions are identical when their text is, from the .type line through the kernel descriptor to the
resource .set lines, after comments are stripped and the labels that carry a per-file counter are renumbered
(.LBB<function>_<block>, .Lfunc_end<function>, .Lpost_getpc<n>, .Ltmp<n>).  Prints the functions that differ, those
missing on either side and those defined more than once on a side; exit status 1 if any differs or is defined twice.
It compares text only: it does not judge what the code does.
"""
import difflib
import re
import shutil
import subprocess
import sys

TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
SET = re.compile(r"^\s*\.set\s+(\S+)\.[a-z_]+,")
FUNC_LABEL = re.compile(r"\.L(BB|func_begin|func_end)\d+")
COUNTED = re.compile(r"\.L(?!BB_|func_begin\b|func_end\b)[A-Za-z_]+\d+")


def strip_comment(line):
    # ';' starts a comment except inside a string (.asciz / .ascii / .section flags)
    out, quoted = [], False
    for ch in line:
        if ch == '"':
            quoted = not quoted
        elif ch == ";" and not quoted:
            break
        out.append(ch)
    return " ".join("".join(out).split())


def normalise(lines):
    seen = {}

    def counted(m):
        return seen.setdefault(m.group(0), ".L%s#%d" % (re.sub(r"\d+$", "", m.group(0)[2:]), len(seen)))

    out = []
    for line in lines:
        line = strip_comment(line)
        if not line:
            continue
        line = FUNC_LABEL.sub(lambda m: ".L" + m.group(1), line)
        out.append(COUNTED.sub(counted, line))
    return out


def functions(path):
    """symbol -> list of normalised bodies (one per definition) in `path`"""
    funcs, name, body, tail = {}, None, [], False
    with open(path) as f:
        for line in f:
            m = TYPE.match(line)
            if m:
                if name:
                    funcs.setdefault(name, []).append(normalise(body))
                name, body, tail = m.group(1), [line], False
                continue
            if name is None:
                continue
            if not tail:
                body.append(line)
                tail = line.startswith(".Lfunc_end")
                continue
            s = SET.match(line)
            if s and s.group(1) == name:
                body.append(line)
            elif line.lstrip().startswith(".section"):   # the resource .set lines of the function are over
                funcs.setdefault(name, []).append(normalise(body))
                name = None
    if name:
        funcs.setdefault(name, []).append(normalise(body))
    return funcs


def side(paths):
    merged = {}
    for p in paths:
        for k, v in functions(p).items():
            merged.setdefault(k, []).extend((p, b) for b in v)
    return merged


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return dict(zip(names, names))
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main(argv):
    if "--" not in argv or argv.index("--") in (0, len(argv) - 1):
        sys.exit(__doc__)
    cut = argv.index("--")
    old, new = side(argv[:cut]), side(argv[cut + 1:])
    twice = sorted(k for s in (old, new) for k, v in s.items() if len(v) > 1)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k][0][1] != new[k][0][1])
    same = len(set(old) & set(new)) - len(differ)
    pretty = demangle(sorted(set(twice + gone + added + differ)))
    for k in differ:
        a, b = old[k][0], new[k][0]
        d = [l for l in difflib.unified_diff(a[1], b[1], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print("DIFFERS  %s\n         %s: %d lines, %s: %d lines, %d changed" % (pretty[k], a[0], len(a[1]), b[0], len(b[1]), len(d)))
    for k in gone:
        print("MISSING in the new files  %s" % pretty[k])
    for k in added:
        print("MISSING in the old files  %s" % pretty[k])
    for k in twice:
        print("DEFINED TWICE on one side  %s" % pretty[k])
    print("%d old, %d new: %d identical, %d differing, %d only old, %d only new, %d defined twice"
          % (len(old), len(new), same, len(differ), len(gone), len(added), len(twice)))
    return 1 if differ or twice else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
