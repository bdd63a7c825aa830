"""Compare the device assembly of every kernel between two builds of the same sources (instruction-for-instruction).

Usage:
    # device assembly of each translation unit, once per source tree
    hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -fPIC [-fno-slp-vectorize] X.hip -o OUT/X.s
    python tools/asm_diff.py OLD_DIR NEW_DIR

Every kernel of OLD_DIR/*.s is looked up in NEW_DIR/*.s of the same name.  Names are compared demangled, by kernel name and
template arguments only (the parameter types are ignored: a parameter block that is renamed or moved between namespaces
changes the mangled name and nothing else; no kernel of the library is overloaded on its parameters), with a
trailing template argument `TAPS = 9` of the new build dropped (the 3x3 instantiations of kernels that gained a tap-count
parameter, and kernels that became templates on it).  Bodies are compared after dropping comments, debug directives and
the numbering of local labels and the text-section directive (a function template lives in a comdat section of its own);
the kernel descriptor (.amdhsa_* lines, kernel-argument size included) is part of the
body.  Kernels that exist only in NEW_DIR are listed as added.  Exit status 1 if any old kernel is missing or differs.
"""
import os
import re
import subprocess
import sys

_FUNC = re.compile(r"^(\S+):[ \t]*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", re.S | re.M)
_DESC = re.compile(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", re.S | re.M)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


_MANGLED = re.compile(r"^(_Z\d+[A-Za-z_]\w*?I(?:L[a-z]\d+E|DF16b|[a-z])+E)v")


def canonical(dem):
    if dem.startswith("_Z"):                  # not demangled (e.g. __bf16 arguments): drop a trailing Li9E template arg
        dem = re.sub(r"Li9EEv", "Ev", dem)
        m = _MANGLED.match(dem)               # name + template arguments; the return type and parameter types go
        return m.group(1) if m else dem
    if dem.startswith("void "):               # a function template's demangled name carries its return type
        dem = dem[len("void "):]
    if dem.endswith(")"):                     # drop the parameter list: the balanced group that ends the name
        depth, i = 0, len(dem)
        while i > 0:
            i -= 1
            depth += (dem[i] == ")") - (dem[i] == "(")
            if depth == 0:
                break
        dem = dem[:i]
    dem = re.sub(r", 9>$", ">", dem)          # kernel<..., 9>  -> kernel<...>
    return re.sub(r"<9>$", "", dem)           # kernel<9>       -> kernel


def bodies(path):
    txt = open(path).read()
    out = {}
    for m in _FUNC.finditer(txt):
        if not m.group(1).startswith("."):
            out[m.group(1)] = m.group(2)
    for m in _DESC.finditer(txt):
        out[m.group(1)] = out.get(m.group(1), "") + "\n" + m.group(2)
    return out


def normalise(body, own_name):
    lines = []
    for line in body.splitlines():
        line = line.split(";")[0].rstrip()
        s = line.strip()
        if not s or s.startswith((".loc", ".file", ".cfi", ".Ltmp", ".text", ".section\t.text")):
            continue      # debug info; the text section (a template's is a comdat group of its own)
        line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
        lines.append(line.replace(own_name, "<self>"))
    return lines


def main(old_dir, new_dir):
    same, bad, added = 0, [], 0
    for f in sorted(os.listdir(old_dir)):
        if not f.endswith(".s"):
            continue
        old = bodies(os.path.join(old_dir, f))
        new = bodies(os.path.join(new_dir, f)) if os.path.exists(os.path.join(new_dir, f)) else {}
        dold, dnew = demangle(list(old)), demangle(list(new))
        by_canon = {}
        dold = {n: canonical(d) for n, d in dold.items()}
        for n, d in dnew.items():
            by_canon.setdefault(canonical(d), []).append(n)
        matched = set()
        for n, body in old.items():
            cands = by_canon.get(dold[n], [])
            if len(cands) != 1:
                bad.append(f"{f}: {dold[n]}: {len(cands)} counterparts")
                continue
            matched.add(cands[0])
            a, b = normalise(body, n), normalise(new[cands[0]], cands[0])
            if a == b:
                same += 1
            else:
                ndiff = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
                bad.append(f"{f}: {dold[n]}: {ndiff} of {len(a)} lines differ")
        for n in new:
            if n not in matched:
                added += 1
                print(f"added  {f}: {dnew[n]}")
    print(f"{same} kernels identical, {len(bad)} differ or missing, {added} added")
    for b in bad:
        print("DIFF  ", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
