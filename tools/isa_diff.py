"""Compare named kernels of two device-assembly listings of the same .hip source (instruction streams only).

    hipcc <build flags of __graft_entry__.HIPCC_FLAGS without -shared> --cuda-device-only -S csrc/X.hip -o before/X.s   (parent tree)
    hipcc ... -o after/X.s                                                                                                (this tree)
    python tools/isa_diff.py before/X.s after/X.s k_encode k_encode_lut k_inc_encode ...

Every kernel of the FIRST listing whose name (the unqualified function name, template arguments aside) is one of the given names is
matched with the symbol of the same mangled name in the second and their instruction streams compared.  Basic-block labels are
normalised (their numbers follow the function's position in the file); assembler directives (.amdhsa_*, sections, symbol names) are
left out.  Kernels of those names that only the second listing has are listed as new.  Exit status 1 if any stream differs or is
missing.  A kernel whose mangled name is gone from the second listing while exactly ONE kernel of the same unqualified name is new
there (its parameter types changed, its body need not have) is compared with that one and reported as "identical (signature changed)".
(tools/kenv_isa_diff.py is the k_env-only predecessor, which also maps a changed template signature.)
"""
import re
import subprocess
import sys

from kenv_isa_diff import functions


def base_name(sym):
    """_ZN3ssd<len><name>... -> name (kernels of namespace ssd), else None"""
    m = re.match(r"_ZN3ssd(\d+)", sym)
    if not m:
        return None
    n = int(m.group(1))
    return sym[m.end():m.end() + n]


def demangle(syms):
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.strip().split("\n")
        except (OSError, subprocess.CalledProcessError):
            continue
        if len(out) == len(syms):
            return dict(zip(syms, out))
    return {s: s for s in syms}


def main(before, after, names):
    a, b = functions(before), functions(after)
    old = sorted(k for k in a if base_name(k) in names)
    new = sorted(k for k in b if base_name(k) in names and k not in a)
    pretty = demangle(old + new)
    bad = 0
    for sym in old:
        other, note = sym, ""
        if sym not in b:            # the same unqualified name under ONE new signature, none of the old ones left
            cands = [k for k in new if base_name(k) == base_name(sym)]
            if len(cands) == 1 and not any(base_name(k) == base_name(sym) for k in old if k in b):
                other, note = cands[0], " (signature changed: %s)" % pretty[cands[0]].replace("ssd::", "")
                new.remove(other)
        same = other in b and a[sym] == b[other]
        print("%-72s %6d instructions  %s%s" % (pretty[sym].replace("ssd::", ""), len(a[sym]), "identical" if same else ("DIFFERENT" if other in b else "MISSING"), note))
        bad += not same
    for sym in new:
        print("%-72s %6d instructions  new" % (pretty[sym].replace("ssd::", ""), len(b[sym])))
    print("%d of %d kernels identical" % (len(old) - bad, len(old)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], set(sys.argv[3:])))
