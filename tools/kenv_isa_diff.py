"""Compare the k_env instantiations of two device-assembly listings of csrc/ssd_env.hip (instruction streams only).

    hipcc <build flags of __graft_entry__.HIPCC_FLAGS without -shared> --cuda-device-only -S ssd_env.hip -o before.s   (parent tree)
    hipcc ... -o after.s                                                                                                 (this tree)
    python tools/kenv_isa_diff.py before.s after.s

k_env<MODE, NT, TAPE, OV> of the first listing is matched with k_env<MODE, NT, TAPE, OV, false> of the second (render mode added a
template flag, and a trailing field to the kernel-argument struct).  Basic-block labels are normalised (their numbers follow the function's position in
the file); assembler directives (.amdhsa_*, sections, symbol names) are left out.  Exit status 1 if any instruction stream differs.
"""
import re
import sys


def functions(path):
    out, name = {}, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", ln)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name and ln.startswith(".Lfunc_end"):
            name = None
            continue
        if name is not None:
            s = ln.split(";")[0].strip()
            if s and not s.startswith("."):
                out[name].append(re.sub(r"\.(LBB|Ltmp|LJTI)\d+_", r".\1_", s))
            elif s.startswith(".LBB"):
                out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def kenv_key(sym):
    m = re.match(r"_ZN3ssd5k_envILi(\d+)ELi(\d+)ELb(\d)ELi(\d+)E(Lb([01])E)?EEv", sym)
    if not m:
        return None
    return (int(m.group(1)), int(m.group(2)), bool(int(m.group(3))), int(m.group(4))), m.group(6) == "1"


def main(before, after):
    a, b = functions(before), functions(after)
    old = {kenv_key(k)[0]: k for k in a if kenv_key(k)}
    new = {kenv_key(k)[0]: k for k in b if kenv_key(k) and not kenv_key(k)[1]}
    rec = sorted(kenv_key(k)[0] for k in b if kenv_key(k) and kenv_key(k)[1])
    bad = []
    for key, sym in sorted(old.items()):
        same = key in new and a[sym] == b[new[key]]
        print("%-28s %6d instructions  %s" % ("k_env<%d, %d, %s, %d>" % key, len(a[sym]), "identical" if same else "DIFFERENT"))
        if not same:
            bad.append(key)
    print("render-mode instantiations (new): %s" % ", ".join("k_env<%d, %d, %s, %d, true>" % k for k in rec))
    print("%d of %d shipped instantiations identical" % (len(old) - len(bad), len(old)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
