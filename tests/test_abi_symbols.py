"""CPU suite: the C-ABI shared library loads and exports every symbol include/ssd_hip.h declares, bound as abi.HIP_SIGNATURES says, and
every struct of abi lays out as the header's (no compute calls)."""
import ctypes
import os
import re

from homophily_marl_amd import abi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declared():
    src = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ssd_[a-z_0-9]+)\s*\(", src)))


def test_header_and_ctypes_table_agree():
    assert _declared() == sorted(abi.HIP_SIGNATURES)


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(abi.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    lib.ssd_abi_version.restype = ctypes.c_int
    assert lib.ssd_abi_version() == abi.ABI_VERSION
    bound = abi.load_library()
    for name, (res, argtypes) in abi.HIP_SIGNATURES.items():
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is res, name


def _c_name(cls):
    """SsdTdLossArgs -> ssd_td_loss_args"""
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


def test_struct_layouts_match_the_header(tmp_path):
    """Every ctypes.Structure of abi is a typedef of the header under its snake-case name and the other way round (the ssd_status enum
    aside), with the header's field names in the header's order; sizeof() and the offsetof() of every field as seen by a C compiler ==
    the ctypes mirror.  ONE program prints them all."""
    import subprocess
    structs = {_c_name(v): v for v in vars(abi).values()
               if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == abi.__name__}
    src = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert sorted(structs) == sorted(set(re.findall(r"^\}\s*(ssd_\w+)\s*;", src, flags=re.M)) - {"ssd_status"})
    bodies = {name: body for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(ssd_\w+)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S))}
    for name, cls in structs.items():       # "int32_t a, b[4]; const float *c, *d;" -> a, b, c, d
        declared = [re.sub(r"\[.*?\]", "", d).split()[-1].lstrip("*") for decl in bodies[name].split(";") if decl.strip() for d in decl.split(",")]
        assert declared == [f[0] for f in cls._fields_], name
    probes = [(c, cls, None) for c, cls in structs.items()] + [(c, cls, f[0]) for c, cls in structs.items() for f in cls._fields_]
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssd_hip.h"\nint main(){\n'
                 + "".join('printf("%%zu\\n", %s);\n' % ("sizeof(%s)" % n if f is None else "offsetof(%s, %s)" % (n, f)) for n, _, f in probes)
                 + "return 0;}\n")
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(cls) if f is None else getattr(cls, f).offset for _, cls, f in probes]
    print("%d structs, %d values" % (len(structs), len(want)))
    assert len(got) == len(want)
    assert got == want, [(n, f, g, w) for (n, _, f), g, w in zip(probes, got, want) if g != w]


def test_oracle_is_not_reachable_from_the_product_package():
    """The product package must never import or link the checker."""
    pkg = os.path.join(ROOT, "homophily_marl_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.replace("The CPU oracle under oracle/ is a separate", "") or f in (), (dp, f)
