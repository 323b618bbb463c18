"""CPU-side checks of the drop-in boundary, the one place that pins the whole C ABI: include/fs3d.h, capi.SYMBOLS and the
exports of the library built for gfx950 name the same 59 functions, every ctypes signature agrees with its prototype, and the
constants of capi.py are the header's (no compute, no GPU).  A new entry is declared, bound and counted here."""
import ctypes
import os
import subprocess

import abi_decls
from cmc_fluid_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FUNCTIONS = 59
INT_TYPES = ("int", "fs3d_precision", "fs3d_status")            # an enum is an int in the C ABI of every target the library builds for
SCALARS = {"double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURNS = {"fs3d_status": ctypes.c_int, "void": None, "const char *": ctypes.c_char_p}
CONSTANT_PREFIXES = ("OPT_", "SWEEP_", "ERR_", "LAYER_", "DIR_")


def test_header_declares_what_the_binding_binds():
    declared = abi_decls.functions()
    assert set(declared) == set(capi.SYMBOLS)
    assert len(declared) == N_FUNCTIONS
    assert list(declared) == list(capi.SYMBOLS), "capi.SYMBOLS is ordered as the header is"


def test_library_exports_every_declared_symbol(built):
    """... and nothing else under the fs3d_ prefix."""
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("fs3d_")}
    declared = set(abi_decls.functions())
    assert declared - exported == set(), "declared, not exported"
    assert exported - declared == set(), "exported, not declared"
    assert b"gfx950" in capi.load().fs3d_version()


def is_ctypes_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def param_agrees(decl, ctype):
    """One parameter declaration of the header against one entry of argtypes."""
    if "*" in decl or "[" in decl:
        return is_ctypes_pointer(ctype)
    ctext = " ".join(decl.split()[:-1])                         # without the parameter's name
    if ctext in INT_TYPES:
        return ctype is ctypes.c_int
    return ctext in SCALARS and ctype is SCALARS[ctext]


def test_every_signature_of_the_binding_agrees_with_its_prototype(built):
    lib = capi.load()
    for name, (ret, params) in abi_decls.functions().items():
        restype, argtypes = capi.SYMBOLS[name]
        assert ret in RETURNS and restype is RETURNS[ret], (name, ret, restype)
        assert len(params) == len(argtypes), (name, params, argtypes)
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert param_agrees(decl, ctype), (name, k, decl, ctype)
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name


def test_the_signature_check_tells_kinds_apart():
    """The check above is worth its name: it refuses each kind of parameter bound as another kind."""
    kinds = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_float]
    pointers = kinds[:3]
    for decl, want in (("const void *vx", pointers), ("int n_seg_out[3]", pointers), ("const char *names[FS3D_N_EVENTS]", pointers),
                       ("int layer", [ctypes.c_int]), ("fs3d_precision prec", [ctypes.c_int]), ("double dt", [ctypes.c_double]),
                       ("size_t elems", [ctypes.c_size_t])):
        assert [t for t in kinds if param_agrees(decl, t)] == want, decl
    assert not param_agrees("long long count", ctypes.c_longlong)       # a type the tables above do not know is refused, not waved through


def test_constants_of_the_binding_are_the_headers():
    enums = abi_decls.enumerators()
    shared = [k for k in enums if hasattr(capi, k[len("FS3D_"):])]
    for k in shared:
        assert getattr(capi, k[len("FS3D_"):]) == enums[k], k
    for k in ("FS3D_OK", "FS3D_F32", "FS3D_F64"):
        assert k in shared, k
    ours = [n for n in dir(capi) if n.startswith(CONSTANT_PREFIXES)]
    assert {n[:n.index("_") + 1] for n in ours} == set(CONSTANT_PREFIXES)
    for n in ours:
        assert "FS3D_" + n in enums, "capi.%s is not in the header" % n
    opts = [v for k, v in enums.items() if k.startswith("FS3D_OPT_")]
    assert len(opts) == len(set(opts)), "two options share an id"
    defines = abi_decls.defines()
    assert defines == {"FS3D_N_GEOM_INFO": len(capi.Solver.GEOMETRY_INFO), "FS3D_N_GETLAYER_INFO": len(capi.Solver.GET_LAYER_INFO),
                       "FS3D_N_EVENTS": capi.N_EVENTS}


def test_no_oracle_in_the_product():
    """The shipped package must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "cmc_fluid_solver_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                text = open(os.path.join(dp, f)).read()
                assert "liboracle" not in text and "from oracle" not in text and "import oracle" not in text, f
    import subprocess
    out = subprocess.run(["ldd", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_create_fails_loudly_without_gpu(built):
    """No silent fallback: without a usable device fs3d_create returns an error status."""
    import torch
    if torch.cuda.is_available():
        return
    lib = capi.load()
    h = ctypes.c_void_p()
    st = lib.fs3d_create(ctypes.byref(h), 0, capi.F32, 8, 8, 8, 0.1, 0.1, 0.1, 0, 8)
    assert st != capi.OK and not h.value
    assert lib.fs3d_last_error(None)
