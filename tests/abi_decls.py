"""What include/fs3d.h declares, for the tests of the C ABI: the one parser of the header (comments stripped first).

functions()    {name: (return type, [parameter declarations])} of every fs3d_* prototype, in the header's order
enumerators()  {FS3D_X: n} of every enumerator
defines()      {FS3D_N_X: n} of every `#define FS3D_N_* n`
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fs3d.h")


def code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def functions():
    text = re.sub(r"^\s*#.*$", "", code(), flags=re.M)           # preprocessor lines end in no semicolon
    out = {}
    for stmt in text.split(";"):
        m = re.match(r"(.*?)\b(fs3d_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt.strip(), flags=re.S)
        if not m:
            continue
        ret, name, params = (" ".join(g.split()) for g in m.groups())
        assert name not in out, name + " is declared twice"
        out[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    assert len(out) == len(re.findall(r"\bfs3d_[a-z0-9_]+\s*\(", text)), "a prototype the parser does not read"
    return out


def enumerators():
    return {k: int(v) for k, v in re.findall(r"\b(FS3D_[A-Z0-9_]+)\s*=\s*(\d+)\b", code())}


def defines():
    return {k: int(v) for k, v in re.findall(r"^\s*#define\s+(FS3D_N_[A-Z0-9_]+)\s+(\d+)\s*$", code(), flags=re.M)}


def declares_status(name):
    """name is declared, with return type fs3d_status."""
    return functions().get(name, (None,))[0] == "fs3d_status"
