"""CPU-side checks of the extension header of moving geometry on x-slabs: include/fs3d_slab_geometry.h declares exactly what
capi.SYMBOLS_SLAB_GEOMETRY binds, the library exports those entries, and include/fs3d.h keeps the function set it had (no GPU)."""
import ctypes
import os
import re

from cmc_fluid_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"fs3d_update_nodes_slab", "fs3d_update_nodes_shape2d_slab", "fs3d_geometry_dead_lines"}


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fs3d_[a-z0-9_]+)\s*\(", text))


def test_the_extension_header_declares_what_the_binding_binds():
    assert declared("fs3d_slab_geometry.h") == set(capi.SYMBOLS_SLAB_GEOMETRY) == ENTRIES


def test_fs3d_h_keeps_its_function_set():
    assert declared("fs3d.h") == set(capi.SYMBOLS)
    assert not ENTRIES & set(capi.SYMBOLS) and not ENTRIES & set(capi.SYMBOLS_MESH_WALLS)


def test_the_library_exports_the_slab_entries(built):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in sorted(ENTRIES):
        assert hasattr(lib, name), "libfs3d_hip.so does not export %s" % name
        assert getattr(capi.load(), name).argtypes == capi.SYMBOLS_SLAB_GEOMETRY[name][1]
    # the slab entries take what their single-context twins take
    assert capi.SYMBOLS_SLAB_GEOMETRY["fs3d_update_nodes_slab"] == capi.SYMBOLS["fs3d_update_nodes"]
    assert capi.SYMBOLS_SLAB_GEOMETRY["fs3d_update_nodes_shape2d_slab"] == capi.SYMBOLS["fs3d_update_nodes_shape2d"]


def test_the_solver_class_has_the_slab_methods():
    assert callable(capi.Solver.update_nodes_slab) and callable(capi.Solver.update_nodes_shape2d_slab) and callable(capi.Solver.dead_lines)
