"""CPU-side checks of the entries of moving geometry on x-slabs: include/fs3d.h declares them, capi.SYMBOLS binds them with the
arguments of their single-context twins, the library exports them (no GPU).  tests/test_capi_symbols.py holds the whole ABI."""
import ctypes

import abi_decls
from cmc_fluid_solver_amd import capi

ENTRIES = {"fs3d_update_nodes_slab", "fs3d_update_nodes_shape2d_slab", "fs3d_geometry_dead_lines"}


def test_the_header_declares_and_the_binding_binds_the_slab_entries():
    for name in sorted(ENTRIES):
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS, name


def test_the_library_exports_the_slab_entries(built):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in sorted(ENTRIES):
        assert hasattr(lib, name), "libfs3d_hip.so does not export %s" % name
        assert getattr(capi.load(), name).argtypes == capi.SYMBOLS[name][1]
    # the slab entries take what their single-context twins take, in the binding and in the header
    declared = abi_decls.functions()
    for slab, twin in (("fs3d_update_nodes_slab", "fs3d_update_nodes"), ("fs3d_update_nodes_shape2d_slab", "fs3d_update_nodes_shape2d")):
        assert capi.SYMBOLS[slab] == capi.SYMBOLS[twin] and declared[slab] == declared[twin], slab


def test_the_solver_class_has_the_slab_methods():
    assert callable(capi.Solver.update_nodes_slab) and callable(capi.Solver.update_nodes_shape2d_slab) and callable(capi.Solver.dead_lines)
