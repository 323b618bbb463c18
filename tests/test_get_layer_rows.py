"""Result output by rows, the parts that need no GPU: slab.out_rows -- the twin of the row range fs3d_get_layer_rows reports --
against a brute-force count, and the three C-ABI entries exist."""
import ctypes as C

import abi_decls
from cmc_fluid_solver_amd import capi
from cmc_fluid_solver_amd.slab import out_rows, slab_range

NEW = ("fs3d_get_layer_rows", "fs3d_get_layer_dev", "fs3d_get_layer_info")


def test_out_rows_is_the_set_of_rows_whose_source_plane_the_slab_owns():
    """Every gx in 1..24, odx in 1..40 and split into 1..8 slabs (slab_range: even where n divides gx, else the first ranks hold
    one plane more; with n > gx the last slabs are empty): the ranges are contiguous, in rank order, partition [0, odx), and each
    is exactly {i : x0 <= i*gx // odx < x1} (FilterToArrays' source plane, TimeLayer3D.h:819-924)."""
    checked = 0
    for gx in range(1, 25):
        for odx in range(1, 41):
            src = [i * gx // odx for i in range(odx)]
            for n in range(1, 9):
                end = 0
                for r in range(n):
                    x0, x1 = slab_range(gx, r, n)
                    i0, i1 = out_rows(x0, x1, gx, odx)
                    assert i0 == end and i1 >= i0, (gx, odx, n, r)
                    assert list(range(i0, i1)) == [i for i in range(odx) if x0 <= src[i] < x1], (gx, odx, n, r)
                    end = i1
                    checked += 1
                assert end == odx, (gx, odx, n)
    assert checked == 24 * 40 * 36


def test_out_rows_of_the_whole_grid_is_everything():
    for gx, odx in ((23, 4), (23, 50), (96, 48), (1, 7)):
        assert out_rows(0, gx, gx, odx) == (0, odx)


def test_header_declares_and_library_exports_the_get_layer_entries(built):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert abi_decls.defines()["FS3D_N_GETLAYER_INFO"] == 3
    assert len(capi.Solver.GET_LAYER_INFO) == 3
