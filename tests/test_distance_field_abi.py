"""The occupancy and distance grids' plumbing without a GPU: the header declares the calls, the library exports them, the
wrapper binds them, dslam_grid is 32 bytes with the header's fields at the header's offsets (as a ctypes type and as a numpy
dtype), header and wrapper state the same limits, bits and far values, and dslam_grid_from_box (host only) follows its law."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "uint32_t": 4, "float": 4}
CALLS = ("dslam_grid_from_box", "dslam_mark_occupancy", "dslam_mark_occupancy_device", "dslam_distance_transform",
         "dslam_distance_transform_device", "dslam_distance_field", "dslam_distance_field_device")
BOUND = ("grid_from_box", "mark_occupancy", "mark_occupancy_device", "distance_transform", "distance_transform_device",
         "distance_field", "distance_field_device")


def header_text():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_layout(name):
    """[(field, offset, size)] and the size of `typedef struct { ... } name;` by the C layout rules (4-byte fields only)."""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", header_text()).group(1)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            size = SIZES[ctype] * int(m.group(2) or 1)
            fields.append((m.group(1), off, size))
            off += size
    return fields, off


def header_macro(name):
    m = re.search(r"#define\s+" + name + r"\s+(.+)", header_text())
    assert m, name
    return int(eval(m.group(1).strip(), {"__builtins__": {}}))


def test_the_calls_are_declared_exported_and_bound(pkg):
    txt = header_text()
    for call in CALLS:
        assert re.search(r"\bint\s+" + call + r"\s*\(", txt), call
    assert set(CALLS) <= pkg.exported_symbols()
    for name in BOUND:
        assert callable(getattr(pkg.CApi, name)), name


def test_the_grid_is_32_bytes_with_the_headers_offsets(pkg):
    fields, size = header_layout("dslam_grid")
    assert fields == [("origin", 0, 12), ("cell", 12, 4), ("dims", 16, 12), ("pad", 28, 4)]
    assert size == 32 and ctypes.sizeof(pkg.Grid) == 32 and pkg.GRID_DTYPE.itemsize == 32
    assert [(n, getattr(pkg.Grid, n).offset, getattr(pkg.Grid, n).size) for n, _ in pkg.Grid._fields_] == fields
    assert [(n, pkg.GRID_DTYPE.fields[n][1], pkg.GRID_DTYPE.fields[n][0].itemsize) for n in pkg.GRID_DTYPE.names] == fields
    assert all(pkg.GRID_DTYPE[n].base.kind == "i" for n in pkg.GRID_DTYPE.names)
    g = pkg.Grid.of((-3, 4, 5), 2, (7, 8, 9))
    assert g.cells == 7 * 8 * 9 and bytes(g) == np.array([-3, 4, 5, 2, 7, 8, 9, 0], "<i4").tobytes()


def test_limits_bits_and_far_values_agree_in_header_and_wrapper(pkg):
    assert header_macro("DSLAM_GRID_MAX_CELL") == pkg.GRID_MAX_CELL == 64
    assert header_macro("DSLAM_GRID_MAX_DIM") == pkg.GRID_MAX_DIM == 1024
    assert header_macro("DSLAM_GRID_MAX_CELLS") == pkg.GRID_MAX_CELLS == 1 << 26
    assert (header_macro("DSLAM_CELL_OBSERVED"), header_macro("DSLAM_CELL_OCCUPIED")) == (pkg.CELL_OBSERVED, pkg.CELL_OCCUPIED) == (1, 2)
    assert (header_macro("DSLAM_SEED_OCCUPIED"), header_macro("DSLAM_SEED_UNKNOWN")) == (pkg.SEED_OCCUPIED, pkg.SEED_UNKNOWN) == (1, 2)
    assert (header_macro("DSLAM_DIST_SQUARED_CELLS"), header_macro("DSLAM_DIST_METRES")) == (pkg.DIST_SQUARED_CELLS, pkg.DIST_METRES) == (0, 1)
    assert header_macro("DSLAM_DIST_MAX_CELLS") == pkg.DIST_MAX_CELLS == 1774 and 1774 > 1023 * math.sqrt(3) > 1771
    assert header_macro("DSLAM_DIST_FAR") == pkg.DIST_FAR == 0x7FFFFFFF


# ---- dslam_grid_from_box: host only, so it runs here -------------------------------------------------------------------
def grid_from_box(pkg, lo, hi, vs, cell):
    lib = ctypes.CDLL(pkg.LIB_PATH)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    g = pkg.Grid.of((9, 9, 9), 9, (9, 9, 9), 9)
    f32p = ctypes.POINTER(ctypes.c_float)
    rc = lib.dslam_grid_from_box(lo.ctypes.data_as(f32p), hi.ctypes.data_as(f32p), ctypes.c_float(vs), ctypes.c_int(cell), ctypes.byref(g))
    return rc, g


def law(lo, hi, vs, cell):
    vs = float(np.float32(vs))
    origin = [math.floor(float(np.float32(v)) / vs) for v in lo]
    dims = [max(1, math.ceil((float(np.float32(h)) / vs - o) / cell)) for h, o in zip(hi, origin)]
    return origin, dims


@pytest.mark.parametrize("lo,hi,vs,cell", [((-0.17, -0.22, 0.25), (0.23, 0.18, 0.65), 0.005, 2),
                                          ((-1.003, 0.0, 0.499), (1.0, 0.0, 0.5), 0.005, 4),
                                          ((0.1, 0.1, 0.1), (0.1, 0.1, 0.1), 0.01, 64),
                                          ((-10.0, -10.0, -1.0), (10.0, 10.0, 2.0), 0.02, 2)])
def test_grid_from_box_follows_its_law(pkg, lo, hi, vs, cell):
    rc, g = grid_from_box(pkg, lo, hi, vs, cell)
    origin, dims = law(lo, hi, vs, cell)
    assert rc == 0 and (list(g.origin), g.cell, list(g.dims), g.pad) == (origin, cell, dims, 0)
    # the box lies inside the grid
    for a in range(3):
        assert g.origin[a] * float(np.float32(vs)) <= lo[a] + 1e-9
        assert (g.origin[a] + cell * g.dims[a]) * float(np.float32(vs)) >= hi[a] - 1e-6


@pytest.mark.parametrize("lo,hi,vs,cell", [((0, 0, 0), (1, 1, 1), 0.005, 0), ((0, 0, 0), (1, 1, 1), 0.005, 65),
                                          ((0, 0, 0), (1, 1, -0.1), 0.005, 1),              # hi < lo
                                          ((0, 0, 0), (6, 1, 1), 0.005, 1),                 # 1200 cells along x
                                          ((0, 0, 0), (4, 4, 4), 0.005, 1),                 # 800^3 cells
                                          ((-6000, 0, 0), (-5999, 1, 1), 0.005, 2),         # below -2^20 voxels
                                          ((5242, 0, 0), (5243, 1, 1), 0.005, 2),           # above 2^20 voxels
                                          ((0, float("nan"), 0), (1, 1, 1), 0.005, 1), ((0, 0, 0), (1, float("inf"), 1), 0.005, 1),
                                          ((0, 0, 0), (1, 1, 1), 0.0, 1), ((0, 0, 0), (1, 1, 1), float("nan"), 1)])
def test_grid_from_box_rejects_what_exceeds_the_limits_and_writes_nothing(pkg, lo, hi, vs, cell):
    rc, g = grid_from_box(pkg, lo, hi, vs, cell)
    assert rc < 0
    assert (list(g.origin), g.cell, list(g.dims), g.pad) == ([9, 9, 9], 9, [9, 9, 9], 9)
