"""The point and ray queries' plumbing without a GPU: the header declares the calls, the library exports them, the wrapper
binds them, the two 48-byte structures have the header's fields at the header's offsets (as ctypes types and as numpy
dtypes), and header and wrapper state the same limits and bits."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "uint32_t": 4, "float": 4}
CALLS = ("dslam_query_points", "dslam_query_points_device", "dslam_cast_rays", "dslam_cast_rays_device")
BOUND = ("query_points", "query_points_device", "cast_rays", "cast_rays_device")


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


def test_the_structures_are_48_bytes_with_the_headers_offsets(pkg):
    for name, struct, dtype in (("dslam_point_sample", pkg.PointSample, pkg.POINT_SAMPLE_DTYPE),
                                ("dslam_ray_hit", pkg.RayHit, pkg.RAY_HIT_DTYPE)):
        fields, size = header_layout(name)
        assert size == 48 and ctypes.sizeof(struct) == 48 and dtype.itemsize == 48, name
        assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields, name
        assert [(n, dtype.fields[n][1], dtype.fields[n][0].itemsize) for n in dtype.names] == fields, name
    assert pkg.POINT_SAMPLE_DTYPE["found_lo"].kind == "u" and pkg.POINT_SAMPLE_DTYPE["status"].kind == "i"
    assert pkg.RAY_HIT_DTYPE["status"].kind == "i" and pkg.RAY_HIT_DTYPE["steps"].kind == "i"


def test_limits_and_bits_agree_in_header_and_wrapper(pkg):
    assert header_macro("DSLAM_QUERY_MAX_ELEMENTS") == pkg.QUERY_MAX_ELEMENTS == 1 << 24
    assert header_macro("DSLAM_QUERY_MAX_RAY_VOXELS") == pkg.QUERY_MAX_RAY_VOXELS == 16384
    assert (header_macro("DSLAM_QUERY_SDF"), header_macro("DSLAM_QUERY_GRADIENT"), header_macro("DSLAM_QUERY_COLOUR")) == \
        (pkg.QUERY_SDF, pkg.QUERY_GRADIENT, pkg.QUERY_COLOUR) == (1, 2, 4)
    assert pkg.QUERY_ALL == 7
    assert header_macro("DSLAM_QUERY_OUTSIDE") == pkg.QUERY_OUTSIDE == 1
