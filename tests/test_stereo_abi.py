"""The stereo matcher's plumbing without a GPU: the header declares the calls, the library exports them, the wrapper binds
them, the ctypes structures and numpy dtypes have the header's fields at the header's offsets, and header, wrapper and
reference state the same limits, defaults and parameter encoding."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "uint32_t": 4, "float": 4}
CALLS = ("dslam_stereo_create", "dslam_stereo_destroy", "dslam_stereo_get_params", "dslam_stereo_match", "dslam_stereo_match_device",
         "dslam_disparity_to_depth", "dslam_disparity_to_depth_device", "dslam_stereo_depth", "dslam_stereo_depth_device",
         "dslam_debug_stereo_download", "dslam_debug_stereo_select", "dslam_debug_stereo_phases")
BOUND = ("create_stereo", "stereo_get_params", "stereo_match", "stereo_match_device", "disparity_to_depth", "disparity_to_depth_device",
         "stereo_depth", "stereo_depth_device", "debug_stereo_download", "debug_stereo_select", "stereo_phases")


def raw_header():
    return open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()


def header_text():
    return re.sub(r"/\*.*?\*/", "", raw_header(), flags=re.S)


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


def macro(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\w+)", header_text()).group(1), 0)


def test_the_calls_are_declared_exported_and_bound(pkg):
    txt = header_text()
    for call in CALLS:
        assert re.search(r"\bint\s+" + call + r"\s*\(", txt), call
    assert set(CALLS) <= pkg.exported_symbols()
    for name in BOUND:
        assert callable(getattr(pkg.CApi, name)), name


def test_structures_match_the_header(pkg):
    for name, struct, dtype, size in (("dslam_stereo_params", pkg.StereoParams, pkg.STEREO_PARAMS_DTYPE, 32),
                                      ("dslam_stereo_calib", pkg.StereoCalib, pkg.STEREO_CALIB_DTYPE, 20)):
        fields, total = header_layout(name)
        assert total == size == ctypes.sizeof(struct) == dtype.itemsize, name
        assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields, name
        assert [(n, dtype.fields[n][1], dtype.fields[n][0].itemsize) for n in dtype.names] == fields, name


def test_limits_and_constants_agree(pkg):
    import ref_stereo as rs
    for name, wrapper, ref in (("DSLAM_STEREO_INVALID", pkg.STEREO_INVALID, rs.INVALID), ("DSLAM_STEREO_COST_OUT", pkg.STEREO_COST_OUT, rs.COST_OUT),
                               ("DSLAM_STEREO_MAX_SIZE", pkg.STEREO_MAX_SIZE, rs.MAX_SIZE), ("DSLAM_STEREO_MAX_P2", pkg.STEREO_MAX_P2, rs.MAX_P2),
                               ("DSLAM_STEREO_CENSUS_LEFT", pkg.STEREO_CENSUS_LEFT, rs.CENSUS_LEFT),
                               ("DSLAM_STEREO_CENSUS_RIGHT", pkg.STEREO_CENSUS_RIGHT, rs.CENSUS_RIGHT), ("DSLAM_STEREO_S", pkg.STEREO_S, rs.WHAT_S)):
        assert macro(name) == wrapper == ref, name
    assert (macro("DSLAM_STEREO_INVALID"), macro("DSLAM_STEREO_COST_OUT")) == (0xFFFF, 63)
    # the bounds the law rests on: every L_r in a byte, S in 16 bits below INVALID
    assert rs.COST_OUT + rs.MAX_P2 == 255 and 8 * 255 < rs.INVALID


def test_defaults_and_encoding_agree(pkg):
    import ref_stereo as rs
    p = pkg.StereoParams()
    assert p.as_dict() == dict(max_disparity=0, p1=0, p2=0, uniqueness=0, lr_max=0, channels=0)   # 0 selects the default
    assert rs.resolve(p.as_dict()) == dict(max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max=1, channels=1) == rs.DEFAULTS
    # the header's comments state the same defaults next to the fields
    for field, default in rs.DEFAULTS.items():
        assert re.search(r"int32_t\s+" + field + r";\s*/\*\s*0 -> " + str(default) + r"\b", raw_header()), field
    # off and exact have codes of their own; the wrapper and the reference decode them alike
    for enc in (dict(uniqueness=-1), dict(lr_max=-1), dict(lr_max=-2), dict(uniqueness=99, lr_max=64, max_disparity=64), dict(channels=4)):
        eff = rs.resolve(enc)
        filled = {k: (enc.get(k) or rs.DEFAULTS[k]) for k in rs.DEFAULTS}   # as dslam_stereo_get_params returns it
        assert pkg.StereoParams(**filled).effective() == eff, enc
    assert rs.resolve(rs.encode(uniqueness=0, lr_max=0)) == dict(rs.DEFAULTS, uniqueness=0, lr_max=0)
    assert rs.resolve(rs.encode(lr_max=-1))["lr_max"] == -1
    for bad in (dict(max_disparity=96), dict(p1=11, p2=10), dict(p2=193), dict(uniqueness=100), dict(uniqueness=-2), dict(lr_max=-3),
                dict(lr_max=65, max_disparity=64), dict(channels=3), dict(p1=-1)):
        with pytest.raises(ValueError):
            rs.resolve(bad)
