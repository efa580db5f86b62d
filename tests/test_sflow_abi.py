"""The scene-flow matcher's plumbing without a GPU: the header declares the calls, the library exports them, the wrapper
binds them, the ctypes structure and numpy dtype have the header's fields at the header's offsets, and header, wrapper and
reference state the same limits, record sizes, defaults and parameter encoding."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("dslam_sflow_create", "dslam_sflow_destroy", "dslam_sflow_get_params", "dslam_sflow_push", "dslam_sflow_push_device",
         "dslam_sflow_match", "dslam_sflow_match_device", "dslam_sflow_features", "dslam_debug_sflow_download", "dslam_debug_sflow_phases")
BOUND = ("create_sflow", "sflow_get_params", "sflow_push", "sflow_push_device", "sflow_match", "sflow_match_device", "sflow_features",
         "debug_sflow_download", "sflow_phases")


def raw_header():
    return open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()


def header_text():
    return re.sub(r"/\*.*?\*/", "", raw_header(), flags=re.S)


def header_layout(name):
    """[(field, offset, size)] and the size of `typedef struct { ... } name;` (int32 fields only)."""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", header_text()).group(1)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype == "int32_t"
        for n in names.split(","):
            fields.append((n.strip(), off, 4))
            off += 4
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


def test_the_structure_matches_the_header(pkg):
    fields, total = header_layout("dslam_sflow_params")
    struct, dtype = pkg.SflowParams, pkg.SFLOW_PARAMS_DTYPE
    assert total == 32 == ctypes.sizeof(struct) == dtype.itemsize
    assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields
    assert [(n, dtype.fields[n][1], dtype.fields[n][0].itemsize) for n in dtype.names] == fields


def test_limits_and_constants_agree(pkg):
    import ref_sflow as rf
    for name, wrapper, ref in (("DSLAM_SFLOW_MAX_SIZE", pkg.SFLOW_MAX_SIZE, rf.MAX_SIZE), ("DSLAM_SFLOW_MAX_NMS_N", pkg.SFLOW_MAX_NMS_N, rf.MAX_NMS_N),
                               ("DSLAM_SFLOW_MAX_BINS", pkg.SFLOW_MAX_BINS, rf.MAX_BINS), ("DSLAM_SFLOW_MAX_FEATURES", pkg.SFLOW_MAX_FEATURES, rf.MAX_FEATURES),
                               ("DSLAM_SFLOW_MARGIN", pkg.SFLOW_MARGIN, rf.MARGIN), ("DSLAM_SFLOW_MAX_COST", pkg.SFLOW_MAX_COST, rf.MAX_COST),
                               ("DSLAM_SFLOW_SOBEL_BOUND", pkg.SFLOW_SOBEL_BOUND, rf.SOBEL_BOUND),
                               ("DSLAM_SFLOW_CHECKER_BOUND", pkg.SFLOW_CHECKER_BOUND, rf.CHECKER_BOUND),
                               ("DSLAM_SFLOW_FEATURE_BYTES", pkg.SFLOW_FEATURE_BYTES, rf.FEATURE_BYTES),
                               ("DSLAM_SFLOW_MATCH_WORDS", pkg.SFLOW_MATCH_WORDS, rf.MATCH_WORDS),
                               ("DSLAM_SFLOW_IMAGE_1C", pkg.SFLOW_IMAGE_1C, rf.IMAGE_1C), ("DSLAM_SFLOW_IMAGE_2C", pkg.SFLOW_IMAGE_2C, rf.IMAGE_2C),
                               ("DSLAM_SFLOW_IMAGE_1P", pkg.SFLOW_IMAGE_1P, rf.IMAGE_1P), ("DSLAM_SFLOW_IMAGE_2P", pkg.SFLOW_IMAGE_2P, rf.IMAGE_2P),
                               ("DSLAM_SFLOW_FILTER_DU", pkg.SFLOW_FILTER_DU, rf.FILTER_DU), ("DSLAM_SFLOW_FILTER_DV", pkg.SFLOW_FILTER_DV, rf.FILTER_DV),
                               ("DSLAM_SFLOW_FILTER_F1", pkg.SFLOW_FILTER_F1, rf.FILTER_F1), ("DSLAM_SFLOW_FILTER_F2", pkg.SFLOW_FILTER_F2, rf.FILTER_F2)):
        assert macro(name) == wrapper == ref, name
    # what the law and the kernels rest on: a record is 12 words; every intermediate of the filters fits int16; a cost fits 13
    # bits, a bin coordinate 13 bits and a feature index 24 bits of a 64-bit key
    assert rf.FEATURE_BYTES == 4 * rf.FEATURE_WORDS == 16 + 2 * len(rf.TAPS) and rf.MATCH_WORDS == 12
    assert max(rf.SOBEL_BOUND, rf.CHECKER_BOUND, rf.BLOB_BOUND) < 2 ** 15
    assert rf.MAX_COST == 32 * 255 < 2 ** 13 and rf.MAX_SIZE < 2 ** 13 and rf.MAX_FEATURES < 2 ** 24


def test_defaults_and_encoding_agree(pkg):
    import ref_sflow as rf
    p = pkg.SflowParams()
    assert p.as_dict() == dict.fromkeys(rf.DEFAULTS, 0)                          # 0 selects the default
    assert rf.resolve(p.as_dict()) == rf.DEFAULTS == dict(nms_n=3, nms_tau=50, match_binsize=50, match_radius=200, match_disp_tolerance=2,
                                                          half_resolution=1, channels=1)
    for field, default in rf.DEFAULTS.items():
        assert re.search(r"int32_t\s+" + field + r";\s*/\*\s*0 -> " + str(default) + r"\b", raw_header()), field
    # off has a code of its own; the wrapper and the reference decode it alike
    for enc in (dict(half_resolution=-1), dict(half_resolution=1), dict(channels=4, nms_n=5), dict(match_radius=100, half_resolution=-1)):
        filled = {k: (enc.get(k) or rf.DEFAULTS[k]) for k in rf.DEFAULTS}           # as dslam_sflow_get_params returns it
        assert pkg.SflowParams(**filled).effective() == rf.resolve(enc), enc
    assert rf.encode(half_resolution=0) == dict(half_resolution=-1) and rf.encode(half_resolution=1) == dict(half_resolution=1)
    with pytest.raises(ValueError):
        rf.resolve(dict(half_resolution=-2))
