"""The view survey's plumbing without a GPU: the header declares the three calls, the library exports them, the wrapper
binds them, and the ctypes structures have the header's fields at the header's offsets."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "float": 4}
CALLS = ("dslam_view_frustum_planes", "dslam_survey_views", "dslam_select_view_maps")


def header_text():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_layout(name):
    """[(field, offset, size)] and the size of `typedef struct { ... } name;` by the C layout rules (arrays included)."""
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


def test_the_three_calls_are_declared_exported_and_bound(pkg):
    txt = header_text()
    for call in CALLS:
        assert re.search(r"\bint\s+" + call + r"\s*\(", txt), call
    assert set(CALLS) <= pkg.exported_symbols()
    assert callable(pkg.CApi.view_frustum_planes) and callable(pkg.CApi.survey_views) and callable(pkg.CApi.select_view_maps)
    assert re.search(r"#define\s+DSLAM_MAX_SURVEY_MAPS\s+256\b", txt) and re.search(r"#define\s+DSLAM_MAX_SURVEY_VIEWS\s+16\b", txt)
    assert (pkg.MAX_SURVEY_MAPS, pkg.MAX_SURVEY_VIEWS) == (256, 16)


def test_ctypes_structures_match_the_header(pkg):
    for name, struct in (("dslam_survey_view", pkg.SurveyView), ("dslam_view_survey_params", pkg.ViewSurveyParams),
                         ("dslam_view_select_params", pkg.ViewSelectParams), ("dslam_view_select_result", pkg.ViewSelectResult)):
        fields, size = header_layout(name)
        assert ctypes.sizeof(struct) == size, name
        assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields, name
    p = pkg.ViewSelectParams()
    assert (p.min_blocks, p.max_maps, p.always_keep, p.pad) == (0, 0, -1, 0)
    assert pkg.ViewSurveyParams().margin_voxels == 0.0


def test_the_reference_states_the_same_limits(pkg):
    import ref_view_survey as rv
    assert (rv.MAX_RENDER_MAPS, rv.MAX_SURVEY_MAPS, rv.MAX_SURVEY_VIEWS) == (pkg.MAX_RENDER_MAPS, pkg.MAX_SURVEY_MAPS, pkg.MAX_SURVEY_VIEWS)
