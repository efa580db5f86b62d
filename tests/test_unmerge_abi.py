"""dslam_unmerge_maps' and dslam_remerge_maps' plumbing without a GPU: the symbols are exported, the header declares them,
and the ctypes structures have the header's fields at the header's offsets."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "int64_t": 8, "float": 4}


def header_text():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_layout(name):
    """[(field, offset, size)] and the size of `typedef struct { ... } name;` by the C layout rules."""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", header_text()).group(1)
    fields, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        size = SIZES[ctype]
        align = max(align, size)
        for n in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((n.strip(), off, size))
            off += size
    return fields, (off + align - 1) // align * align


def test_library_exports_the_entry_points(pkg):
    assert {"dslam_unmerge_maps", "dslam_remerge_maps"} <= pkg.exported_symbols()


def test_header_declares_the_entry_points():
    txt = header_text()
    assert re.search(r"\bint\s+dslam_unmerge_maps\s*\(\s*dslam_engine\s*\*\s*\w+\s*,\s*const\s+dslam_scene\s*\*\s*\w+\s*,\s*dslam_scene\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s+\w+\[16\]\s*,\s*const\s+dslam_unmerge_params\s*\*\s*\w+\s*,\s*dslam_unmerge_result\s*\*", txt)
    assert re.search(r"\bint\s+dslam_remerge_maps\s*\(\s*dslam_engine\s*\*\s*\w+\s*,\s*const\s+dslam_scene\s*\*\s*\w+\s*,\s*dslam_scene\s*\*\s*\w+\s*,"
                     r"\s*const\s+float\s+\w+\[16\]\s*,\s*const\s+float\s+\w+\[16\]\s*,\s*const\s+dslam_merge_params\s*\*\s*\w+\s*,"
                     r"\s*dslam_unmerge_result\s*\*\s*\w+\s*,\s*dslam_merge_result\s*\*", txt)


def test_ctypes_structures_match_the_header(pkg):
    for name, struct in (("dslam_unmerge_params", pkg.UnmergeParams), ("dslam_unmerge_result", pkg.UnmergeResult)):
        fields, size = header_layout(name)
        assert ctypes.sizeof(struct) == size, name
        assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields, name
    assert [n for n, _, _ in header_layout("dslam_unmerge_result")[0]] == [
        "src_blocks", "blocks_touched", "src_candidates", "out_of_range", "candidates_without_block", "voxels_changed",
        "depth_underweight", "colour_underweight"]
    assert [n for n, _, _ in header_layout("dslam_unmerge_params")[0]] == ["with_colour", "reserved"]
    assert callable(pkg.CApi.unmerge_maps) and callable(pkg.CApi.remerge_maps)
    p = pkg.UnmergeParams()
    assert (p.with_colour, p.reserved) == (1, 0)
