"""The packed-map host calls' plumbing without a GPU: the header declares them, the library exports them, the wrapper binds
them, and the ctypes structure has the header's fields at the header's offsets."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"char": 1, "int16_t": 2, "int32_t": 4, "uint32_t": 4, "int64_t": 8}
CALLS = ("dslam_pack_layout", "dslam_pack_header_read")


def header_text():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_layout(name):
    """[(field, offset, size)] and the size of `typedef struct { ... } name;` by the C layout rules: every member at the
    next multiple of its element size."""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", header_text()).group(1)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            off = -(-off // SIZES[ctype]) * SIZES[ctype]
            size = SIZES[ctype] * int(m.group(2) or 1)
            fields.append((m.group(1), off, size))
            off += size
    return fields, off


def test_the_binding_exists(pkg):
    """Fails on a tree without the calls."""
    assert all(callable(getattr(pkg.CApi, name, None)) for name in ("pack_layout", "pack_header_read"))
    assert hasattr(pkg, "PackInfo")


def test_the_calls_are_declared_and_exported(pkg):
    txt = header_text()
    for call in CALLS:
        assert re.search(r"\bint\s+" + call + r"\s*\(", txt), call
    assert set(CALLS) <= pkg.exported_symbols()
    # what the library does not hold is not declared either
    assert "dslam_scene_pack" not in txt and not any("scene_pack" in name for name in pkg.exported_symbols())


def test_the_ctypes_structure_matches_the_header(pkg):
    fields, size = header_layout("dslam_pack_info")
    assert size == 64 == ctypes.sizeof(pkg.PackInfo)
    assert [(n, getattr(pkg.PackInfo, n).offset, getattr(pkg.PackInfo, n).size) for n, _ in pkg.PackInfo._fields_] == fields
    # ... and the reference's header format is the same 64 bytes
    import ref_pack
    raw = ref_pack.HEADER.pack(b"DSPK", 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0)
    info = pkg.PackInfo.from_buffer_copy(raw)
    assert (info.magic, info.version, info.num_buckets, info.num_excess, info.blocks, info.free_excess) == (b"DSPK", 1, 2, 3, 4, 5)
    assert (info.voxel_size_bits, info.mu_bits, info.blocks_offset, info.total_bytes) == (6, 7, 8, 9)
    assert list(info.bbox_min) == [10, 11, 12] and list(info.bbox_max) == [13, 14, 15] and info.reserved == 0
