"""The fern index's plumbing without a GPU: the header declares the calls, the library exports them, the wrapper binds them,
the ctypes structures have the header's fields at the header's offsets, and header, wrapper and reference state the same
limits and defaults."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "uint32_t": 4, "float": 4}
CALLS = ("dslam_fern_index_create", "dslam_fern_index_destroy", "dslam_fern_index_count", "dslam_fern_index_table",
         "dslam_fern_index_reset", "dslam_fern_encode", "dslam_fern_query", "dslam_fern_process", "dslam_fern_add_from_store",
         "dslam_fern_query_stored")
BOUND = ("create_fern_index", "fern_index_count", "fern_index_table", "fern_index_reset", "fern_encode", "fern_query",
         "fern_process", "fern_add_from_store", "fern_query_stored")


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


def test_the_calls_are_declared_exported_and_bound(pkg):
    txt = header_text()
    for call in CALLS:
        assert re.search(r"\bint\s+" + call + r"\s*\(", txt), call
    assert set(CALLS) <= pkg.exported_symbols()
    for name in BOUND:
        assert callable(getattr(pkg.CApi, name)), name


def test_the_limits_are_64_everywhere(pkg):
    import ref_fern as rf
    txt = header_text()
    for macro in ("DSLAM_FERN_MAX_MATCHES", "DSLAM_FERN_MAX_QUERIES", "DSLAM_FERN_CODE_DWORDS"):
        assert re.search(r"#define\s+" + macro + r"\s+64\b", txt), macro
    assert (pkg.FERN_MAX_MATCHES, pkg.FERN_MAX_QUERIES, pkg.FERN_CODE_DWORDS) == (64, 64, 64)
    assert (rf.MAX_MATCHES, rf.MAX_QUERIES, rf.CODE_DWORDS) == (64, 64, 64)


def test_ctypes_structures_match_the_header(pkg):
    for name, struct in (("dslam_fern_params", pkg.FernParams), ("dslam_fern_match", pkg.FernMatch)):
        fields, size = header_layout(name)
        assert ctypes.sizeof(struct) == size, name
        assert [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_] == fields, name
    assert pkg.FernParams.seed.size == 4 and pkg.FernParams(seed=0xFFFFFFFF).seed == 0xFFFFFFFF   # unsigned
    assert pkg.FERN_MATCH_DTYPE.itemsize == ctypes.sizeof(pkg.FernMatch)
    assert [pkg.FERN_MATCH_DTYPE.fields[n][1] for n in ("id", "dissimilarity")] == [pkg.FernMatch.id.offset, pkg.FernMatch.dissimilarity.offset]


def test_the_defaults_are_as_stated(pkg):
    import ref_fern as rf
    p = pkg.FernParams()
    assert p.as_dict() == dict(num_ferns=0, cell=0, channels=0, depth_min_mm=0, depth_max_mm=0, seed=0)   # 0 selects the default
    assert rf.resolve(p.as_dict()) == dict(num_ferns=512, cell=8, channels=1, depth_min_mm=300, depth_max_mm=10000, seed=0)
    # the header's comments state the same defaults next to the fields
    raw = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    for field, default in (("num_ferns", 512), ("cell", 8), ("channels", 1), ("depth_min_mm", 300), ("depth_max_mm", 10000)):
        assert re.search(r"int32_t\s+" + field + r";\s*/\*\s*0 -> " + str(default) + r"\b", raw), field
