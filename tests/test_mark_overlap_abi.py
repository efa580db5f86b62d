"""dslam_debug_mark_overlap_counts without a GPU: the header declares it, the library exports it, the wrapper binds it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "dslam_debug_mark_overlap_counts"


def test_the_call_is_declared_exported_and_bound(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dslam_fusion.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + CALL + r"\s*\(\s*dslam_engine\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*\)", txt)
    assert CALL in pkg.exported_symbols()
    assert callable(getattr(pkg.CApi, "debug_mark_overlap_counts", None))
