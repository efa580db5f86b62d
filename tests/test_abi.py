"""No-GPU checks of the drop-in boundary: the library is built, loads, and exports exactly what include/*.h declares."""
import ctypes
import os
import re

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dslam_[a-z0-9_]+)\s*\(", txt)))


def test_library_is_built_and_exports_every_declared_symbol(pkg):
    assert os.path.exists(pkg.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    exported = pkg.exported_symbols()
    declared = _declared()
    assert len(declared) > 40
    missing = [d for d in declared if d not in exported]
    assert not missing, f"declared in include/dslam_fusion.h but not exported: {missing}"


def test_library_loads_and_reports_version(pkg):
    # bind the library to the HIP runtime open_engine() uses (torch's), as open_engine() does: a library first bound to
    # another libamdhip64 stays bound to it for the rest of the process, and the GPU tests after this one find no device
    pkg._share_torch_hip_runtime()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    lib.dslam_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.dslam_version()


def test_code_object_targets_gfx950(pkg):
    data = open(pkg.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"k_integrate" in data


def test_struct_layouts(pkg):
    assert pkg.HASH_ENTRY_DTYPE.itemsize == 16 and pkg.VOXEL_DTYPE.itemsize == 8
    assert pkg.HASH_ENTRY_DTYPE.fields["offset"][1] == 8 and pkg.HASH_ENTRY_DTYPE.fields["ptr"][1] == 12
    assert pkg.VOXEL_DTYPE.fields["w_depth"][1] == 2 and pkg.VOXEL_DTYPE.fields["w_color"][1] == 6
    assert ctypes.sizeof(pkg.SceneParams) == 44 and ctypes.sizeof(pkg.Stats) == 56


def test_engine_creation_fails_loudly_without_gpu(pkg):
    """The product has no CPU path: without a HIP device engine creation must raise, not fall back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.DslamError):
        pkg.open_engine(0)


def test_no_kernel_uses_scratch(pkg, tmp_path):
    """Every gfx950 kernel must keep its working set in registers: private (scratch) memory costs the occupancy the
    latency-bound kernels live on, and a scratch-using build once hung a rocprofv3 counter pass.  Compiles each
    translation unit to assembly (device side only) and reads the code-object metadata."""
    import concurrent.futures
    import glob
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    srcs = sorted(glob.glob(os.path.join(pkg.CSRC_DIR, "*.hip")))
    assert len(srcs) >= 6

    def scan(src):
        out = tmp_path / (os.path.basename(src) + ".s")
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-S",
                        "--cuda-device-only", "-o", str(out), src], check=True, capture_output=True)
        text = out.read_text()
        return [(m.group(1), int(m.group(2))) for m in re.finditer(r"\.set (\S+)\.private_seg_size, (\d+)", text)]

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        results = [kv for res in pool.map(scan, srcs) for kv in res]
    assert len(results) >= 40, "kernel metadata not found"
    offenders = [(k, v) for k, v in results if v != 0]
    assert not offenders, f"kernels with scratch: {offenders}"
