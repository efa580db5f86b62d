"""The two host functions of the many-starts tracker without a GPU: dslam_camera_pose_lattice against
a float64 numpy statement of its law and dslam_select_start_poses against numpy on random scores.  Both are pure host
functions, so the library is loaded as test_view_survey_ref.py loads it and no engine is opened."""
import ctypes

import numpy as np
import pytest

F32P, I32P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._share_torch_hip_runtime()
    return ctypes.CDLL(pkg.LIB_PATH)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose(rotvec, t):
    """world -> camera, float32, from a rotation vector and a translation."""
    M = np.eye(4)
    th = np.linalg.norm(rotvec)
    M[:3, :3] = rodrigues(rotvec, th) if th > 0 else np.eye(3)
    M[:3, 3] = t
    return M.astype(np.float32)


def lattice_reference(M, lat):
    """The law in float64: [(ir, iz, iy, ix)], [poses] in the order the header states."""
    M = np.asarray(M, np.float32).astype(np.float64)
    R, c = M[:3, :3].T, -M[:3, :3].T @ M[:3, 3]
    index, poses = [], []
    for ir in range(-lat.nr, lat.nr + 1):
        Rn = (rodrigues(list(lat.axis), ir * float(lat.step_r)) if lat.nr > 0 else np.eye(3)) @ R
        for iz in range(-lat.nt[2], lat.nt[2] + 1):
            for iy in range(-lat.nt[1], lat.nt[1] + 1):
                for ix in range(-lat.nt[0], lat.nt[0] + 1):
                    cn = c + float(lat.step_t) * np.array([ix, iy, iz], np.float64)
                    P = np.eye(4)
                    P[:3, :3], P[:3, 3] = Rn.T, -Rn.T @ cn
                    index.append((ir, iz, iy, ix))
                    poses.append(P)
    return index, np.array(poses)


def call_lattice(pkg, lib, M, lat, capacity=None, fill=-7.0):
    cap = lat.count if capacity is None else capacity
    out = np.full(max(cap, 1) * 16, fill, np.float32)
    count = ctypes.c_int32(-1)
    rc = lib.dslam_camera_pose_lattice(pkg.mat_to_abi(M).ctypes.data_as(F32P), ctypes.byref(lat), out.ctypes.data_as(F32P),
                                       ctypes.c_int(cap), ctypes.byref(count))
    return rc, out, count.value


M0 = pose(np.array([0.21, -0.4, 0.13]), (0.3, -0.2, 1.1))


@pytest.mark.parametrize("lat_args", [
    dict(nt=(1, 2, 0), step_t=0.05, nr=2, step_r=0.03, axis=(0.2, 1.0, -0.1)),
    dict(nt=(0, 0, 0), step_t=0.0, nr=0, step_r=0.0, axis=(0.0, 0.0, 0.0)),     # the centre alone; no axis needed
    dict(nt=(2, 0, 1), step_t=0.013, nr=0, step_r=0.5, axis=(0.0, 0.0, 0.0)),
    dict(nt=(0, 0, 0), step_t=0.1, nr=3, step_r=0.4, axis=(0.0, 0.0, 2.0)),
])
def test_lattice_against_the_float64_statement(pkg, lib, lat_args):
    lat = pkg.PoseLattice(**lat_args)
    rc, out, count = call_lattice(pkg, lib, M0, lat)
    index, want = lattice_reference(M0, lat)
    assert rc == 0 and count == lat.count == len(index)
    got = out.reshape(count, 4, 4).transpose(0, 2, 1)
    # the order: ir slowest, ix fastest; every node is the float64 law rounded to float32 (the two float64 evaluations may
    # add in another order: a few float32 ulps of entries of magnitude about 1 are allowed, a lattice step is 1e-2)
    assert np.abs(got.astype(np.float64) - want).max() < 1e-6
    centre = index.index((0, 0, 0, 0))
    assert got[centre].tobytes() == M0.tobytes()
    for P in got.astype(np.float64):
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(P[:3, :3]) - 1.0) < 1e-6
        assert P[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    # what the nodes mean: camera centres on the translation lattice, orientations turned about the axis
    for (ir, iz, iy, ix), P in zip(index, got.astype(np.float64)):
        c0 = -M0[:3, :3].astype(np.float64).T @ M0[:3, 3].astype(np.float64)
        c = -P[:3, :3].T @ P[:3, 3]
        assert np.abs(c - (c0 + float(lat.step_t) * np.array([ix, iy, iz]))).max() < 1e-6


def test_a_centre_pose_that_does_not_survive_its_own_inverse_is_still_returned_byte_for_byte(pkg, lib):
    """A pose within the 1e-4 orthonormality allowance: its inverse's inverse rounds elsewhere, the centre node does not."""
    M = M0.copy()
    M[:3, :3] *= np.float32(1.00003)
    lat = pkg.PoseLattice(nt=(1, 0, 0), step_t=0.02)
    rc, out, count = call_lattice(pkg, lib, M, lat)
    assert rc == 0 and count == 3
    assert out.reshape(3, 4, 4).transpose(0, 2, 1)[1].tobytes() == M.tobytes()


def test_lattice_rejections_leave_the_poses_untouched(pkg, lib):
    good = dict(nt=(1, 1, 1), step_t=0.05, nr=1, step_r=0.03, axis=(0.0, 1.0, 0.0))

    def refused(M=M0, capacity=None, count=None, **over):
        lat = pkg.PoseLattice(**{**good, **over})
        rc, out, got = call_lattice(pkg, lib, M, lat, capacity=81 if capacity is None else capacity)
        assert rc == -1 and (out == -7.0).all()
        assert got == (lat.count if count is None else count)   # always filled

    refused(capacity=80)                                  # 81 nodes
    refused(axis=(0.0, 0.0, 0.0))
    refused(axis=(0.0, np.nan, 1.0))
    refused(axis=(np.inf, 0.0, 1.0))
    refused(nt=(1, -1, 1), count=0)
    refused(nr=-1, count=0)
    refused(step_t=-0.01)
    refused(step_r=-0.01)
    refused(step_t=np.nan)
    nan, skew = M0.copy(), M0.copy()
    nan[2, 3] = np.nan
    skew[:3, :3] *= 1.01
    refused(M=nan)
    refused(M=skew)
    # NULL arguments
    lat = pkg.PoseLattice(**good)
    out, count = np.full(81 * 16, -7.0, np.float32), ctypes.c_int32(-1)
    m = pkg.mat_to_abi(M0)
    for null in range(4):
        args = [m.ctypes.data_as(F32P), ctypes.byref(lat), out.ctypes.data_as(F32P), ctypes.c_int(81), ctypes.byref(count)]
        args[null if null < 3 else 4] = None
        assert lib.dslam_camera_pose_lattice(*args) == -1 and (out == -7.0).all()
    # a zero axis is fine without rotation nodes, and the accepted call fills everything
    rc, out, count = call_lattice(pkg, lib, M0, pkg.PoseLattice(**{**good, "nr": 0, "axis": (0.0, 0.0, 0.0)}))
    assert rc == 0 and count == 27 and not (out == -7.0).any()


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
def select_reference(valid, cost, min_valid, max_keep):
    ok = [k for k in range(len(valid)) if valid[k] >= min_valid and not np.isnan(cost[k])]
    ok.sort(key=lambda k: (cost[k], k))
    return ok[:max_keep]


def call_select(pkg, lib, valid, cost, min_valid, max_keep):
    n = len(valid)
    scores = (pkg.PoseScore * n)(*[pkg.PoseScore(1000 + k, int(valid[k]), float(cost[k]), 0) for k in range(n)])
    kept = np.full(max(max_keep, 1) + 1, -7, np.int32)
    count = ctypes.c_int32(-1)
    rc = lib.dslam_select_start_poses(scores, ctypes.c_int(n), ctypes.c_int(min_valid), ctypes.c_int(max_keep),
                                      kept.ctypes.data_as(I32P), ctypes.byref(count))
    assert rc == 0 and (kept[count.value:] == -7).all()
    return kept[:count.value].tolist()


def test_selection_against_numpy_on_random_scores(pkg, lib):
    rng = np.random.default_rng(24)
    seen = dict(ties=0, nan=0, at_min=0, below_min=0, short=0, none=0)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        min_valid = int(rng.integers(0, 50))
        valid = rng.integers(0, 100, n)
        # costs from a few values (ties), NaN among them; valid at min_valid and one below it
        cost = rng.choice(np.array([0.1, 0.1000001, 0.25, 0.5, 0.5625, np.nan, np.inf], np.float32), n)
        valid[rng.integers(0, n)] = min_valid
        valid[rng.integers(0, n)] = min_valid - 1
        for max_keep in (0, 1, int(rng.integers(1, n + 1)), n + 5):
            want = select_reference(valid, cost, min_valid, max_keep)
            assert call_select(pkg, lib, valid, cost, min_valid, max_keep) == want
            qualifies = sum(1 for k in range(n) if valid[k] >= min_valid and not np.isnan(cost[k]))
            seen["short"] += max_keep > qualifies
            seen["none"] += max_keep == 0 and not want
        kept = select_reference(valid, cost, min_valid, n)
        seen["ties"] += len({float(cost[k]) for k in kept}) < len(kept)
        seen["nan"] += bool(np.isnan(cost[valid >= min_valid]).any())
        seen["at_min"] += any(valid[k] == min_valid for k in kept)
        seen["below_min"] += bool((valid == min_valid - 1).any())
    print(seen)
    assert all(v >= 20 for v in seen.values()), seen


def test_selection_edges(pkg, lib):
    valid, cost = [99, 100, 100, 100, 100], np.array([0.0, 0.3, np.nan, 0.2, 0.2], np.float32)
    assert call_select(pkg, lib, valid, cost, 100, 10) == [3, 4, 1]     # 99 is below; NaN never; ties by index
    assert call_select(pkg, lib, valid, cost, 100, 2) == [3, 4]
    assert call_select(pkg, lib, valid, cost, 100, 0) == []
    assert call_select(pkg, lib, valid, cost, 99, 1) == [0]
    assert call_select(pkg, lib, valid, cost, 101, 3) == []
    scores = (pkg.PoseScore * 1)()
    kept, count = np.zeros(1, np.int32), ctypes.c_int32(-1)
    i32 = kept.ctypes.data_as(I32P)
    assert lib.dslam_select_start_poses(None, 1, 0, 1, i32, ctypes.byref(count)) == -1
    assert lib.dslam_select_start_poses(scores, 1, 0, 1, None, ctypes.byref(count)) == -1
    assert lib.dslam_select_start_poses(scores, 1, 0, 1, i32, None) == -1
    assert lib.dslam_select_start_poses(scores, 0, 0, 1, i32, ctypes.byref(count)) == -1
    assert lib.dslam_select_start_poses(scores, 1, -1, 1, i32, ctypes.byref(count)) == -1
    assert lib.dslam_select_start_poses(scores, 1, 0, -1, i32, ctypes.byref(count)) == -1
    assert count.value == -1
