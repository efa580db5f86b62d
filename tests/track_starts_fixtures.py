"""The relocalisation case the many-starts tracker's tests share (test_track_starts_ref.py fixes it on the float64 reference,
test_gpu_track_starts.py runs it on the GPU), a numpy statement of dslam_camera_pose_lattice, and the
mirror's rule for the winner.  Everything is computed once per process."""
import functools

import numpy as np

import ref64_track_sdf as rt
import track_sdf_fixtures as fx

# The true pose of three_maps moved by D_MU truncation bands (mu = 4 voxels) along Fixture.start's direction, no rotation.
# Measured with ref64_track_sdf.track (RUN_PARAMS): from 1 mu (4.0 voxels) the run ends at 0.0118 voxel; from 2 mu
# (8.0 voxels) it ends at 24.4 voxels, from 3 mu (12.0) at 23.4: 2 is the smallest multiple from which the single call
# ends no closer than half its start distance.
D_MU = 2
# The lattice around that start: 3 x 3 x 3 camera centres one mu (0.02 m) apart, no rotation nodes.  Measured on level 2
# with ref64_track_sdf.evaluate: node 20 = (ix, iy, iz) = (+1, -1, +1) is the cheapest with cost 0.04205 and all 432 pixels
# valid, 1.235 voxels from the truth; the runner-up (node 19) costs 0.1879, and 19 of the 27 nodes have min_valid pixels.
# ref64_track_sdf.track from node 20 ends 0.01185 voxel from the truth after 22 evaluations (stop reason 0).
LATTICE = dict(nt=(1, 1, 1), step_t=0.02, nr=0, step_r=0.0, axis=(0.0, 0.0, 0.0))
SCORE_LEVEL, KEEP = 2, 4
BEST_NODE, BEST_NODE_DISTANCE, REFERENCE_END = 20, 1.235, 0.01185


def fixture():
    return fx.three_maps()


def displaced(f, k_mu=D_MU):
    return f.start(0.0, k_mu * f.maps[0].mu / f.vs)


def lattice_poses(M, nt, step_t, nr=0, step_r=0.0, axis=(0.0, 0.0, 0.0)):
    """dslam_camera_pose_lattice in float64 numpy: [count, 4, 4] float32, ir slowest and ix fastest, the centre node M itself."""
    M = np.asarray(M, np.float32)
    Md = M.astype(np.float64)
    R, c = Md[:3, :3].T, -Md[:3, :3].T @ Md[:3, 3]
    a = np.asarray(axis, np.float64)
    out = []
    for ir in range(-nr, nr + 1):
        Rot = np.eye(3)
        if nr > 0:
            u = a / np.linalg.norm(a)
            K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
            Rot = np.eye(3) + np.sin(ir * float(step_r)) * K + (1.0 - np.cos(ir * float(step_r))) * (K @ K)
        Rn = Rot @ R
        for iz in range(-nt[2], nt[2] + 1):
            for iy in range(-nt[1], nt[1] + 1):
                for ix in range(-nt[0], nt[0] + 1):
                    if (ir, iz, iy, ix) == (0, 0, 0, 0):
                        out.append(M.copy())
                        continue
                    P = np.eye(4)
                    P[:3, :3] = Rn.T
                    P[:3, 3] = -Rn.T @ (c + float(step_t) * np.array([ix, iy, iz], np.float64))
                    out.append(P.astype(np.float32))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def reference_scores():
    """(the lattice's poses, ref64 evaluations of them on SCORE_LEVEL) for the displaced start."""
    f = fixture()
    nodes = lattice_poses(displaced(f), **LATTICE)
    depth, intr = rt.pyramid(f.depth0, f.intr, SCORE_LEVEL + 1)[SCORE_LEVEL]
    return nodes, [rt.evaluate(f.posed, depth, intr, rt.camera_to_world(M, f.vs)) for M in nodes]


def select(valid, cost, min_valid, max_keep):
    """dslam_select_start_poses."""
    ok = [k for k in range(len(valid)) if valid[k] >= min_valid and not np.isnan(cost[k])]
    return sorted(ok, key=lambda k: (cost[k], k))[:max_keep]


def winner(results, min_valid):
    """The mirror's rule: the lowest cost_last among the starts with valid_last >= min_valid and a stop reason other than 3,
    ties to the lower index; None if there is none.  results: objects with valid_last, stop_reason, cost_last."""
    ok = [k for k, r in enumerate(results) if r.valid_last >= min_valid and r.stop_reason != 3]
    return min(ok, key=lambda k: (results[k].cost_last, k)) if ok else None
