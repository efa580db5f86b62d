"""The view survey and the map selection stated from the header's text: the frustum planes in numpy
float64 in the stated order, the device law in numpy float32 element operations (numpy contracts nothing), the selection in
plain Python.  Shares no text with the engine.

Planes.  A view is (M world -> camera 4 x 4 in metres, (fx, fy, cx, cy), width, height, near_m, far_m), every number
taken as float32 and converted to float64.  R = M[:3, :3], t~ = M[:3, 3] / vs.  Camera-frame normals: left (fx, 0, cx + 1),
right (-fx, 0, width - cx), top (0, fy, cy + 1), bottom (0, -fy, height - cy), each divided by sqrt(a a + b b) of its two
non-zero entries; near (0, 0, 1) with d_c = -(near_m / vs); far (0, 0, -1) with d_c = far_m / vs.  World frame:
n_w[j] = (R[0][j] n_c[0] + R[1][j] n_c[1]) + R[2][j] n_c[2], d_w = ((n_c[0] t~[0] + n_c[1] t~[1]) + n_c[2] t~[2]) + d_c.  far_m == 0:
row 5 is (0, 0, 0, +inf).  Row 6 = (R[2][0], R[2][1], R[2][2], t~[2]).  Rounded to float32 once.

Survey.  Y~_i = (R^T, -(R^T t~)) of T~_i in float64, the translation entries -((r0 t0 + r1 t1) + r2 t2), rounded to float32;
a resident entry (ptr >= 0) at block position B has the centre c = 8 B + 4 and the world point p = Y~_i c, rows
((a x + b y) + c z) + d in float32 (a T_i that is exactly the identity: p = c); s_k = ((n_x p_x + n_y p_y) + n_z p_z) + d; the
block reaches when s_k >= -rho for k = 0..5, rho = float32(6.92820323027550917 + margin); z from row 6 in the same order,
zi = int(clip(floor(z), -2147483648, 2147483520)).
"""
import numpy as np

MAX_RENDER_MAPS = 64
MAX_SURVEY_MAPS, MAX_SURVEY_VIEWS = 256, 16
DEFAULT_MARGIN = 2.0
RADIUS = 6.92820323027550917          # 4 sqrt(3)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class View:
    def __init__(self, M, intr, width, height, near_m, far_m):
        self.M = np.asarray(M, np.float32).reshape(4, 4)
        self.intr = np.asarray(intr, np.float32).reshape(4)
        self.width, self.height = int(width), int(height)
        self.near_m, self.far_m = np.float32(near_m), np.float32(far_m)


def rho_of(margin=0.0):
    margin = np.float32(margin)
    return np.float32(RADIUS + float(margin if margin != 0 else np.float32(DEFAULT_MARGIN)))


def frustum_planes(view, vs):
    """[7, 4] float32."""
    vs = float(np.float32(vs))
    M = view.M.astype(np.float64)
    R = [[float(M[r, c]) for c in range(3)] for r in range(3)]
    tv = [float(M[r, 3]) / vs for r in range(3)]
    fx, fy, cx, cy = (float(v) for v in view.intr)

    def side(a, b):
        length = np.sqrt(a * a + b * b)
        return a / length, b / length

    nc = [[0.0, 0.0, 0.0] for _ in range(6)]
    dc = [0.0] * 6
    nc[0][0], nc[0][2] = side(fx, cx + 1.0)
    nc[1][0], nc[1][2] = side(-fx, float(view.width) - cx)
    nc[2][1], nc[2][2] = side(fy, cy + 1.0)
    nc[3][1], nc[3][2] = side(-fy, float(view.height) - cy)
    nc[4][2], dc[4] = 1.0, -(float(view.near_m) / vs)
    nc[5][2], dc[5] = -1.0, float(view.far_m) / vs
    out = np.zeros((7, 4), np.float64)
    for k in range(6):
        for j in range(3):
            out[k, j] = (R[0][j] * nc[k][0] + R[1][j] * nc[k][1]) + R[2][j] * nc[k][2]
        out[k, 3] = ((nc[k][0] * tv[0] + nc[k][1] * tv[1]) + nc[k][2] * tv[2]) + dc[k]
    if view.far_m == 0:
        out[5] = (0.0, 0.0, 0.0, np.inf)
    out[6] = (R[2][0], R[2][1], R[2][2], tv[2])
    return out.astype(np.float32)


def inverse_pose32(T, vs):
    """(Y~ [3, 4] float32, whether T is exactly the identity) of T: world -> map, 4 x 4 float32 in metres."""
    T = np.asarray(T, np.float32)
    vs = float(np.float32(vs))
    R = T[:3, :3].astype(np.float64)
    t = [float(T[r, 3]) / vs for r in range(3)]
    Y = np.zeros((3, 4), np.float64)
    for r in range(3):
        for c in range(3):
            Y[r, c] = R[c, r]
        Y[r, 3] = -((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2])
    return Y.astype(np.float32), bool(np.array_equal(T, np.eye(4, dtype=np.float32)))


def rows32(A, x, y, z):
    """((a x + b y) + c z) + d per row of A [rows, 4] float32 on float32 arrays; [n, rows] float32."""
    A = np.asarray(A, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(len(A))], -1)
    assert out.dtype == np.float32
    return out


def world_points(B, T, vs):
    """The world points p [n, 3] float32 of the centres of the blocks B [n, 3] of a map under T."""
    c = (np.asarray(B, np.int64) * 8 + 4).astype(np.float32)     # exact
    Y, identity = inverse_pose32(T, vs)
    return c if identity else rows32(Y, c[:, 0], c[:, 1], c[:, 2])


def plane_values(planes, p):
    """(s [n, 6] float32, z [n] float32) of world points p [n, 3] float32."""
    v = rows32(planes, p[:, 0], p[:, 1], p[:, 2])
    return v[:, :6], v[:, 6]


def reaching(planes, p, rho):
    s, z = plane_values(planes, p)
    with np.errstate(invalid="ignore"):
        reach = np.all(s >= -np.float32(rho), axis=1)
        zi = np.clip(np.floor(z.astype(np.float64)), -2147483648.0, 2147483520.0)
    zi = np.where(np.isnan(zi), 0.0, zi).astype(np.int64)
    return reach, zi


def resident_blocks(table):
    table = np.asarray(table)
    return table["pos"][table["ptr"] >= 0].astype(np.int64)


def survey(tables, T, vs, views, margin=0.0):
    """(live [N], reach [V, N], nearest [V, N], farthest [V, N]) int64 of hash tables `tables` (HASH_ENTRY_DTYPE arrays)."""
    n, nv = len(tables), len(views)
    rho = rho_of(margin)
    live = np.zeros(n, np.int64)
    reach = np.zeros((nv, n), np.int64)
    nearest = np.full((nv, n), INT32_MAX, np.int64)
    farthest = np.full((nv, n), INT32_MIN, np.int64)
    planes = [frustum_planes(v, vs) for v in views]
    for i in range(n):
        B = resident_blocks(tables[i])
        live[i] = len(B)
        if not len(B):
            continue
        p = world_points(B, T[i], vs)
        for v in range(nv):
            ok, zi = reaching(planes[v], p, rho)
            reach[v, i] = int(ok.sum())
            if ok.any():
                nearest[v, i], farthest[v, i] = int(zi[ok].min()), int(zi[ok].max())
    return live, reach, nearest, farthest


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
def select(reach, nearest, min_blocks=0, max_maps=0, always_keep=-1):
    """dslam_select_view_maps: (the kept indices ascending, dict(reaching, selected))."""
    nv, n = len(reach), len(reach[0])
    min_blocks = min_blocks or 1
    max_maps = max_maps or MAX_RENDER_MAPS
    assert max_maps <= MAX_RENDER_MAPS and -1 <= always_keep < n
    cands = [i for i in range(n) if i == always_keep or max(int(reach[v][i]) for v in range(nv)) >= min_blocks]
    if len(cands) <= max_maps:
        kept = list(cands)
    else:
        kept = [always_keep] if always_keep >= 0 else []
        rest = sorted((i for i in cands if i != always_keep),
                      key=lambda i: (min(int(nearest[v][i]) for v in range(nv)), -sum(int(reach[v][i]) for v in range(nv)), i))
        kept += rest[:max_maps - len(kept)]
    return sorted(kept), dict(reaching=len(cands), selected=len(kept))
