"""Float64 reference of the composite mesh over several local maps (dslam_mesh_scene_multi), on analytic_maps.py,
ref64.py and ref64_multimap.py (Posed, _trilinear).

The law, map i of the list on its own voxel lattice, T~ = T with its translation in voxel units,
A_ij = T~_j T~_i^-1, B_i = T~_i^-1:
  own gate       a cube is skipped when one of its 8 corner voxels of map i is missing or holds sdf 32767;
  coverage gate  ... or when a map j < i holds a voxel with w_depth > 0 and sdf != 32767 at iround(A_ij (g + 1/2));
  corner values  per lattice point: the own voxel (sdf / 32767, its w_depth; colour, its w_color) and every other map's
                 trilinear read (value and trilinear weight) at A_ij (g + corner), combined in list order: only the own
                 map found -> its value, several ->
                 sum(w v) / sum(w), sum(w) == 0 -> the own value;
  triangles      case table and sdfInterp crossings in map-i voxel coordinates, then (B_i v) * voxel_size.
Everything is evaluated in float64; a cube is a `tie` when a predicate is within tie_tol of flipping: a blended corner
value next to 0 (case index, sdfInterp's 1e-5 thresholds), a transformed lattice point next to an integer coordinate
across which the read's `found` changes, or a cube centre next to a half where iround flips.
"""
import numpy as np

import ref64
import test_mc_tables as mct
from ref64_multimap import Posed, _trilinear  # noqa: F401  (Posed: what callers build the list from)

F = np.float32
TABLE = np.array(mct.load_table(), np.int64)            # [256, 16]
NTRI = (TABLE[:, 0:15:3] >= 0).sum(1)                   # triangles per case
CORNERS = mct.CORNERS.astype(np.int64)                  # [8, 3]
EDGES = np.array(mct.EDGES, np.int64)                   # [12, 2]
_L = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1)[..., ::-1].reshape(729, 3)  # x + 9y + 81z
_V = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)[..., ::-1].reshape(512, 3)  # x + 8y + 64z
_CUBE_LATTICE = ((_V[:, None, :] + CORNERS[None]) * np.array([1, 9, 81])).sum(-1)  # [512, 8] lattice index of corner k


def voxel_transform(pm):
    """T~: the float32 world -> map transform with its translation in voxel units, as float64 4x4."""
    T = np.asarray(pm.T, F).astype(np.float64)
    T[:3, 3] /= float(F(pm.m.vs))
    T[3] = (0.0, 0.0, 0.0, 1.0)
    return T


def live_blocks(m):
    """Block positions of the entries with a resident block, in table order (the mesh's block order)."""
    idx = np.nonzero(m.hash["ptr"] >= 0)[0]
    return m.hash["pos"][idx].astype(np.int64)


def _same_pose(a, b):
    return np.array_equal(np.asarray(a.T, F).view(np.uint32), np.asarray(b.T, F).view(np.uint32))


def _any_found(pm, q):
    q0 = np.floor(q).astype(np.int64)
    f = np.zeros(len(q), bool)
    for d in np.ndindex(2, 2, 2):
        f |= pm.m.lookup(q0 + np.array(d))[2]
    return f


def _found_flip(pm, q, tol):
    """A coordinate of q lies within tol of an integer and `found` differs on the two sides."""
    tie = np.zeros(len(q), bool)
    for a in range(3):
        r = np.round(q[:, a])
        near = np.nonzero(np.abs(q[:, a] - r) < tol)[0]
        if len(near):
            lo, hi = q[near].copy(), q[near].copy()
            lo[:, a], hi[:, a] = r[near] - 0.25, r[near] + 0.25
            tie[near] |= _any_found(pm, lo) != _any_found(pm, hi)
    return tie


def _crossing(v1, v2, a, b):
    """sdfInterp between values v1, v2 [n] of quantities a, b [n, c]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (0.0 - v1) / (v2 - v1)
    out = a + t[:, None] * (b - a)
    take1 = (np.abs(v1) < 1e-5) | ((np.abs(v2) >= 1e-5) & (np.abs(v1 - v2) < 1e-5))
    take2 = (np.abs(v1) >= 1e-5) & (np.abs(v2) < 1e-5)
    return np.where(take1[:, None], a, np.where(take2[:, None], b, out))


def mesh_maps(maps, colour=False, tie_tol=1e-4):
    """One dict per map of the list, every cube of every live block in mesh order (blocks in table order, voxels z/y/x):
    g [n, 3] corner-0 voxel, kept [n] (the cube leaves triangles), produce [n] (its own gate passes and its case has
    triangles), tie [n], ntri [n] (0 where not kept), tris [n, 5, 3, 3] world metres (nan past ntri), cols likewise
    in [0, 1] or None."""
    vs = float(F(maps[0].m.vs))
    Tv = [voxel_transform(pm) for pm in maps]
    out = []
    for i, pm in enumerate(maps):
        m = pm.m
        B = np.linalg.inv(Tv[i])
        blocks = live_blocks(m)
        nb = len(blocks)
        P = (blocks[:, None, :] * 8 + _L[None]).reshape(-1, 3)                      # lattice points, [nb * 729, 3]
        s16, clr, found = m.lookup(P)
        own_wd, own_wc = pm.weights(P, found)
        own = s16 / 32767.0
        own_c = clr.astype(np.float64)
        bad = ~found | (s16 == 32767)
        num, den, nf = np.zeros(len(P)), np.zeros(len(P)), np.zeros(len(P), np.int64)
        cnum, cden = np.zeros((len(P), 3)), np.zeros(len(P))
        tie_p = np.zeros(len(P), bool)
        Pf = P.astype(np.float64)
        for j, pj in enumerate(maps):
            if j == i:
                v, w, f = own, own_wd, found
                c, wc = own_c, own_wc
            else:
                A = np.eye(4) if _same_pose(pm, pj) else Tv[j] @ B
                q = Pf @ A[:3, :3].T + A[:3, 3]
                v, w, f = _trilinear(pj, q)
                if colour:
                    c, wc, _ = _trilinear(pj, q, colour=True)
                tie_p |= _found_flip(pj, q, tie_tol)
            num += np.where(f, w * v, 0.0)
            den += np.where(f, w, 0.0)
            nf += f
            if colour:
                cnum += np.where(f[:, None], wc[:, None] * c, 0.0)
                cden += np.where(f, wc, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = np.where((nf > 1) & (den > 0), num / den, own)
            col = np.where(((nf > 1) & (cden > 0))[:, None], cnum / cden[:, None], own_c) if colour else None
        tie_p |= found & (nf > 1) & (np.abs(val) < tie_tol + 1e-5)
        # cubes
        idx = (np.arange(nb)[:, None, None] * 729 + _CUBE_LATTICE[None]).reshape(-1, 8)   # [nb * 512, 8]
        g = (blocks[:, None, :] * 8 + _V[None]).reshape(-1, 3)
        cv = val[idx]
        case = ((cv < 0) << np.arange(8)).sum(1)
        produce = ~bad[idx].any(1) & (NTRI[case] > 0)
        tie = tie_p[idx].any(1)
        covered = np.zeros(len(g), bool)
        centre = g + 0.5
        for j in range(i):
            pj = maps[j]
            same = _same_pose(pm, pj)
            A = np.eye(4) if same else Tv[j] @ B
            c = centre @ A[:3, :3].T + A[:3, 3]
            near = ref64._iround(c)
            s, _, f = pj.m.lookup(near)
            covered |= f & (pj.weights(near, f)[0] > 0) & (s != 32767)
            if not same:
                frac = np.abs(c) - np.floor(np.abs(c))
                tie |= np.any(np.abs(frac - 0.5) < tie_tol, axis=1)
        kept = produce & ~covered
        ntri = np.where(kept, NTRI[case], 0)
        tris = np.full((len(g), 5, 3, 3), np.nan)
        cols = np.full((len(g), 5, 3, 3), np.nan) if colour else None
        for t in range(5):
            sel = np.nonzero(ntri > t)[0]
            if len(sel) == 0:
                continue
            for k in range(3):
                e = TABLE[case[sel], 3 * t + k]
                a, b = EDGES[e, 0], EDGES[e, 1]
                v1, v2 = cv[sel, a], cv[sel, b]
                pa, pb = (g[sel] + CORNERS[a]).astype(np.float64), (g[sel] + CORNERS[b]).astype(np.float64)
                p = _crossing(v1, v2, pa, pb)
                if not pm.identity:
                    p = p @ B[:3, :3].T + B[:3, 3]
                tris[sel, t, k] = p * vs
                if colour:
                    cols[sel, t, k] = _crossing(v1, v2, col[idx[sel, a]], col[idx[sel, b]]) / 255.0
        out.append(dict(g=g, kept=kept, produce=produce, tie=tie, ntri=ntri, tris=tris, cols=cols, T=Tv[i]))
    return out


def tie_share(ref):
    """Tie cubes as a share of the triangle-producing cubes, over all maps of a mesh_maps result."""
    prod = sum(int(r["produce"].sum()) for r in ref)
    ties = sum(int((r["tie"] & r["produce"]).sum()) for r in ref)
    return ties / max(prod, 1)


def triangles(ref):
    """The reference's triangle list [n, 3, 3] in mesh order."""
    parts = []
    for r in ref:
        for c in np.nonzero(r["ntri"] > 0)[0]:
            parts.append(r["tris"][c, :r["ntri"][c]])
    return np.concatenate(parts) if parts else np.zeros((0, 3, 3))


def cubes_of_triangles(r, tri, vs, what="map"):
    """Of triangles [n, 3, 3] (world metres, in mesh order) of the map whose mesh_maps entry is r: the index into r's
    cubes of the cube each came from.  A triangle belongs to the cube its centroid falls into in the map's frame.

    The one exception is a collapsed triangle on a cube face (two vertices within 1e-5 voxel of each other, centroid within
    1e-3 voxel of a face): a lattice value within sdfInterp's 1e-5 of 0 pulls the crossings of its edges onto the lattice
    point, and the centroid of what is left cannot tell the cubes that share the face apart.  Such a triangle goes to a cube
    that touches the face and holds all three vertices: a tie cube if there is one (a cube with such a lattice value is a
    tie), and among several the first in mesh order that is not before the preceding triangle's cube -- the mesh lists the
    cubes in r's order and a cube's triangles together."""
    vs = float(F(vs))
    q = (np.asarray(tri, np.float64) / vs) @ r["T"][:3, :3].T + r["T"][:3, 3]     # [n, 3, 3] in the map's voxel frame
    cen = q.mean(axis=1)
    gq = np.floor(cen).astype(np.int64)
    lo = np.minimum(r["g"].min(0), gq.min(0) - 1 if len(gq) else r["g"].min(0))
    span = np.maximum(r["g"].max(0), gq.max(0) + 1 if len(gq) else r["g"].max(0)) - lo + 1
    key = lambda a: ((a[..., 0] - lo[0]) * span[1] + (a[..., 1] - lo[1])) * span[2] + (a[..., 2] - lo[2])
    rk = key(r["g"])
    order = np.argsort(rk)

    def find(g):
        """index of the cubes at g, -1 where the map has none"""
        at = np.minimum(np.searchsorted(rk[order], key(g)), len(rk) - 1)
        return np.where(rk[order[at]] == key(g), order[at], -1)

    cube = find(gq)
    frac = cen - gq
    on_face = np.any((frac < 1e-3) | (frac > 1.0 - 1e-3), axis=1)
    collapsed = np.zeros(len(q), bool)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        collapsed |= np.abs(q[:, a] - q[:, b]).max(axis=1) < 1e-5
    for t in np.nonzero(on_face & collapsed)[0]:
        signs = np.array(list(np.ndindex(2, 2, 2))) * 2 - 1
        options = np.unique(np.floor(cen[t][None] + 2e-3 * signs).astype(np.int64), axis=0)
        holds = np.all((q[t][None] >= options[:, None, :] - 1e-3) & (q[t][None] <= options[:, None, :] + 1 + 1e-3), axis=(1, 2))
        idx = find(options)
        idx = np.sort(idx[holds & (idx >= 0)])
        assert len(idx), f"{what}: a triangle on a cube face belongs to no cube of the map's live blocks"
        if r["tie"][idx].any():   # (a collapsed triangle comes from a cube with such a lattice value: a tie)
            idx = idx[r["tie"][idx]]
        later = idx[idx >= (cube[t - 1] if t else -1)]
        cube[t] = later[0] if len(later) else idx[0]
    assert (cube >= 0).all(), f"{what}: triangles outside every cube of the map's live blocks"
    return cube


def compare(ref, pos, col, counts, vs, vert_tol=1e-3, col_tol=1.0 / 255.0):
    """A triangle list (pos / col [n, 3, 3], counts per map) against a mesh_maps result, cube by cube off the ties: each
    triangle goes to the cube it came from (cubes_of_triangles); kept / skipped, triangle counts, vertices (within vert_tol
    voxel) and colours must agree.  Returns dict(cubes compared, max vertex error in voxels, max colour error)."""
    assert int(np.sum(counts)) == len(pos)
    start, n_cmp, worst_v, worst_c = 0, 0, 0.0, 0.0
    vs = float(F(vs))
    for i, r in enumerate(ref):
        tri = pos[start:start + counts[i]].astype(np.float64)
        tcol = None if col is None else col[start:start + counts[i]].astype(np.float64)
        start += counts[i]
        cube = cubes_of_triangles(r, tri, vs, f"map {i}")
        rk = r["g"]
        got = np.bincount(cube, minlength=len(rk))
        chk = ~r["tie"]
        wrong = chk & (got != r["ntri"])
        assert not wrong.any(), (f"map {i}: {wrong.sum()} cubes off a tie differ in kept / triangle count, "
                                 f"first at voxel {r['g'][np.argmax(wrong)]}: {got[np.argmax(wrong)]} vs {r['ntri'][np.argmax(wrong)]}")
        first = np.full(len(rk), -1, np.int64)   # a cube's triangles are consecutive: index of its first one
        seen = np.nonzero(np.r_[True, cube[1:] != cube[:-1]])[0] if len(cube) else np.zeros(0, np.int64)
        first[cube[seen]] = seen
        assert len(seen) == (got > 0).sum(), f"map {i}: the triangles of a cube are not consecutive"
        for c in np.nonzero(chk & (r["ntri"] > 0))[0]:
            n = r["ntri"][c]
            dv = np.abs(tri[first[c]:first[c] + n] - r["tris"][c, :n]).max() / vs
            worst_v = max(worst_v, dv)
            if tcol is not None:
                worst_c = max(worst_c, np.abs(tcol[first[c]:first[c] + n] - r["cols"][c, :n]).max())
        n_cmp += int((chk & r["produce"]).sum())
    assert worst_v <= vert_tol, f"vertices up to {worst_v:.3g} voxel from the reference"
    assert worst_c <= col_tol, f"colours up to {worst_c * 255:.3g} / 255 from the reference"
    return dict(cubes=n_cmp, max_vertex=worst_v, max_colour=worst_c)
