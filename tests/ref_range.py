"""The law of the render front end: which entries FindVisibleBlocks lists, what ProjectSingleBlock makes of each listed
block, which of them the render-tile budget lets through, and the (min, max) range image castRay marches between.

Written from SURVEY.md A.6 (block visibility; `refmap.block_visibility` is that law and is reused, not restated) and A.7
(FindVisibleBlocks, CreateExpectedDepths), in the style of refmap.py: numpy, vectorised over blocks, nothing taken from
either engine.  The rule of ref64.py applies: every predicate (a corner behind z = 1e-6, the cell a projected corner
falls into, a block in front of VERY_CLOSE, a corner inside the image) is evaluated in np.float32 in the spec's operation
order, the same expression in float64 beside it, and an element on which the two disagree is a *tie* and is counted.
Off the ties everything here is exact: entry indices, integer boxes, tile counts, and z values that are float32 results
of a fixed operation order, so the range image is predicted bit for bit.

The law, per listed block (ProjectSingleBlock):
  * the eight corners (pos + (c & 1, c >> 1 & 1, c >> 2 & 1)) * 8 * voxelSize go through M (row r = ((m_r0 x + m_r1 y) +
    m_r2 z) + m_r3); a corner with z < 1e-6 is skipped;
  * px = (fx x / z + cx) / 8, py likewise; the box starts at (W/8, H/8, -1, -1) (integer division) and takes
    min(floor), max(ceil) over the corners that were not skipped; zmin, zmax likewise from (FAR_AWAY, VERY_CLOSE);
  * the box is clamped to 0 and to W-1 / H-1 -- the full image size although the cells are 1/8 scale: upstream's rule;
  * invalid if the box is empty or zmax < VERY_CLOSE; zmin is raised to VERY_CLOSE; req = ceil(w/16) * ceil(h/16).
The budget (MAX_RENDERING_BLOCKS), in list order: an entry with req != 0 is dropped when accepted + req >= budget, and a
dropped entry does not count; the rule applies only if the list's total of req is >= budget.
The range image: (FAR_AWAY, VERY_CLOSE) where no accepted box covers a cell, else min(zmin) / max(zmax) over the accepted
boxes that do.  Only the ceil(W/8) x ceil(H/8) corner is read by castRay and only that corner is predicted.

A floor or ceil that differs between the two number types counts as a tie only if it differs after clipping to [-1, W]
(x) or [-1, H] (y): below -1 and above W (H) the start values and the clamps decide, whatever the value is.

Block coordinates are assumed within +-32766: the engines add the corner offset in `short`, which wraps at 32767, and
that wrap is not part of this model.
"""
import numpy as np

import refmap

F = np.float32
FAR_AWAY, VERY_CLOSE = F(999999.9), F(0.05)
MAX_RENDERING_BLOCKS = 65536 * 4


def project_blocks(pos, M, intr, vs, W, H, T=F, skip_below=1e-6):
    """ProjectSingleBlock in number type T on blocks pos [n, 3].  Returns dict(box [n, 4] int64 (ulx, uly, lrx, lry) after
    the clamps, z [n, 2] of type T (zmin raised), req [n] int64 (0 = invalid), skipped [n, 8] bool, cells [n, 8, 4] int64:
    floor(px), ceil(px), floor(py), ceil(py) per corner clipped to [-1, W] / [-1, H] (0 where the corner is skipped),
    in_front [n] bool: not (zmax < VERY_CLOSE)).  `skip_below` is the law's 1e-6; a fixture passes another value only to
    show that the threshold decides cells of its image."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    # (the corner offset is added in 16 bits: only 32767 + 1 wraps, -32768 is as good a block as any)
    assert pos.min(initial=0) >= -32768 and pos.max(initial=0) <= 32766, "block coordinate at the end of the short range"
    n = len(pos)
    M = np.asarray(M, F).astype(T)
    fx, fy, cx, cy = (T(F(v)) for v in intr)
    vs = T(F(vs))
    ulx, uly = np.full(n, float(W // 8)), np.full(n, float(H // 8))
    lrx, lry = np.full(n, -1.0), np.full(n, -1.0)
    zmin, zmax = np.full(n, T(FAR_AWAY), T), np.full(n, T(VERY_CLOSE), T)
    skipped = np.zeros((n, 8), bool)
    cells = np.zeros((n, 8, 4), np.int64)
    for corner in range(8):
        t = pos + np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
        x, y, z = ((t[:, k].astype(T) * T(8)) * vs for k in range(3))
        qx, qy, qz = (((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3))
        skip = qz < T(F(skip_below))
        good = ~skip
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            px = ((fx * qx) / qz + cx) / T(8)
            py = ((fy * qy) / qz + cy) / T(8)
        px, py = np.where(good, px, T(0)).astype(np.float64), np.where(good, py, T(0)).astype(np.float64)
        fl_x, ce_x, fl_y, ce_y = np.floor(px), np.ceil(px), np.floor(py), np.ceil(py)
        ulx = np.where(good & (ulx > fl_x), fl_x, ulx)
        lrx = np.where(good & (lrx < ce_x), ce_x, lrx)
        uly = np.where(good & (uly > fl_y), fl_y, uly)
        lry = np.where(good & (lry < ce_y), ce_y, lry)
        zmin = np.where(good & (zmin > qz), qz, zmin)
        zmax = np.where(good & (zmax < qz), qz, zmax)
        skipped[:, corner] = skip
        for k, (a, hi) in enumerate(((fl_x, W), (ce_x, W), (fl_y, H), (ce_y, H))):
            cells[:, corner, k] = np.where(good, np.clip(a, -1, hi), 0).astype(np.int64)
    ulx, uly = np.maximum(ulx, 0), np.maximum(uly, 0)
    lrx, lry = np.minimum(lrx, W - 1), np.minimum(lry, H - 1)
    in_front = ~(zmax < T(VERY_CLOSE))
    valid = ~(ulx > lrx) & ~(uly > lry) & in_front
    zmin = np.where(zmin < T(VERY_CLOSE), T(VERY_CLOSE), zmin)
    box = np.stack([ulx, uly, lrx, lry], 1).astype(np.int64)
    w, h = box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1
    req = np.where(valid, -(-w // 16) * -(-h // 16), 0).astype(np.int64)
    return dict(box=box, z=np.stack([zmin, zmax], 1).astype(T), req=req, skipped=skipped, cells=cells, in_front=in_front)


def apply_budget(req, budget):
    """(accepted [n] bool, total): the sequential drop rule over req in list order."""
    req = np.asarray(req, np.int64)
    total = int(req.sum())
    keep = req != 0
    if total >= budget:
        num = 0
        for i in np.nonzero(keep)[0]:
            if num + req[i] >= budget:
                keep[i] = False
            else:
                num += int(req[i])
    return keep, total


def splat(box, lo, hi, cw, ch, lo_init, hi_init):
    """Per cell of the [ch, cw] corner: min of lo / max of hi over the boxes [n, 4] that cover it (inclusive bounds);
    the initial values where none does.  One pass per cell row, vectorised over boxes and columns."""
    box = np.asarray(box, np.int64).reshape(-1, 4)
    out = np.empty((ch, cw, 2), np.result_type(lo, hi) if len(box) else np.float32)
    out[..., 0], out[..., 1] = lo_init, hi_init
    if not len(box):
        return out
    xs = np.arange(cw)
    in_x = (box[:, 0, None] <= xs) & (xs <= box[:, 2, None])  # [n, cw]
    for y in range(ch):
        rows = np.nonzero((box[:, 1] <= y) & (y <= box[:, 3]))[0]
        if not len(rows):
            continue
        m = in_x[rows]
        out[y, :, 0] = np.where(m, np.asarray(lo)[rows, None], lo_init).min(0)
        out[y, :, 1] = np.where(m, np.asarray(hi)[rows, None], hi_init).max(0)
    return out


def cover(box, cw, ch, widen=0):
    """[ch, cw] bool: cells inside any of the boxes, each widened by `widen` cells."""
    box = np.asarray(box, np.int64).reshape(-1, 4) + np.array([-widen, -widen, widen, widen])
    c = splat(box, np.zeros(len(box)), np.ones(len(box)), cw, ch, 1.0, 0.0)
    return c[..., 1] > 0


class RangeLaw:
    """FindVisibleBlocks + CreateExpectedDepths of one hash table at one pose.

    ids: the visible list (entry indices, ascending) by the float32 verdicts;  vis_tie_ids: entries with ptr >= 0 whose
    visibility verdict differs between float32 and float64 (listed or not).
    Per listed block: pos, box, z (float32), req, accepted;  proj_tie [len(ids)]: a corner's skip verdict, a clipped
    floor / ceil or the VERY_CLOSE verdict differs;  tie_block = proj_tie or the entry is in vis_tie_ids.
    total: sum of req;  budget_on: total >= budget;  image [ch, cw, 2] float32;  tie_cells [ch, cw] bool: the cells of the
    boxes (both number types) of every tie block, listed or only a visibility tie, widened by one cell."""

    def __init__(self, table, M, intr, vs, W, H, budget=MAX_RENDERING_BLOCKS, skip_below=1e-6):
        table = np.asarray(table)
        self.W, self.H, self.cw, self.ch, self.budget = W, H, -(-W // 8), -(-H // 8), budget
        resident = np.nonzero(table["ptr"] >= 0)[0]
        rpos = table["pos"][resident].astype(np.int64)
        v32, _ = refmap.block_visibility(rpos, M, intr, vs, W, H, F)
        v64, _ = refmap.block_visibility(rpos, M, intr, vs, W, H, np.float64)
        self.resident = resident
        self.ids = resident[v32].astype(np.int32)
        self.vis_tie_ids = resident[v32 != v64].astype(np.int32)
        # projections of the listed blocks and of the visibility ties that are not listed
        extra = resident[~v32 & v64]
        every = np.concatenate([self.ids, extra]).astype(np.int64)
        pos = table["pos"][every].astype(np.int64)
        p32 = project_blocks(pos, M, intr, vs, W, H, F, skip_below)
        p64 = project_blocks(pos, M, intr, vs, W, H, np.float64, skip_below)
        tie = ((p32["skipped"] != p64["skipped"]).any(1) | (p32["cells"] != p64["cells"]).any((1, 2))
               | (p32["in_front"] != p64["in_front"]))
        n = len(self.ids)
        self.pos, self.box, self.z, self.req = pos[:n], p32["box"][:n], p32["z"][:n].astype(F), p32["req"][:n]
        self.box64, self.req64 = p64["box"][:n], p64["req"][:n]
        self.proj_tie = tie[:n]
        self.tie_block = self.proj_tie | np.isin(self.ids, self.vis_tie_ids)
        self.skipped = p32["skipped"][:n]
        self.accepted, self.total = apply_budget(self.req, budget)
        self.budget_on = self.total >= budget
        a = self.accepted
        self.image = splat(self.box[a], self.z[a, 0], self.z[a, 1], self.cw, self.ch, FAR_AWAY, VERY_CLOSE).astype(F)
        t = np.concatenate([self.tie_block, np.ones(len(extra), bool)])
        tb = np.concatenate([p32["box"][t], p64["box"][t]])
        self.tie_cells = cover(tb, self.cw, self.ch, widen=1)
        self.n_tie_blocks = int(self.tie_block.sum()) + len(extra)

    def tie_shares(self):
        """(tie blocks / listed blocks, tie cells / corner cells)"""
        return self.n_tie_blocks / max(len(self.ids), 1), float(self.tie_cells.mean())

    def tile_cells(self):
        """[n] int64: the largest number of cells one 16 x 16-cell tile of the corner holds of each listed block's box."""
        b = self.box
        best = np.zeros(len(b), np.int64)
        for ty in range(0, self.ch, 16):
            for tx in range(0, self.cw, 16):
                w = np.minimum(b[:, 2], tx + 15) - np.maximum(b[:, 0], tx) + 1
                h = np.minimum(b[:, 3], ty + 15) - np.maximum(b[:, 1], ty) + 1
                best = np.maximum(best, np.where((w > 0) & (h > 0) & (self.req != 0), w * h, 0))
        return best
