"""A model of the map's bookkeeping: which blocks exist, where their entries sit, what the pools and lists hold.

Written from SURVEY.md A.1 (layouts, hashIndex), A.2 (lookup), A.4 (MARK / COMMIT / VISIBLE / REALLOC), A.6 (block
visibility), A.9 with DESIGN.md section 5 (visible-list rings, Decay in both modes, SlideWindow, batch release) and A.10
(reset).  numpy and plain Python, stated over sets: a pass is "the samples of the walk", "the requests per slot and their
winners", "the commits in ascending slot order", never a pixel loop or a table sweep.  Every quantity it predicts is
an integer, so it predicts the state exactly; nothing here has a tolerance.

The rule of ref64.py applies to everything geometric: a predicate (the block a marched point falls into, the four
depth gates, the step count, a corner inside the image) is evaluated in np.float32 in the spec's operation order, the
same expression in float64 beside it, and an element on which the two disagree is a *tie* and is counted.

In the model: the hash table (A.1 layout) with a dictionary view block -> entry, both free stacks, the allocation
scratch (types, coordinates), a render state's type bytes and visible list, swap states, the two list rings and
last_seen per voxel-block slot, the integer depth weights per voxel (Decay's predicate reads them; the caller feeds
them from ref64.integrate), and the counters of dslam_get_stats these calls move.
Of A.8 the integer part is in: which entries hold a host copy, its depth weights, the states, and which blocks
swap-in merges (w = min(w_host + w_device, maxW)) and swap-out parks, in ProcessFrame, SlideWindow, the direct
swap-in / swap-out calls and SaveToGlobalMemory (`save_to_global`).  Every merge and every park is also written to
`events`, in order, so that a caller who carries voxel values (refmap_checks.Rig, with ref64.combine_stored) can move them
the same way.  Both list rings are driven: q = 1 is the defusion ring of ProcessFrame(isDefusion), SlideWindowDefusionPart
and DecayDefusionPart.  Out of the model: voxel values (sdf, colour), the transfer buffers, the batched re-integration,
sharding.  FindVisibleBlocks and CreateExpectedDepths (the visible list of a free view, the projected boxes, the render-tile
budget and the range image) are stated in ref_range.py, which takes `block_visibility` from here.
"""
import numpy as np

F = np.float32
HASH_ENTRY_DTYPE = np.dtype(
    {"names": ["pos", "_pad", "offset", "ptr"], "formats": [("<i2", 3), "<i2", "<i4", "<i4"], "offsets": [0, 6, 8, 12],
     "itemsize": 16})


def hash_index(b, num_buckets):
    """A.1 hashIndex on integer block coordinates [..., 3]: uint32 products, xor, mask."""
    b = np.asarray(b, np.int64) & 0xFFFFFFFF
    h = ((b[..., 0] * 73856093) & 0xFFFFFFFF) ^ ((b[..., 1] * 19349669) & 0xFFFFFFFF) ^ ((b[..., 2] * 83492791) & 0xFFFFFFFF)
    return (h & (num_buckets - 1)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Matrix4::inv in float (A.4: invM_d is that function applied to M_d)
# ---------------------------------------------------------------------------------------------------------------------
_PAIRS_A = [(10, 15), (11, 14), (9, 15), (11, 13), (9, 14), (10, 13), (8, 15), (11, 12), (8, 14), (10, 12), (8, 13), (9, 12)]
_PAIRS_B = [(2, 7), (3, 6), (1, 7), (3, 5), (1, 6), (2, 5), (0, 7), (3, 4), (0, 6), (2, 4), (0, 5), (1, 4)]
# cofactor k = (t[a] s[i] + t[b] s[j] + t[c] s[l]) - (the same shape): ((a, i), (b, j), (c, l)), ((...), (...), (...))
_COF_A = [(((0, 5), (3, 6), (4, 7)), ((1, 5), (2, 6), (5, 7))), (((1, 4), (6, 6), (9, 7)), ((0, 4), (7, 6), (8, 7))),
          (((2, 4), (7, 5), (10, 7)), ((3, 4), (6, 5), (11, 7))), (((5, 4), (8, 5), (11, 6)), ((4, 4), (9, 5), (10, 6))),
          (((1, 1), (2, 2), (5, 3)), ((0, 1), (3, 2), (4, 3))), (((0, 0), (7, 2), (8, 3)), ((1, 0), (6, 2), (9, 3))),
          (((3, 0), (6, 1), (11, 3)), ((2, 0), (7, 1), (10, 3))), (((4, 0), (9, 1), (10, 2)), ((5, 0), (8, 1), (11, 2)))]
_COF_B = [(((0, 13), (3, 14), (4, 15)), ((1, 13), (2, 14), (5, 15))), (((1, 12), (6, 14), (9, 15)), ((0, 12), (7, 14), (8, 15))),
          (((2, 12), (7, 13), (10, 15)), ((3, 12), (6, 13), (11, 15))), (((5, 12), (8, 13), (11, 14)), ((4, 12), (9, 13), (10, 14))),
          (((2, 10), (5, 11), (1, 9)), ((4, 11), (0, 9), (3, 10))), (((8, 11), (0, 8), (7, 10)), ((6, 10), (9, 11), (1, 8))),
          (((6, 9), (11, 11), (3, 8)), ((10, 11), (2, 8), (7, 9))), (((10, 10), (4, 8), (9, 9)), ((8, 9), (11, 10), (5, 8)))]


def inv_f32(M):
    """ORUtils Matrix4::inv: cofactor expansion over twelve 2x2 products per half, every operation a float32 one,
    the cofactors times (1 / det).  M[row, col] in, the inverse [row, col] out.
    The walk's block coordinates depend on the rounding of this inverse, so the model has to round as the engines do:
    this one function is a restatement of the upstream routine operation by operation (the index tables above are its
    sixteen cofactors), pinned bit for bit against the oracle's export of it -- the one part of the model that is
    checked by, not independent of, the code under test."""
    s = [F(v) for v in np.asarray(M, F).ravel()]  # s[4 r + c] = M[r, c]
    d = []
    for pairs, cofs in ((_PAIRS_A, _COF_A), (_PAIRS_B, _COF_B)):
        t = [s[a] * s[b] for a, b in pairs]
        for pos, neg in cofs:
            (a, i), (b, j), (c, k) = pos
            (e, l), (f, m), (g, n) = neg
            d.append((t[a] * s[i] + t[b] * s[j] + t[c] * s[k]) - (t[e] * s[l] + t[f] * s[m] + t[g] * s[n]))
    det = s[0] * d[0] + s[1] * d[1] + s[2] * d[2] + s[3] * d[3]
    r = F(1) / det
    return np.array([v * r for v in d], F).reshape(4, 4).T  # d is column-major


def mat_vec_f32(M, x, y, z):
    """Matrix4f * (x, y, z, 1): row r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3, float32, no fused multiply-add."""
    M = np.asarray(M, F)
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


# ---------------------------------------------------------------------------------------------------------------------
# A.4 MARK: the walk
# ---------------------------------------------------------------------------------------------------------------------
def _walk(depth, M, invM, intr, vs, mu, fmin, fmax, T):
    """The walk in the number type T (np.float32 or np.float64).  Per pixel: gate, steps; per (pixel, step): block."""
    H, W = depth.shape
    d = depth.reshape(-1).astype(T)
    vs, mu, fmin, fmax = T(F(vs)), T(F(mu)), T(F(fmin)), T(F(fmax))
    fx, fy, cx, cy = (T(F(v)) for v in intr)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gate = ~((d <= 0) | ((d - mu) < 0) | ((d - mu) < fmin) | ((d + mu) > fmax))
        pix = np.arange(W * H)
        x, y = (pix % W).astype(T), (pix // W).astype(T)
        pcx, pcy, pcz = d * ((x - cx) * (T(1) / fx)), d * ((y - cy) * (T(1) / fy)), d
        n = np.sqrt(pcx * pcx + pcy * pcy + pcz * pcz)
        one_over_block = T(1) / (vs * T(8))
        invM = np.asarray(invM, T)
        ends = []
        for s in (T(1) - mu / n, T(1) + mu / n):
            q = [((invM[r, 0] * (pcx * s) + invM[r, 1] * (pcy * s)) + invM[r, 2] * (pcz * s)) + invM[r, 3] for r in range(3)]
            ends.append([c * one_over_block for c in q])
        p, pe = ends
        dr = [b - a for a, b in zip(p, pe)]
        nd = np.sqrt(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2])
        steps = np.where(gate, np.ceil(T(2) * np.where(gate, nd, T(0))), 0).astype(np.int64)
        div = (steps - 1).astype(T)
        dr = [c / div for c in dr]
        smax = int(steps.max()) if gate.any() else 0
        blocks = np.zeros((W * H, max(smax, 1), 3), np.int64)
        for i in range(smax):
            for k in range(3):
                blocks[:, i, k] = np.where(i < steps, np.floor(np.where(i < steps, p[k], T(0))), 0).astype(np.int64)
            p = [a + b for a, b in zip(p, dr)]
    return gate, steps, blocks


class Walk:
    """Every (pixel index, step, block) of MARK for one depth image, float32; float64 beside it for the ties.
    pix, step, block: the samples, in row-major pixel order and step order; key = pix * key_stride + step orders them
    as the sequential loop meets them.  tie[i]: sample i sits at a pixel whose gate or step count differs between the
    two walks (`step_tie`), or in another block (`block_tie`, only where the step counts agree)."""

    def __init__(self, depth, M, intr, vs, mu, fmin, fmax):
        depth = np.asarray(depth, F)
        M = np.asarray(M, F)
        self.invM32 = inv_f32(M)
        g32, s32, b32 = _walk(depth, M, self.invM32, intr, vs, mu, fmin, fmax, F)
        g64, s64, b64 = _walk(depth, M, np.linalg.inv(M.astype(np.float64)), intr, vs, mu, fmin, fmax, np.float64)
        assert not g32.any() or s32[g32].min() >= 2, "a band shorter than two steps: dir / (steps - 1) is undefined"
        smax = b32.shape[1]
        valid = np.arange(smax)[None, :] < s32[:, None]
        self.pix, self.step = (a.astype(np.int64) for a in np.nonzero(valid))
        self.block = b32[valid]
        assert self.block.min(initial=0) >= -32768 and self.block.max(initial=0) <= 32767, "block coordinate outside int16"
        self.key_stride = smax + 1
        self.key = self.pix * self.key_stride + self.step
        self.gate_ties = int((g32 != g64).sum())
        self.step_tie_pixels = int((g32 & g64 & (s32 != s64)).sum())
        pix_bad = (g32 != g64) | (s32 != s64)
        self.step_tie = pix_bad[self.pix]
        b64p = np.zeros_like(b32)
        k = min(smax, b64.shape[1])
        b64p[:, :k] = b64[:, :k]
        self.block_tie = ~self.step_tie & (b64p[valid] != self.block).any(axis=1)
        self.tie = self.step_tie | self.block_tie
        self.n_pixels = int(g32.sum())
        self.steps = s32
        self.n = len(self.pix)


# ---------------------------------------------------------------------------------------------------------------------
# A.6 block visibility
# ---------------------------------------------------------------------------------------------------------------------
# corner order 000,001,011,111,110,100,010,101, each reached from the previous one by adding or subtracting the block
# edge (float): the moves below, as (axis, sign) lists
_CORNER_MOVES = [[], [(2, 1)], [(1, 1)], [(0, 1)], [(2, -1)], [(1, -1)], [(0, -1), (1, 1)], [(0, 1), (1, -1), (2, 1)]]


def block_visibility(pos, M, intr, vs, W, H, T=F):
    """(visible, visible in the enlarged image) of blocks pos [n, 3] in number type T."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    factor = T(8) * T(F(vs))
    fx, fy, cx, cy = (T(F(v)) for v in intr)
    M = np.asarray(M, F).astype(T)
    pt = [pos[:, k].astype(T) * factor for k in range(3)]
    vis = np.zeros(len(pos), bool)
    enl = np.zeros(len(pos), bool)
    lx, hx, ly, hy = -(W // 8), W + W // 8, -(H // 8), H + H // 8
    for moves in _CORNER_MOVES:
        for axis, sign in moves:
            pt[axis] = pt[axis] + factor if sign > 0 else pt[axis] - factor
        c = [((M[r, 0] * pt[0] + M[r, 1] * pt[1]) + M[r, 2] * pt[2]) + M[r, 3] for r in range(3)]
        ok = ~(c[2] < T(F(1e-10)))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            u = (fx * c[0]) / c[2] + cx
            v = (fy * c[1]) / c[2] + cy
        vis |= ok & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        enl |= ok & (u >= lx) & (u < hx) & (v >= ly) & (v < hy)
    return vis, enl


def exit_side(pos, M, intr, vs, W, H):
    """Where a block that failed the re-test went (float64, by its centre): 'behind', 'left', 'right', 'top', 'bottom'."""
    c = (np.asarray(pos, np.float64) + 0.5) * 8 * float(F(vs))
    M = np.asarray(M, np.float64)
    pc = M[:3, :3] @ c + M[:3, 3]
    if pc[2] <= 0:
        return "behind"
    fx, fy, cx, cy = (float(F(v)) for v in intr)
    u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
    du, dv = max(-u, u - W), max(-v, v - H)
    if du >= dv:
        return "left" if u < W / 2 else "right"
    return "top" if v < H / 2 else "bottom"


# ---------------------------------------------------------------------------------------------------------------------
# the map
# ---------------------------------------------------------------------------------------------------------------------
class MapModel:
    def __init__(self, params, W, H):
        p = params
        self.vs, self.mu, self.fmin, self.fmax = p.voxel_size, p.mu, p.frustum_min, p.frustum_max
        self.nb, self.nx, self.nl = p.num_buckets, p.num_excess, p.num_local_blocks
        self.n_entries = self.nb + self.nx
        self.swapping = bool(p.use_swapping)
        self.bits = 64 * (p.history_words if p.history_words > 0 else 4)
        self.W, self.H = W, H
        self.max_w = p.max_w
        self.reset()

    # -- A.10 ----------------------------------------------------------------------------------------------------------
    def reset(self):
        self.hash = np.zeros(self.n_entries, HASH_ENTRY_DTYPE)
        self.hash["ptr"] = -2
        self.alloc_list = np.arange(self.nl, dtype=np.int32)
        self.last_free = self.nl - 1
        self.excess_list = np.arange(self.nx, dtype=np.int32)
        self.last_free_ex = self.nx - 1
        self.alloc_type = np.zeros(self.n_entries, np.uint8)
        self.coords = np.zeros((self.n_entries, 4), np.int16)
        if not hasattr(self, "visible_type"):  # the render state is not the scene's: ResetScene leaves it alone
            self.visible_type = np.zeros(self.n_entries, np.uint8)
            self.visible_ids = np.zeros(0, np.int32)
        self.swap_state = np.zeros(self.n_entries, np.uint8)
        self.last_seen = np.full(self.nl, -1, np.int32)
        self.w = np.zeros((self.nl, 512), np.uint8)  # depth weights per voxel
        self.lists = [{}, {}]  # per ring: list index -> set of voxel-block slots
        self.head, self.next, self.cursor = [0, 0], [0, 0], [0, 0]
        self.frame_counter = 0
        self.decayed = self.slid = self.alloc_failures = 0
        self.has_stored = np.zeros(self.n_entries, bool)  # host store (swapping scenes): which entries hold a block,
        self.stored_w = np.zeros((self.n_entries, 512), np.uint8) if self.swapping else None  # and its depth weights
        self.last_swapped_in = self.last_swapped_out = 0
        self.events = []  # ("merge" | "park", entry, slot) in the order they happen; the caller empties it
        self._reindex()

    def load(self, hash_table, alloc_list, last_free, excess_list, last_free_ex, weights=None):
        """upload_scene_state (+ upload_voxel_blocks' weights) applied to the model."""
        self.hash = np.array(hash_table, HASH_ENTRY_DTYPE)
        self.alloc_list, self.last_free = np.array(alloc_list, np.int32), int(last_free)
        self.excess_list, self.last_free_ex = np.array(excess_list, np.int32), int(last_free_ex)
        if weights is not None:
            self.w = np.array(weights, np.uint8).reshape(self.nl, 512)
        self._reindex()

    def _reindex(self):
        occ = np.nonzero(self.hash["ptr"] >= -1)[0]
        self.index = {tuple(int(c) for c in self.hash["pos"][t]): int(t) for t in occ}

    def chain(self, head):
        out = [int(head)]
        while self.hash["offset"][out[-1]] >= 1:
            out.append(self.nb + int(self.hash["offset"][out[-1]]) - 1)
        return out

    def bucket_of(self, t):
        return t if t < self.nb else int(hash_index(self.hash["pos"][t], self.nb))

    def stats(self):
        return dict(last_free_block_id=self.last_free, last_free_excess_id=self.last_free_ex,
                    no_visible_entries=len(self.visible_ids), decayed_block_count=self.decayed,
                    slid_block_count=self.slid, frame_counter=self.frame_counter,
                    fusion_fifo_len=self.next[0] - self.head[0], defusion_fifo_len=self.next[1] - self.head[1],
                    alloc_failures=self.alloc_failures, last_swapped_in=self.last_swapped_in,
                    last_swapped_out=self.last_swapped_out)

    def _relist(self):
        self.visible_ids = np.nonzero(self.visible_type > 0)[0][:self.nl].astype(np.int32)

    def resident_visible(self):
        """(entry ids, slots, block positions) of the listed entries that hold a voxel block."""
        ids = self.visible_ids[self.hash["ptr"][self.visible_ids] >= 0]
        return ids, self.hash["ptr"][ids].astype(np.int64), self.hash["pos"][ids].astype(np.int64)

    # -- A.4 -----------------------------------------------------------------------------------------------------------
    def allocate(self, depth, M, intr, only_update_visible_list=False):
        """One AllocateSceneFromDepth.  Returns the pass' reach and tie counts."""
        info = {}
        wk = Walk(depth, M, intr, self.vs, self.mu, self.fmin, self.fmax)
        info.update(samples=wk.n, pixels=wk.n_pixels, gate_ties=wk.gate_ties, step_tie_pixels=wk.step_tie_pixels,
                    step_tie_samples=int(wk.step_tie.sum()), block_ties=int(wk.block_tie.sum()),
                    negative_blocks=int((wk.block < 0).any(axis=1).sum()))
        vt = self.visible_type
        vt[self.visible_ids] = 3
        self.alloc_type[:] = 0
        # the distinct blocks of the walk, each with its last sample in sequential order
        ub, inv = np.unique(wk.block, axis=0, return_inverse=True) if wk.n else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
        inv = inv.reshape(-1)
        last = np.full(len(ub), -1, np.int64)
        np.maximum.at(last, inv, np.arange(wk.n))
        requests = {}  # slot -> list of (key of the block's last sample, sample index, block, type)
        found = 0
        for k, b in enumerate(ub):
            b = tuple(int(c) for c in b)
            t = self.index.get(b)
            if t is not None:  # A.2: present (resident or parked on the host)
                vt[t] = 2 if self.hash["ptr"][t] == -1 else 1
                found += 1
                continue
            h = int(hash_index(b, self.nb))
            if self.hash["ptr"][h] < -1:
                slot, typ = h, 1  # empty bucket head
            else:
                slot, typ = self.chain(h)[-1], 2  # the end of an occupied bucket's chain
            requests.setdefault(slot, []).append((int(wk.key[last[k]]), int(last[k]), b, typ))
        winners = {slot: max(r) for slot, r in requests.items()}  # the largest (pixel, step) wins the slot
        info.update(found_blocks=found, requests=sum(len(r) for r in requests.values()), slots=len(winners),
                    contended_slots=sum(len(r) > 1 for r in requests.values()),
                    chain_end_requests=sum(w[3] == 2 for w in winners.values()),
                    commit_ties=int(sum(wk.block_tie[w[1]] for w in winners.values())),
                    commit_step_ties=int(sum(wk.step_tie[w[1]] for w in winners.values())))
        for slot, (_, _, b, typ) in winners.items():
            self.alloc_type[slot] = typ
            self.coords[slot] = (b[0], b[1], b[2], 1)
            if typ == 1:
                vt[slot] = 1
        # COMMIT in ascending slot order against the two free stacks
        self.alloc_failures = 0
        failed = {1: 0, 2: 0}
        if not only_update_visible_list:
            for slot in sorted(winners):
                _, _, b, typ = winners[slot]
                if typ == 1:
                    if self.last_free >= 0:
                        self.hash[slot] = (b, 0, 0, self.alloc_list[self.last_free])
                        self.last_free -= 1
                    else:
                        vt[slot] = 0
                        failed[1] += 1
                else:
                    if self.last_free >= 0 and self.last_free_ex >= 0:
                        o = int(self.excess_list[self.last_free_ex])
                        self.hash["offset"][slot] = o + 1
                        self.hash[self.nb + o] = (b, 0, 0, self.alloc_list[self.last_free])
                        vt[self.nb + o] = 1
                        self.last_free -= 1
                        self.last_free_ex -= 1
                    else:
                        failed[2] += 1
            self.alloc_failures = failed[1] + failed[2]
            self._reindex()
        info.update(failed_type1=failed[1], failed_type2=failed[2])
        # VISIBLE: entries of the previous list that this frame did not touch are re-tested (A.6)
        re = np.nonzero(vt == 3)[0]
        exits = dict(behind=0, left=0, right=0, top=0, bottom=0)
        vis_ties = 0
        if len(re):
            pos = self.hash["pos"][re]
            v32, e32 = block_visibility(pos, M, intr, self.vs, self.W, self.H, F)
            v64, e64 = block_visibility(pos, M, intr, self.vs, self.W, self.H, np.float64)
            keep, keep64 = (e32, e64) if self.swapping else (v32, v64)
            vis_ties = int((keep != keep64).sum())
            for t, p3 in zip(re[~keep], pos[~keep]):
                exits[exit_side(p3, M, intr, self.vs, self.W, self.H)] += 1
            vt[re[~keep]] = 0
            info["kept_by_margin"] = int((keep & ~v32).sum())
        info.update(retested=len(re), exits=exits, visibility_ties=vis_ties)
        if self.swapping:
            sel = (vt > 0) & (self.swap_state != 2)
            self.swap_state[sel] = 1
        self._relist()
        # REALLOC: visible entries parked on the host get a voxel block back
        re_ok = re_fail = 0
        if self.swapping:
            for t in np.nonzero((vt > 0) & (self.hash["ptr"] == -1))[0]:
                if self.last_free >= 0:
                    self.hash["ptr"][t] = self.alloc_list[self.last_free]
                    self.last_free -= 1
                    re_ok += 1
                else:
                    re_fail += 1
        info.update(reallocated=re_ok, realloc_failed=re_fail, type2_visible=int((vt == 2).sum()))
        return info

    # -- rings -------------------------------------------------------------------------------------------------
    def push_visible_list(self, q=0):
        """ProcessFrame queues the frame's list: the resident listed blocks, stamped with the frame counter."""
        wrapped = 0
        if self.next[q] - self.head[q] == self.bits:  # a full ring drops its oldest list; nothing is released
            self.lists[q].pop(self.head[q])
            self.head[q] += 1
            self.cursor[q] = max(self.cursor[q], self.head[q])
            wrapped = 1
        _, slots, _ = self.resident_visible()
        self.lists[q][self.next[q]] = set(int(s) for s in slots)
        self.next[q] += 1
        self.last_seen[slots] = self.frame_counter
        self.frame_counter += 1
        return wrapped

    def referenced(self, slot):
        return any(slot in l for ring in self.lists for l in ring.values())

    def _forget(self, slot):
        for ring in self.lists:
            for l in ring.values():
                l.discard(slot)
        self.last_seen[slot] = -1
        self.w[slot] = 0

    # -- A.8, the integer part: states, slots and depth weights (sdf and colour are out of the model) ---------------------
    TRANSFER = 0x1000

    def _merge_stored(self, t, slot):
        """CombineVoxelInformation's weights: where the host copy has a measurement, w = min(w_host + w_device, maxW)."""
        self.events.append(("merge", t, slot))
        src, dst = self.stored_w[t].astype(np.int64), self.w[slot].astype(np.int64)
        self.w[slot] = np.where(src != 0, np.minimum(src + dst, self.max_w), dst).astype(np.uint8)

    def _park(self, t):
        """The block of entry t goes to the host store; the entry stays, its slot returns to the pool."""
        slot = int(self.hash["ptr"][t])
        self.events.append(("park", t, slot))
        self.stored_w[t] = self.w[slot]
        self.has_stored[t] = True
        self.last_free += 1
        self.alloc_list[self.last_free] = slot
        self._forget(slot)
        self.hash["ptr"][t] = -1

    def swap_in(self):
        need = np.nonzero(self.swap_state == 1)[0][:self.TRANSFER]
        for t in need:
            if self.has_stored[t] and self.hash["ptr"][t] >= 0:
                self._merge_stored(int(t), int(self.hash["ptr"][t]))
        self.swap_state[need] = 2
        self.last_swapped_in = len(need)

    def swap_out(self):
        """Merged blocks (state 2) that are resident and not visible leave for the host, at most TRANSFER per call."""
        out = np.nonzero((self.swap_state == 2) & (self.hash["ptr"] >= 0) & (self.visible_type == 0))[0][:self.TRANSFER]
        for t in out:
            self.swap_state[t] = 0
            self._park(int(t))
        self.last_swapped_out = len(out)

    def save_to_global(self):
        """SaveToGlobalMemory(scene), A.8's last line: nothing resident stays behind.  Every pending entry (state 1) is
        merged, whatever the transfer size; the resident entries that never were visible since they got their block
        (state 0) count as merged too, after taking in a host copy if they have one; then every resident entry is
        parked, visible or not.  The call has no render state: type bytes and the visible list stay as they were."""
        while (self.swap_state == 1).any():
            self.swap_in()
        fresh = np.nonzero((self.swap_state == 0) & (self.hash["ptr"] >= 0))[0]
        with_copy = int(self.has_stored[fresh].sum())
        for t in fresh:
            if self.has_stored[t]:
                self._merge_stored(int(t), int(self.hash["ptr"][t]))
        self.swap_state[fresh] = 2
        out = np.nonzero((self.swap_state == 2) & (self.hash["ptr"] >= 0))[0]
        for t in out:
            self.swap_state[t] = 0
            self._park(int(t))
        self.last_swapped_in, self.last_swapped_out = 0, len(out)
        return dict(promoted=len(fresh), promoted_with_copy=with_copy, parked=len(out),
                    parked_visible=int((self.visible_type[out] > 0).sum()))

    # -- batch release -----------------------------------------------------------------------------------------
    def release(self, batch):
        """Entries `batch` (ascending) leave the table.  Returns how many were heads alone / heads of a chain / middle /
        tail entries, and the number of chains that lost several entries at once."""
        reach = dict(head_alone=0, head_of_chain=0, middle=0, tail=0, multi=0, head_and_first_child=0)
        if not len(batch):
            return reach
        gone = set(int(t) for t in batch)
        for t in sorted(gone):  # slots return to the pool in candidate order
            slot = int(self.hash["ptr"][t])
            self.last_free += 1
            self.alloc_list[self.last_free] = slot
            self._forget(slot)
        freed = []
        for head in sorted({self.bucket_of(t) for t in gone}):
            ch = self.chain(head)
            lost = [t for t in ch if t in gone]
            reach["multi"] += len(lost) > 1
            reach["head_and_first_child"] += len(ch) > 1 and ch[0] in gone and ch[1] in gone
            for t in lost:
                i = ch.index(t)
                kind = ("head_alone" if len(ch) == 1 else "head_of_chain") if i == 0 else ("tail" if i == len(ch) - 1 else "middle")
                reach[kind] += 1
            survivors = [t for t in ch if t not in gone]
            entries = [self.hash[t].copy() for t in survivors]
            types = [self.visible_type[t] for t in survivors]
            # the survivors keep their order; the first one sits in the head, the others stay where they are
            places = survivors if head not in gone else [head] + survivors[1:]
            for t in ch:
                self.hash[t] = ((0, 0, 0), 0, 0, -2)
                self.visible_type[t] = 0
            for i, (t, e, ty) in enumerate(zip(places, entries, types)):
                e["offset"] = (places[i + 1] - self.nb) + 1 if i + 1 < len(places) else 0
                self.hash[t] = e
                self.visible_type[t] = ty
            freed += [t - self.nb for t in ch[1:] if t not in places]
        for x in sorted(freed):  # freed excess slots go back in ascending order
            self.last_free_ex += 1
            self.excess_list[self.last_free_ex] = x
        self._reindex()
        self._relist()
        return reach

    # -- A.9 / DESIGN 5: Decay -------------------------------------------------------------------------------------------
    def _decay_candidates(self, cand, max_weight):
        slots = self.hash["ptr"][cand]
        w = self.w[slots]
        w[(w > 0) & (w <= max_weight)] = 0
        self.w[slots] = w
        if self.swapping:  # entries of a swapping scene are never unlinked
            return dict(candidates=len(cand), released=0)
        empty = [int(t) for t, e in zip(cand, ~(w > 0).any(axis=1)) if e]
        self.decayed += len(empty)
        reach = self.release(empty)
        reach.update(candidates=len(cand), released=len(empty))
        return reach

    def decay(self, max_weight, min_age, force_all, q=0):
        total = {}

        def add(r):
            for k, v in r.items():
                total[k] = total.get(k, 0) + int(v)

        if not force_all:  # aged-list mode: every list once, when it is min_age lists old
            newest = self.next[q] - 1
            k = max(self.cursor[q], self.head[q])
            while k <= newest - min_age:
                l = self.lists[q][k]
                res = np.nonzero(self.hash["ptr"] >= 0)[0]
                cand = res[np.array([int(s) in l for s in self.hash["ptr"][res]], bool)]
                add(self._decay_candidates(cand, max_weight))
                k += 1
            self.cursor[q] = max(self.cursor[q], k)
        else:  # gated sweep: every resident block with last_seen <= newest - min_age, once per observation epoch
            threshold = self.frame_counter - 1 - min_age
            res = np.nonzero(self.hash["ptr"] >= 0)[0]
            ls = self.last_seen[self.hash["ptr"][res]]
            sel = (ls >= 0) & (ls <= threshold)
            cand = res[sel]
            total["at_gate"] = int((ls == threshold).sum())
            total["one_young"] = int((ls == threshold + 1).sum())
            total["already_swept"] = int((ls <= -2).sum())
            self.last_seen[self.hash["ptr"][cand]] = -2 - ls[sel]
            add(self._decay_candidates(cand, max_weight))
        return total

    # -- SlideWindow -------------------------------------------------------------------------------------------
    def slide_window(self, max_age, q=0):
        total = dict(pops=0, only_in_popped=0, also_newer=0, parked=0, parked_merged=0)
        max_age = max(max_age, 0)
        while self.next[q] - self.head[q] > max_age:
            l = self.lists[q].pop(self.head[q])
            self.head[q] += 1
            self.cursor[q] = max(self.cursor[q], self.head[q])
            res = np.nonzero(self.hash["ptr"] >= 0)[0]
            inl = [t for t in res if int(self.hash["ptr"][t]) in l]
            rem = [int(t) for t in inl if not self.referenced(int(self.hash["ptr"][t]))]
            total["pops"] += 1
            total["only_in_popped"] += len(rem)
            total["also_newer"] += len(inl) - len(rem)
            self.slid += len(rem)
            if not self.swapping:
                for k, v in self.release(rem).items():
                    total[k] = total.get(k, 0) + int(v)
                continue
            for t in rem:  # a swapping scene parks the block: the entry stays, the voxel block goes back to the pool
                if self.swap_state[t] != 2 and self.has_stored[t]:  # a host copy not merged yet is merged first
                    self._merge_stored(t, int(self.hash["ptr"][t]))
                    total["parked_merged"] += 1
                self._park(t)
                self.swap_state[t] = 0
                self.visible_type[t] = 0
                total["parked"] += 1
            if rem:
                self._relist()
        return total
