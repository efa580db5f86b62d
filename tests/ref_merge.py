"""The law of dslam_merge_maps (include/dslam_fusion.h) restated sequentially in numpy: float32
where the law says float32, integers elsewhere.  Written from the law's text; the kernels are held to it byte for byte
(test_gpu_merge.py), and test_merge_ref.py checks the restatement itself on the analytic pairs.

A map is a `State`: hash table, the two free lists with their tops, every voxel block -- what the engine's download calls
return and `analytic_maps.Map` builds.  `merge(src, dst, X, ...)` changes `dst` in place and returns the result fields."""
import numpy as np

import analytic_maps as am

F = np.float32
RANGE = F(262144.0)   # voxel coordinates whose block coordinate fits a short: [-RANGE, RANGE)
LOCAL = np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], -1)   # l -> (x, y, z), x fastest
TAPS = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)])


class State:
    def __init__(self, hash_table, alloc_list, last_free, excess_list, last_free_ex, vba, num_buckets, vs, mu, max_w=100):
        self.hash = np.array(hash_table, dtype=am.HASH_ENTRY_DTYPE)
        self.alloc_list, self.excess_list = np.array(alloc_list, np.int32), np.array(excess_list, np.int32)
        self.last_free, self.last_free_ex = int(last_free), int(last_free_ex)
        self.vba = np.array(vba, dtype=am.VOXEL_DTYPE).reshape(-1, 512)
        self.num_buckets, self.vs, self.mu, self.max_w = int(num_buckets), vs, mu, max_w

    @classmethod
    def of_map(cls, m, max_w=100):
        return cls(m.hash, m.alloc_list, m.last_free, m.excess_list, m.last_free_ex, m.vba, m.num_buckets, m.vs, m.mu, max_w)

    @classmethod
    def empty(cls, num_buckets, num_excess, num_local_blocks, vs=am.VS, mu=am.MU, max_w=100):
        table = np.zeros(num_buckets + num_excess, am.HASH_ENTRY_DTYPE)
        table["ptr"] = -2
        vba = np.zeros((num_local_blocks, 512), am.VOXEL_DTYPE)
        vba["sdf"] = 32767
        return cls(table, np.arange(num_local_blocks), num_local_blocks - 1, np.arange(num_excess), num_excess - 1, vba,
                   num_buckets, vs, mu, max_w)

    def copy(self):
        return State(self.hash, self.alloc_list, self.last_free, self.excess_list, self.last_free_ex, self.vba,
                     self.num_buckets, self.vs, self.mu, self.max_w)

    @property
    def num_excess(self):
        return len(self.hash) - self.num_buckets

    @property
    def num_local_blocks(self):
        return len(self.vba)

    def live(self):
        """Resident entries, ascending by hash index."""
        return np.flatnonzero(self.hash["ptr"] >= 0)

    def scene_params(self, pkg, **over):
        kw = dict(voxel_size=self.vs, mu=self.mu, max_w=self.max_w, frustum_min=0.05, frustum_max=5.0,
                  num_local_blocks=self.num_local_blocks, num_buckets=self.num_buckets, num_excess=self.num_excess)
        kw.update(over)
        return pkg.SceneParams(**kw)

    def upload(self, api, scene):
        api.upload_scene_state(scene, self.hash, self.alloc_list, self.last_free, self.excess_list, self.last_free_ex)
        api.upload_voxel_blocks(scene, 0, self.vba)

    @classmethod
    def download(cls, api, scene, like):
        st = api.stats(scene)
        return cls(api.download_hash_table(scene), api.download_allocation_list(scene), st["last_free_block_id"],
                   api.download_excess_list(scene), st["last_free_excess_id"], api.download_voxel_blocks(scene),
                   like.num_buckets, like.vs, like.mu, like.max_w)

    def voxels_by_position(self):
        """{block position: its 512 voxels}: the map as a function position -> voxel."""
        return {tuple(int(c) for c in self.hash["pos"][t]): self.vba[self.hash["ptr"][t]] for t in self.live()}

    def differences(self, other):
        """Names of the parts that differ byte for byte (empty: the same state)."""
        out = []
        if self.hash.tobytes() != other.hash.tobytes():
            bad = np.flatnonzero(self.hash.view(np.uint8).reshape(-1, 16).view(np.uint64).reshape(-1, 2)
                                 != other.hash.view(np.uint8).reshape(-1, 16).view(np.uint64).reshape(-1, 2))
            out.append(f"hash table ({len(bad)} words, first entry {bad[0] // 2 if len(bad) else -1})")
        if self.alloc_list.tobytes() != other.alloc_list.tobytes():
            out.append("allocation list")
        if self.excess_list.tobytes() != other.excess_list.tobytes():
            out.append("excess list")
        if (self.last_free, self.last_free_ex) != (other.last_free, other.last_free_ex):
            out.append(f"tops {(self.last_free, self.last_free_ex)} / {(other.last_free, other.last_free_ex)}")
        a, b = self.vba.view(np.uint64).reshape(-1, 512), other.vba.view(np.uint64).reshape(-1, 512)
        if a.shape != b.shape or (a != b).any():
            bad = np.argwhere(a != b)
            out.append(f"voxel blocks ({len(bad)} voxels, first block {bad[0][0]} voxel {bad[0][1]}: "
                       f"{self.vba[bad[0][0], bad[0][1]]} / {other.vba[bad[0][0], bad[0][1]]})")
        return out


# ---------------------------------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------------------------------
def transforms(X, vs):
    """(X~, Y~, identity): 3 x 4 float32 each, formed in double from the float32 X (4x4, metres) and float32 voxel size."""
    X = np.asarray(X, F)
    identity = bool(np.array_equal(X, np.eye(4, dtype=F)))
    R = X[:3, :3].astype(np.float64)
    t = X[:3, 3].astype(np.float64) / np.float64(F(vs))
    Xt = np.concatenate([R, t[:, None]], 1).astype(F)
    y = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
    Yt = np.concatenate([R.T, y[:, None]], 1).astype(F)
    return Xt, Yt, identity


def to_map(T, identity, p):
    """q = T p per row as ((a x + b y) + c z) + d, float32; the identity reads at p itself."""
    p = np.asarray(p, F)
    if identity:
        return p
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], -1).astype(F)


def lerp8(s, c):
    """Trilinear blend of the 8 taps s[..., k] at fractions c[..., 3], float32: x, then y, then z."""
    s = [np.asarray(s[..., k], F) for k in range(8)]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    one = F(1.0)
    ux, uy, uz = one - cx, one - cy, one - cz
    x00, x10 = ux * s[0] + cx * s[1], ux * s[2] + cx * s[3]
    x01, x11 = ux * s[4] + cx * s[5], ux * s[6] + cx * s[7]
    y0, y1 = uy * x00 + cy * x10, uy * x01 + cy * x11
    return (uz * y0 + cz * y1).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# table
# ---------------------------------------------------------------------------------------------------------------------
def lookup(st, B):
    """(entry, None) of block B in the table, or (None, (slot, type)): the slot an allocation pass would use for it."""
    h = int(am.hash_index(np.asarray(B), st.num_buckets))
    e = st.hash[h]
    if e["ptr"] < -1:
        return None, (h, 1)
    while True:
        if e["ptr"] >= -1 and tuple(e["pos"]) == tuple(B):
            return h, None
        if e["offset"] < 1:
            return None, (h, 2)
        h = st.num_buckets + int(e["offset"]) - 1
        e = st.hash[h]


class SourceReader:
    """The source as a function voxel position -> stored voxel; absent blocks read as the empty voxel."""

    def __init__(self, st):
        live = st.live()
        pos = st.hash["pos"][live].astype(np.int64)
        self.codes = self._code(pos)
        order = np.argsort(self.codes)
        self.codes, self.ptrs = self.codes[order], st.hash["ptr"][live][order].astype(np.int64)
        self.vba = st.vba
        self.empty = np.zeros((), am.VOXEL_DTYPE)
        self.empty["sdf"] = 32767

    @staticmethod
    def _code(b):
        return ((b[..., 0] + 32768) << 32) | ((b[..., 1] + 32768) << 16) | (b[..., 2] + 32768)

    def read(self, p):
        p = np.asarray(p, np.int64)
        b = p >> 3
        ok = np.all((b >= -32768) & (b <= 32767), axis=-1)
        out = np.full(p.shape[:-1], self.empty, am.VOXEL_DTYPE)
        if len(self.codes) == 0:
            return out
        code = self._code(np.where(ok[..., None], b, 0))
        i = np.clip(np.searchsorted(self.codes, code), 0, len(self.codes) - 1)
        found = ok & (self.codes[i] == code)
        lin = (p[..., 0] & 7) | ((p[..., 1] & 7) << 3) | ((p[..., 2] & 7) << 6)
        out[found] = self.vba[self.ptrs[i[found]], lin[found]]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the voxel merge (CombineVoxelInformation, float32 as the law states it)
# ---------------------------------------------------------------------------------------------------------------------
def combine(res, dst, max_w):
    """`res` (the resampled voxels, the "host copy") merged into `dst` (the resident voxels); returns the new voxels."""
    out = dst.copy()
    ow, nw = res["w_depth"].astype(np.int64), dst["w_depth"].astype(np.int64)
    m = ow != 0
    newF = dst["sdf"].astype(F) / F(32767.0)
    oldF = res["sdf"].astype(F) / F(32767.0)
    newF = ow.astype(F) * oldF + nw.astype(F) * newF
    sw = ow + nw
    with np.errstate(divide="ignore", invalid="ignore"):
        newF = newF / sw.astype(F)
    sdf = np.trunc(np.where(m, newF, F(0)) * F(32767.0)).astype(np.int16)
    out["sdf"] = np.where(m, sdf, dst["sdf"])
    out["w_depth"] = np.where(m, np.minimum(sw, max_w), nw).astype(np.uint8)
    ow, nw = res["w_color"].astype(np.int64), dst["w_color"].astype(np.int64)
    m = ow != 0
    sw = ow + nw
    v = dst["clr"].astype(F) / F(255.0)
    oc = res["clr"].astype(F) / F(255.0)
    v = oc * ow.astype(F)[..., None] + v * nw.astype(F)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = v / sw.astype(F)[..., None]
    nc = np.trunc(np.where(m[..., None], v, F(0)) * F(255.0)).astype(np.int64).astype(np.uint8)
    out["clr"] = np.where(m[..., None], nc, dst["clr"])
    out["w_color"] = np.where(m, np.minimum(sw, max_w), nw).astype(np.uint8)
    return out


def resample(reader, Yt, identity, P, with_colour):
    """The source read at the destination voxels P [n, 3] (int): packed voxels, the empty voxel where nothing is given."""
    n = len(P)
    out = np.full(n, reader.empty, am.VOXEL_DTYPE)
    if identity:
        out = reader.read(P)
        if not with_colour:
            out["w_color"] = 0
        return out
    q = to_map(Yt, False, P.astype(F))
    inr = np.all(np.abs(q) < RANGE, axis=-1)
    f = np.floor(q)
    c = (q - f).astype(F)
    cell = np.where(inr[:, None], f, 0).astype(np.int64)
    taps = np.stack([reader.read(cell + TAPS[k]) for k in range(8)], -1)   # [n, 8]
    ok = inr & np.all(taps["w_depth"] > 0, axis=-1)
    d = lerp8(taps["sdf"].astype(F) / F(32767.0), c)
    out["sdf"] = np.where(ok, np.trunc(d * F(32767.0)).astype(np.int16), 32767)
    out["w_depth"] = np.where(ok, taps["w_depth"].min(axis=-1), 0)
    cok = ok & np.all(taps["w_color"] > 0, axis=-1) & bool(with_colour)
    for ch in range(3):
        v = lerp8(taps["clr"][..., ch].astype(F), c) + F(0.5)
        out["clr"][:, ch] = np.where(cok, np.trunc(v).astype(np.int64).astype(np.uint8), 0)
    out["w_color"] = np.where(cok, taps["w_color"].min(axis=-1), 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------------------------
def targets(src, Xt, identity):
    """{target block: largest key that names it}, candidates, out of range -- phase 1."""
    live = src.live()
    pos = src.hash["pos"][live].astype(np.int64)
    vox = src.vba[src.hash["ptr"][live]]                                   # [n, 512]
    P = pos[:, None, :] * 8 + LOCAL[None]
    keys = np.arange(len(live), dtype=np.int64)[:, None] * 512 + np.arange(512)[None] + 1
    cand = vox["w_depth"] > 0
    q = to_map(Xt, identity, P.astype(F))
    t = np.floor(q + F(0.5))
    inr = np.all((t >= -RANGE) & (t < RANGE), axis=-1)
    use = cand & inr
    B = t[use].astype(np.int64) >> 3
    best = {}
    if len(B):
        uniq, inverse = np.unique(B, axis=0, return_inverse=True)
        top = np.zeros(len(uniq), np.int64)
        np.maximum.at(top, inverse.reshape(-1), keys[use])
        best = {tuple(int(v) for v in b): int(k) for b, k in zip(uniq, top)}
    return best, len(live), int(cand.sum()), int((cand & ~inr).sum())


def merge(src, dst, X, max_passes=0, with_colour=1):
    assert src.vs == dst.vs and src.mu == dst.mu
    Xt, Yt, identity = transforms(X, src.vs)
    max_passes = max_passes or 16
    best, n_live, n_cand, n_oor = targets(src, Xt, identity)
    res = dict(passes=0, exhausted=0, src_blocks=n_live, blocks_allocated=0, blocks_touched=0, requests_unserved=0,
               src_candidates=n_cand, out_of_range=n_oor, voxels_changed=0)
    touched = set()
    nb = dst.num_buckets
    while True:
        requests = {}                                   # slot -> (key, B, type): a slot keeps the largest key that asked
        for B, key in best.items():
            entry, miss = lookup(dst, B)
            if entry is not None:
                touched.add(entry)
            elif miss[0] not in requests or requests[miss[0]][0] < key:
                requests[miss[0]] = (key, B, miss[1])
        res["passes"] += 1
        if not requests:
            break
        served = 0
        for slot in sorted(requests):                   # ascending hash index; a request that finds a pool empty takes nothing
            key, B, typ = requests[slot]
            if dst.last_free < 0 or (typ == 2 and dst.last_free_ex < 0):
                continue
            ptr = int(dst.alloc_list[dst.last_free])
            dst.last_free -= 1
            entry = slot
            if typ == 2:
                off = int(dst.excess_list[dst.last_free_ex])
                dst.last_free_ex -= 1
                dst.hash["offset"][slot] = off + 1
                entry = nb + off
            dst.hash[entry] = (B, 0, 0, ptr)
            touched.add(entry)
            served += 1
        res["blocks_allocated"] += served
        if served == 0 or res["passes"] >= max_passes:
            res["exhausted"] = 1
            res["requests_unserved"] = len(requests) - served
            break
    res["blocks_touched"] = len(touched)
    reader = SourceReader(src)
    for entry in sorted(touched):
        e = dst.hash[entry]
        P = e["pos"].astype(np.int64)[None] * 8 + LOCAL
        was = dst.vba[e["ptr"]]
        now = combine(resample(reader, Yt, identity, P, with_colour), was, dst.max_w)
        changed = now.view(np.uint64) != was.view(np.uint64)
        res["voxels_changed"] += int(changed.sum())
        dst.vba[e["ptr"]] = now
    return res
