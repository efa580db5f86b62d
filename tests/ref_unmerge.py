"""The law of dslam_unmerge_maps and dslam_remerge_maps (include/dslam_fusion.h) restated
sequentially in numpy on ref_merge.State: float32 where the law says float32, integers elsewhere.  Written from the law's
text; the kernels are held to it byte for byte (test_gpu_unmerge.py), and test_unmerge_ref.py checks the restatement itself.
The transforms, the targets, the table lookup and the resampled voxel are ref_merge's: the unmerge shares them with the merge.

The round trip merge -> unmerge, and why it is not exact
---------------------------------------------------------
Weights.  While nothing clamps at max_w the merge adds ws to W0 and the unmerge takes ws off W0 + ws: exact.

Depth values, in raw units (S = 32767), for a voxel with W0 > 0 before the merge, resampled weight ws, W = W0 + ws, r = W / W0.
  * The merge stores M = trunc(E + e1) with E = (ws s + W0 d) / W the exact mean of the raw values and e1 its float32
    error.  Truncation toward zero loses less than one unit: |M - E| < 1 + |e1|.
  * The unmerge computes (W M - ws s) / W0 = d + r (M - E): the subtraction multiplies the merge's loss by r.
  * Its own truncation loses less than one unit more.
  So |raw_after - raw_before| < r (1 + |e1|) + |e2| + 1, e2 the float32 error of the unmerge's expression.
  The float32 terms, u = 2^-24 (round to nearest), every stored value at most 1 in magnitude: v / S costs u per operand,
  the two products and their sum or difference 3 u (W0 + ws) in the numerator at most, the division and the product with S
  one u each.  Merge: |e1| <= 5 u S.  Unmerge: numerator error <= u (2 W + 2 ws + W0) <= 4 u W, over W0, plus two u:
  |e2| <= u S (4 r + 1).  Together:
        |raw_after - raw_before| < r + 1 + u S (9 r + 1),      u S = 0.00195
  and, both sides of the difference being integers, |raw_after - raw_before| <= ceil(r + 1 + u S (9 r + 1)) - 1.
  For the uniform pairs (ws, W0) = (1, 1), (3, 5), (7, 2), (40, 3) that is 3, 2, 5, 15 = floor(r + 1).
  The clamp to [-1, 1] moves the result towards the interval that holds d and cannot add error.
  A voxel with W0 = 0 (one the merge created) has rem = 0: it becomes the empty depth half exactly.

Colour channels (S = 255), Wc0 > 0 before the merge, resampled wcs, rc = (Wc0 + wcs) / Wc0: combine truncates
(unsigned char)(v * 255) just as float_to_sdf does, so the same three steps give
        |c_after - c_before| <= ceil(rc + 1 + u 255 (9 rc + 1)) - 1
(the values are not negative, so the truncations all lose downwards: c_after <= c_before when the float terms vanish).  A
voxel with Wc0 = 0 returns to three zero channels and w_color 0.

With a clamp at max_w during the merge the weights no longer add up (W' = max_w < W0 + ws) and neither statement holds."""
import math

import numpy as np

import ref_merge as rm

F = np.float32
U = 2.0 ** -24


def depth_bound(W0, ws):
    """Largest |raw sdf after - raw sdf before| the round trip may leave on a voxel of weight W0 > 0 (derivation above)."""
    r = (W0 + ws) / W0
    return math.ceil(r + 1.0 + U * 32767.0 * (9.0 * r + 1.0)) - 1


def colour_bound(Wc0, wcs):
    rc = (Wc0 + wcs) / Wc0
    return math.ceil(rc + 1.0 + U * 255.0 * (9.0 * rc + 1.0)) - 1


def bounds(W0, ws, S):
    """depth_bound (S = 32767) / colour_bound (S = 255) on arrays (W0 > 0)."""
    r = (W0 + ws) / W0
    return np.ceil(r + 1.0 + U * S * (9.0 * r + 1.0)) - 1.0


def uncombine(res, dst):
    """`res` (the resampled voxels) taken out of `dst` (the resident voxels): (the new voxels, depth halves underweight,
    colour halves underweight) -- the inverse of ref_merge.combine, the two halves independent."""
    out = dst.copy()
    ws, W = res["w_depth"].astype(np.int64), dst["w_depth"].astype(np.int64)
    under_d = (ws != 0) & (W < ws)
    live = (ws != 0) & ~under_d
    rem = W - ws
    last, part = live & (rem == 0), live & (rem > 0)
    Fd = dst["sdf"].astype(F) / F(32767.0)
    Fs = res["sdf"].astype(F) / F(32767.0)
    num = W.astype(F) * Fd - ws.astype(F) * Fs
    with np.errstate(divide="ignore", invalid="ignore"):
        Fn = num / rem.astype(F)
    Fn = np.where(part, Fn, F(0))
    Fn = np.where(Fn < F(-1.0), F(-1.0), np.where(Fn > F(1.0), F(1.0), Fn)).astype(F)
    sdf = np.trunc(Fn * F(32767.0)).astype(np.int16)
    out["sdf"] = np.where(last, 32767, np.where(part, sdf, dst["sdf"]))
    out["w_depth"] = np.where(live, rem, W).astype(np.uint8)

    wcs, Wc = res["w_color"].astype(np.int64), dst["w_color"].astype(np.int64)
    under_c = (wcs != 0) & (Wc < wcs)
    live = (wcs != 0) & ~under_c
    rem = Wc - wcs
    last, part = live & (rem == 0), live & (rem > 0)
    v = (dst["clr"].astype(F) / F(255.0)) * Wc.astype(F)[..., None] - (res["clr"].astype(F) / F(255.0)) * wcs.astype(F)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = v / rem.astype(F)[..., None]
    v = np.where(part[..., None], v, F(0))
    v = np.where(v < F(0.0), F(0.0), np.where(v > F(1.0), F(1.0), v)).astype(F)
    nc = np.trunc(v * F(255.0)).astype(np.int64).astype(np.uint8)
    out["clr"] = np.where(last[..., None], 0, np.where(part[..., None], nc, dst["clr"]))
    out["w_color"] = np.where(live, rem, Wc).astype(np.uint8)
    return out, int(under_d.sum()), int(under_c.sum())


def target_counts(src, Xt, identity):
    """{target block: candidate voxels that name it} -- ref_merge.targets' candidates, counted per block."""
    live = src.live()
    pos = src.hash["pos"][live].astype(np.int64)
    vox = src.vba[src.hash["ptr"][live]]
    P = pos[:, None, :] * 8 + rm.LOCAL[None]
    t = np.floor(rm.to_map(Xt, identity, P.astype(F)) + F(0.5))
    use = (vox["w_depth"] > 0) & np.all((t >= -rm.RANGE) & (t < rm.RANGE), axis=-1)
    B = t[use].astype(np.int64) >> 3
    if not len(B):
        return {}
    uniq, n = np.unique(B, axis=0, return_counts=True)
    return {tuple(int(v) for v in b): int(k) for b, k in zip(uniq, n)}


def unmerge(src, dst, X, with_colour=1):
    """dslam_unmerge_maps: changes the voxel blocks of `dst` in place (nothing else of it) and returns the result fields."""
    assert src.vs == dst.vs and src.mu == dst.mu
    Xt, Yt, identity = rm.transforms(X, src.vs)
    best, n_live, n_cand, n_oor = rm.targets(src, Xt, identity)
    counts = target_counts(src, Xt, identity)
    assert set(counts) == set(best)
    res = dict(src_blocks=n_live, blocks_touched=0, src_candidates=n_cand, out_of_range=n_oor, candidates_without_block=0,
               voxels_changed=0, depth_underweight=0, colour_underweight=0)
    touched = set()
    for B in best:
        entry, _ = rm.lookup(dst, B)
        if entry is not None:
            touched.add(entry)
        else:
            res["candidates_without_block"] += counts[B]
    res["blocks_touched"] = len(touched)
    reader = rm.SourceReader(src)
    for entry in sorted(touched):
        e = dst.hash[entry]
        if e["ptr"] < 0:
            continue
        P = e["pos"].astype(np.int64)[None] * 8 + rm.LOCAL
        was = dst.vba[e["ptr"]]
        now, under_d, under_c = uncombine(rm.resample(reader, Yt, identity, P, with_colour), was)
        res["voxels_changed"] += int((now.view(np.uint64) != was.view(np.uint64)).sum())
        res["depth_underweight"] += under_d
        res["colour_underweight"] += under_c
        dst.vba[e["ptr"]] = now
    return res


ZERO_UNMERGE = dict(src_blocks=0, blocks_touched=0, src_candidates=0, out_of_range=0, candidates_without_block=0,
                    voxels_changed=0, depth_underweight=0, colour_underweight=0)
ZERO_MERGE = dict(passes=0, exhausted=0, src_blocks=0, blocks_allocated=0, blocks_touched=0, requests_unserved=0,
                  src_candidates=0, out_of_range=0, voxels_changed=0)


def remerge(src, dst, X_old, X_new, max_passes=0, with_colour=1):
    """dslam_remerge_maps: (unmerge result, merge result); nothing at all when the two transforms are bit-identical."""
    if np.asarray(X_old, F).tobytes() == np.asarray(X_new, F).tobytes():
        return dict(ZERO_UNMERGE), dict(ZERO_MERGE)
    un = unmerge(src, dst, X_old, with_colour=with_colour)
    return un, rm.merge(src, dst, X_new, max_passes=max_passes, with_colour=with_colour)


# ---------------------------------------------------------------------------------------------------------------------
# the round trip, voxel by voxel (test_unmerge_ref.py on the reference's bytes, test_gpu_unmerge.py on the device's)
# ---------------------------------------------------------------------------------------------------------------------
def check_round_trip(what, src, before, merged, after, X, with_colour=1):
    """`after` = `merged` with `src` taken out again under X, `merged` = `before` with `src` merged in: every property of
    the round trip, on every voxel of every resident block.  Returns the figures."""
    assert after.hash.tobytes() == merged.hash.tobytes(), f"{what}: the unmerge wrote the hash table"
    assert after.alloc_list.tobytes() == merged.alloc_list.tobytes() and after.excess_list.tobytes() == merged.excess_list.tobytes()
    assert (after.last_free, after.last_free_ex) == (merged.last_free, merged.last_free_ex)
    _, Yt, identity = rm.transforms(X, src.vs)
    reader = rm.SourceReader(src)
    live = merged.live()
    ptrs = merged.hash["ptr"][live]
    rest = np.setdiff1d(np.arange(len(merged.vba)), ptrs)
    assert after.vba[rest].tobytes() == before.vba[rest].tobytes(), f"{what}: a block outside the table changed"
    out = dict(voxels=0, observed=0, created=0, worst_sdf=0, worst_sdf_bound=0, worst_colour=0, coloured=0)
    for entry in live:
        e = merged.hash[entry]
        P = e["pos"].astype(np.int64)[None] * 8 + rm.LOCAL
        r = rm.resample(reader, Yt, identity, P, with_colour)
        old, new = before.vba[e["ptr"]], after.vba[e["ptr"]]
        ws, W0 = r["w_depth"].astype(np.int64), old["w_depth"].astype(np.int64)
        wcs, Wc0 = r["w_color"].astype(np.int64), old["w_color"].astype(np.int64)
        assert np.array_equal(new["w_depth"], old["w_depth"]), f"{what}: block {e['pos']}: a w_depth did not return"
        assert np.array_equal(new["w_color"], old["w_color"]), f"{what}: block {e['pos']}: a w_color did not return"
        idle = ws == 0
        assert new[idle].tobytes() == old[idle].tobytes(), f"{what}: a voxel the source gives nothing to changed"
        # observed before the merge: within the derived bound, no voxel excluded
        m = (W0 > 0) & ~idle
        diff = np.abs(new["sdf"].astype(np.int64) - old["sdf"].astype(np.int64))
        lim = bounds(np.maximum(W0, 1), ws, 32767.0)
        assert (diff[m] <= lim[m]).all(), (f"{what}: block {e['pos']}: raw sdf off by {diff[m].max()}, "
                                           f"bound {lim[m][np.argmax(diff[m] - lim[m])]}")
        if m.any():
            k = np.argmax(diff[m])
            if diff[m][k] >= out["worst_sdf"]:
                out["worst_sdf"], out["worst_sdf_bound"] = int(diff[m][k]), int(lim[m][k])
        # created by the merge: the empty depth half again
        c = (W0 == 0) & ~idle
        assert (new["sdf"][c] == 32767).all() and (new["w_depth"][c] == 0).all()
        whole = c & (Wc0 == 0) & (old["sdf"] == 32767) & ~old["clr"].any(axis=1)
        assert (new[whole].view(np.uint64) == np.uint64(32767)).all(), f"{what}: a voxel the merge created is not empty again"
        # colour
        mc = (Wc0 > 0) & (wcs > 0)
        cdiff = np.abs(new["clr"].astype(np.int64) - old["clr"].astype(np.int64)).max(axis=1)
        clim = bounds(np.maximum(Wc0, 1), wcs, 255.0)
        assert (cdiff[mc] <= clim[mc]).all(), f"{what}: block {e['pos']}: a colour channel off by {cdiff[mc].max()}"
        cc = (Wc0 == 0) & (wcs > 0)
        assert not new["clr"][cc].any(), f"{what}: a colour the merge created did not return to 0"
        same = wcs == 0
        assert new["clr"][same].tobytes() == old["clr"][same].tobytes()
        out["voxels"] += 512
        out["observed"] += int(m.sum())
        out["created"] += int(whole.sum())
        out["coloured"] += int(mc.sum())
        out["worst_colour"] = max(out["worst_colour"], int(cdiff[mc].max()) if mc.any() else 0)
    return out
