"""ref_merge.py alone, on the analytic pairs of register_fixtures.py: the sequential restatement of dslam_merge_maps' law
 has the properties the law promises.  No GPU."""
import functools
import types

import numpy as np

import analytic_maps as am
import ref64
import ref_merge as rm
import refmap
import register_fixtures as fx
import util
import weighted_fixtures as wf

I4 = fx.I4


def box():
    return fx.box_pair("small")


def empty_for(m, num_buckets=0x400, spare=4):
    n = len(m.block_pos)
    nx = 2 * n + (-(num_buckets + 2 * n)) % 16
    return rm.State.empty(num_buckets, nx, spare * n)


@functools.lru_cache(maxsize=None)
def merged_box():
    pair = box()
    src, dst = rm.State.of_map(pair.src_map), rm.State.of_map(pair.dst_map)
    before = dst.copy()
    res = rm.merge(src, dst, pair.X_true.astype(np.float32))
    return src, before, dst, res


def check_table(st):
    """The independent map model's invariants on a merged table."""
    params = types.SimpleNamespace(voxel_size=st.vs, mu=st.mu, frustum_min=0.05, frustum_max=5.0, num_buckets=st.num_buckets,
                                   num_excess=st.num_excess, num_local_blocks=st.num_local_blocks, use_swapping=0,
                                   history_words=0, max_w=st.max_w)
    snap = dict(hash=st.hash, alloc_list=st.alloc_list, excess_list=st.excess_list,
                stats=dict(last_free_block_id=st.last_free, last_free_excess_id=st.last_free_ex))
    util.check_invariants(snap, params)                      # slots and excess slots are partitions, positions unique
    model = refmap.MapModel(params, 8, 8)
    model.load(st.hash, st.alloc_list, st.last_free, st.excess_list, st.last_free_ex)
    occupied = np.flatnonzero(st.hash["ptr"] >= -1)
    assert len(model.index) == len(occupied)                 # no duplicate position
    reached = set()
    for head in range(st.num_buckets):
        if st.hash["ptr"][head] >= -1:
            chain = model.chain(head)
            assert all(model.bucket_of(t) == head for t in chain)
            reached.update(chain)
    assert reached == set(int(t) for t in occupied)          # chains closed: every occupied entry hangs off its bucket
    n = int((st.hash["ptr"] >= 0).sum())
    assert st.last_free == st.num_local_blocks - 1 - n       # pool tops = entries with a block
    assert st.last_free_ex == st.num_excess - 1 - int((st.hash["ptr"][st.num_buckets:] >= -1).sum())


def test_identity_onto_an_empty_map_reproduces_the_source():
    src = rm.State.of_map(box().src_map)
    dst = empty_for(box().src_map)
    res = rm.merge(src, dst, I4)
    a, b = src.voxels_by_position(), dst.voxels_by_position()
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert res["src_blocks"] == res["blocks_allocated"] == res["blocks_touched"] == 268 and res["exhausted"] == 0
    assert res["src_candidates"] == res["voxels_changed"] == 268 * 512
    check_table(dst)
    again = rm.merge(src, dst, I4)                           # now every block is a hit: one pass, weights double
    assert again["passes"] == 1 and again["blocks_allocated"] == 0 and again["blocks_touched"] == 268
    assert (np.concatenate(list(dst.voxels_by_position().values()))["w_depth"] == 2).all()


def test_weights_add_and_clamp():
    geom = am.Plane((0.1, 0.05, -1.0), -0.40)
    a = am.build_map(geom, am.VS, am.MU, (-0.15, -0.10, 0.2), (0.10, 0.10, 0.62), w_depth=3)
    b = am.build_map(geom, am.VS, am.MU, (-0.05, -0.10, 0.2), (0.20, 0.10, 0.62), w_depth=99)
    for X in (I4, fx.off_lattice(1.5, 0.45)):
        src, dst = rm.State.of_map(a), rm.State.of_map(b)
        before = dst.copy()
        rm.merge(src, dst, X)
        Xt, Yt, identity = rm.transforms(X, am.VS)
        reader = rm.SourceReader(src)
        seen = 0
        for entry in dst.live():
            e = dst.hash[entry]
            P = e["pos"].astype(np.int64)[None] * 8 + rm.LOCAL
            r = rm.resample(reader, Yt, identity, P, 1)
            old = before.vba[e["ptr"]] if before.hash["ptr"][entry] == e["ptr"] else np.full(512, reader.empty, am.VOXEL_DTYPE)
            want = np.minimum(old["w_depth"].astype(int) + r["w_depth"].astype(int), 100)
            assert np.array_equal(dst.vba[e["ptr"]]["w_depth"], want)
            seen += int((want == 100).sum())
        assert seen > 1000                                   # the clamp was reached


def test_merged_sdf_lies_between_its_inputs():
    src, before, dst, res = merged_box()
    pair = box()
    Xt, Yt, identity = rm.transforms(pair.X_true.astype(np.float32), am.VS)
    reader = rm.SourceReader(src)
    both = 0
    for entry in before.live():
        e = before.hash[entry]
        P = e["pos"].astype(np.int64)[None] * 8 + rm.LOCAL
        r = rm.resample(reader, Yt, identity, P, 1)
        old, new = before.vba[e["ptr"]], dst.vba[e["ptr"]]
        m = (r["w_depth"] > 0) & (old["w_depth"] > 0)
        lo = np.minimum(r["sdf"], old["sdf"]).astype(int) - 1   # float_to_sdf truncates toward zero: one raw step
        hi = np.maximum(r["sdf"], old["sdf"]).astype(int) + 1
        assert ((new["sdf"][m] >= lo[m]) & (new["sdf"][m] <= hi[m])).all()
        # ... and the float32 merge is one of the results the integer reading of the swap-in merge permits
        a, b, info = ref64.combine_stored(r, old, dst.max_w)
        ref64.check_combined(new, a, b, info, "merged block")
        both += int(m.sum())
    assert both > 50000


def test_merged_tables_pass_the_map_model():
    check_table(merged_box()[2])
    for pair in (fx.holes_pair(), fx.negative_pair()):
        dst = rm.State.of_map(pair.dst_map)
        res = rm.merge(rm.State.of_map(pair.src_map), dst, pair.X_true.astype(np.float32))
        assert res["exhausted"] == 0 and res["blocks_allocated"] > 100
        check_table(dst)


def test_64_buckets_need_three_passes_or_more():
    pair = box()
    dst = empty_for(pair.dst_map, num_buckets=0x40)
    res = rm.merge(rm.State.of_map(pair.src_map), dst, pair.X_true.astype(np.float32))
    assert res["passes"] >= 3 and res["exhausted"] == 0
    check_table(dst)
    stopped = empty_for(pair.dst_map, num_buckets=0x40)
    res2 = rm.merge(rm.State.of_map(pair.src_map), stopped, pair.X_true.astype(np.float32), max_passes=2)
    assert res2["passes"] == 2 and res2["exhausted"] == 1 and 0 < res2["blocks_allocated"] < res["blocks_allocated"]
    check_table(stopped)


def test_short_pools_report_what_was_not_served():
    src, before, full, res = merged_box()
    X = box().X_true.astype(np.float32)
    need = res["blocks_allocated"]
    assert need == 124
    dst = before.copy()
    dst.last_free = need - 7 - 1                            # 7 blocks short
    r = rm.merge(src, dst, X)
    # the pass in which the pool ran dry serves what is left; the next one serves nothing and reports the slots still
    # asked for: 7 blocks in 7 different slots here
    assert r["exhausted"] == 1 and r["blocks_allocated"] == need - 7 and r["requests_unserved"] == 7 and dst.last_free == -1
    dst = before.copy()
    dst.last_free_ex = 10 - 1                               # 10 excess slots: only chain-end requests go unserved
    r = rm.merge(src, dst, X)
    assert r["exhausted"] == 1 and dst.last_free_ex == -1 and dst.last_free >= 0
    # the first pass serves its 52 empty bucket heads and the first 10 chain ends; the second pass finds the remaining
    # 124 - 62 blocks at 62 different chain ends and can serve none of them
    assert r["passes"] == 2 and r["blocks_allocated"] == 62 and r["requests_unserved"] == 62
    a, b = full.voxels_by_position(), dst.voxels_by_position()
    assert set(b) < set(a) and all(a[k].tobytes() == b[k].tobytes() for k in b)   # what was served is the full merge's


def test_merging_the_counterpart_does_not_raise_the_error_to_the_analytic_sdf():
    src, before, dst, res = merged_box()
    pair = box()
    X = pair.X_true.astype(np.float32)
    geom = pair.dst_map.geom
    Xt, Yt, identity = rm.transforms(X, am.VS)
    reader = rm.SourceReader(src)
    err_merged, err_source = [], []
    for entry in dst.live():
        e = dst.hash[entry]
        P = e["pos"].astype(np.int64)[None] * 8 + rm.LOCAL
        new = dst.vba[e["ptr"]]
        old = before.vba[e["ptr"]] if before.hash["ptr"][entry] == e["ptr"] else np.full(512, reader.empty, am.VOXEL_DTYPE)
        changed = new.view(np.uint64) != old.view(np.uint64)
        if not changed.any():
            continue
        exact = np.clip(geom.sdf(P[changed] * am.VS) / am.MU, -1.0, 1.0)
        r = rm.resample(reader, Yt, identity, P[changed], 1)
        err_merged.append(np.abs(new["sdf"][changed] / 32767.0 - exact))
        err_source.append(np.abs(r["sdf"] / 32767.0 - exact))
    merged, source = float(np.concatenate(err_merged).mean()), float(np.concatenate(err_source).mean())
    print(f"mean |sdf - analytic| over {len(np.concatenate(err_merged))} changed voxels: merged {merged:.6f}, "
          f"resampled from the source alone {source:.6f} (units of mu)")
    assert merged <= source


# ---------------------------------------------------------------------------------------------------------------------
# weights that vary from voxel to voxel: the smallest of the 8 taps' weights, the two gates
# ---------------------------------------------------------------------------------------------------------------------
def weighted_transforms():
    shift = np.eye(4, dtype=np.float32)
    shift[:3, 3] = np.array((3, -5, 2), np.float64) * am.VS
    return {"identity": I4, "translation": shift, "off_lattice": fx.off_lattice(1.5, 0.45)}


def test_weighted_pair_minimum_of_the_taps_and_both_gates():
    """ref_merge.merge alone on weighted_fixtures.weighted_planes (source w_depth 1 .. 7 with unobserved voxels inside its
    blocks, w_color 0 .. 3; destination w_depth up to 99) under the identity, a whole-voxel translation and an off-lattice
    transform: on a sample, voxel by voxel in a plain loop over the stored source voxels, w_depth' = min(w_dst + the smallest
    w_depth of the taps, max_w) and the colour half idles exactly where a tap has no w_color; over all voxels
    (weighted_fixtures.merge_outcomes) the same, and each outcome the GPU cases rely on occurs at least 1000 times."""
    a, b = wf.weighted_planes()
    stored = {tuple(int(v) for v in pos): vox for pos, vox in zip(a.block_pos, a.voxels)}
    for name, X in weighted_transforms().items():
        src, dst = rm.State.of_map(a), rm.State.of_map(b)
        before = dst.copy()
        res = rm.merge(src, dst, X)
        assert res["exhausted"] == 0
        check_table(dst)
        counts = wf.merge_outcomes(a, before, dst, X)
        print(f"{name}: {res['voxels_changed']} voxels changed, {counts}")
        assert counts["changed"] == res["voxels_changed"]
        assert min(counts[k] for k in ("changed", "gated", "colour_live", "colour_idle")) >= 1000 and counts["clamped"] > 0, counts
        # the sample, tap by tap
        _, Yt, identity = rm.transforms(X, am.VS)
        live = dst.live()
        rng = np.random.default_rng(3)
        gated = idle = 0
        for entry, l in zip(live[rng.integers(0, len(live), 1500)], rng.integers(0, 512, 1500)):
            e = dst.hash[entry]
            P = e["pos"].astype(np.int64) * 8 + rm.LOCAL[l]
            if identity:
                taps = [tuple(P)]
            else:
                q = rm.to_map(Yt, False, P.astype(np.float32)[None])[0]
                x0, y0, z0 = (int(np.floor(v)) for v in q)
                taps = [(x0 + dx, y0 + dy, z0 + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
            wds, wcs = [], []
            for x, y, z in taps:
                vox = stored.get((x >> 3, y >> 3, z >> 3))
                v = None if vox is None else vox[(x & 7) + 8 * (y & 7) + 64 * (z & 7)]
                wds.append(0 if v is None else int(v["w_depth"]))
                wcs.append(0 if v is None else int(v["w_color"]))
            r = min(wds)
            old = before.vba[e["ptr"]][l] if before.hash["ptr"][entry] == e["ptr"] else None
            old_w = 0 if old is None else int(old["w_depth"])
            new = dst.vba[e["ptr"]][l]
            assert int(new["w_depth"]) == min(old_w + r, 100), (name, P, wds)
            unchanged = (old is None and int(new["w_color"]) == 0 and not new["clr"].any()) or \
                        (old is not None and new["clr"].tobytes() == old["clr"].tobytes() and new["w_color"] == old["w_color"])
            assert unchanged == (r == 0 or min(wcs) == 0), (name, P, wds, wcs)
            gated += r == 0 and max(wds) > 0
            idle += r > 0 and min(wcs) == 0
        assert idle > 50 and (identity or gated > 50), (gated, idle)   # (the clamp: counts["clamped"], over all voxels)
