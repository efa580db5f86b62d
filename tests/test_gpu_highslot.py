"""Every voxel access at pool slots above 2 GiB and near 4 GiB (fixtures and the law in highslot_fixtures.py).

A kernel reaches a block at byte 4096 * ptr of the voxel pool, and before this file no test had a pool above 1 GiB.  Here
maps live in a pool of POOL = DSLAM_MAX_LOCAL_BLOCKS slots with their blocks in the lowest slots, either side of byte 2^31
and in the last slots below 2^32, neighbours in different bands.  Two kinds of checks:

* the float64 check bodies of ref64_checks.py and test_gpu_track_sdf.py run unchanged on relocated maps;
* the law "no result depends on which slots hold the blocks": the same calls on a low twin (the small pool the existing
  fixtures use, which the rest of the suite pins to float64 and oracle references) and on the POOL scene give byte-identical
  outputs and equal slot-free states (highslot_fixtures.canonical).

At most two POOL scenes (4 GiB each) are alive at any time; every test closes its own.  Voxels of a POOL scene only ever
travel by slot run."""
import contextlib

import numpy as np
import pytest

import analytic_maps as am
import highslot_fixtures as hs
import ref64_checks as rc
import refvoxel_checks as rv
import register_fixtures as rf
import test_gpu_track_sdf as tts
import track_sdf_fixtures as tf
import util

pytestmark = pytest.mark.gpu

IMAGES = ("DEPTH", "SHADED", "COLOUR_FROM_VOLUME", "COLOUR_FROM_NORMAL")
N_FUSE = 0x2000          # allocations the banded list of a fusion scene deals (the low twin's whole pool)
MAX_TRIANGLES = 1 << 17  # passed explicitly: the default of 32 per pool slot would depend on the pool


@contextlib.contextmanager
def closing(*handles):
    try:
        yield handles
    finally:
        for h in handles:
            h.close()


def high_scene(gpu, pkg, m, **over):
    """Map `m` relocated into a POOL scene; the fixture's teeth are asserted on what the engine holds."""
    r = hs.relocate(m)
    scene = gpu.create_scene(r.scene_params(pkg, **over))
    hs.upload_sparse(gpu, scene, r)
    hs.scene_teeth(gpu, scene)
    return scene


def low_scene(gpu, pkg, m, **over):
    scene = gpu.create_scene(m.scene_params(pkg, **over))
    am.upload(gpu, scene, m)
    return scene


def reads(gpu, pkg, scene, rs, M, intr):
    """(c) every read of one map: name -> bytes-comparable array."""
    out = {}
    for name in IMAGES:
        out[name] = gpu.get_image(scene, rs, M, intr, getattr(pkg, "IMAGE_" + name)).copy()
    out["list after GetImage"] = gpu.download_visible_ids(rs)
    out["range after GetImage"] = gpu.download_range_image(rs)
    gpu.find_visible_blocks(scene, rs, M, intr)
    out["visible ids"], out["visible types"] = gpu.download_visible_ids(rs), gpu.download_visible_types(rs)
    gpu.create_expected_depths(scene, rs, M, intr)
    out["range image"] = gpu.download_range_image(rs)
    out["ICP points"], out["ICP normals"] = gpu.create_icp_maps(scene, rs, M, intr)
    out["tracking raycast"] = gpu.download_raycast_image(rs)
    out["raycast result"] = gpu.download_raycast_result(rs)
    out["depth int16"] = gpu.get_depth_image_int16(scene, rs, M, intr, 1000)
    out["mesh"], out["mesh colours"] = gpu.mesh_scene(scene, MAX_TRIANGLES, colour=True)
    assert len(out["mesh"]) < MAX_TRIANGLES - 1
    return out


def assert_same_outputs(low, high, what):
    assert sorted(low) == sorted(high)
    for k in low:
        a, b = np.asarray(low[k]), np.asarray(high[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {k} differs between the low twin and the POOL scene"


# ---------------------------------------------------------------------------------------------------------------------
# h. the limit
# ---------------------------------------------------------------------------------------------------------------------
def test_the_pool_limit(pkg, gpu):
    p = dict(voxel_size=0.005, mu=0.02, max_w=100, frustum_min=0.2, frustum_max=3.0, num_buckets=0x400, num_excess=0x100)
    ext = gpu.device_alloc(4096)   # never touched: the refusal comes before anything looks at the buffer
    try:
        for buf in (None, ext):
            with pytest.raises(pkg.DslamError, match=r"status -1 .*DSLAM_MAX_LOCAL_BLOCKS \(1048576 blocks"):
                gpu.create_scene(pkg.SceneParams(num_local_blocks=hs.POOL + 1, **p), buf)
    finally:
        gpu.device_free(ext)
    with closing(gpu.create_scene(pkg.SceneParams(num_local_blocks=hs.POOL, **p))) as (s,):
        assert s.params.num_local_blocks == hs.POOL == 0x100000
        st = gpu.stats(s)
        assert st["last_free_block_id"] == hs.TOP and st["num_allocated_blocks"] == hs.POOL


# ---------------------------------------------------------------------------------------------------------------------
# the float64 check bodies on relocated maps
# ---------------------------------------------------------------------------------------------------------------------
class Closing:
    """The engine with every scene it creates remembered, so that a check body's POOL scenes can be closed after it."""

    def __init__(self, api):
        self._api, self.made = api, []

    def __getattr__(self, name):
        return getattr(self._api, name)

    def create_scene(self, *a, **kw):
        s = self._api.create_scene(*a, **kw)
        self.made.append(s)
        return s

    def close_scenes(self):
        for s in self.made:
            s.close()
        self.made = []


@pytest.fixture
def tracked(gpu):
    t = Closing(gpu)
    yield t
    t.close_scenes()


def test_raycast_against_float64_on_a_relocated_map(pkg, tracked):
    build, W, H, cam, colour = rc.raycast_cases()["colour_plane"]
    m = hs.relocate(build())
    print(hs.teeth(m.block_pos, m.ptrs))
    M, intr = rc.camera(W, H, **cam)
    print(rc.check_raycast(tracked, pkg, m, M, intr, W, H, colour=True, icp=True))


def test_mesh_against_float64_on_a_relocated_map(pkg, tracked):
    build, bound = rc.mesh_cases()["sphere_outside"]
    m = hs.relocate(build())
    print(hs.teeth(m.block_pos, m.ptrs))
    print(rc.check_mesh(tracked, pkg, m, surface_bound=bound, max_triangles=MAX_TRIANGLES))


def test_integration_against_float64_in_a_banded_pool(pkg, synth, tracked):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl, num_local_blocks=hs.POOL)
    print(rc.check_integration(tracked, pkg, wl, range(4), p, deintegrate=(1, 2), alloc_list=hs.banded_alloc_list(N_FUSE),
                               live_only=True))
    print(hs.scene_teeth(tracked, tracked.made[0]))


def test_track_sdf_evaluation_against_float64_on_relocated_maps(pkg, tracked):
    """three_maps with its first and its last map relocated (two POOL scenes), the middle one as the fixture has it."""
    f = tf.three_maps()
    scenes = [high_scene(tracked, pkg, f.maps[0]), tts.upload_map(tracked, pkg, f.maps[1]), high_scene(tracked, pkg, f.maps[2])]
    view = tracked.create_view(f.w, f.h)
    tracked.view_update(view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    ev, _, _ = tts.check_evaluation(pkg, tracked, lambda _: (scenes, view), f, f.start(2.0, 0.3))
    assert ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates


# ---------------------------------------------------------------------------------------------------------------------
# c. reads of one map
# ---------------------------------------------------------------------------------------------------------------------
READ_CASES = ("colour_plane", "box_corner", "sphere_inside")


@pytest.mark.parametrize("case", sorted(READ_CASES))
def test_reads_of_one_map(pkg, gpu, case):
    build, W, H, cam, _ = rc.raycast_cases()[case]
    m = build()
    M, intr = rc.camera(W, H, **cam)
    low = low_scene(gpu, pkg, m)
    want = reads(gpu, pkg, low, gpu.create_render_state(low, W, H), M, intr)
    assert (want["DEPTH"] > 0).sum() > 0.1 * W * H and len(want["mesh"]) > 1000 and len(want["visible ids"]) > 50
    with closing(high_scene(gpu, pkg, m)) as (high,):
        got = reads(gpu, pkg, high, gpu.create_render_state(high, W, H), M, intr)
        assert_same_outputs(want, got, case)
        hs.assert_same_canonical(hs.canonical(gpu, low), hs.canonical(gpu, high), f"{case} after the reads")


# ---------------------------------------------------------------------------------------------------------------------
# a. fusion and upkeep
# ---------------------------------------------------------------------------------------------------------------------
class Twins:
    """The same calls on a low scene and on a POOL scene; after each, equal canonical states and equal reads."""

    def __init__(self, gpu, pkg, wl_size, start, **params):
        self.gpu, self.pkg, (self.W, self.H) = gpu, pkg, wl_size
        low = dict(params)
        low.setdefault("num_local_blocks", N_FUSE)
        self.scenes = [gpu.create_scene(pkg.SceneParams(**low)),
                       gpu.create_scene(pkg.SceneParams(**dict(params, num_local_blocks=hs.POOL)))]
        if start == "banded":
            gpu.upload_scene_state(self.scenes[1], allocation_list=hs.banded_alloc_list(N_FUSE), last_free_block_id=hs.TOP)
        self.rs = [gpu.create_render_state(s, self.W, self.H) for s in self.scenes]
        self.views = [gpu.create_view(self.W, self.H) for _ in self.scenes]

    def close(self):
        self.scenes[1].close()

    def each(self, fn):
        """fn(scene, rs, view) on both; its results must be equal bytes."""
        out = [fn(s, r, v) for s, r, v in zip(self.scenes, self.rs, self.views)]
        if out[0] is not None:
            assert_same_outputs(*out, "a call's outputs")
        return out[0]

    def compare(self, what, M=None, intr=None):
        c = [hs.canonical(self.gpu, s, r) for s, r in zip(self.scenes, self.rs)]
        hs.assert_same_canonical(*c, what)
        if M is not None:
            free = [self.gpu.create_render_state(s, self.W, self.H) for s in self.scenes]   # (the fusion list stays as it is)
            out = [reads(self.gpu, self.pkg, s, r, M, intr) for s, r in zip(self.scenes, free)]
            assert_same_outputs(*out, what)
            assert (out[0]["DEPTH"] > 0).sum() > 100, f"{what}: the camera sees nothing"
            for r in free:
                r.close()
        return c[0]


@pytest.mark.parametrize("start", ["banded", "fresh"])
def test_fusion_and_upkeep(pkg, synth, gpu, start):
    """Four frames, a re-integration batch over three stored keyframes, six more frames with the window following, decay in
    both modes, and two frames into the slots the upkeep freed.  `fresh`: a plain new POOL scene, whose blocks land at TOP
    downwards."""
    wl = synth.s_tiny(61, 47)
    kw = dict(num_buckets=0x4000, num_excess=0x800, **wl.scene_kwargs)
    t = Twins(gpu, pkg, (wl.W, wl.H), start, **kw)
    try:
        stores = [gpu.create_frame_store(wl.W, wl.H, 4) for _ in t.scenes]
        for s, fs in zip(t.scenes, stores):
            gpu.frame_store_enable_lists(fs, s)
        frames = [wl.frame(2 * i) for i in range(12)]   # 4 degrees of yaw apart
        for i in range(4):
            rgba, mm, M = frames[i]

            def fuse(scene, rs, view):
                fs = stores[t.scenes.index(scene)]
                gpu.view_update(view, rgba, mm, timestamp=float(i))
                gpu.frame_store_put_view(fs, i, view)
                gpu.process_frame(scene, view, rs, M, wl.intr)
                gpu.frame_store_put_visible_list(fs, i, scene, rs)
            t.each(fuse)
            t.compare(f"{start}: frame {i}", M, wl.intr)
        figures = hs.scene_teeth(gpu, t.scenes[1]) if start == "banded" else None
        live = hs.canonical(gpu, t.scenes[1])["slots"]
        if start == "fresh":
            assert live.max() == hs.TOP and live.min() == hs.TOP - len(live) + 1 and len(live) > 100
        print(f"{start}: {len(live)} live blocks, {figures}")
        # the keyframes 1 .. 3 corrected by a small motion, in one batch
        old = [frames[k][2] for k in (1, 2, 3)]
        D = np.eye(4, dtype=np.float32)
        D[:3, 3] = (0.01, -0.005, 0.008)
        new = [(D @ M).astype(np.float32) for M in old]
        t.each(lambda scene, rs, view: gpu.reintegrate_batch(scene, view, rs, stores[t.scenes.index(scene)], [1, 2, 3], old, new,
                                                             wl.intr))
        t.compare(f"{start}: reintegrate_batch", frames[3][2], wl.intr)
        # the camera moves on, the window follows it (as util.run_sequence slides: whenever more than three lists wait)
        def fuse_on(i, slide):
            rgba, mm, M = frames[i]

            def call(scene, rs, view):
                gpu.view_update(view, rgba, mm, timestamp=float(i))
                gpu.process_frame(scene, view, rs, M, wl.intr)
                if slide and gpu.stats(scene, rs)["fusion_fifo_len"] > 3:
                    gpu.slide_window(scene, rs, 3)
            t.each(call)
        for i in range(4, 10):
            fuse_on(i, True)
            c = t.compare(f"{start}: frame {i} and slide_window")
        assert c["counters"]["slid_block_count"] > 0, "the window released nothing"
        t.compare(f"{start}: reads after the window", frames[9][2], wl.intr)
        for force in (False, True):
            t.each(lambda scene, rs, view: gpu.decay(scene, rs, 2, 1, force))
            c = t.compare(f"{start}: decay, force_all_voxels {force}", frames[9][2], wl.intr)
        assert c["counters"]["decayed_block_count"] > 0, "decay released nothing"
        for i in (10, 11):   # into the slots the upkeep freed
            fuse_on(i, False)
        t.compare(f"{start}: frames after the upkeep", frames[11][2], wl.intr)
    finally:
        t.close()


FORMS = {"plain": (100, 0), "depth_weights": (255, 1), "two_cameras": (100, 2), "stop": (4, 3), "deprocess": (100, 1),
         "deprocess_stop": (4, 2)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_voxel_update_forms(pkg, gpu, form):
    """One case of each voxel-update form of refvoxel_checks: its crafted measurement and crafted voxels (random and edge
    rows) on both twins, then the one call."""
    max_w, pose_k = FORMS[form]
    assert form in rv.FORMS
    twins = []
    try:
        for pool, banded in ((0x800, False), (hs.POOL, True)):
            api = _BandedApi(gpu, banded)
            twins.append(api)
            api.case = rv.Case(api, pkg, max_w, rv.MU_STEPS[0], form, pose_k, num_local_blocks=pool)
            api.case.call()
        lo, hi = twins
        assert len(lo.case.ptrs) == len(hi.case.ptrs) >= 200 and lo.case.crafted.tobytes() == hi.case.crafted.tobytes()
        assert lo.case.conditions() == hi.case.conditions()
        print(form, hs.scene_teeth(gpu, hi.case.scene))
        hs.assert_same_canonical(hs.canonical(gpu, lo.case.scene, lo.case.rs), hs.canonical(gpu, hi.case.scene, hi.case.rs), form)
        # and the low twin against the exact reference, as test_gpu_voxel_update.py has it: the law carries it to the POOL scene
        lo.case.check()
    finally:
        for api in twins:
            if api.pool_scene is not None:
                api.pool_scene.close()


class _BandedApi:
    """The engine as refvoxel_checks.Case uses it, for a pool of any size: a new scene of POOL blocks starts from the banded
    allocation list, and the whole-pool download / upload with which Case plants its crafted voxels moves the live blocks
    only, by slot run (the rows of every other slot are the fresh pool's and are not written back)."""

    def __init__(self, api, banded):
        self._api, self.banded, self.pool_scene, self.live = api, banded, None, None

    def __getattr__(self, name):
        return getattr(self._api, name)

    def create_scene(self, params):
        s = self._api.create_scene(params)
        if params.num_local_blocks == hs.POOL:
            self.pool_scene = s
            if self.banded:
                self._api.upload_scene_state(s, allocation_list=hs.banded_alloc_list(N_FUSE), last_free_block_id=hs.TOP)
        return s

    def download_voxel_blocks(self, scene, first=0, count=None):
        if scene is not self.pool_scene:
            return self._api.download_voxel_blocks(scene, first, count)
        h = self._api.download_hash_table(scene)
        self.live = np.sort(h["ptr"][h["ptr"] >= 0].astype(np.int64))
        return hs.SparsePool.download(self._api, scene, self.live)

    def upload_voxel_blocks(self, scene, first, blocks):
        if scene is not self.pool_scene:
            return self._api.upload_voxel_blocks(scene, first, blocks)
        assert first == 0 and isinstance(blocks, hs.SparsePool)
        blocks.upload(self._api, scene)


# ---------------------------------------------------------------------------------------------------------------------
# b. swapping
# ---------------------------------------------------------------------------------------------------------------------
def test_swapping(pkg, synth, gpu):
    """Swap out, swap in, flush and re-allocation with the blocks in the bands: eight frames on a swapping scene (every
    ProcessFrame swaps in what the view needs and out what left it), SaveToGlobalMemory after the sixth."""
    wl = synth.s_tiny(61, 47)
    t = Twins(gpu, pkg, (wl.W, wl.H), "banded", num_buckets=0x4000, num_excess=0x800, use_swapping=1, **wl.scene_kwargs)
    try:
        for i in range(8):
            rgba, mm, M = wl.frame(2 * i)

            def fuse(scene, rs, view):
                gpu.view_update(view, rgba, mm, timestamp=float(i))
                gpu.process_frame(scene, view, rs, M, wl.intr)
                if i == 5:
                    gpu.save_to_global_memory(scene)
            t.each(fuse)
            c = t.compare(f"swapping: frame {i}")
            if i == 3:
                print(hs.scene_teeth(gpu, t.scenes[1]))
        out = np.nonzero(c["table"]["ptr"] == -1)[0]
        assert len(out) >= 8, f"{len(out)} blocks are swapped out at the end"
        for e in out:
            a, b = (gpu.download_stored_block(s, int(e)) for s in t.scenes)
            assert a[0] and b[0] and a[1].tobytes() == b[1].tobytes(), f"stored block of entry {e}"
        t.compare("swapping: reads at the end", wl.frame(14)[2], wl.intr)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. reads of several maps
# ---------------------------------------------------------------------------------------------------------------------
def multi_reads(gpu, pkg, f, scenes, T, rs, view):
    out = {}
    for name in IMAGES:
        out[name] = gpu.get_image_multi(scenes, T, rs, f.M_true, f.intr, getattr(pkg, "IMAGE_" + name)).copy()
    out["mesh"], out["mesh colours"], out["mesh counts"] = gpu.mesh_scene_multi(scenes, T, MAX_TRIANGLES, colour=True)
    params = pkg.TrackSdfParams(**tf.RUN_PARAMS)
    out["tracked pose"], res = gpu.track_camera_sdf(view, scenes, T, f.start(), f.intr, params)
    out["tracking result"] = np.frombuffer(bytes(res), np.uint8)
    out["tracking sums"] = gpu.debug_track_sdf_sums()
    starts = np.stack([f.start(), f.start(2.0, 0.3), f.M_true])
    scores = gpu.score_camera_poses(view, scenes, T, starts, f.intr)
    out["scores"] = np.frombuffer(bytes(scores), np.uint8)
    out["poses of the starts"], res = gpu.track_camera_sdf_starts(view, scenes, T, starts, f.intr, params)
    out["results of the starts"] = np.frombuffer(bytes(res), np.uint8)
    out["sums of the starts"] = np.stack([gpu.debug_track_sdf_start_sums(k) for k in range(len(starts))])
    if len(scenes) > 1:
        for k, a in enumerate(gpu.survey_overlaps(scenes, T)):
            out[f"overlap survey {k}"] = a
    views = [pkg.SurveyView.of(f.M_true, f.intr, f.w, f.h, 0.05, 5.0), pkg.SurveyView.of(f.start(40.0, 6.0), f.intr, f.w, f.h, 0.3, 0.0)]
    for k, a in enumerate(gpu.survey_views(scenes, T, views)):
        out[f"view survey {k}"] = a
    return out


@pytest.mark.parametrize("high", ["first", "last", "alone"])
def test_reads_of_several_maps(pkg, gpu, high):
    f = tf.three_maps()
    pick = [0] if high == "alone" else [0, 1, 2]
    hi_at = 2 if high == "last" else 0
    T = [f.T[i] for i in pick]
    low = [low_scene(gpu, pkg, f.maps[i]) for i in pick]
    view = gpu.create_view(f.w, f.h)
    gpu.view_update(view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    want = multi_reads(gpu, pkg, f, low, T, gpu.create_render_state(max(low, key=lambda s: s.params.num_local_blocks), f.w, f.h), view)
    assert (want["DEPTH"] > 0).sum() > 1000 and want["mesh counts"].min() > 0
    with closing(high_scene(gpu, pkg, f.maps[hi_at])) as (h,):
        mixed = list(low)
        mixed[pick.index(hi_at)] = h
        got = multi_reads(gpu, pkg, f, mixed, T, gpu.create_render_state(h, f.w, f.h), view)
        assert_same_outputs(want, got, f"the high map {high}")


@pytest.mark.parametrize("high", ["src", "dst", "both"])
def test_register_maps(pkg, gpu, high):
    pair = rf.box_pair("small")
    X0 = rf.off_lattice()
    lo = [low_scene(gpu, pkg, pair.src_map), low_scene(gpu, pkg, pair.dst_map)]
    X, res = gpu.register_maps(lo[0], lo[1], X0)
    want = dict(X=X, result=np.frombuffer(bytes(res), np.uint8), sums=gpu.debug_register_sums())
    assert pair.distance(X) < 0.25 * pair.distance(X0)
    with closing(*[high_scene(gpu, pkg, m) for m, w in ((pair.src_map, "src"), (pair.dst_map, "dst")) if high in (w, "both")]) as hi:
        hi = list(hi)
        src = hi.pop(0) if high in ("src", "both") else lo[0]
        dst = hi.pop(0) if high in ("dst", "both") else lo[1]
        X, res = gpu.register_maps(src, dst, X0)
        assert_same_outputs(want, dict(X=X, result=np.frombuffer(bytes(res), np.uint8), sums=gpu.debug_register_sums()),
                            f"register_maps, {high} high")


@pytest.mark.parametrize("high", ["first", "last"])
def test_register_graph(pkg, gpu, high):
    import register_graph_fixtures as gf
    name, pairs, anchor = gf.CASES["triangle"]
    ms = gf.map_set(name)
    starts = gf.off_lattice_starts()

    def run(scenes):
        T, res, pres = gpu.register_graph(scenes, starts, pairs, anchor)
        out = dict(T=T, result=np.frombuffer(bytes(res), np.uint8))
        for k, p in enumerate(pres):
            out[f"pair {k}"] = np.frombuffer(bytes(p), np.uint8)
            out[f"sums {k}"] = gpu.debug_register_graph_sums(k)
        return out
    lo = [low_scene(gpu, pkg, m) for m in ms.maps]
    want = run(lo)
    at = 0 if high == "first" else len(lo) - 1
    with closing(high_scene(gpu, pkg, ms.maps[at])) as (h,):
        mixed = list(lo)
        mixed[at] = h
        assert_same_outputs(want, run(mixed), f"register_graph, the high map {high}")


# ---------------------------------------------------------------------------------------------------------------------
# e. writes across maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("high", ["src", "dst", "both"])
def test_merge_unmerge_remerge(pkg, gpu, high):
    pair = rf.box_pair("small")
    X = pair.X_true.astype(np.float32)
    X2 = rf.near_truth(pair)

    def run(src, dst):
        out = []
        r = gpu.merge_maps(src, dst, X)
        out.append((dict(result=np.frombuffer(bytes(r), np.uint8)), hs.canonical(gpu, dst)))
        un, re = gpu.remerge_maps(src, dst, X, X2)
        out.append((dict(un=np.frombuffer(bytes(un), np.uint8), re=np.frombuffer(bytes(re), np.uint8)), hs.canonical(gpu, dst)))
        r = gpu.unmerge_maps(src, dst, X2)
        out.append((dict(result=np.frombuffer(bytes(r), np.uint8)), hs.canonical(gpu, dst)))
        out.append((dict(), hs.canonical(gpu, src)))
        return out
    want = run(low_scene(gpu, pkg, pair.src_map), low_scene(gpu, pkg, pair.dst_map))
    assert want[0][1]["counters"]["blocks_in_use"] > len(pair.dst_map.block_pos), "the merge allocated nothing"
    with closing(*[high_scene(gpu, pkg, m) for m, w in ((pair.src_map, "src"), (pair.dst_map, "dst")) if high in (w, "both")]) as hi:
        hi = list(hi)
        src = hi.pop(0) if high in ("src", "both") else low_scene(gpu, pkg, pair.src_map)
        dst = hi.pop(0) if high in ("dst", "both") else low_scene(gpu, pkg, pair.dst_map)
        got = run(src, dst)
        for step, ((wr, wc), (gr, gc)) in enumerate(zip(want, got)):
            assert_same_outputs(wr, gr, f"{high} high, step {step}")
            hs.assert_same_canonical(wc, gc, f"{high} high, step {step}")


# ---------------------------------------------------------------------------------------------------------------------
# f. pack and unpack
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack(pkg, gpu):
    build, W, H, cam, _ = rc.raycast_cases()["colour_plane"]
    m = build()
    M, intr = rc.camera(W, H, **cam)
    low = low_scene(gpu, pkg, m)
    total = gpu.pack_scene(low).total_bytes
    bufs = [gpu.host_alloc((total,), np.uint8) for _ in range(2)]
    try:
        gpu.pack_scene(low, bufs[0].ctypes.data, total)
        want = reads(gpu, pkg, low, gpu.create_render_state(low, W, H), M, intr)
        with closing(high_scene(gpu, pkg, m)) as (high,):
            info = gpu.pack_scene(high, bufs[1].ctypes.data, total)
            assert info.total_bytes == total and info.blocks == len(m.block_pos)
            assert bufs[0].tobytes() == bufs[1].tobytes(), "the packed image depends on the slots"
        with closing(gpu.create_scene(m.scene_params(pkg, num_local_blocks=hs.POOL))) as (fresh,):
            gpu.unpack_scene(fresh, bufs[1].ctypes.data, total)
            c = hs.canonical(gpu, fresh)
            n = len(m.block_pos)
            assert np.array_equal(np.sort(c["slots"]), np.arange(hs.POOL - n, hs.POOL)), "the blocks do not sit at TOP downwards"
            got = reads(gpu, pkg, fresh, gpu.create_render_state(fresh, W, H), M, intr)
            assert_same_outputs(want, got, "reads of the unpacked POOL scene")
            low2 = gpu.create_scene(m.scene_params(pkg))
            gpu.unpack_scene(low2, bufs[0].ctypes.data, total)
            hs.assert_same_canonical(hs.canonical(gpu, low2), c, "unpacked")
    finally:
        for b in bufs:
            gpu.host_free(b)


# ---------------------------------------------------------------------------------------------------------------------
# g. the shard exchange
# ---------------------------------------------------------------------------------------------------------------------
def _signatures(slots, replica):
    """shard_fixtures.signatures for the named slots only: voxel v of block s on replica q holds q << 48 | s << 16 | v."""
    s = np.asarray(slots, np.uint64)[:, None]
    return (np.uint64(replica) << np.uint64(48)) | (s << np.uint64(16)) | np.arange(512, dtype=np.uint64)[None, :]


def test_shard_exchange_in_the_bands(pkg, gpu):
    """refshard_checks.check_exchange's plan, pack and unpack against the law of ref_shard.py on a POOL scene whose dirty set
    lies in all three bands, four shards of 16-slot chunks.  shard_fixtures.Crafted gives every slot of the pool an entry and
    a signature block, which a host cannot hold for POOL slots; here the dirty slots have entries, and they, the holes
    between them and two slots beyond each end of a band hold signature blocks: the slots a wrong pack or unpack would read
    or write first."""
    import ref_shard as law
    import refshard_checks as chk
    import shard_fixtures as sf
    n, shards, chunk = hs.POOL, 4, 16
    assert law.valid_layout(n, shards, chunk)
    spans = [(0, 44), (hs.M31 - 22, hs.M31 + 22), (hs.POOL - 44, hs.POOL)]
    dirty = np.concatenate([np.arange(a, b) for a, b in spans])
    dirty = dirty[np.arange(len(dirty)) % 5 != 3]                       # holes: clean slots between dirty ones
    known = np.unique(np.concatenate([np.arange(max(a - 2, 0), min(b + 2, n)) for a, b in spans]))
    lists, counts = law.plan(set(dirty.tolist()), n, shards, chunk)
    for slots in lists:                                                 # every shard owns dirty slots in two bands or more
        assert len(np.unique(hs.band_of(slots, 64))) >= 2 and len(slots) >= 8
    assert {0, hs.M31 - 1, hs.M31, hs.TOP} <= set(dirty.tolist())
    p = pkg.SceneParams(voxel_size=0.02, mu=0.08, max_w=100, frustum_min=0.2, frustum_max=3.0, num_local_blocks=n,
                        num_buckets=sf.NUM_BUCKETS, num_excess=sf.NUM_EXCESS, history_words=1)
    W, H = 16, 12
    with closing(gpu.create_scene(p)) as (scene,):
        rs, view = gpu.create_render_state(scene, W, H), gpu.create_view(W, H)
        gpu.view_update(view, np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.int16))
        table = gpu.download_hash_table(scene)
        where = np.random.default_rng(5).choice(sf.NUM_BUCKETS, len(dirty) + 2, replace=False)
        entries, no_block = where[:len(dirty)], where[len(dirty):]
        table["ptr"][entries] = dirty
        table["ptr"][no_block] = (-1, -2)
        k = np.arange(len(where))
        table["pos"][where] = np.stack([k % 16 - 8, (k // 16) % 16 - 8, 10 + k // 256], 1)
        # checked before anything is uploaded: an out-of-range ptr would index the pool out of bounds on the device
        ptr = table["ptr"].astype(np.int64)
        assert np.array_equal(np.sort(ptr[ptr >= 0]), dirty) and (ptr >= -2).all() and (ptr < n).all()
        gpu.upload_scene_state(scene, hash_table=table, allocation_list=np.zeros(n, np.int32), last_free_block_id=-1)
        pool = hs.SparsePool(known, _signatures(known, 0))
        pool.upload(gpu, scene)
        gpu.track_dirty(scene, True)
        ids = np.concatenate([entries, no_block]).astype(np.int32)
        np.random.default_rng(9).shuffle(ids)
        for part in (ids[:len(ids) // 2], ids[len(ids) // 2:]):
            gpu.upload_visible_ids(rs, part)
            gpu.integrate_into_scene(scene, view, rs, np.eye(4, dtype=np.float32), np.array([20.0, 20.0, 7.5, 5.5], np.float32))
        assert np.array_equal(hs.SparsePool.download(gpu, scene, known).rows, pool.rows), "marking changed a voxel"
        assert gpu.shard_dirty_plan(scene, shards, chunk) == counts, "counts"
        send = sf.Buffer(gpu, max(counts) + 2)
        for r in range(shards):
            for cap in chk.caps_for(counts[r]):
                chk.check_pack(gpu, scene, send, pool, lists, r, cap, "bands")
        for stride in (max(counts), max(counts) - 1):
            body = np.full((shards, stride, 512), np.uint64(sf.PADDING) * np.uint64(0x0101010101010101), np.uint64)
            for r, slots in enumerate(lists):
                body[r, :min(len(slots), stride)] = _signatures(slots[:stride], r)
            recv = sf.Buffer(gpu, shards * stride)
            recv.fill(sf.PATTERN)
            recv.load(body)
            for q, skip in [(r, r) for r in range(shards)] + [(shards, -1)]:
                mine = hs.SparsePool(known, _signatures(known, q))
                mine.upload(gpu, scene)
                gpu.shard_dirty_unpack(scene, skip, recv.ptr, stride)
                sf.sync(gpu)
                want = law.unpack(mine, lists, skip, body, stride)
                got = hs.SparsePool.download(gpu, scene, known)
                bad = known[(got.rows != want.rows).any(1)]
                assert not len(bad), f"unpack on replica {q} (skip {skip}) at stride {stride}: slots {bad[:8].tolist()} differ from the law"
                assert recv.guards_intact(sf.PATTERN)
            assert np.array_equal(recv.host(sf.GUARD, sf.GUARD + recv.blocks), body.view(np.uint8).reshape(-1, 4096))
        gpu.track_dirty(scene, False)
        print(f"counts {counts}")
