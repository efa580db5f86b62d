"""dslam_survey_overlaps and dslam_select_register_pairs on the MI355X against ref_overlap.py: the
counts are integers, so every comparison is exact.  The fixture maps under three sets of poses, maps whose overlap follows
from set arithmetic, the work split with its edges (a five-block map, a map without a block, entries that are not
resident, poses past the block range and past every int, stale rows), the full 64 maps, read-only-ness, repeatability and
the asynchronous engine, every rejection, the selection through the library, survey -> select -> register_graph end to
end, and the ITMLib mirror (SurveyLocalMapOverlaps, AlignAllLocalMaps)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import overlap_fixtures as of
import ref64_register as rr
import ref_overlap as ro
import register_fixtures as fx
import register_graph_fixtures as gf
import util

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "overlap_harness")


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


@pytest.fixture(scope="module")
def scenes(pkg, gpu):
    """Uploaded fixture maps, one scene per (map, copy), shared by the tests of this file (none of them writes a map)."""
    cache = {}

    def get(m, copy=0):
        if (id(m), copy) not in cache:
            cache[(id(m), copy)] = (m, upload_map(gpu, pkg, m))
        return cache[(id(m), copy)][1]

    return get


def check_survey(gpu, what, tables, handles, T, vs=am.VS):
    """One survey against the reference, exactly.  Returns the reference's (live, blocks, octants)."""
    T = np.asarray(T, np.float32)
    live, blocks, octants = gpu.survey_overlaps(handles, T)
    want = ro.survey(tables, T, vs)
    print(f"{what}: live {live.tolist()}, shared blocks {blocks.tolist() if len(live) <= 6 else '...'}, shared octants "
          f"{octants.tolist() if len(live) <= 6 else '...'}")
    assert live.tolist() == want[0].tolist(), what
    assert np.array_equal(blocks, want[1]), (what, blocks, want[1])
    assert np.array_equal(octants, want[2]), (what, octants, want[2])
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fixture maps of the joint registration under three sets of poses
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_maps_under_three_pose_sets(gpu, scenes):
    ms = gf.map_set("large")
    tables = [ro.Table.of_map(m) for m in ms.maps]
    handles = [scenes(m) for m in ms.maps]
    # of the fixture: every map keeps resident blocks in its excess list, so the chain walk is exercised
    assert all((t.table["ptr"][t.num_buckets:] >= 0).any() for t in tables)
    partial = 0
    for what, T in (("identity poses", gf.identity_starts()), ("true poses", np.stack(ms.T_true).astype(np.float32)),
                    ("off the lattice", gf.off_lattice_starts())):
        live, blocks, octants = check_survey(gpu, what, tables, handles, T)
        assert all(octants[s, d] >= 64 for s in range(3) for d in range(3))
        X = ro.pair_transforms32(T, am.VS)
        per_block = np.concatenate([ro.shared_mask(tables[s], tables[d], X[s, d]).sum(axis=1) for s in range(3) for d in range(3) if s != d])
        partial += int(((per_block >= 1) & (per_block <= 7)).sum())
    # ... and some block shares between 1 and 7 of its octants
    assert partial > 0
    # shared_blocks_out may be NULL
    n = 3
    T = gf.off_lattice_starts()
    live, octants = np.zeros(n, np.int32), np.zeros((n, n), np.int32)
    ptrs = (C.c_void_p * n)(*[s.ptr for s in handles])
    t_abi = np.ascontiguousarray(np.transpose(T, (0, 2, 1))).reshape(-1)
    i32 = C.POINTER(C.c_int32)
    gpu._call("survey_overlaps", gpu._engine, ptrs, t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(n),
              live.ctypes.data_as(i32), None, octants.ctypes.data_as(i32))
    assert np.array_equal(octants, gpu.survey_overlaps(handles, T)[2])


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole blocks, a rotation of 90 degrees, half a block: the counts of set arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of.set_cases(), ids=lambda c: c.name)
def test_against_set_arithmetic(gpu, scenes, case):
    handles = [scenes(m) for m in case.maps]
    live, blocks, octants = gpu.survey_overlaps(handles, case.T)
    print(f"{case.name}: blocks {blocks.tolist()}, octants {octants.tolist()}; set arithmetic {case.want}")
    assert live.tolist() == [len(m.block_pos) for m in case.maps]
    assert (blocks[0, 1], octants[0, 1], blocks[1, 0], octants[1, 0]) == case.want
    assert (blocks[0, 0], octants[0, 0], blocks[1, 1], octants[1, 1]) == (live[0], 8 * live[0], live[1], 8 * live[1])
    check_survey(gpu, case.name, [ro.Table.of_map(m) for m in case.maps], handles, case.T, of.VS_EXACT)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the work split and its edges
# ---------------------------------------------------------------------------------------------------------------------
def test_work_split_and_edges(pkg, gpu, scenes):
    big, box, few = fx.sphere_pair().dst_map, fx.box_pair("small"), gf.few_map()
    assert len(big.block_pos) == 585 and len(few.block_pos) == 5
    # a map some of whose entries are not resident (ptr < 0, as a swapped-out block's): bucket heads and excess entries
    holed = box.dst_map
    table = holed.hash.copy()
    resident = np.flatnonzero(table["ptr"] >= 0)
    gone = np.concatenate([resident[resident < holed.num_buckets][::7], resident[resident >= holed.num_buckets][::3]])
    assert (gone < holed.num_buckets).any() and (gone >= holed.num_buckets).any()
    table["ptr"][gone] = -1
    holed_scene = gpu.create_scene(holed.scene_params(pkg))
    gpu.upload_scene_state(holed_scene, table, holed.alloc_list, holed.last_free, holed.excess_list, holed.last_free_ex)
    gpu.upload_voxel_blocks(holed_scene, 0, holed.vba)
    empty = gpu.create_scene(few.scene_params(pkg))
    empty_table = ro.Table(gpu.download_hash_table(empty), few.num_buckets)
    assert not (empty_table.table["ptr"] >= 0).any()

    tables = [ro.Table.of_map(big), ro.Table.of_map(few), empty_table, ro.Table(table, holed.num_buckets),
              ro.Table.of_map(box.src_map), ro.Table.of_map(few), ro.Table.of_map(few)]
    handles = [scenes(big), scenes(few), empty, holed_scene, scenes(box.src_map), scenes(few, 1), scenes(few, 2)]
    past_blocks = np.eye(4, dtype=np.float32)
    past_blocks[0, 3] = 2000.0          # 4e5 voxels: block 5e4, past the int16 range of a block coordinate
    past_int = np.eye(4, dtype=np.float32)
    past_int[1, 3] = 1.0e8              # 2e10 voxels: past every int
    T = np.stack([I4, I4, I4, fx.off_lattice(), fx.off_lattice(1.5, 0.45), past_blocks, past_int])
    live, blocks, octants = check_survey(gpu, "585 + 5 + 0 + holes + far", tables, handles, T)
    assert live.tolist()[:3] == [585, 5, 0] and live[3] == len(resident) - len(gone)
    assert not octants[2].any() and not octants[:, 2].any() and not blocks[2].any() and not blocks[:, 2].any()
    assert octants[1, 0] > 0 and octants[0, 3] > 0 and octants[3, 4] > 0 and octants[4, 3] > 0
    # what is not resident counts neither as source nor as destination: the same maps with every entry resident give more
    full = ro.survey([tables[4], ro.Table.of_map(holed)], T[[4, 3]], am.VS)
    assert full[2][0, 1] > octants[4, 3] and full[2][1, 0] > octants[3, 4] and full[0][1] == live[3] + len(gone)
    for far in (5, 6):
        others = [i for i in range(7) if i != far]
        assert not octants[far, others].any() and not octants[others, far].any() and octants[far, far] == 40
    # the five-block map with one other, straight after: the rows of the call before are stale
    check_survey(gpu, "5 blocks after the large call", [tables[1], tables[4]], [handles[1], handles[4]], np.stack([I4, fx.off_lattice()]))
    check_survey(gpu, "nothing after the large call", [tables[2], tables[1]], [handles[2], handles[1]], np.stack([I4, I4]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. DSLAM_MAX_RENDER_MAPS maps: full descriptor tables, the widest rows
# ---------------------------------------------------------------------------------------------------------------------
def test_sixty_four_maps(pkg, gpu):
    few = gf.few_map()
    n = pkg.MAX_RENDER_MAPS
    handles = [upload_map(gpu, pkg, few) for _ in range(n)]
    T = np.stack([I4] * n).copy()
    # neighbours one block apart along y, the axis three of the five blocks are lined up on
    assert few.block_pos.tolist()[::2] == [[-3, -3, 13], [-3, -2, 13], [-3, -1, 13]]
    T[:, 1, 3] = np.arange(n, dtype=np.float32) * np.float32(8 * am.VS)
    live, blocks, octants = check_survey(gpu, "64 maps", [ro.Table.of_map(few)] * n, handles, T)
    assert live.tolist() == [5] * n and octants.diagonal().tolist() == [40] * n
    assert octants[0, :4].tolist() == [40, 16, 8, 0] and octants[5, 2:6].tolist() == [0, 8, 16, 40]
    assert np.count_nonzero(octants) == n + 2 * (n - 1) + 2 * (n - 2)
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. read-only, repeatable, asynchronous
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    ms = gf.map_set("small")
    handles = [upload_map(gpu, pkg, m) for m in ms.maps]
    before = [util.snapshot(gpu, s) for s in handles]
    T = gf.off_lattice_starts()

    def run():
        return tuple(a.tobytes() for a in gpu.survey_overlaps(handles, T))

    first, second = run(), run()
    assert first == second
    want = ro.survey([ro.Table.of_map(m) for m in ms.maps], T, am.VS)
    assert first == tuple(a.astype(np.int32).tobytes() for a in want)
    # an asynchronous engine with work in flight: frames being fused into a fourth scene
    wl = synth.s_tiny()
    other = gpu.create_scene(util.small_params(pkg, wl))
    rs = gpu.create_render_state(other, wl.W, wl.H)
    view = gpu.create_view(wl.W, wl.H)
    try:
        gpu.set_async(True)
        for i in range(3):
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(other, view, rs, M, wl.intr)
        third = run()
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert third == first
    for s, snap, what in zip(handles, before, ("map 0", "map 1", "map 2")):
        util.assert_same_state(snap, util.snapshot(gpu, s), what)
        assert snap["stats"] == gpu.stats(s), what


# ---------------------------------------------------------------------------------------------------------------------
# 6. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_outputs_untouched(pkg, gpu, scenes):
    ms = gf.map_set("small")
    good = [scenes(m) for m in ms.maps]
    other_vs = upload_map(gpu, pkg, ms.maps[2], voxel_size=0.006)
    other_mu = upload_map(gpu, pkg, ms.maps[2], mu=0.03)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = upload_map(second, pkg, ms.maps[2])
    start = gf.off_lattice_starts()
    i32 = C.POINTER(C.c_int32)

    def call(handles=good, T0=start, n_maps=None, null=()):
        n = len(handles)
        t_abi = np.ascontiguousarray(np.transpose(np.asarray(T0, np.float32), (0, 2, 1))).reshape(-1).copy()
        ptrs = (C.c_void_p * n)(*[None if s is None else s.ptr for s in handles])
        live, blocks, octants = np.full(n, -7, np.int32), np.full((n, n), -7, np.int32), np.full((n, n), -7, np.int32)
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("survey_overlaps", gpu._engine, None if "scenes" in null else ptrs,
                      None if "T" in null else t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(n if n_maps is None else n_maps),
                      None if "live" in null else live.ctypes.data_as(i32), blocks.ctypes.data_as(i32),
                      None if "octants" in null else octants.ctypes.data_as(i32))
        assert (live == -7).all() and (blocks == -7).all() and (octants == -7).all()

    for what in ("scenes", "T", "live", "octants"):
        call(null=(what,))
    call(handles=[good[0], None, good[2]])
    call(n_maps=1)
    call(n_maps=0)
    call(n_maps=pkg.MAX_RENDER_MAPS + 1)
    call(handles=[good[0], good[1], good[0]])
    call(handles=[good[0], good[1], foreign])
    call(handles=[good[0], good[1], other_vs])
    call(handles=[good[0], good[1], other_mu])
    nan, inf, skew = start.copy(), start.copy(), start.copy()
    nan[1, 1, 3] = np.nan
    inf[2, 0, 3] = np.inf
    skew[2, :3, :3] *= 1.001
    call(T0=nan)
    call(T0=inf)
    call(T0=skew)
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu.select_register_pairs([5, 5, 5], np.full((3, 3), 64), pkg.PairSelectParams(max_pairs=1))
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu.select_register_pairs([5, 5], np.full((2, 2), 64), pkg.PairSelectParams(min_shared_octants=-1))
    # ... and the engine still answers
    assert gpu.survey_overlaps(good, start)[0].tolist() == [len(m.block_pos) for m in ms.maps]


# ---------------------------------------------------------------------------------------------------------------------
# 7. the selection through the library
# ---------------------------------------------------------------------------------------------------------------------
def test_selection_through_the_library(pkg, gpu):
    capped = spanning_only = 0
    for live, shared, params in of.selection_cases():
        pairs, component, res = gpu.select_register_pairs(live, shared, pkg.PairSelectParams(**params))
        want_pairs, want_component, want, _ = ro.select(live, shared, **params)
        assert [tuple(p) for p in pairs.tolist()] == want_pairs and component.tolist() == want_component
        assert dict(qualifying=res.qualifying, selected=res.selected, num_components=res.num_components) == want
        capped += res.selected < res.qualifying
        spanning_only += res.selected < res.qualifying and params["max_pairs"] == len(live) - 1
    assert capped >= 20 and spanning_only >= 5
    live, shared, _ = of.selection_cases()[3]
    assert [tuple(p) for p in gpu.select_register_pairs(live, shared)[0].tolist()] == ro.select(live, shared)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 8. survey -> select -> register_graph
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_with_a_map_far_away(pkg, gpu, scenes):
    ms = gf.map_set("small")
    handles = [scenes(m) for m in ms.maps] + [scenes(fx.sphere_pair().dst_map)]
    T = np.concatenate([gf.off_lattice_starts(), gf.FAR[None]])
    live, blocks, octants = gpu.survey_overlaps(handles, T)
    pairs, component, sel = gpu.select_register_pairs(live, octants)
    print(f"shared octants {octants.tolist()}; selected {pairs.tolist()}, components {component.tolist()}")
    assert sel.num_components == 2 and component.tolist() == [0, 0, 0, 3]
    assert len(pairs) == 6 and pairs.max() == 2                 # every ordered pair of the three, none with the fourth
    T_out, res, pres = gpu.register_graph(handles[:3], T[:3], pairs, 0)
    print(f"register_graph on the selected pairs: {res.as_dict()}; valid at the start {[p.valid_first for p in pres]}")
    assert res.stop_reason != 3 and res.active_pairs == len(pairs) and all(p.active for p in pres)
    assert res.cost_last < res.cost_first
    # what the coarse count promised and what registration found: the ratio DESIGN.md section 16 tabulates
    for (s, d), p in zip(pairs.tolist(), pres):
        print(f"  pair ({s}, {d}): valid_first / shared_octants = {p.valid_first} / {octants[s, d]} = {p.valid_first / octants[s, d]:.2f}")


# ---------------------------------------------------------------------------------------------------------------------
# 9. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
MIRROR_FRAMES = dict(W=80, H=60, n_frames=4, stride=4)   # S-tiny keyframes 0, 4, 8, 12 (as test_gpu_register_graph.py)


def run_harness(pkg, gpu, synth, tmp_path, with_far):
    """overlap_harness on the S-tiny keyframes; returns what it wrote and the same maps re-fused through the C ABI."""
    W, H, n_frames, stride = (MIRROR_FRAMES[k] for k in ("W", "H", "n_frames", "stride"))
    wl = synth.s_tiny(W, H)
    p = util.small_params(pkg, wl)
    vs = p.voxel_size
    D1 = rr.rigid(5e-3, fx.AXIS, np.array([0.6, -0.64, 0.48]) * vs).astype(np.float32)
    D2 = rr.rigid(-4e-3, gf.AXIS2, 0.8 * vs * gf.DIR2 / np.linalg.norm(gf.DIR2)).astype(np.float32)
    frames = [wl.frame(stride * i) for i in range(n_frames)]
    fin, fout = tmp_path / f"frames{with_far}.bin", tmp_path / f"out{with_far}.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for rgba, mm, M in frames:
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        f.write(pkg.mat_to_abi(D1).tobytes()); f.write(pkg.mat_to_abi(D2).tobytes())
        f.write(struct.pack("<2i", 0, with_far))
    run = subprocess.run([HARNESS, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    n, = struct.unpack_from("<i", raw, 0)
    at = 4
    out = dict(n=n, stdout=run.stdout.strip())

    def take(count, dtype=np.float32):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    for name in ("T_before", "T_all", "T_pairs"):
        out[name] = take(16 * n).reshape(n, 4, 4).transpose(0, 2, 1)
    fused = take(16 * n * n_frames).reshape(n, n_frames, 4, 4).transpose(0, 1, 3, 2)
    out["live"], out["shared"] = take(n, np.int32), take(n * n, np.int32).reshape(n, n)
    out["sel"] = pkg.PairSelectResult.from_buffer_copy(raw[at:at + 16]); at += 16
    out["component"] = take(n, np.int32)
    out["pairs"] = take(2 * out["sel"].selected, np.int32).reshape(-1, 2)
    for key in ("all", "pairs_run"):
        aligned, = struct.unpack_from("<i", raw, at); at += 4
        out["aligned_" + key] = aligned
        if aligned < 0:
            break
        reported, = struct.unpack_from("<i", raw, at); at += 4
        out["res_" + key] = pkg.RegisterGraphResult.from_buffer_copy(raw[at:at + 24]); at += 24
        out["pres_" + key] = [pkg.RegisterPairResult.from_buffer_copy(raw[at + 24 * k:at + 24 * k + 24]) for k in range(reported)]
        at += 24 * reported
    assert at == len(raw)
    # the same maps through the C ABI
    made = []
    view = gpu.create_view(wl.W, wl.H)
    for k in range(n):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (rgba, mm, _) in enumerate(frames):
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    return out, made


def test_mirror_survey_and_align_all_local_maps(pkg, gpu, synth, tmp_path):
    """Three maps: the harness's survey and selection are the C ABI's on the same maps, and AlignAllLocalMaps returns what
    AlignLocalMaps returns for the selected pairs, byte for byte -- which is what dslam_register_graph gives through
    _capi.py."""
    out, made = run_harness(pkg, gpu, synth, tmp_path, 0)
    live, blocks, octants = gpu.survey_overlaps(made, out["T_before"])
    pairs, component, sel = gpu.select_register_pairs(live, octants)
    print(f"mirror: {out['stdout']}; shared octants {octants.tolist()}, pairs {pairs.tolist()}")
    assert out["n"] == 3 and out["live"].tolist() == live.tolist() and np.array_equal(out["shared"], octants)
    assert bytes(out["sel"]) == bytes(sel) and out["component"].tolist() == component.tolist() and np.array_equal(out["pairs"], pairs)
    assert sel.num_components == 1 and sel.selected == 6 and live.min() > 0
    want = ro.survey([ro.Table.of_scene(gpu, s) for s in made], out["T_before"], made[0].params.voxel_size)
    assert live.tolist() == want[0].tolist() and np.array_equal(octants, want[2]) and np.array_equal(blocks, want[1])
    # AlignAllLocalMaps is AlignLocalMaps on the selected pairs ...
    assert out["aligned_all"] == out["aligned_pairs_run"] >= 0
    assert bytes(out["res_all"]) == bytes(out["res_pairs_run"])
    assert [bytes(p) for p in out["pres_all"]] == [bytes(p) for p in out["pres_pairs_run"]] and len(out["pres_all"]) == 6
    assert out["T_all"].tobytes() == out["T_pairs"].tobytes()
    # ... which is dslam_register_graph on them
    T, res, pres = gpu.register_graph(made, out["T_before"], pairs, 0)
    assert bytes(res) == bytes(out["res_all"]) and [bytes(p) for p in pres] == [bytes(p) for p in out["pres_all"]]
    assert out["aligned_all"] == int(res.stop_reason == 0)
    assert out["T_all"].tobytes() == (T if out["aligned_all"] else out["T_before"]).tobytes()
    assert res.stop_reason != 3 and res.active_pairs == 6 and res.cost_last < res.cost_first


def test_mirror_refuses_unconnected_maps(pkg, gpu, synth, tmp_path):
    """With a fourth map believed 3 m away the maps fall into two components: AlignAllLocalMaps returns false, makes no
    registration call and leaves all four poses alone."""
    out, made = run_harness(pkg, gpu, synth, tmp_path, 1)
    live, blocks, octants = gpu.survey_overlaps(made, out["T_before"])
    pairs, component, sel = gpu.select_register_pairs(live, octants)
    print(f"mirror: {out['stdout']}; shared octants {octants.tolist()}")
    assert out["n"] == 4 and out["live"].tolist() == live.tolist() and np.array_equal(out["shared"], octants)
    assert bytes(out["sel"]) == bytes(sel) and np.array_equal(out["pairs"], pairs)
    assert out["component"].tolist() == component.tolist() == [0, 0, 0, 3] and sel.num_components == 2
    assert not octants[3, :3].any() and not octants[:3, 3].any()
    assert out["aligned_all"] == 0 and out["aligned_pairs_run"] == -1
    assert bytes(out["res_all"]) == bytes(pkg.RegisterGraphResult())          # no registration call was made
    assert all(bytes(p) == bytes(pkg.RegisterPairResult()) for p in out["pres_all"])
    assert out["T_all"].tobytes() == out["T_before"].tobytes() == out["T_pairs"].tobytes()
    assert abs(out["T_before"][3, 2, 3] - out["T_before"][0, 2, 3] - 3.0) < 1e-6
