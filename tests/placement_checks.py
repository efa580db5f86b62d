"""Check bodies shared by test_oracle_placement.py (CPU oracle) and test_gpu_placement.py (HIP engine): the reads of one
map, the voxel update and the allocation pass on fixtures moved far from the world origin (placement_fixtures.py; DESIGN
section 27).  The bodies are those of the origin -- ref64_checks, refvoxel_checks, refrange_checks, the map model -- given
the moved map, the moved pose and the size of the coordinates (ref64.Scale)."""
import functools

import numpy as np

import placement_fixtures as pf
F32 = np.float32
import ref64
import ref64_checks as rc
import ref_range as rr
import refmap_checks as rmc
import refrange_checks as rq
import refvoxel_checks as rv

RAYCAST_CASES = ("plane_64x48", "sphere_outside", "box_corner", "colour_plane")
MESH_CASES = ("plane", "sphere_outside")
PLACEMENTS = tuple(pf.placements(np.zeros((1, 3), np.int64)))  # the names; D depends on the map
HEAVY = ("near+-+", "near-+-", "far+", "edge_pos", "edge_neg")  # the placements of the heavier items

# How many times D is halved for the ray march's tier (a), per case and placement class, so that the rays the float64
# march calls ties stay under placement_fixtures.TIE_CAP: measured with the reference alone by
# test_placement_fixtures.py, which also asserts that one halving fewer misses the cap.  The mesh, the range image, the
# voxel update, the allocation pass and the parity runs have no such ties and sit at the full D.
HALVINGS = {
    ("plane_64x48", "near"): 1, ("plane_64x48", "far"): 2, ("plane_64x48", "edge"): 5,
    ("sphere_outside", "near"): 2, ("sphere_outside", "far"): 3, ("sphere_outside", "edge"): 6,
    ("box_corner", "near"): 1, ("box_corner", "far"): 2, ("box_corner", "edge"): 5,
    ("colour_plane", "near"): 1, ("colour_plane", "far"): 3, ("colour_plane", "edge"): 5,
}


@functools.lru_cache(maxsize=None)
def _origin_map(case):
    build, W, H, cam, colour = rc.raycast_cases()[case]
    M, intr = rc.camera(W, H, **cam)
    return build(), M, intr, W, H, colour


@functools.lru_cache(maxsize=None)
def _origin_mesh_map(case):
    return rc.mesh_cases()[case][0]()


def placement_of(block_pos, pname, halvings=0):
    kind, D = pf.placements(block_pos)[pname]
    return kind, pf.halved(D, halvings)


@functools.lru_cache(maxsize=None)
def raycast_fixture(case, pname, halvings=None):
    """(moved map, moved pose, intr, W, H, colour, scale, class, D used)."""
    m0, M0, intr, W, H, colour = _origin_map(case)
    kind = pf.placements(m0.block_pos)[pname][0]
    k = HALVINGS[(case, kind)] if halvings is None else halvings
    _, D = placement_of(m0.block_pos, pname, k)
    m = pf.shift_map(m0, D)
    return m, pf.shift_pose(M0, D, m.vs), intr, W, H, colour, ref64.Scale(pf.P(m)), kind, D


@functools.lru_cache(maxsize=None)
def raycast_reference(case, pname, halvings=None):
    m, M, intr, W, H, _, scale, _, _ = raycast_fixture(case, pname, halvings)
    return rc.reference_rays(m, M, intr, W, H, scale)


def tie_share(ref):
    """The share of the float64 march's hits it calls ties: the figure TIE_CAP bounds."""
    return float((ref["tie"] & ref["hit"]).sum()) / max(int(ref["hit"].sum()), 1)


def map_teeth(api, scene, m, pname, full_D):
    return pf.teeth(api.download_hash_table(scene), m.D, pname if pname.startswith("edge") and full_D else None)


def run_raycast(api, pkg, case, pname):
    """check_raycast with every image type, the ICP maps, the raycast result and the int16 depth image."""
    m, M, intr, W, H, colour, scale, kind, D = raycast_fixture(case, pname)
    ref = raycast_reference(case, pname)
    assert tie_share(ref) <= pf.TIE_CAP[kind]
    out = rc.check_raycast(api, pkg, m, M, intr, W, H, colour=colour, scale=scale, ref=ref, extras=True)
    scene = api.create_scene(m.scene_params(pkg))
    rc.am.upload(api, scene, m)
    out.update(D=D, P=scale.P, u=scale.u, tie_share=tie_share(ref), max_chain=m.max_chain,
               teeth=map_teeth(api, scene, m, pname, HALVINGS[(case, kind)] == 0))
    for k in ("a_max", "a_p99", "result_max"):
        out[k + "_in_u"] = out[k] / scale.u
    return out


FULL_D_PLACEMENTS = ("far+", "far-", "edge_pos", "edge_neg")
# At EDGE_NEG the camera stands beyond voxel coordinate -2^18, where float32's spacing doubles once more: with a tie
# tolerance of a quarter voxel the float64 march vouches for fewer than ten rays of a fixture.  There the march is held to
# the oracle ray for ray (run_raycast_images), and the oracle to the float64 march at EDGE_POS, one binade below.
UNTIED_PLACEMENTS = ("far+", "far-", "edge_pos")


def run_raycast_images(api, pkg, case, pname):
    """Every product of the ray march at the full D, for comparison between two engines: depth image, raycast result,
    ICP points and normals, the three 8-bit images."""
    m, M, intr, W, H, colour, scale, kind, D = raycast_fixture(case, pname, 0)
    scene, rs = rc.load_map(api, pkg, m, W, H)
    out = dict(depth=api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH), result=api.download_raycast_result(rs))
    for name in ("IMAGE_SHADED", "IMAGE_COLOUR_FROM_NORMAL", "IMAGE_COLOUR_FROM_VOLUME"):
        out[name] = api.get_image(scene, rs, M, intr, getattr(pkg, name))
    api.find_visible_blocks(scene, rs, M, intr)
    out["icp_points"], out["icp_normals"] = api.create_icp_maps(scene, rs, M, intr)
    out["teeth"] = map_teeth(api, scene, m, pname, True)
    return out


def run_raycast_full(api, pkg, case, pname):
    """The ray march at the full D, the table's true ends included, where the tie cap cannot be met: check_raycast_untied,
    on the rays that are no tie.  At an edge the map holds a block exactly at the last or first coordinate on every axis."""
    m, M, intr, W, H, colour, scale, kind, D = raycast_fixture(case, pname, 0)
    ref = raycast_reference(case, pname, 0)
    out = rc.check_raycast_untied(api, pkg, m, M, intr, W, H, scale, ref)
    scene = api.create_scene(m.scene_params(pkg))
    rc.am.upload(api, scene, m)
    out.update(D=D, P=scale.P, u=scale.u, tie_share=tie_share(ref), teeth=map_teeth(api, scene, m, pname, True),
               a_max_in_u=out["a_max"] / scale.u, result_max_in_u=out["result_max"] / scale.u)
    return out


def run_mesh(api, pkg, case, pname):
    """check_mesh with colours at the full D; max_triangles explicit (five per cube of every block at the most)."""
    m0 = _origin_mesh_map(case)
    kind, D = placement_of(m0.block_pos, pname)
    m = pf.shift_map(m0, D)
    scale = ref64.Scale(pf.P(m))
    out = rc.check_mesh(api, pkg, m, surface_bound=rc.mesh_cases()[case][1], max_triangles=len(m.block_pos) * 512 * 5 + 2,
                        scale=scale, colour=True)
    scene = api.create_scene(m.scene_params(pkg))
    rc.am.upload(api, scene, m)
    out.update(D=D, P=scale.P, u=scale.u, vertex_max_in_u=out["vertex_max"] / scale.u, teeth=map_teeth(api, scene, m, pname, True))
    return out


def range_law(pname, case="box_corner"):
    """(RangeLaw of the moved map's own table at the moved pose, placement class): the reference alone."""
    m0, M0, intr, W, H, _ = _origin_map(case)
    kind, D = placement_of(m0.block_pos, pname)
    m = pf.shift_map(m0, D)
    return rr.RangeLaw(m.hash, pf.shift_pose(M0, D, m.vs), intr, F32(m.vs), W, H), kind


def allocation_model_passes(pkg, synth, pname):
    """The map model's own figures of the allocation fixture's two passes (no engine), and the placement class."""
    kind, D = alloc_D(pname)
    wl = pf.Shifted(synth.s_tiny(61, 47), D)
    rig = rmc.Rig(None, pkg, rmc.scene_params(pkg, vs=0.02, mu_vox=rmc.MU_OFF, num_local_blocks=0x800, num_buckets=0x400,
                                              num_excess=0x800), wl.W, wl.H)
    out = []
    for i, (yaw, pitch) in ALLOC_FRAMES:
        rgba, mm, _ = wl.frame(i)
        rig.frame(rgba, mm)
        out.append(rig.m.allocate(rig.depth, rmc.turned(synth, wl, i, yaw, pitch), wl.intr, False))
    return out, kind


def run_range(api, pkg, pname, case="box_corner"):
    """The visible list and the range image of GetImage against ref_range.RangeLaw at the full D."""
    m0, M0, intr, W, H, _ = _origin_map(case)
    kind, D = placement_of(m0.block_pos, pname)
    m = pf.shift_map(m0, D)
    M = pf.shift_pose(M0, D, m.vs)
    scene, rs = rc.load_map(api, pkg, m, W, H)
    table = api.download_hash_table(scene)
    ref = rr.RangeLaw(table, M, intr, scene.params.voxel_size, W, H)
    # the cap is on the listed blocks the law calls ties (a range image has neither hits nor voxels); a tie block takes
    # the cells of its box, widened by one, out of the comparison, and enough covered cells must stay in it
    blocks, cells = ref.tie_shares()
    assert len(ref.ids) >= 100 and ((ref.image[..., 0] != rr.FAR_AWAY) & ~ref.tie_cells).sum() >= 20
    assert blocks <= pf.TIE_CAP[kind], (blocks, cells)
    api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH)
    rq.compare_list(api, scene, rs, ref, table, pname)
    rq.compare_range(api, rs, ref, pname)
    return dict(D=D, listed=len(ref.ids), tie_blocks=blocks, tie_cells=cells, teeth=map_teeth(api, scene, m, pname, True))


# ---------------------------------------------------------------------------------------------------------------------
# the voxel update: refvoxel_checks' crafted cases under a moved pose.  Their exactness survives the move: the voxel size
# is 2^-6 m, so a shift of D blocks is D / 8 m, and every coordinate up to 4096 m is a multiple of 2^-10 below 2^24 of
# them -- float32 holds each product and sum of the mat-vec exactly, in any order.
# ---------------------------------------------------------------------------------------------------------------------
def update_cases():
    """(max_w, mu in steps, form, pose): every kernel form once with mu = 2^-4, the poses in turn, and the plain and the
    de-integrating form with the mu whose quotient eta / mu rounds."""
    return ([(100, rv.MU_STEPS[0], form, j % 4) for j, form in enumerate(rv.FORMS)]
            + [(100, rv.MU_STEPS[1], "plain", 1), (100, rv.MU_STEPS[1], "deprocess", 2)])


@functools.lru_cache(maxsize=None)
def update_D(pose_k, mu_steps, pname):
    """D of a crafted case: from the blocks its depth image can ask for at the origin (float64, reference alone)."""
    M = rv.pose(pose_k)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for seed in range(3):  # the images differ by seed in their low bits only; the plane and the span are the case's
        _, raw = rv.images(mu_steps, seed)
        a, b = pf.requested_extent(raw.astype(np.float64) * rv.STEP, M, rv.INTR, rv.VS, mu_steps * rv.STEP, 3.0)
        lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    return pf.edge_safe(lo, hi, pname)


def run_update(api, pkg, max_w, mu_steps, form, pose_k, pname):
    kind, D = update_D(pose_k, mu_steps, pname)
    c = rv.Case(api, pkg, max_w, mu_steps, form, pose_k, D=D)
    lo, hi = c.pos.min(axis=0), c.pos.max(axis=0)
    assert lo.min() >= pf.FIRST_BLOCK and hi.max() <= pf.LAST_BLOCK
    c.call()
    out = c.check()
    out.update(D=D, lo=lo.tolist(), hi=hi.tolist())
    return out


def run_update_batch(api, pkg, mode, max_w, mu_steps, pose_k, pname):
    kind, D = update_D(pose_k, mu_steps, pname)
    if kind == "edge":  # the three keyframes' old and corrected poses differ by a few voxels: two blocks further in
        D = tuple(int(v - np.sign(v) * 2) for v in D)
    b, h2, figures = rv.run_batch(api, pkg, mode, max_w, mu_steps, pose_k, D=D)
    return dict(D=D, steps=len(figures))


# ---------------------------------------------------------------------------------------------------------------------
# the allocation pass against the map model, which hashes positions itself
# ---------------------------------------------------------------------------------------------------------------------
ALLOC_FRAMES = ((0, (0.0, 0.0)), (5, (0.21, -0.13)))


@functools.lru_cache(maxsize=None)
def alloc_D(pname):
    from dslam_amd.harness import synth
    wl = synth.s_tiny(61, 47)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, (yaw, pitch) in ALLOC_FRAMES:
        _, mm, _ = wl.frame(i)
        a, b = pf.requested_extent(mm.astype(np.float64) / 1000.0, rmc.turned(synth, wl, i, yaw, pitch), wl.intr, 0.02,
                                   rmc.MU_OFF * 0.02, 3.0)
        lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    return pf.edge_safe(lo, hi, pname)


def run_allocation(api, pkg, synth, pname):
    """A.4 MARK / COMMIT / VISIBLE under moved poses: two frames' allocation passes against refmap.MapModel, which walks
    the rays in float32 in the spec's order and hashes the positions itself.  Far out the float32 and the float64 walk
    disagree on the block of more samples than at the origin (the model's block ties: capped here per placement class,
    from the model alone); the comparison is with the float32 walk, every block, whatever the ties."""
    kind, D = alloc_D(pname)
    wl = pf.Shifted(synth.s_tiny(61, 47), D)
    rig = rmc.Rig(api, pkg, rmc.scene_params(pkg, vs=0.02, mu_vox=rmc.MU_OFF, num_local_blocks=0x800, num_buckets=0x400,
                                             num_excess=0x800), wl.W, wl.H)
    out = []
    for i, (yaw, pitch) in ALLOC_FRAMES:
        rgba, mm, _ = wl.frame(i)
        rig.frame(rgba, mm)
        M = rmc.turned(synth, wl, i, yaw, pitch)
        info = rig.m.allocate(rig.depth, M, wl.intr, False)
        assert info["block_ties"] + info["visibility_ties"] + info["gate_ties"] <= pf.TIE_CAP[kind] * info["samples"], info
        assert info["step_tie_samples"] == 0, info
        api.allocate_scene_from_depth(rig.scene, rig.view, rig.rs, M, wl.intr, False)
        rig.compare(f"{pname} frame {i} allocate", scratch=True)
        out.append(info)
    assert out[0]["slots"] >= 150 and out[1]["found_blocks"] >= 50 and out[1]["slots"] >= 50, out
    table = api.download_hash_table(rig.scene)
    return dict(D=D, passes=out, teeth=pf.teeth(table, D, pname if kind == "edge" else None))


# ---------------------------------------------------------------------------------------------------------------------
# parity of the two engines, bit for bit, on sequences fused far from the origin: the kernels' regrouped mat-vecs against
# the oracle's full ones where the operands are large
# ---------------------------------------------------------------------------------------------------------------------
PARITY_PLACEMENTS = ("near+-+", "edge_neg")
SEQUENCE_FRAMES, BATCH_FRAMES = 8, 12
BATCH_PICKS, BATCH_SECOND = (7, 9, 8, 2, 11, 5), (3, 9, 7)


def batch_new_poses(synth, wl):
    """frame -> the corrected world -> camera poses scenarios.batch_scenario fuses it under."""
    out = {}
    for ids, seed in ((list(BATCH_PICKS), 0), (list(BATCH_SECOND) + [BATCH_FRAMES], 1)):
        for n, i in enumerate(ids):
            out.setdefault(i, []).append(synth.world_to_camera(wl.pose(i) @ synth.pose_matrix(
                synth.look_rotation(0.003 * (n + 1 + seed), -0.002 * (1 + seed)), [0.004 + 0.002 * seed, 0.001 * n, -0.003])))
    return out


@functools.lru_cache(maxsize=None)
def parity_extent(which):
    from dslam_amd.harness import synth
    wl = synth.s_tiny()
    if which == "sequence":
        return pf.workload_extent(wl, range(SEQUENCE_FRAMES))
    return pf.workload_extent(wl, range(BATCH_FRAMES + 1), batch_new_poses(synth, wl))


def parity_D(which, pname):
    return pf.edge_safe(*parity_extent(which), pname)


def run_parity_sequence(api, pkg, synth, pname):
    """util.run_sequence with decay and slide under moved poses; returns (full state, mesh with colours, the smallest
    and largest block coordinate held after any frame)."""
    import scenarios
    import util
    kind, D = parity_D("sequence", pname)
    wl = pf.Shifted(synth.s_tiny(), D)
    ext = [np.full(3, 1 << 20), np.full(3, -(1 << 20))]

    def after(i, scene, rs, view):
        h = api.download_hash_table(scene)
        pos = h["pos"][h["ptr"] >= 0].astype(np.int64)
        ext[0], ext[1] = np.minimum(ext[0], pos.min(axis=0)), np.maximum(ext[1], pos.max(axis=0))

    scene, rs, view = util.run_sequence(api, pkg, wl, util.small_params(pkg, wl), SEQUENCE_FRAMES, decay=(2, 2, True), slide=3,
                                        after_frame=after)
    return scenarios.full_state(api, scene, rs), api.mesh_scene(scene, colour=True), ext


def run_parity_batch(api, pkg, synth, pname, call):
    import scenarios
    import util
    kind, D = parity_D("batch", pname)
    wl = pf.Shifted(synth.s_tiny(), D)
    return scenarios.batch_scenario(api, pkg, synth, wl, util.small_params(pkg, wl, history_words=1), True, call, n_frames=BATCH_FRAMES,
                                    picks=BATCH_PICKS, second=BATCH_SECOND)
