"""Check bodies shared by test_oracle_mapmodel.py (CPU oracle) and test_gpu_mapmodel.py (HIP engine): each drives an
engine and the map model of refmap.py through the same calls and compares the whole integer state after every call.
With `api=None` a body runs the model alone: the reach counts and the tie caps every case asserts come from the model
and the inputs, never from an engine.

What is compared (exactly): the table bytes of every entry with ptr >= -1, ptr / offset of all entries, both free
stacks up to their tops, visible ids, type bytes (as dslam_download_visible_types hands them out: without the pass'
generation bit), swap states, last_seen, the allocation scratch (types; coordinates where a type is set), the depth
weight of every voxel, and the counters of dslam_get_stats the modelled calls move."""
import os

import numpy as np

import analytic_maps as am
import ref64
import refmap

TIE_LIMIT = 1e-3  # of the walk samples (the figure ref64_checks.TIE_LIMIT uses for voxels)
MU_OFF = 3.46     # mu / voxelSize with mu / (2 voxelSize) = 1.73: 0.23 from an integer, the step count is never a tie
MU_SHIPPED = 4.0  # what harness/synth.py and upstream's defaults use: 2 |dir| = 2.0 give or take an ulp
EMPTY = np.zeros(1, am.VOXEL_DTYPE)
EMPTY["sdf"] = 32767


def scene_params(pkg, vs=0.02, mu_vox=MU_OFF, **kw):
    base = dict(voxel_size=vs, mu=mu_vox * vs, max_w=100, frustum_min=0.2, frustum_max=3.0, num_local_blocks=0x1000,
                num_buckets=0x400, num_excess=0x1000)
    base.update(kw)
    return pkg.SceneParams(**base)


class Rig:
    """One scene, render state and view of an engine (or none) beside one MapModel."""

    def __init__(self, api, pkg, params, W, H):
        self.api, self.W, self.H = api, W, H
        if api is not None:
            self.scene = api.create_scene(params)
            self.rs = api.create_render_state(self.scene, W, H)
            self.view = api.create_view(W, H)
            params = self.scene.params
        self.m = refmap.MapModel(params, W, H)
        self.vox = np.repeat(EMPTY, self.m.nl * 512).reshape(self.m.nl, 512)
        self.max_w = params.max_w
        self.samples = self.block_ties = self.step_tie_samples = self.vis_ties = self.gate_ties = 0
        half = params.mu / (2.0 * params.voxel_size)  # 2 |dir|: the step count is its ceil
        self.shipped_mu = abs(half - round(half)) < 0.1  # on the rounding edge: step ties are counted apart
        self.calls = 0

    # -- inputs --------------------------------------------------------------------------------------------------------
    def frame(self, rgba, mm):
        self.rgba = np.ascontiguousarray(rgba, np.uint8)
        self.depth = ref64.depth_to_float(mm).astype(np.float32)
        if self.api is not None:
            self.api.view_update(self.view, self.rgba, mm)
            assert np.array_equal(self.api.download_view_depth(self.view), self.depth), "depth conversion (A.3)"

    def load(self, hash_table, alloc_list, last_free, excess_list, last_free_ex):
        self.m.load(hash_table, alloc_list, last_free, excess_list, last_free_ex)
        if self.api is not None:
            self.api.upload_scene_state(self.scene, self.m.hash, self.m.alloc_list, last_free, self.m.excess_list, last_free_ex)

    def set_weights(self, slots, w):
        """upload_voxel_blocks: every voxel of the given slots gets depth weight w (sdf 0)."""
        for s in slots:
            self.vox[s]["w_depth"] = w
            self.vox[s]["sdf"] = 0
            self.m.w[s] = w
            if self.api is not None:
                self.api.upload_voxel_blocks(self.scene, int(s), self.vox[s:s + 1])

    # -- calls ---------------------------------------------------------------------------------------------------------
    def _count(self, info):
        self.samples += info["samples"]
        self.block_ties += info["block_ties"]
        self.step_tie_samples += info["step_tie_samples"]
        self.vis_ties += info["visibility_ties"]
        self.gate_ties += info["gate_ties"]
        assert info["commit_ties"] == 0, f"a commit of this pass was decided by a block tie: {info}"
        if not self.shipped_mu:
            assert info["commit_step_ties"] == 0 and info["step_tie_samples"] == 0, info

    def allocate(self, M, intr, only=False, what=""):
        info = self.m.allocate(self.depth, M, intr, only)
        self._count(info)
        if self.api is not None:
            self.api.allocate_scene_from_depth(self.scene, self.view, self.rs, M, intr, only)
        self.compare(f"{what} allocate", scratch=True)
        return info

    def process_frame(self, M, intr, what=""):
        if self.api is not None:  # sdf / colour may be 1 LSB from ref64: re-read; the weights are the model's own
            got = self.api.download_voxel_blocks(self.scene)
            assert np.array_equal(got["w_depth"], self.m.w), f"{what}: depth weights before fusion"
            self.vox = got
        info = self.m.allocate(self.depth, M, intr, False)
        self._count(info)
        ids, slots, pos = self.m.resident_visible()
        ref, _ = ref64.integrate(self.vox[slots], pos, self.depth, self.rgba, M, intr, self.m.vs, self.m.mu, self.max_w)
        self.vox[slots] = ref
        self.m.w[slots] = ref["w_depth"]
        info["wrapped"] = self.m.push_visible_list(0)
        info["fused_blocks"] = len(slots)
        if self.m.swapping:  # ProcessFrame ends with swap-in and swap-out (A.8)
            self.m.swap_in()
            self.m.swap_out()
            info.update(swapped_in=self.m.last_swapped_in, swapped_out=self.m.last_swapped_out)
            self._after_upkeep()
        if self.api is not None:
            self.api.process_frame(self.scene, self.view, self.rs, M, intr)
        self.compare(f"{what} process_frame", scratch=True)
        return info

    def _after_upkeep(self):
        gone = (self.m.w == 0) & (self.vox["w_depth"] > 0)
        self.vox[gone] = EMPTY[0]
        self.vox["w_depth"] = self.m.w  # merged weights (the merged sdf / colour are re-read from an engine, or unused)

    def decay(self, max_weight, min_age, force_all, what=""):
        info = self.m.decay(max_weight, min_age, force_all)
        self._after_upkeep()
        if self.api is not None:
            self.api.decay(self.scene, self.rs, max_weight, min_age, force_all)
        self.compare(f"{what} decay({max_weight}, {min_age}, {force_all})")
        return info

    def slide_window(self, max_age, what=""):
        info = self.m.slide_window(max_age)
        self._after_upkeep()
        if self.api is not None:
            self.api.slide_window(self.scene, self.rs, max_age)
        self.compare(f"{what} slide_window({max_age})")
        return info

    def reset(self):
        self.m.reset()
        self.vox[:] = EMPTY[0]
        if self.api is not None:
            self.api.reset_scene(self.scene)
        self.compare("reset")  # the render state is not the scene's: its type bytes and list stay

    # -- the comparison ------------------------------------------------------------------------------------------------
    def compare(self, what, scratch=False, weights=True):
        self.calls += 1
        if self.api is None:
            return
        api, m = self.api, self.m
        what = f"call {self.calls} ({what})"
        h = api.download_hash_table(self.scene)
        assert np.array_equal(h["ptr"], m.hash["ptr"]), f"{what}: ptr differs at entries {np.nonzero(h['ptr'] != m.hash['ptr'])[0][:8]}"
        assert np.array_equal(h["offset"], m.hash["offset"]), f"{what}: offset differs at {np.nonzero(h['offset'] != m.hash['offset'])[0][:8]}"
        occ = m.hash["ptr"] >= -1
        assert h[occ].tobytes() == m.hash[occ].tobytes(), f"{what}: bytes of occupied entries differ"
        st, ms = api.stats(self.scene, self.rs), m.stats()
        for k, v in ms.items():
            assert st[k] == v, f"{what}: stats[{k}] = {st[k]}, model {v}"
        al, xl = api.download_allocation_list(self.scene), api.download_excess_list(self.scene)
        assert np.array_equal(al[:m.last_free + 1], m.alloc_list[:m.last_free + 1]), f"{what}: voxel-block free stack differs"
        assert np.array_equal(xl[:m.last_free_ex + 1], m.excess_list[:m.last_free_ex + 1]), f"{what}: excess free stack differs"
        assert np.array_equal(api.download_visible_ids(self.rs), m.visible_ids), f"{what}: visible list differs"
        ty = api.download_visible_types(self.rs)
        assert np.array_equal(ty, m.visible_type), f"{what}: type bytes differ at {np.nonzero(ty != m.visible_type)[0][:8]}"
        if m.swapping:
            assert np.array_equal(api.download_swap_states(self.scene), m.swap_state), f"{what}: swap states differ"
            for t in range(m.n_entries):  # the host store: which entries hold a copy, and its depth weights
                has, blk = api.download_stored_block(self.scene, t)
                assert has == bool(m.has_stored[t]), f"{what}: host copy of entry {t}: {has}, model {bool(m.has_stored[t])}"
                if has:
                    assert np.array_equal(blk["w_depth"], m.stored_w[t]), f"{what}: stored weights of entry {t} differ"
        assert np.array_equal(api.download_last_seen(self.scene), m.last_seen), f"{what}: last_seen differs"
        if scratch:
            ty, co = api.download_alloc_scratch(self.scene)
            assert np.array_equal(ty, m.alloc_type), f"{what}: allocation types differ"
            sel = m.alloc_type > 0
            assert np.array_equal(co[sel], m.coords[sel]), f"{what}: block coordinates of the requests differ"
        if weights:
            w = api.download_voxel_blocks(self.scene)["w_depth"]
            assert np.array_equal(w, m.w), f"{what}: depth weights differ in {(w != m.w).any(axis=1).sum()} blocks"

    def finish(self):
        """The tie caps of the case, from the model's counts alone.  Returns the figures."""
        assert self.block_ties + self.vis_ties + self.gate_ties <= TIE_LIMIT * max(self.samples, 1), \
            f"{self.block_ties} block + {self.vis_ties} visibility + {self.gate_ties} gate ties in {self.samples} samples"
        if not self.shipped_mu:
            assert self.step_tie_samples == 0
        return dict(samples=self.samples, block_ties=self.block_ties, step_tie_samples=self.step_tie_samples,
                    visibility_ties=self.vis_ties, gate_ties=self.gate_ties, calls=self.calls)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def tiny(synth, W, H):
    return synth.s_tiny(W, H)


def turned(synth, wl, i, yaw=0.0, pitch=0.0):
    """World -> camera pose of frame i's camera turned by yaw (about its y) and pitch (about its x)."""
    T = wl.pose(i) @ synth.pose_matrix(synth.look_rotation(yaw, pitch), [0.0, 0.0, 0.0])
    return synth.world_to_camera(T)


def max_chain(m):
    return max((len(m.chain(h)) for h in np.nonzero(m.hash["ptr"][:m.nb] >= -1)[0]), default=0)


# ---------------------------------------------------------------------------------------------------------------------
# single-pass cases.  Each returns the reach counts it asserted.
# ---------------------------------------------------------------------------------------------------------------------
def case_frames(api, pkg, synth, which, mu_vox):
    """A.4 MARK / COMMIT / VISIBLE: first frame into an empty table, later frames under rotated poses."""
    if which == "tiny_61x47":
        wl, vs, kw = synth.s_tiny(61, 47), 0.02, dict(num_local_blocks=0x800, num_buckets=0x400, num_excess=0x800)
    elif which == "room_61x47":
        wl, vs, kw = synth.s_room(61, 47), 0.005, dict(num_local_blocks=0x4000, num_buckets=0x1000, num_excess=0x4000)
    else:
        wl, vs, kw = synth.s_room(640, 480), 0.005, dict(num_local_blocks=0x20000, num_buckets=0x10000, num_excess=0x8000)
    rig = Rig(api, pkg, scene_params(pkg, vs=vs, mu_vox=mu_vox, **kw), wl.W, wl.H)
    assert (wl.W * wl.H) % 64 != 0 or which == "room_640x480"
    big = which == "room_640x480"
    out = []
    for i, (yaw, pitch) in ((0, (0.0, 0.0)), (5, (0.21, -0.13))) if not big else ((3, (0.1, 0.05)),):
        rgba, mm, _ = wl.frame(i)
        rig.frame(rgba, mm)
        M = turned(synth, wl, i, yaw, pitch)
        if big:  # once, allocation only: the weights of 131072 blocks are not downloaded
            info = rig.m.allocate(rig.depth, M, wl.intr)
            rig._count(info)
            if api is not None:
                api.allocate_scene_from_depth(rig.scene, rig.view, rig.rs, M, wl.intr, False)
            rig.compare("640x480 allocate", scratch=True, weights=False)
        else:
            info = rig.process_frame(M, wl.intr, f"{which} frame {i}")
        out.append(info)
    assert out[0]["slots"] >= (5000 if big else 150) and out[0]["found_blocks"] == 0, out[0]
    if not big:
        assert out[1]["found_blocks"] >= 50 and out[1]["slots"] >= 50 and out[1]["retested"] >= 10, out[1]
    if mu_vox == MU_SHIPPED:  # about half the pixels take 3 steps by float32 rounding alone: counted apart
        assert out[0]["step_tie_pixels"] >= out[0]["pixels"] // 10, out[0]
    return dict(passes=out, ties=rig.finish())


def case_three_planes(api, pkg, synth):
    """floor against truncation: a camera at the world origin inside the room, blocks on both sides of x, y, z = 0."""
    wl = synth.s_tiny(61, 47)
    rig = Rig(api, pkg, scene_params(pkg, num_local_blocks=0x1000), wl.W, wl.H)
    reach = dict(negative=0, mixed=0)
    signs = set()
    for k, (yaw, pitch) in enumerate([(0.3, 0.2), (2.1, -0.4), (-1.9, 0.5), (3.6, 1.2), (0.9, -1.25)]):
        T = synth.pose_matrix(synth.look_rotation(yaw, pitch), [0.013, -0.007, 0.011])
        z, rgba = synth.render(wl.prims, wl.intr.astype(np.float64), wl.W, wl.H, T)
        rig.frame(rgba, synth.depth_to_mm_rgbd(z))
        rig.allocate(synth.world_to_camera(T), wl.intr, what=f"three planes {k}")
        b = rig.m.hash["pos"][rig.m.hash["ptr"] >= 0].astype(np.int64)
        signs |= {tuple(s) for s in np.unique(np.sign(b + 0.5), axis=0)}
        reach["negative"] = int((b < 0).any(axis=1).sum())
        reach["mixed"] = int(((b < 0).any(axis=1) & (b >= 0).any(axis=1)).sum())
    assert len(signs) == 8, f"blocks in {len(signs)} of the 8 octants"
    assert reach["negative"] >= 200 and reach["mixed"] >= 100, reach
    return dict(reach=reach, ties=rig.finish())


def case_gates(api, pkg):
    """The four depth gates of MARK and A.3's raw-value cuts, one image column band per side of each."""
    W, H = 45, 37
    # the frustum limits are put exactly ON a depth value: d - mu == frustum_min at 300 mm and d + mu == frustum_max at
    # 2500 mm in float32, so that `<` against `<=` and `>` against `>=` decide those two bands
    f32 = np.float32
    mu32_ = f32(MU_OFF * 0.02)
    d_lo, d_hi = f32(300) * f32(0.001) + f32(0), f32(2500) * f32(0.001) + f32(0)
    p = scene_params(pkg, frustum_min=float(d_lo - mu32_), frustum_max=float(d_hi + mu32_))
    assert f32(p.frustum_min) == d_lo - f32(p.mu) and f32(p.frustum_max) == d_hi + f32(p.mu)
    mu, fmin, fmax = np.float32(p.mu).astype(np.float64), float(f32(p.frustum_min)), float(f32(p.frustum_max))
    lo, hi = 300, 2500  # the first millimetre value with d - mu >= frustum_min, the last with d + mu <= frustum_max
    values = [0, -7, 32001, 32000, 30, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 1500]
    mm = np.zeros((H, W), np.int16)
    for k, v in enumerate(values):
        mm[:, k * W // len(values):(k + 1) * W // len(values)] = v
    rig = Rig(api, pkg, p, W, H)
    rig.frame(np.zeros((H, W, 4), np.uint8), mm)
    M, intr = ref64_camera(W, H, yaw=0.17, pitch=-0.11, t=(0.01, 0.02, -0.03))
    info = rig.allocate(M, intr, what="gates")
    d = rig.depth.astype(np.float64)
    mu32 = float(np.float32(p.mu))
    reach = dict(raw_cut=int((rig.depth == -1).sum()), nonpositive=int((d <= 0).sum()),
                 below_zero_band=int(((d > 0) & (d - mu32 < 0)).sum()),
                 below_min=int(((d - mu32 >= 0) & (d - mu32 < fmin)).sum()), above_max=int((d + mu32 > fmax).sum()),
                 inside=info["pixels"])
    band = H * (W // len(values))
    assert reach["raw_cut"] >= 3 * band and reach["below_zero_band"] >= band and reach["below_min"] >= band, reach
    assert reach["above_max"] >= 2 * band and reach["inside"] >= 5 * band, reach
    # the exact split: lo, lo + 1, hi - 1, hi and 1500 are inside, everything else is out
    inside = np.isin(mm, [lo, lo + 1, hi - 1, hi, 1500])
    assert reach["inside"] == int(inside.sum()), (reach, int(inside.sum()))
    return dict(reach=reach, ties=rig.finish())


def ref64_camera(W, H, **kw):
    import ref64_checks
    return ref64_checks.camera(W, H, **kw)


def case_chains(api, pkg, synth, num_buckets):
    """A.4's slot rule: several blocks contend for one slot (the losers come in the next pass), requests at chain ends."""
    wl = synth.s_tiny(61, 47)
    rig = Rig(api, pkg, scene_params(pkg, num_buckets=num_buckets, num_local_blocks=0x1000, num_excess=0x1000), wl.W, wl.H)
    rgba, mm, M = wl.frame(2)
    rig.frame(rgba, mm)
    M = turned(synth, wl, 2, 0.15, 0.1)
    a = rig.allocate(M, wl.intr, what="pass 1")
    b = rig.allocate(M, wl.intr, what="pass 2")
    c = rig.allocate(M, wl.intr, what="pass 3")
    rgba, mm, _ = wl.frame(9)
    rig.frame(rgba, mm)
    d = rig.allocate(turned(synth, wl, 9, -0.3, 0.2), wl.intr, what="later frame")
    assert a["contended_slots"] >= 30 and a["requests"] > a["slots"], a
    assert b["slots"] >= 30 and b["chain_end_requests"] >= 30, b  # the losers of pass 1, now at chain ends
    assert d["chain_end_requests"] >= 20 and max_chain(rig.m) >= 4, (d, max_chain(rig.m))
    return dict(passes=[a, b, c, d], max_chain=max_chain(rig.m), ties=rig.finish())


def case_exhaustion(api, pkg, synth, which):
    """A.4's failure rule: a stack that runs dry inside a pass, the restored tops, alloc_failures."""
    wl = synth.s_tiny(61, 47)
    kw = dict(blocks=dict(num_local_blocks=0x60, num_excess=0x800), excess=dict(num_local_blocks=0x1000, num_excess=0x20),
              both=dict(num_local_blocks=0xfc, num_excess=0x10))[which]
    rig = Rig(api, pkg, scene_params(pkg, num_buckets=0x100, **kw), wl.W, wl.H)
    rgba, mm, _ = wl.frame(2)
    rig.frame(rgba, mm)
    M = turned(synth, wl, 2, 0.15, 0.1)
    infos = [rig.allocate(M, wl.intr, what=f"{which} pass {k}") for k in range(3)]
    if which == "both":  # the excess list is dry by now; another view's new bucket heads use up the blocks as well
        rgba, mm, _ = wl.frame(50)
        rig.frame(rgba, mm)
        infos += [rig.allocate(turned(synth, wl, 50), wl.intr, what=f"{which} second view, pass {k}") for k in range(2)]
    f1, f2 = sum(i["failed_type1"] for i in infos), sum(i["failed_type2"] for i in infos)
    if which == "blocks":
        assert f1 >= 10 and rig.m.last_free == -1 and rig.m.last_free_ex >= 0, (f1, f2)
    elif which == "excess":
        assert f2 >= 10 and f1 == 0 and rig.m.last_free_ex == -1 and rig.m.last_free >= 0, (f1, f2)
    else:
        assert rig.m.last_free_ex == -1 and rig.m.last_free == -1 and f1 >= 10 and f2 >= 10, (f1, f2, rig.m.last_free)
        assert infos[2]["failed_type2"] >= 10 and infos[2]["failed_type1"] == 0, infos[2]  # excess alone, blocks left
    assert rig.m.alloc_failures >= 1
    return dict(failed_type1=f1, failed_type2=f2, ties=rig.finish())


def case_only_visible(api, pkg, synth):
    """onlyUpdateVisibleList on a populated table: no table byte changes, found entries become visible."""
    wl = synth.s_tiny(61, 47)
    rig = Rig(api, pkg, scene_params(pkg, num_buckets=0x100), wl.W, wl.H)
    rgba, mm, _ = wl.frame(0)
    rig.frame(rgba, mm)
    rig.allocate(turned(synth, wl, 0), wl.intr)
    rig.allocate(turned(synth, wl, 0), wl.intr)
    before = (rig.m.hash.copy(), rig.m.last_free, rig.m.last_free_ex)
    rgba, mm, _ = wl.frame(6)
    rig.frame(rgba, mm)
    info = rig.allocate(turned(synth, wl, 6, 0.1, 0.0), wl.intr, only=True, what="only visible")
    assert np.array_equal(before[0], rig.m.hash) and before[1:] == (rig.m.last_free, rig.m.last_free_ex)
    assert info["found_blocks"] >= 50 and info["slots"] >= 10, info  # requests were marked and none was committed
    return dict(info=info, ties=rig.finish())


def case_retest(api, pkg, synth, swapping):
    """VISIBLE's re-test (A.6): listed blocks leave through each image edge and behind the camera; with swapping the
    enlarged margins W / 8, H / 8 (odd W, H), entries with ptr = -1, the swap-state rule and REALLOC."""
    wl = synth.s_tiny(61, 47)
    rig = Rig(api, pkg, scene_params(pkg, num_buckets=0x100, use_swapping=int(swapping)), wl.W, wl.H)
    rgba, mm, _ = wl.frame(0)
    exits = dict(behind=0, left=0, right=0, top=0, bottom=0)
    margin = 0
    blank = np.zeros_like(mm)
    for yaw, pitch in ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.45), (0.0, -0.45), (np.pi, 0.0), (0.12, 0.08), (-0.1, -0.07)):
        rig.frame(rgba, mm)
        rig.allocate(turned(synth, wl, 0), wl.intr)
        rig.frame(rgba, blank)  # nothing marked: the whole previous list goes through the re-test
        info = rig.allocate(turned(synth, wl, 0, yaw, pitch), wl.intr, what=f"turned {yaw:.2f} {pitch:.2f}")
        assert info["retested"] >= 100
        for k, v in info["exits"].items():
            exits[k] += v
        margin += info.get("kept_by_margin", 0)
    assert all(v >= 20 for v in exits.values()), exits
    out = dict(exits=exits, kept_by_margin=margin)
    if swapping:
        assert margin >= 10, margin
        # park a third of the resident entries on the host (ptr = -1, their blocks back on the stack)
        rig.frame(rgba, mm)
        rig.allocate(turned(synth, wl, 0), wl.intr)
        res = np.nonzero(rig.m.hash["ptr"] >= 0)[0]
        park = res[::3]
        h = rig.m.hash.copy()
        al, lf = rig.m.alloc_list.copy(), rig.m.last_free
        for t in park:
            lf += 1
            al[lf] = h["ptr"][t]
            h["ptr"][t] = -1
        rig.load(h, al, lf, rig.m.excess_list, rig.m.last_free_ex)
        a = rig.allocate(turned(synth, wl, 0), wl.intr, what="parked entries")
        assert a["type2_visible"] >= 20 and a["reallocated"] >= 20 and a["realloc_failed"] == 0, a
        # the same with an empty stack: REALLOC must leave ptr = -1 and the top at -1
        h = rig.m.hash.copy()
        for t in park:
            h["ptr"][t] = -1
        rig.load(h, rig.m.alloc_list, -1, rig.m.excess_list, rig.m.last_free_ex)
        b = rig.allocate(turned(synth, wl, 0), wl.intr, what="parked entries, empty stack")
        assert b["realloc_failed"] >= 20 and b["reallocated"] == 0 and rig.m.last_free == -1, b
        assert int((rig.m.swap_state == 1).sum()) >= 100
        out.update(type2=a["type2_visible"], reallocated=a["reallocated"], realloc_failed=b["realloc_failed"])
    out["ties"] = rig.finish()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# upkeep cases
# ---------------------------------------------------------------------------------------------------------------------
def _fused_rig(api, pkg, synth, frames, W=40, H=30, passes=0, **kw):
    wl = synth.s_tiny(W, H)
    p = dict(num_buckets=0x40, num_local_blocks=0x400, num_excess=0x400)
    p.update(kw)
    rig = Rig(api, pkg, scene_params(pkg, **p), W, H)
    for i in frames:
        rgba, mm, M = wl.frame(i)
        rig.frame(rgba, mm)
        for _ in range(passes):  # a chain end takes one request per pass: chains grow by one entry each
            rig.allocate(M, wl.intr, what=f"frame {i}")
        rig.process_frame(M, wl.intr, f"frame {i}")
    return rig, wl


def case_decay_thresholds(api, pkg, synth):
    """Decay's two predicates: 0 < w <= maxWeight with weights at maxWeight and maxWeight + 1; last_seen exactly at,
    one below and one above newest - minAge; a second call in the same observation epoch; then the aged-list mode."""
    rig, wl = _fused_rig(api, pkg, synth, [0, 12, 24, 36, 48])  # the camera turns: every frame leaves blocks behind
    res = np.nonzero(rig.m.hash["ptr"] >= 0)[0]
    slots = rig.m.hash["ptr"][res]
    rig.set_weights(slots[0::4], 7)  # = maxWeight: reset, block released
    rig.set_weights(slots[1::4], 8)  # = maxWeight + 1: kept
    a = rig.decay(7, 2, True, "gated sweep")
    assert a["at_gate"] >= 5 and a["one_young"] >= 5 and a["candidates"] > a["at_gate"], a
    assert a["released"] >= 20 and a["released"] < a["candidates"], a
    b = rig.decay(7, 2, True, "same epoch")
    assert b["already_swept"] >= 5 and b["candidates"] == 0, b
    c = rig.decay(7, 2, False, "aged lists")
    assert c["candidates"] >= 20, c
    d = rig.decay(255, 0, True, "everything left")
    assert d["released"] >= 20, d
    return dict(sweep=a, again=b, aged=c, last=d, ties=rig.finish())


def case_decay_modes_agree(api, pkg, synth):
    """A.9's last sentence: when every block is in exactly one list, both modes do the same.  Each frame is fused into
    a table of its own blocks only (the camera jumps), one rig per mode, the same calls."""
    out = []
    for force_all in (False, True):
        rig, wl = _fused_rig(api, pkg, synth, [])
        for k, i in enumerate((0, 120, 240)):
            rgba, mm, M = wl.frame(i)
            rig.frame(rgba, mm)
            info = rig.process_frame(M, wl.intr, f"frame {i}")
            # only blocks this frame did not see may remain listed from before: none, the views do not overlap
            in_lists = [s for l in rig.m.lists[0].values() for s in l]
            assert len(in_lists) == len(set(in_lists)), "a block is in two lists: the premise of the case does not hold"
            rig.decay(1, 1, force_all, f"after frame {i}")
        out.append((rig.m.hash.copy(), rig.m.alloc_list[:rig.m.last_free + 1].copy(), rig.m.decayed, rig.m.w.copy()))
        ties = rig.finish()
        in_lists = [s for l in rig.m.lists[0].values() for s in l]
        assert len(in_lists) == len(set(in_lists)), "a block is in two lists: the premise of the case does not hold"
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert np.array_equal(out[0][3], out[1][3]) and out[0][2] >= 20, out[0][2]
    return dict(decayed=out[0][2], ties=ties)


def case_release(api, pkg, synth, seed):
    """Batch release on long chains: a head without a chain, a head with a chain, a middle entry, a tail, several
    entries of one chain at once including the head with its first child; the order of both free stacks."""
    rig, wl = _fused_rig(api, pkg, synth, [0, 20], passes=4, num_buckets=0x40)
    rng = np.random.default_rng(seed)
    res = np.nonzero(rig.m.hash["ptr"] >= 0)[0]
    keep = res[rng.random(len(res)) < 0.5]
    rig.set_weights(rig.m.hash["ptr"][keep], 200)
    r = rig.decay(100, 0, True, "release half")
    for k in ("head_of_chain", "middle", "tail", "multi", "head_and_first_child"):
        assert r[k] >= 3, r
    free = rig.m.excess_list[:rig.m.last_free_ex + 1]
    assert r["released"] >= 50 and len(free) > rig.m.nx - len(res)
    r2 = rig.decay(255, 0, True, "same epoch: nothing")
    assert r2["candidates"] == 0
    rgba, mm, M = wl.frame(20)
    rig.frame(rgba, mm)
    again = rig.process_frame(M, wl.intr, "re-observe")  # pops the stacks in the order the release left them
    assert again["slots"] >= 30, again
    r3 = rig.decay(255, 0, True, "everything")
    assert r3["head_alone"] + r3["head_of_chain"] >= 10, r3
    # heads without a chain: a table with many more buckets than blocks, one pass per frame
    lone, _ = _fused_rig(api, pkg, synth, [0, 20], num_buckets=0x2000)
    res = np.nonzero(lone.m.hash["ptr"] >= 0)[0]
    keep = res[rng.random(len(res)) < 0.5]
    lone.set_weights(lone.m.hash["ptr"][keep], 200)
    r4 = lone.decay(100, 0, True, "lone heads")
    assert r4["head_alone"] >= 50 and r4["released"] >= 50, r4
    lone.finish()
    return dict(first=r, last=r3, lone=r4, ties=rig.finish())


def case_slide_window(api, pkg, synth):
    """SlideWindow: blocks only in the popped list, blocks also in a newer list, and a ring that has wrapped
    (history_words = 1: 64 lists; 70 are pushed)."""
    rig, wl = _fused_rig(api, pkg, synth, [], W=32, H=24, history_words=1, num_buckets=0x40)
    wrapped = 0
    for i in range(70):
        rgba, mm, M = wl.frame(3 * i)
        rig.frame(rgba, mm)
        wrapped += rig.process_frame(M, wl.intr, f"frame {i}")["wrapped"]
    assert wrapped == 6 and rig.m.stats()["fusion_fifo_len"] == 64
    a = rig.slide_window(60, "to 60")
    b = rig.slide_window(20, "to 20")
    c = rig.slide_window(0, "to 0")
    tot = {k: a.get(k, 0) + b.get(k, 0) + c.get(k, 0) for k in ("pops", "only_in_popped", "also_newer", "middle", "tail")}
    assert tot["pops"] == 64 and tot["only_in_popped"] >= 50 and tot["also_newer"] >= 50, tot
    # what is left was only in the six lists the full ring dropped: dropping a list releases nothing
    left = rig.m.hash["ptr"][rig.m.hash["ptr"] >= 0]
    assert rig.m.stats()["fusion_fifo_len"] == 0 and not any(rig.m.referenced(int(s)) for s in left)
    tot["left_by_dropped_lists"] = len(left)
    # A.10, with the render state's list and type bytes still naming entries of the map that is gone: the next pass
    # re-tests them against emptied entries
    rgba, mm, M = wl.frame(5)
    rig.frame(rgba, mm)
    rig.process_frame(M, wl.intr, "before reset")
    stale = len(rig.m.visible_ids)
    rig.reset()
    assert stale >= 30 and len(rig.m.visible_ids) == stale and rig.m.last_free == rig.m.nl - 1
    rgba, mm, M = wl.frame(40)
    rig.frame(rgba, mm)
    a = rig.process_frame(M, wl.intr, "after reset")
    assert a["retested"] >= 10 and a["found_blocks"] == 0 and a["slots"] >= 30, a
    rig.process_frame(M, wl.intr, "after reset, again")
    tot["stale_list_at_reset"] = stale
    return dict(total=tot, wrapped=wrapped, ties=rig.finish())


def case_swapping_window(api, pkg, synth):
    """A scene with host swapping: ProcessFrame's swap-out parks blocks that left the view, a block that comes back is
    re-allocated and merged with its host copy, Decay resets voxels but unlinks nothing, and SlideWindow parks the
    blocks no list holds any more (ptr = -1, entry kept, state 0, type byte 0, slot back on the stack)."""
    rig, wl = _fused_rig(api, pkg, synth, [], use_swapping=1, num_buckets=0x80)
    reach = dict(swapped_in=0, swapped_out=0, reallocated=0, type2=0)
    for i in (0, 40, 80, 120, 0, 40, 80):
        rgba, mm, M = wl.frame(i)
        rig.frame(rgba, mm)
        info = rig.process_frame(M, wl.intr, f"swapping frame {i}")
        for k in ("swapped_in", "swapped_out", "reallocated"):
            reach[k] += info[k]
        reach["type2"] += info["type2_visible"]
    reach["merged_with_host_copy"] = int((rig.m.has_stored & (rig.m.hash["ptr"] >= 0)).sum())
    assert reach["swapped_out"] >= 50 and reach["reallocated"] >= 30 and reach["merged_with_host_copy"] >= 30, reach
    table = rig.m.hash.copy()
    d = rig.decay(1, 0, True, "decay in a swapping scene")
    assert d["candidates"] >= 30 and d["released"] == 0 and np.array_equal(table, rig.m.hash), d
    a = rig.slide_window(2, "swapping, to 2")
    b = rig.slide_window(0, "swapping, to 0")
    reach["parked"] = a["parked"] + b["parked"]
    reach["parked_merged"] = a["parked_merged"] + b["parked_merged"]
    assert reach["parked"] >= 30 and int((rig.m.hash["ptr"] == -1).sum()) >= 100, reach
    assert int((rig.m.hash["ptr"] >= -1).sum()) == int(rig.m.has_stored.sum()) + int((rig.m.hash["ptr"] >= 0).sum())
    rgba, mm, M = wl.frame(0)
    rig.frame(rgba, mm)
    back = rig.process_frame(M, wl.intr, "after the window")
    assert back["reallocated"] >= 30 and back["swapped_in"] >= 30, back
    reach["reallocated_after_window"] = back["reallocated"]
    return dict(reach=reach, decay=d, ties=rig.finish())


# ---------------------------------------------------------------------------------------------------------------------
# seeded sequences
# ---------------------------------------------------------------------------------------------------------------------
def seeds(default_count=12):
    spec = os.environ.get("DSLAM_MAPMODEL_SEEDS")
    if spec:
        first, count = (int(v) for v in spec.split(":"))
        return list(range(first, first + count))
    return list(range(default_count))


def run_sequence(api, pkg, synth, seed, n_calls=30, mu_vox=MU_OFF):
    rng = np.random.default_rng(1000 + seed)
    W, H = 96, 72
    wl = synth.s_tiny(W, H)
    rig = Rig(api, pkg, scene_params(pkg, mu_vox=mu_vox, num_buckets=int(rng.choice([0x80, 0x100, 0x400])),
                                     num_local_blocks=int(rng.choice([0x300, 0x600, 0x1000])),
                                     num_excess=int(rng.choice([0x80, 0x400, 0x1000])), history_words=1), W, H)
    log = []
    frame = int(rng.integers(0, 180))
    for _ in range(n_calls):
        op = rng.choice(["frame"] * 6 + ["allocate"] * 2 + ["decay_sweep"] * 2 + ["decay_aged"] * 2 + ["slide"] * 2 + ["reset"])
        if op in ("frame", "allocate"):
            frame += int(rng.integers(1, 12))
            rgba, mm, _ = wl.frame(frame)
            rig.frame(rgba, mm)
            M = turned(synth, wl, frame, float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.15, 0.15)))
            if op == "frame":
                rig.process_frame(M, wl.intr, f"seed {seed}")
            else:
                rig.allocate(M, wl.intr, only=bool(rng.integers(0, 2)), what=f"seed {seed}")
        elif op == "reset":
            rig.reset()
        elif op == "slide":
            rig.slide_window(int(rng.integers(0, 5)), f"seed {seed}")
        else:
            rig.decay(int(rng.choice([1, 2, 255])), int(rng.integers(0, 4)), op == "decay_sweep", f"seed {seed}")
        log.append(op)
    return dict(ops=log, decayed=rig.m.decayed, slid=rig.m.slid, ties=rig.finish())


# ---------------------------------------------------------------------------------------------------------------------
# two geometric checks that share no text with the model: float64, the depth image and the downloaded table only
# ---------------------------------------------------------------------------------------------------------------------
def geometry_cases():
    return {"tilted_plane": (am.Plane((np.sin(0.35), 0.0, -np.cos(0.35)), -0.5 * np.cos(0.35)), dict(yaw=0.2, pitch=-0.1)),
            "sphere": (am.Sphere((0.03, -0.02, 0.45), 0.16), dict(yaw=-0.15, pitch=0.12, roll=0.3)),
            "box_corner": (am.BoxCorner((0.16, 0.12, 0.55)), dict(yaw=0.25, pitch=0.2, roll=-0.2))}


def check_geometry(api, pkg, case, W=96, H=72):
    geom, cam = geometry_cases()[case]
    vs, mu = 0.005, MU_OFF * 0.005
    M, intr = ref64_camera(W, H, t=(0.004, -0.003, 0.002), **cam)
    T = np.linalg.inv(M.astype(np.float64))
    fx, fy, cx, cy = (float(v) for v in intr)
    ys, xs = np.mgrid[0:H, 0:W]
    dirs_c = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs, float)], -1).reshape(-1, 3)
    z = geom.ray_depth(T[:3, 3], dirs_c @ T[:3, :3].T)  # direction with camera z = 1: the ray parameter is the z-depth
    mm = np.where(np.isfinite(z) & (z < 30.0), np.floor(1000.0 * np.nan_to_num(z) + 0.5), 0).astype(np.int16).reshape(H, W)
    params = scene_params(pkg, vs=vs, num_local_blocks=0x4000, num_buckets=0x40000, num_excess=0x1000)
    scene = api.create_scene(params)
    rs = api.create_render_state(scene, W, H)
    view = api.create_view(W, H)
    api.view_update(view, np.zeros((H, W, 4), np.uint8), mm)
    for _ in range(2):
        api.allocate_scene_from_depth(scene, view, rs, M, intr)
    assert api.stats(scene, rs)["alloc_failures"] == 0
    d = api.download_view_depth(view).astype(np.float64).reshape(-1)
    h = api.download_hash_table(scene)
    resident = h["pos"][h["ptr"] >= 0].astype(np.int64)
    have = {tuple(b) for b in resident}
    mu64, fmin, fmax = float(np.float32(mu)), float(np.float32(0.2)), float(np.float32(3.0))
    valid = (d > 0) & (d - mu64 >= fmin) & (d + mu64 <= fmax)
    assert valid.sum() >= 1000, int(valid.sum())
    pc = dirs_c[valid] * d[valid, None]
    n = np.linalg.norm(pc, axis=1, keepdims=True)
    block = 8 * float(np.float32(vs))
    ends = [((pc * s) @ T[:3, :3].T + T[:3, 3]) / block for s in (1 - mu64 / n, 1 + mu64 / n)]
    # (1) both end points of every valid pixel's band lie in resident blocks
    near_face = missing = 0
    for e in ends:
        on_face = (np.abs(e - np.round(e)) < 1e-4).any(axis=1)
        near_face += int(on_face.sum())
        b = np.floor(e).astype(np.int64)
        missing += sum(1 for bb, f in zip(b, on_face) if not f and tuple(bb) not in have)
    assert missing == 0, f"{missing} band end points in blocks that are not resident"
    assert near_face <= TIE_LIMIT * 2 * len(pc), near_face
    # (2) no resident block lies outside the band.  A block b is allocated only because some sample s of some pixel has
    # floor(s) = b, so |centre - s| <= half a block diagonal, sqrt(3) / 2 blocks.  The samples are p + i dir with
    # dir = (pe - p) / (steps - 1), i <= steps - 1: every one lies ON the pixel's segment [p, pe] in exact arithmetic.
    # One step of the walk, |dir| <= |pe - p| / (steps - 1) <= 1/2 block since steps >= 2 |pe - p|, is allowed on top
    # for the rounding of the engine's float32 march.
    bound = np.sqrt(3.0) / 2.0 + 0.5
    p0, p1 = ends
    seg = p1 - p0
    ss = np.sum(seg * seg, axis=1)
    worst = 0.0
    for c in np.array_split(resident + 0.5, max(1, len(resident) // 256)):
        t = np.clip(np.einsum("bpk,pk->bp", c[:, None, :] - p0[None], seg) / ss[None], 0.0, 1.0)
        dist = np.linalg.norm(c[:, None, :] - (p0[None] + t[..., None] * seg[None]), axis=2).min(axis=1)
        worst = max(worst, float(dist.max()))
    assert worst <= bound, f"a resident block centre lies {worst:.3f} blocks from every band (bound {bound:.3f})"
    assert len(resident) >= 100, len(resident)
    return dict(blocks=len(resident), pixels=int(valid.sum()), near_face=near_face, worst_distance=worst)
