"""Check bodies shared by test_oracle_mapmodel.py (CPU oracle) and test_gpu_mapmodel.py (HIP engine): each drives an
engine and the map model of refmap.py through the same calls and compares the whole integer state after every call.
With `api=None` a body runs the model alone: the reach counts and the tie caps every case asserts come from the model
and the inputs, never from an engine.

What is compared (exactly): the table bytes of every entry with ptr >= -1, ptr / offset of all entries, both free
stacks up to their tops, visible ids, type bytes (as dslam_download_visible_types hands them out: without the pass'
generation bit), swap states, last_seen, the allocation scratch (types; coordinates where a type is set), the depth
weight of every voxel, and the counters of dslam_get_stats the modelled calls move.

In a scene with host swapping the Rig also carries every voxel's sdf and colour, on the device and in the host store, as
an interval [lo, hi] of permitted values: an integration leaves ref64.integrate's value give or take 1 LSB (the rule of
ref64_checks), a merge takes the interval of ref64.combine_stored (exact unless a tie), a park moves a block to the host
store byte for byte, and everything else leaves a voxel as it was.  After every call the engine's voxels and stored blocks
must lie inside, and the Rig then takes the engine's bytes as the next call's inputs: a block no call touches is compared
byte for byte, and a merge's inputs are what the engine held before the call."""
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
        if self.m.swapping:  # the upper ends of the value intervals (vox is the lower end), and the host store likewise
            self.vox_hi = self.vox.copy()
            self.stored = np.repeat(EMPTY, self.m.n_entries * 512).reshape(self.m.n_entries, 512)
            self.stored_hi = self.stored.copy()
        self.merges = dict(blocks=0, values=0, ties=0, exact_blocks=0, worst_err=dict(sdf=0.0, clr=0.0),
                           off_truncation=dict(sdf=0, clr=0), worst_distance_off_truncation=dict(sdf=0.0, clr=0.0))
        self._exact_merges = []
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
            if self.m.swapping:
                self.vox_hi[s] = self.vox[s]
            if self.api is not None:
                self.api.upload_voxel_blocks(self.scene, int(s), self.vox[s:s + 1])

    def set_blocks(self, slots, blocks):
        """upload_voxel_blocks: the given slots get the given voxels, every byte."""
        for s, b in zip(slots, blocks):
            self.vox[s] = b
            self.m.w[s] = b["w_depth"]
            if self.m.swapping:
                self.vox_hi[s] = b
            if self.api is not None:
                self.api.upload_voxel_blocks(self.scene, int(s), self.vox[s:s + 1])

    # -- voxel values in a swapping scene --------------------------------------------------------------------------------
    def _sync(self, what):
        """Before a call: the engine's voxels become the call's inputs (they were checked after the previous call)."""
        if self.api is not None:
            got = self.api.download_voxel_blocks(self.scene)
            assert np.array_equal(got["w_depth"], self.m.w), f"{what}: depth weights before the call"
            self.vox = got
            if self.m.swapping:
                self.vox_hi = got.copy()

    def _integrated(self, slots, ref):
        """ref64.integrate's result for the given slots: weights exact, sdf and colour to 1 LSB."""
        self.vox[slots] = ref
        self.m.w[slots] = ref["w_depth"]
        if self.m.swapping:
            lo, hi = ref.copy(), ref.copy()
            lo["sdf"], hi["sdf"] = np.maximum(ref["sdf"].astype(np.int64) - 1, -32767), np.minimum(ref["sdf"].astype(np.int64) + 1, 32767)
            lo["clr"], hi["clr"] = np.maximum(ref["clr"].astype(np.int64) - 1, 0), np.minimum(ref["clr"].astype(np.int64) + 1, 255)
            self.vox[slots], self.vox_hi[slots] = lo, hi

    def _move_values(self):
        """Carry the values through the merges and parks the model logged, in their order."""
        ev, self.m.events = self.m.events, []
        if not self.m.swapping:
            return
        i = 0
        while i < len(ev):
            j = i
            while j < len(ev) and ev[j][0] == ev[i][0]:
                j += 1
            t, s = np.array([e[1] for e in ev[i:j]]), np.array([e[2] for e in ev[i:j]])
            if ev[i][0] == "merge":
                exact = np.array_equal(self.stored[t], self.stored_hi[t]) and np.array_equal(self.vox[s], self.vox_hi[s])
                lo, hi, info = ref64.combine_stored(self.stored[t], self.vox[s], self.max_w)
                if not exact:
                    hi = ref64.combine_stored(self.stored_hi[t], self.vox_hi[s], self.max_w)[1]
                self.vox[s], self.vox_hi[s] = lo, hi
                self.merges["blocks"] += len(s)
                self.merges["values"] += int(info["merged_depth"].sum()) + 3 * int(info["merged_colour"].sum())
                self.merges["ties"] += int(info["tie_sdf"].sum()) + int(info["tie_clr"].sum())
                if exact:
                    self._exact_merges.append((s, lo, hi, info))
            else:
                self.stored[t], self.stored_hi[t] = self.vox[s], self.vox_hi[s]
                self.vox[s] = self.vox_hi[s] = EMPTY[0]
                kept = []  # a block merged and parked by one call is checked in the host store, by its interval
                for ms, lo, hi, info in self._exact_merges:
                    k = ~np.isin(ms, s)
                    if k.any():
                        kept.append((ms[k], lo[k], hi[k], {n: v[k] for n, v in info.items()}))
                self._exact_merges = kept
            i = j

    @staticmethod
    def _inside(got, lo, hi, what):
        for f in ("w_depth", "w_color", "_pad"):
            assert np.array_equal(got[f], lo[f]), f"{what}: {f} differs in {int((got[f] != lo[f]).sum())} voxels"
        for f in ("sdf", "clr"):
            g = got[f].astype(np.int64)
            bad = (g < lo[f]) | (g > hi[f])
            assert not bad.any(), (f"{what}: {int(bad.sum())} {f} values outside the permitted interval; first got "
                                   f"{g[bad][:4]}, permitted {lo[f][bad][:4]} .. {hi[f][bad][:4]}")

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

    def process_frame(self, M, intr, what="", is_defusion=False):
        self._sync(what)  # sdf / colour may be 1 LSB from ref64: re-read; the weights are the model's own
        info = self.m.allocate(self.depth, M, intr, False)
        self._count(info)
        ids, slots, pos = self.m.resident_visible()
        ref, _ = ref64.integrate(self.vox[slots], pos, self.depth, self.rgba, M, intr, self.m.vs, self.m.mu, self.max_w)
        self._integrated(slots, ref)
        info["wrapped"] = self.m.push_visible_list(1 if is_defusion else 0)  # A.11: the flag only routes the list
        info["fused_blocks"] = len(slots)
        if self.m.swapping:  # ProcessFrame ends with swap-in and swap-out (A.8)
            self.m.swap_in()
            self.m.swap_out()
            info.update(swapped_in=self.m.last_swapped_in, swapped_out=self.m.last_swapped_out)
            self._after_upkeep()
        if self.api is not None:
            self.api.process_frame(self.scene, self.view, self.rs, M, intr, is_defusion=is_defusion)
        self.compare(f"{what} process_frame" + (" (defusion ring)" if is_defusion else ""), scratch=True)
        return info

    def deprocess_frame(self, M, intr, what=""):
        """A.11 DeProcessFrame: a visible-list-only pass at the pose, then the inverse update; no list is queued, and a
        swapping scene neither merges nor parks."""
        self._sync(what)
        info = self.m.allocate(self.depth, M, intr, True)
        self._count(info)
        ids, slots, pos = self.m.resident_visible()
        ref, _ = ref64.integrate(self.vox[slots], pos, self.depth, self.rgba, M, intr, self.m.vs, self.m.mu, self.max_w,
                                 deintegrate=True)
        info["emptied_voxels"] = int(((ref["w_depth"] == 0) & (self.m.w[slots] > 0)).sum())
        info["defused_blocks"] = int((ref["w_depth"] != self.m.w[slots]).any(axis=1).sum())
        self._integrated(slots, ref)
        if self.api is not None:
            self.api.deprocess_frame(self.scene, self.view, self.rs, M, intr)
        self.compare(f"{what} deprocess_frame", scratch=True)
        return info

    def _after_upkeep(self):
        """Voxels the model reset (Decay) or moved away, and the values of the blocks it merged or parked."""
        self._move_values()
        for vox in (self.vox, self.vox_hi) if self.m.swapping else (self.vox,):
            gone = (self.m.w == 0) & (vox["w_depth"] > 0)
            vox[gone] = EMPTY[0]
            if self.m.swapping:
                assert np.array_equal(vox["w_depth"], self.m.w), "combine_stored's depth weights and the model's differ"
            vox["w_depth"] = self.m.w

    def decay(self, max_weight, min_age, force_all, what="", defusion_part=False):
        info = self.m.decay(max_weight, min_age, force_all, q=1 if defusion_part else 0)
        self._after_upkeep()
        if self.api is not None:
            self.api.decay(self.scene, self.rs, max_weight, min_age, force_all, defusion_part=defusion_part)
        self.compare(f"{what} decay({max_weight}, {min_age}, {force_all}, defusion_part={defusion_part})")
        return info

    def slide_window(self, max_age, what=""):
        info = self.m.slide_window(max_age)
        self._after_upkeep()
        if self.api is not None:
            self.api.slide_window(self.scene, self.rs, max_age)
        self.compare(f"{what} slide_window({max_age})")
        return info

    def slide_window_defusion_part(self, max_age, max_size, what=""):
        """SlideWindow's rule on the defusion ring until max_size lists remain; max_age is not used."""
        info = self.m.slide_window(max_size, q=1)
        self._after_upkeep()
        if self.api is not None:
            self.api.slide_window_defusion_part(self.scene, self.rs, max_age, max_size)
        self.compare(f"{what} slide_window_defusion_part({max_age}, {max_size})")
        return info

    def swap_in(self, what=""):
        self.m.swap_in()
        self._after_upkeep()
        if self.api is not None:
            self.api.swap_in(self.scene, self.rs)
        self.compare(f"{what} swap_in")
        return dict(swapped_in=self.m.last_swapped_in)

    def swap_out(self, what=""):
        self.m.swap_out()
        self._after_upkeep()
        if self.api is not None:
            self.api.swap_out(self.scene, self.rs)
        self.compare(f"{what} swap_out")
        return dict(swapped_out=self.m.last_swapped_out)

    def flush(self, what=""):
        info = self.m.save_to_global()
        self._after_upkeep()
        if self.api is not None:
            self.api.save_to_global_memory(self.scene)
        self.compare(f"{what} save_to_global_memory")
        return info

    def reset(self):
        self.m.reset()
        self.vox[:] = EMPTY[0]
        if self.m.swapping:
            self.vox_hi[:] = EMPTY[0]
            self.stored[:] = EMPTY[0]
            self.stored_hi[:] = EMPTY[0]
        if self.api is not None:
            self.api.reset_scene(self.scene)
        self.compare("reset")  # the render state is not the scene's: its type bytes and list stay

    # -- the comparison ------------------------------------------------------------------------------------------------
    def compare(self, what, scratch=False, weights=True):
        self.calls += 1
        if self.api is None:
            self._exact_merges = []
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
            held = []
            for t in range(m.n_entries):  # the host store: which entries hold a copy, its depth weights, its bytes
                has, blk = api.download_stored_block(self.scene, t)
                assert has == bool(m.has_stored[t]), f"{what}: host copy of entry {t}: {has}, model {bool(m.has_stored[t])}"
                if has:
                    assert np.array_equal(blk["w_depth"], m.stored_w[t]), f"{what}: stored weights of entry {t} differ"
                    held.append(blk)
            if held:
                t, held = np.nonzero(m.has_stored)[0], np.stack(held)
                self._inside(held, self.stored[t], self.stored_hi[t], f"{what}: stored blocks")
                self.stored[t], self.stored_hi[t] = held, held
        assert np.array_equal(api.download_last_seen(self.scene), m.last_seen), f"{what}: last_seen differs"
        if scratch:
            ty, co = api.download_alloc_scratch(self.scene)
            assert np.array_equal(ty, m.alloc_type), f"{what}: allocation types differ"
            sel = m.alloc_type > 0
            assert np.array_equal(co[sel], m.coords[sel]), f"{what}: block coordinates of the requests differ"
        if weights:
            got = api.download_voxel_blocks(self.scene)
            w = got["w_depth"]
            assert np.array_equal(w, m.w), f"{what}: depth weights differ in {(w != m.w).any(axis=1).sum()} blocks"
            if m.swapping:
                self._inside(got, self.vox, self.vox_hi, f"{what}: voxel blocks")
                for s, lo, hi, info in self._exact_merges:  # inputs known to the byte: the merge's own figures
                    fig = ref64.check_combined(got[s], lo, hi, info, f"{what}: merged blocks")
                    self.merges["exact_blocks"] += len(s)
                    for f in ("sdf", "clr"):
                        self.merges["worst_err"][f] = max(self.merges["worst_err"][f], fig[f]["worst_err"])
                        self.merges["off_truncation"][f] += fig[f]["off_truncation"]
                        self.merges["worst_distance_off_truncation"][f] = max(
                            self.merges["worst_distance_off_truncation"][f], fig[f]["worst_distance_off_truncation"])
                self.vox, self.vox_hi = got, got.copy()
        self._exact_merges = []

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
# A.8's merge on chosen voxels, the flush, the defusion ring
# ---------------------------------------------------------------------------------------------------------------------
def _const_block(sdf, wd, clr, wc, pad=0):
    b = np.zeros(512, am.VOXEL_DTYPE)
    b["sdf"], b["w_depth"], b["clr"], b["w_color"], b["_pad"] = sdf, wd, clr, wc, pad
    return b


def crafted_blocks(seed, k, max_w):
    """(host, device): k voxel blocks for each side of a merge.  The first half is seeded-random over the full ranges
    (sdf -32767 .. 32767, colour 0 .. 255, depth and colour weights drawn independently, host weights 1 .. max_w, device
    weights 0 .. max_w, a random pad byte); the second half cycles through the edge rows, each filling a whole block so
    that every lane and every 16-byte chunk of a lane sees it."""
    rng = np.random.default_rng(seed)
    n = k // 2
    host, dev = np.zeros((k, 512), am.VOXEL_DTYPE), np.zeros((k, 512), am.VOXEL_DTYPE)
    for b, lo in ((host, 1), (dev, 0)):
        b["sdf"][:n] = rng.integers(-32767, 32768, (n, 512))
        b["clr"][:n] = rng.integers(0, 256, (n, 512, 3))
        b["w_depth"][:n] = rng.integers(lo, max_w + 1, (n, 512))
        b["w_color"][:n] = rng.integers(lo, max_w + 1, (n, 512))
        b["_pad"][:n] = rng.integers(0, 256, (n, 512))
    c = lambda w: min(w, max_w)
    half = max_w // 2
    rows = [  # (host: sdf, w_depth, colour, w_color), (device: the same)
        ((1234, 0, (9, 8, 7), 0), (-555, c(3), (1, 2, 3), c(2))),                    # host weight 0: nothing changes
        ((-12345, c(5), (200, 100, 50), c(7)), (-20000, 0, (31, 32, 33), 0)),         # device weight 0
        ((1000, max_w, (10, 250, 128), max_w), (-3001, max_w, (251, 11, 127), max_w)),  # both at max_w
        ((20001, half, (3, 60, 255), half), (-7, max_w - half, (254, 61, 0), max_w - half)),          # sum == max_w
        ((20001, half + 1, (3, 60, 255), half + 1), (-7, max_w - half, (254, 61, 0), max_w - half)),  # sum == max_w + 1
        ((777, c(3), (77, 77, 77), c(2)), (777, c(2), (77, 77, 77), c(3))),           # equal values: q is an integer
        ((32767, c(3), (255, 255, 255), c(3)), (32767, c(2), (255, 255, 255), c(1))),  # +1 on both sides; 255 on 255
        ((-32767, c(2), (0, 0, 0), c(3)), (-32767, c(3), (255, 255, 255), c(2))),      # -1 on both sides; 0 on 255
        ((32767, c(2), (255, 0, 255), c(1)), (-32767, c(3), (0, 255, 0), c(3))),       # +1 against -1
        ((4321, 0, (90, 80, 70), c(3)), (-99, c(2), (10, 20, 31), c(2))),             # depth half idle, colour half merges
        ((4321, c(3), (90, 80, 70), 0), (-99, c(2), (10, 20, 31), c(2))),             # the reverse
        ((1234, 0, (9, 8, 7), 0), (-4321, 0, (50, 60, 70), 0)),                       # no weight anywhere, values kept
    ]
    for i in range(n, k):
        h, d = rows[(i - n) % len(rows)]
        host[i], dev[i] = _const_block(*h, pad=(17 * i) & 255), _const_block(*d, pad=(29 * i + 5) & 255)
        if h[1] == 0 and d[1] > 0:  # an idle depth half must hand back EVERY device value: one per voxel, both signs
            dev[i]["sdf"] = (np.arange(512) * 127 + 61 * i) % 65535 - 32767
        if h[3] == 0 and d[3] > 0:
            dev[i]["clr"] = ((np.arange(512)[:, None] * np.array([1, 3, 7]) + 11 * i) % 256)
    return host, dev


def crafted_reach(host, dev, max_w):
    """How many voxels of the crafted pair reach each edge row (from the data, not from how it was built)."""
    h, d = host.reshape(-1), dev.reshape(-1)
    hw, dw, hc, dc = (a.astype(np.int64) for a in (h["w_depth"], d["w_depth"], h["w_color"], d["w_color"]))
    both = (hw > 0) & (dw > 0)
    allc = lambda a, v: (a["clr"] == v).all(axis=1)
    return dict(host_weight_0=int(((hw == 0) & (hc == 0) & (dw > 0) & (dc > 0) & (h["sdf"] != 32767) & (h["sdf"] != d["sdf"])).sum()),
                no_weight_anywhere=int(((hw == 0) & (hc == 0) & (dw == 0) & (dc == 0) & (d["sdf"] != 32767) & (d["clr"] != 0).all(axis=1)).sum()),
                device_weight_0=int(((dw == 0) & (hw > 0)).sum()), device_colour_weight_0=int(((dc == 0) & (hc > 0)).sum()),
                both_at_max=int(((hw == max_w) & (dw == max_w) & (hc == max_w) & (dc == max_w)).sum()),
                sum_is_max=int((both & (hw + dw == max_w)).sum()), sum_is_max_plus_1=int((both & (hw + dw == max_w + 1)).sum()),
                colour_sum_is_max=int(((hc > 0) & (dc > 0) & (hc + dc == max_w)).sum()),
                colour_sum_is_max_plus_1=int(((hc > 0) & (dc > 0) & (hc + dc == max_w + 1)).sum()),
                clamped=int((both & (hw + dw > max_w)).sum()),
                equal_sdf=int((both & (h["sdf"] == d["sdf"]) & (np.abs(h["sdf"]) < 32767)).sum()),
                plus_on_plus=int((both & (h["sdf"] == 32767) & (d["sdf"] == 32767)).sum()),
                minus_on_minus=int((both & (h["sdf"] == -32767) & (d["sdf"] == -32767)).sum()),
                plus_on_minus=int((both & (h["sdf"] == 32767) & (d["sdf"] == -32767)).sum()),
                colour_255_on_255=int(((hc > 0) & (dc > 0) & allc(h, 255) & allc(d, 255)).sum()),
                colour_0_on_255=int(((hc > 0) & (dc > 0) & allc(h, 0) & allc(d, 255)).sum()),
                depth_idle_colour_merges=int(((hw == 0) & (hc > 0)).sum()), colour_idle_depth_merges=int(((hw > 0) & (hc == 0)).sum()),
                unequal_weights=int(((hw != hc) & (hw > 0) & (hc > 0)).sum()))


def case_crafted_merge(api, pkg, synth, max_w, K=64):
    """A.8's merge with both sides chosen by the test: K blocks are overwritten with the host-side voxels and parked by
    ProcessFrame's swap-out, come back through an allocation pass, are overwritten with the device-side voxels and merged
    by a direct swap-in, and are parked again by a direct swap-out; every voxel against ref64.combine_stored."""
    host, dev = crafted_blocks(400 + max_w, K, max_w)
    reach = crafted_reach(host, dev, max_w)
    assert all(v >= 512 for v in reach.values()), reach
    lo, hi, info = ref64.combine_stored(host, dev, max_w)
    rnd = {k: v[:K // 2] for k, v in info.items()}
    share = ref64.merge_tie_share(rnd)
    if max_w == 100:  # the cap for weights up to 100, from the reference alone
        assert share <= 0.08, share
    out = dict(reach=reach, tie_share_random_half=share, tie_share_all=ref64.merge_tie_share(info))
    # the reference against itself where the answer is known without it
    assert np.array_equal(lo[host["w_depth"] == 0]["sdf"], dev[host["w_depth"] == 0]["sdf"])
    z = (dev["w_depth"] == 0) & (host["w_depth"] > 0)
    toward_zero = host[z]["sdf"] - np.sign(host[z]["sdf"])  # q is the host's value, an integer: a tie on its inner side
    assert np.array_equal(np.where(host[z]["sdf"] > 0, hi[z]["sdf"], lo[z]["sdf"]), host[z]["sdf"])
    assert np.array_equal(np.where(host[z]["sdf"] > 0, lo[z]["sdf"], hi[z]["sdf"]), toward_zero)
    assert np.array_equal(lo[z]["w_depth"], host[z]["w_depth"])

    rig, wl = _fused_rig(api, pkg, synth, [0], use_swapping=1, num_buckets=0x80, max_w=max_w)
    _, _, M0 = wl.frame(0)
    rgba1, mm1, M1 = wl.frame(120)
    # (1) K visible entries that the second pose does not keep
    ids, slots, pos = rig.m.resident_visible()
    _, enl = refmap.block_visibility(pos, M1, wl.intr, rig.m.vs, wl.W, wl.H)
    pick = np.nonzero(~enl)[0]
    assert len(pick) >= K, len(pick)
    pick = pick[np.linspace(0, len(pick) - 1, K).astype(np.int64)]
    ents, first_slots = ids[pick], slots[pick]
    rig.set_blocks(first_slots, host)
    untouched = rig.vox.copy()
    # (2) the camera turns away: ProcessFrame's swap-out parks them, byte for byte, and resets their slots
    rig.frame(rgba1, mm1)
    rig.process_frame(M1, wl.intr, "crafted: turned away")
    assert (rig.m.hash["ptr"][ents] == -1).all() and rig.m.has_stored[ents].all() and (rig.m.swap_state[ents] == 0).all()
    assert rig.stored[ents].tobytes() == host.tobytes() and rig.stored_hi[ents].tobytes() == host.tobytes()
    assert (rig.vox[first_slots] == EMPTY[0]).all()
    if api is not None:
        for t, b in zip(ents, host):
            has, blk = api.download_stored_block(rig.scene, int(t))
            assert has and blk.tobytes() == b.tobytes(), f"stored block of entry {t} is not the block that was parked"
        assert (api.download_voxel_blocks(rig.scene)[first_slots] == EMPTY[0]).all(), "a vacated slot is not empty"
    # (3) back at the first pose with an allocation pass alone: re-allocated, pending
    rgba0, mm0, _ = wl.frame(0)
    rig.frame(rgba0, mm0)
    a = rig.allocate(M0, wl.intr, what="crafted: back")
    new_slots = rig.m.hash["ptr"][ents].astype(np.int64)
    assert (new_slots >= 0).all() and (rig.m.swap_state[ents] == 1).all() and a["reallocated"] >= K, a
    rig.set_blocks(new_slots, dev)
    before = rig.vox.copy()
    stored_before = rig.stored.copy()
    rig.swap_in("crafted")
    assert (rig.m.swap_state[ents] == 2).all() and rig.m.last_swapped_in >= K
    assert np.array_equal(rig.stored, stored_before)
    others = np.setdiff1d(np.arange(rig.m.nl), rig.m.hash["ptr"][(rig.m.hash["ptr"] >= 0) & rig.m.has_stored])
    assert np.array_equal(rig.vox[others], before[others]) and len(others) >= 64
    if api is not None:
        got = api.download_voxel_blocks(rig.scene)
        out["figures"] = ref64.check_combined(got[new_slots], lo, hi, info, f"crafted merge, max_w {max_w}")
        out["figures_random_half"] = ref64.check_combined(got[new_slots[:K // 2]], lo[:K // 2], hi[:K // 2], rnd)
        assert got[others].tobytes() == before[others].tobytes(), "a block outside the merge changed"
        for t, b in zip(ents, host):
            assert api.download_stored_block(rig.scene, int(t))[1].tobytes() == b.tobytes(), "swap-in changed a stored copy"
        merged = got[new_slots]
    else:
        merged = None
    # (4) away again, an allocation pass and a direct swap-out: the stored copy is the merged block now
    rig.frame(rgba1, mm1)
    rig.allocate(M1, wl.intr, what="crafted: away again")
    rig.swap_out("crafted")
    assert (rig.m.hash["ptr"][ents] == -1).all() and rig.m.last_swapped_out >= K
    if api is not None:
        for t, b in zip(ents, merged):
            assert api.download_stored_block(rig.scene, int(t))[1].tobytes() == b.tobytes(), \
                f"entry {t}: the second park did not refresh the stored copy"
    out.update(merges=rig.merges, ties=rig.finish())
    return out


def case_flush(api, pkg, synth):
    """SaveToGlobalMemory on a scene with visible blocks, pending entries, and resident entries in state 0 with and
    without a host copy; then frames that re-allocate and merge what was flushed, a second flush (the stored copies are
    refreshed), Decay and SlideWindow."""
    rig, wl = _fused_rig(api, pkg, synth, [0], use_swapping=1, num_buckets=0x80)
    m = rig.m
    # resident entries in state 0 without a host copy: the table of a map, loaded into a scene that was reset
    table = (m.hash.copy(), m.alloc_list.copy(), m.last_free, m.excess_list.copy(), m.last_free_ex)
    rig.reset()
    rig.load(*table)
    slots = m.hash["ptr"][m.hash["ptr"] >= 0]
    rig.set_weights(slots[0::2], 3)
    f0 = rig.flush("never visible")
    assert f0["promoted"] == len(slots) >= 100 and f0["promoted_with_copy"] == 0 and f0["parked"] == len(slots), f0
    for i in (0, 40, 80):  # every block comes back and takes its copy in
        rgba, mm, M = wl.frame(i)
        rig.frame(rgba, mm)
        rig.process_frame(M, wl.intr, f"flush case, frame {i}")
    # resident entries in state 0 with a host copy: parked entries handed a block behind the engine's back
    h, al, lf = m.hash.copy(), m.alloc_list.copy(), m.last_free
    parked = np.nonzero((h["ptr"] == -1) & m.has_stored & (m.swap_state == 0))[0][::2]
    for t in parked:
        h["ptr"][t] = al[lf]
        lf -= 1
    rig.load(h, al, lf, m.excess_list, m.last_free_ex)
    give = m.hash["ptr"][parked]
    rig.set_weights(give[0::2], 3)
    rig.set_weights(give[1::2], m.max_w)
    # pending entries: an allocation pass at an earlier pose re-allocates parked blocks and leaves them in state 1
    rgba, mm, M = wl.frame(40)
    rig.frame(rgba, mm)
    a = rig.allocate(M, wl.intr, what="flush: pending")
    pending = int(((m.swap_state == 1) & m.has_stored & (m.hash["ptr"] >= 0)).sum())
    resident = int((m.hash["ptr"] >= 0).sum())
    f = rig.flush("first")
    assert pending >= 30 and f["promoted_with_copy"] >= 20, (pending, f, a)
    assert f["parked"] == resident and f["parked_visible"] >= 30 and not (m.hash["ptr"] >= 0).any(), f
    assert m.last_free == m.nl - 1 and not (m.swap_state != 0).any()
    listed_without_block = int((m.hash["ptr"][m.visible_ids] == -1).sum())
    assert listed_without_block >= 30  # the render state was not touched: the next pass finds these entries listed
    reach = dict(never_visible=f0, pending=pending, first=f, listed_without_block=listed_without_block)
    back = rig.process_frame(M, wl.intr, "after the flush")
    assert back["reallocated"] >= 30 and back["swapped_in"] >= 30 and back["retested"] >= 10, back
    rgba, mm, M = wl.frame(80)
    rig.frame(rgba, mm)
    rig.process_frame(M, wl.intr, "after the flush, turned")
    f2 = rig.flush("second")
    assert f2["parked"] >= 30 and f2["promoted"] == 0, f2
    rgba, mm, M = wl.frame(60)
    rig.frame(rgba, mm)
    again = rig.process_frame(M, wl.intr, "after the second flush")
    d = rig.decay(1, 0, True, "flush case")
    s = rig.slide_window(1, "flush case")
    s0 = rig.slide_window(0, "flush case")
    assert again["reallocated"] >= 30 and d["candidates"] >= 30 and s["parked"] + s0["parked"] >= 30, (again, d, s, s0)
    rig.flush("nothing resident")
    assert m.last_swapped_out == 0
    reach.update(second=f2, reallocated=back["reallocated"] + again["reallocated"], merges=rig.merges)
    assert rig.merges["blocks"] >= 100, rig.merges
    return dict(reach=reach, ties=rig.finish())


def case_defusion_ring(api, pkg, synth, swapping, first_ring):
    """The defusion ring (A.11): keyframes are fused, some are de-integrated and fused again at perturbed
    poses with isDefusion, so that their lists go to ring 1; then one ring is emptied (`first_ring`), the other one is
    decayed and trimmed, list by list, and emptied as well.  A block both rings hold must outlive either."""
    rig, wl = _fused_rig(api, pkg, synth, [], use_swapping=int(swapping), num_buckets=0x80)
    m = rig.m
    keyframes = [0, 10, 20, 30, 40, 50]
    for i in keyframes:
        rgba, mm, M = wl.frame(i)
        rig.frame(rgba, mm)
        rig.process_frame(M, wl.intr, f"keyframe {i}")
    defused = 0
    for k, i in enumerate((10, 30, 50, 20)):
        rgba, mm, M = wl.frame(i)
        rig.frame(rgba, mm)
        defused += rig.deprocess_frame(M, wl.intr, f"keyframe {i}")["defused_blocks"]
        rig.process_frame(turned(synth, wl, i, 0.05 * (k + 1), -0.04 * (k + 1)), wl.intr, f"keyframe {i} again", is_defusion=True)
    ring = [set().union(*m.lists[q].values()) for q in (0, 1)]
    reach = dict(only_fusion=len(ring[0] - ring[1]), only_defusion=len(ring[1] - ring[0]), both=len(ring[0] & ring[1]),
                 defused_blocks=defused)
    assert reach["only_defusion"] >= 30 and reach["both"] >= 30 and defused >= 100, reach
    # (a swapping scene has parked what left the view: every block still resident was listed by a re-fusion as well)
    assert reach["only_fusion"] >= (0 if swapping else 30), reach
    assert m.stats()["fusion_fifo_len"] == 6 and m.stats()["defusion_fifo_len"] == 4
    held = lambda: {int(s) for s in m.hash["ptr"][m.hash["ptr"] >= 0]}
    both = ring[0] & ring[1] & held()
    a = rig.decay(1, 1, False, "defusion ring, aged lists", defusion_part=True)
    assert a["candidates"] >= 30, a
    if first_ring == 0:
        w = rig.slide_window(2, "fusion ring to 2")
        w0 = rig.slide_window(0, "fusion ring to 0")
        gone = w["only_in_popped"] + w0["only_in_popped"]
        assert gone >= (0 if swapping else 30) and m.stats()["fusion_fifo_len"] == 0 and m.stats()["defusion_fifo_len"] == 4
        survivors = {s for s in both if m.referenced(s)} & held()
        assert len(survivors) >= 30 and all(any(s in l for l in m.lists[1].values()) for s in survivors), len(survivors)
        b = rig.decay(1, 0, True, "defusion ring, sweep", defusion_part=True)
        t = rig.slide_window_defusion_part(6, 3, "to 3")
        t1 = rig.slide_window_defusion_part(0, 1, "to 1")
        assert t["pops"] == 1 and t1["pops"] == 2 and m.stats()["defusion_fifo_len"] == 1
        t0 = rig.slide_window_defusion_part(6, 0, "to 0")
    else:
        t = rig.slide_window_defusion_part(6, 3, "to 3")
        t1 = rig.slide_window_defusion_part(0, 1, "to 1")
        assert t["pops"] == 1 and t1["pops"] == 2 and m.stats()["defusion_fifo_len"] == 1 and m.stats()["fusion_fifo_len"] == 6
        t0 = rig.slide_window_defusion_part(6, 0, "to 0")
        gone = t["only_in_popped"] + t1["only_in_popped"] + t0["only_in_popped"]
        assert gone >= 30 and m.stats()["defusion_fifo_len"] == 0
        survivors = {s for s in both if m.referenced(s)} & held()
        assert len(survivors) >= 30 and all(any(s in l for l in m.lists[0].values()) for s in survivors), len(survivors)
        b = rig.decay(1, 0, True, "fusion ring left, sweep", defusion_part=True)
        rig.slide_window(2, "fusion ring to 2")
        rig.slide_window(0, "fusion ring to 0")
    assert m.stats()["fusion_fifo_len"] == 0 and m.stats()["defusion_fifo_len"] == 0
    if swapping:
        assert not (m.hash["ptr"] >= 0).any() and m.has_stored.sum() >= 100  # every block parked, every entry kept
    else:
        assert not (m.hash["ptr"] >= -1).any() and m.last_free == m.nl - 1  # every block released
    reach.update(survivors=len(survivors), left_with_first_ring=gone, slid=m.slid, merges=rig.merges["blocks"])
    # a frame afterwards: the stacks, the table and (swapping) the host store are used as the calls left them
    rgba, mm, M = wl.frame(20)
    rig.frame(rgba, mm)
    rig.process_frame(M, wl.intr, "afterwards")
    return dict(reach=reach, ties=rig.finish())


# ---------------------------------------------------------------------------------------------------------------------
# seeded sequences
# ---------------------------------------------------------------------------------------------------------------------
FIRST_NEW_SEED = 12  # seeds below it run exactly the sequences they always ran


def seeds(default_count=18):
    spec = os.environ.get("DSLAM_MAPMODEL_SEEDS")
    if spec:
        first, count = (int(v) for v in spec.split(":"))
        return list(range(first, first + count))
    return list(range(default_count))


def run_sequence(api, pkg, synth, seed, n_calls=30, mu_vox=MU_OFF, script=None, swapping=None):
    """Seeds from FIRST_NEW_SEED on (and scripted sequences) also draw the defusion-ring calls, and every third of them
    runs on a scene with host swapping, where the direct swap calls and the flush join the mix.  What is new is drawn
    from a stream of its own (`xr`), so the calls and arguments of the older seeds are what they were."""
    rng = np.random.default_rng(1000 + seed)
    xr = np.random.default_rng(77000 + seed)
    new = seed >= FIRST_NEW_SEED or script is not None
    if swapping is None:
        swapping = new and seed % 3 == 0
    W, H = 96, 72
    wl = synth.s_tiny(W, H)
    kw = dict(use_swapping=1) if swapping else {}
    rig = Rig(api, pkg, scene_params(pkg, mu_vox=mu_vox, num_buckets=int(rng.choice([0x80, 0x100, 0x400])),
                                     num_local_blocks=int(rng.choice([0x300, 0x600, 0x1000])),
                                     num_excess=int(rng.choice([0x80, 0x400, 0x1000])), history_words=1, **kw), W, H)
    extra = ["refuse"] * 3 + ["slide_defusion", "decay_defusion"] + (["swap_in", "swap_out", "flush"] * 2 if swapping else [])
    log, infos, fused = [], [], []
    frame = int(rng.integers(0, 180))
    for k in range(len(script) if script is not None else n_calls):
        op = rng.choice(["frame"] * 6 + ["allocate"] * 2 + ["decay_sweep"] * 2 + ["decay_aged"] * 2 + ["slide"] * 2 + ["reset"])
        if script is not None:
            op = script[k]
        elif new and xr.random() < 0.45:
            op = xr.choice(extra)
        info = None
        if op in ("frame", "allocate"):
            frame += int(rng.integers(1, 12))
            rgba, mm, _ = wl.frame(frame)
            rig.frame(rgba, mm)
            M = turned(synth, wl, frame, float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.15, 0.15)))
            if op == "frame":
                info = rig.process_frame(M, wl.intr, f"seed {seed}")
                fused.append((frame, M))
            else:
                info = rig.allocate(M, wl.intr, only=bool(rng.integers(0, 2)), what=f"seed {seed}")
        elif op == "reset":
            rig.reset()
            fused = []
        elif op == "slide":
            info = rig.slide_window(int(rng.integers(0, 5)), f"seed {seed}")
        elif op in ("decay_sweep", "decay_aged"):
            info = rig.decay(int(rng.choice([1, 2, 255])), int(rng.integers(0, 4)), op == "decay_sweep", f"seed {seed}")
        elif op == "refuse":  # online correction's step: a fused keyframe leaves the map and comes back at a corrected pose
            if fused:
                j = int(xr.integers(0, len(fused)))
                f, M = fused[j]
                rgba, mm, _ = wl.frame(f)
                rig.frame(rgba, mm)
                rig.deprocess_frame(M, wl.intr, f"seed {seed}")
                M = turned(synth, wl, f, float(xr.uniform(-0.2, 0.2)), float(xr.uniform(-0.15, 0.15)))
                info = rig.process_frame(M, wl.intr, f"seed {seed}", is_defusion=True)
                fused[j] = (f, M)
        elif op == "slide_defusion":
            info = rig.slide_window_defusion_part(int(xr.integers(0, 5)), int(xr.integers(0, 4)), f"seed {seed}")
        elif op == "decay_defusion":
            info = rig.decay(int(xr.choice([1, 2, 255])), int(xr.integers(0, 3)), bool(xr.integers(0, 2)), f"seed {seed}",
                             defusion_part=True)
        elif op == "swap_in":
            info = rig.swap_in(f"seed {seed}")
        elif op == "swap_out":
            info = rig.swap_out(f"seed {seed}")
        elif op == "flush":
            info = rig.flush(f"seed {seed}")
        else:
            raise ValueError(op)
        log.append(str(op))
        infos.append(info)
    return dict(ops=log, infos=infos, swapping=bool(swapping), decayed=rig.m.decayed, slid=rig.m.slid, merges=rig.merges,
                ties=rig.finish())


FLUSH_SCRIPT = ["frame", "frame", "frame", "flush", "frame", "frame", "decay_sweep", "slide", "frame", "allocate", "swap_in",
                "flush", "frame", "refuse", "swap_out", "slide_defusion", "frame"]


def case_flush_sequence(api, pkg, synth):
    """A scripted sequence at the sequences' size: a flush followed by frames that re-allocate and merge the flushed
    blocks, a Decay and a SlideWindow, then a second flush behind a direct swap-in."""
    out = run_sequence(api, pkg, synth, 2, script=FLUSH_SCRIPT, swapping=True)
    i = FLUSH_SCRIPT.index("flush")
    assert out["infos"][i]["parked"] >= 100 and out["infos"][i]["parked_visible"] >= 50, out["infos"][i]
    after = out["infos"][i + 1]
    assert after["reallocated"] >= 50 and after["swapped_in"] >= 50, after
    assert out["infos"][i + 3]["candidates"] >= 30 and out["infos"][i + 4]["parked"] >= 30, out["infos"][i + 3:i + 5]
    assert out["merges"]["blocks"] >= 200, out["merges"]
    return out


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
