"""ctypes view of the C ABI declared in include/dslam_fusion.h.

`CApi(path, prefix)` binds one shared library that exports the dslam_fusion.h entry points under a symbol
prefix.  The product binds libdslam_fusion.so with prefix ``dslam_`` (see __init__.py); the test suite binds
the CPU oracle with prefix ``oracle_`` through the same class so parity tests drive both identically.
Nothing in this file computes anything: it converts numpy arrays to pointers and back.

Matrix convention: Python callers pass ordinary 4x4 arrays indexed M[row, col]; the ABI wants
ORUtils::Matrix4f storage, column-major float[16] (reference: InfiniTamDriver.cpp:208-226), i.e. M.T.ravel().
"""
import ctypes as C
import os

import numpy as np

HASH_ENTRY_DTYPE = np.dtype(
    {"names": ["pos", "_pad", "offset", "ptr"], "formats": [("<i2", 3), "<i2", "<i4", "<i4"], "offsets": [0, 6, 8, 12],
     "itemsize": 16})
VOXEL_DTYPE = np.dtype(
    {"names": ["sdf", "w_depth", "clr", "w_color", "_pad"], "formats": ["<i2", "u1", ("u1", 3), "u1", "u1"],
     "offsets": [0, 2, 3, 6, 7], "itemsize": 8})

BLOCK_SIZE3 = 512
IMAGE_SHADED, IMAGE_COLOUR_FROM_VOLUME, IMAGE_COLOUR_FROM_NORMAL, IMAGE_DEPTH = 0, 1, 2, 3
MAX_RENDER_MAPS = 64  # DSLAM_MAX_RENDER_MAPS


class SceneParams(C.Structure):
    """dslam_scene_params (ITMSceneParams + pool sizes)."""
    _fields_ = [("voxel_size", C.c_float), ("mu", C.c_float), ("max_w", C.c_int32), ("frustum_min", C.c_float),
                ("frustum_max", C.c_float), ("stop_integrating_at_max_w", C.c_int32),
                ("num_local_blocks", C.c_int32), ("num_buckets", C.c_int32), ("num_excess", C.c_int32),
                ("use_swapping", C.c_int32), ("history_words", C.c_int32)]

    def __init__(self, voxel_size=0.005, mu=0.02, max_w=100, frustum_min=0.2, frustum_max=3.0,
                 stop_integrating_at_max_w=0, num_local_blocks=0, num_buckets=0, num_excess=0, use_swapping=0,
                 history_words=0):
        super().__init__(voxel_size, mu, max_w, frustum_min, frustum_max, stop_integrating_at_max_w,
                         num_local_blocks, num_buckets, num_excess, use_swapping, history_words)


class TrackerParams(C.Structure):
    """dslam_tracker_params (ITMLibSettings' depth-tracker fields; upstream defaults)."""
    _fields_ = [("no_hierarchy_levels", C.c_int32), ("no_icp_run_till_level", C.c_int32), ("dist_thresh", C.c_float),
                ("termination_threshold", C.c_float), ("regime", C.c_int32 * 8)]

    def __init__(self, levels=5, run_till_level=0, dist_thresh=0.1 * 0.1, termination_threshold=1e-3, regime=None):
        regime = list(regime) if regime is not None else [3, 3, 1, 1, 1]
        regime = (regime + [4] * 8)[:8]
        super().__init__(levels, run_till_level, dist_thresh, termination_threshold, (C.c_int32 * 8)(*regime))


class TrackerResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("valid_points_last", C.c_int32), ("f_last", C.c_float), ("pad", C.c_int32)]


class TrackSdfParams(C.Structure):
    """dslam_track_sdf_params; a field left at 0 selects its default (run_till_level 0 is the full resolution)."""
    _fields_ = [("no_hierarchy_levels", C.c_int32), ("run_till_level", C.c_int32), ("max_evaluations", C.c_int32),
                ("min_valid", C.c_int32), ("residual_gate", C.c_float), ("term_rotation", C.c_float),
                ("term_translation_voxels", C.c_float), ("pad", C.c_int32)]

    def __init__(self, no_hierarchy_levels=0, run_till_level=0, max_evaluations=0, min_valid=0, residual_gate=0.0,
                 term_rotation=0.0, term_translation_voxels=0.0):
        super().__init__(no_hierarchy_levels, run_till_level, max_evaluations, min_valid, residual_gate, term_rotation,
                         term_translation_voxels, 0)


class TrackSdfResult(C.Structure):
    """dslam_track_sdf_result."""
    _fields_ = [("evaluations", C.c_int32), ("levels_stepped", C.c_int32), ("stop_reason", C.c_int32),
                ("candidates", C.c_int32), ("valid_last", C.c_int32), ("cost_first", C.c_float), ("cost_last", C.c_float),
                ("conditioning", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(TrackSdfParams) == 32 and C.sizeof(TrackSdfResult) == 32  # the header's layouts


class TrackSdfRgbParams(C.Structure):
    """dslam_track_sdf_rgb_params: dslam_track_sdf_params (its fields are this constructor's too) and the photometric
    term's colour_weight (0 -> 1), colour_gate (0 -> 0.25), colour_levels (0 -> 1)."""
    _fields_ = [("base", TrackSdfParams), ("colour_weight", C.c_float), ("colour_gate", C.c_float),
                ("colour_levels", C.c_int32), ("pad", C.c_int32)]

    def __init__(self, colour_weight=0.0, colour_gate=0.0, colour_levels=0, **base):
        super().__init__(TrackSdfParams(**base), colour_weight, colour_gate, colour_levels, 0)


class TrackSdfRgbResult(C.Structure):
    """dslam_track_sdf_rgb_result."""
    _fields_ = [("base", TrackSdfResult), ("colour_valid_last", C.c_int32), ("colour_rms_last", C.c_float),
                ("cost_depth_last", C.c_float), ("cost_colour_last", C.c_float)]

    def as_dict(self):
        return dict(self.base.as_dict(), **{n: getattr(self, n) for n, _ in self._fields_[1:]})


assert C.sizeof(TrackSdfRgbParams) == 48 and C.sizeof(TrackSdfRgbResult) == 48  # the header's layouts


MAX_TRACK_STARTS = 256   # DSLAM_MAX_TRACK_STARTS


class PoseScore(C.Structure):
    """dslam_pose_score."""
    _fields_ = [("candidates", C.c_int32), ("valid", C.c_int32), ("cost", C.c_float), ("pad", C.c_int32)]


class PoseLattice(C.Structure):
    """dslam_pose_lattice: nt translation nodes to each side per world axis, step_t metres apart; nr rotation nodes to each
    side about `axis`, step_r radians apart."""
    _fields_ = [("nt", C.c_int32 * 3), ("step_t", C.c_float), ("nr", C.c_int32), ("step_r", C.c_float), ("axis", C.c_float * 3),
                ("pad", C.c_int32)]

    def __init__(self, nt=(0, 0, 0), step_t=0.0, nr=0, step_r=0.0, axis=(0.0, 0.0, 0.0)):
        super().__init__((C.c_int32 * 3)(*nt), step_t, nr, step_r, (C.c_float * 3)(*axis), 0)

    @property
    def count(self):
        return (2 * self.nr + 1) * (2 * self.nt[0] + 1) * (2 * self.nt[1] + 1) * (2 * self.nt[2] + 1)


assert C.sizeof(PoseScore) == 16 and C.sizeof(PoseLattice) == 40  # the header's layouts


class RegisterParams(C.Structure):
    """dslam_register_params; a field left at 0 selects its default."""
    _fields_ = [("band", C.c_float), ("residual_gate", C.c_float), ("max_evaluations", C.c_int32),
                ("min_valid", C.c_int32), ("term_rotation", C.c_float), ("term_translation_voxels", C.c_float)]

    def __init__(self, band=0.0, residual_gate=0.0, max_evaluations=0, min_valid=0, term_rotation=0.0,
                 term_translation_voxels=0.0):
        super().__init__(band, residual_gate, max_evaluations, min_valid, term_rotation, term_translation_voxels)


class RegisterResult(C.Structure):
    """dslam_register_result."""
    _fields_ = [("evaluations", C.c_int32), ("stop_reason", C.c_int32), ("candidates", C.c_int32),
                ("valid_last", C.c_int32), ("cost_first", C.c_float), ("cost_last", C.c_float),
                ("conditioning", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(RegisterParams) == 24 and C.sizeof(RegisterResult) == 32  # the header's layouts

MAX_REGISTER_PAIRS = 128   # DSLAM_MAX_REGISTER_PAIRS


class RegisterGraphResult(C.Structure):
    """dslam_register_graph_result."""
    _fields_ = [("evaluations", C.c_int32), ("stop_reason", C.c_int32), ("active_pairs", C.c_int32),
                ("cost_first", C.c_float), ("cost_last", C.c_float), ("conditioning", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RegisterPairResult(C.Structure):
    """dslam_register_pair_result."""
    _fields_ = [("candidates", C.c_int32), ("valid_first", C.c_int32), ("valid_last", C.c_int32), ("active", C.c_int32),
                ("cost_first", C.c_float), ("cost_last", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(RegisterGraphResult) == 24 and C.sizeof(RegisterPairResult) == 24  # the header's layouts


class PairSelectParams(C.Structure):
    """dslam_pair_select_params; min_shared_octants / max_pairs left at 0 select their defaults."""
    _fields_ = [("min_shared_octants", C.c_int32), ("one_direction", C.c_int32), ("max_pairs", C.c_int32), ("pad", C.c_int32)]

    def __init__(self, min_shared_octants=0, one_direction=0, max_pairs=0):
        super().__init__(min_shared_octants, one_direction, max_pairs, 0)


class PairSelectResult(C.Structure):
    """dslam_pair_select_result."""
    _fields_ = [("qualifying", C.c_int32), ("selected", C.c_int32), ("num_components", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(PairSelectParams) == 16 and C.sizeof(PairSelectResult) == 16  # the header's layouts


MAX_SURVEY_MAPS, MAX_SURVEY_VIEWS = 256, 16   # DSLAM_MAX_SURVEY_MAPS, DSLAM_MAX_SURVEY_VIEWS


class SurveyView(C.Structure):
    """dslam_survey_view: M world -> camera as the ABI stores it (column-major), intrinsics (fx, fy, cx, cy), image size,
    near and far distance in metres (far_m 0: no far plane)."""
    _fields_ = [("M", C.c_float * 16), ("intrinsics", C.c_float * 4), ("width", C.c_int32), ("height", C.c_int32),
                ("near_m", C.c_float), ("far_m", C.c_float)]

    @classmethod
    def of(cls, M, intr, width, height, near_m, far_m):
        """From a 4x4 math matrix (M[row, col]) and (fx, fy, cx, cy)."""
        return cls((C.c_float * 16)(*mat_to_abi(M).tolist()), (C.c_float * 4)(*np.asarray(intr, np.float32).tolist()),
                   int(width), int(height), float(near_m), float(far_m))


class ViewSurveyParams(C.Structure):
    """dslam_view_survey_params; margin_voxels left at 0 selects its default."""
    _fields_ = [("margin_voxels", C.c_float), ("pad", C.c_int32 * 3)]

    def __init__(self, margin_voxels=0.0):
        super().__init__(margin_voxels, (C.c_int32 * 3)(0, 0, 0))


class ViewSelectParams(C.Structure):
    """dslam_view_select_params; min_blocks / max_maps left at 0 select their defaults, always_keep -1: no map."""
    _fields_ = [("min_blocks", C.c_int32), ("max_maps", C.c_int32), ("always_keep", C.c_int32), ("pad", C.c_int32)]

    def __init__(self, min_blocks=0, max_maps=0, always_keep=-1):
        super().__init__(min_blocks, max_maps, always_keep, 0)


class ViewSelectResult(C.Structure):
    """dslam_view_select_result."""
    _fields_ = [("reaching", C.c_int32), ("selected", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(SurveyView) == 96 and C.sizeof(ViewSurveyParams) == 16  # the header's layouts
assert C.sizeof(ViewSelectParams) == 16 and C.sizeof(ViewSelectResult) == 8


FERN_MAX_MATCHES, FERN_MAX_QUERIES, FERN_CODE_DWORDS = 64, 64, 64   # DSLAM_FERN_MAX_MATCHES, _MAX_QUERIES, _CODE_DWORDS


class FernParams(C.Structure):
    """dslam_fern_params; a field left at 0 selects its default (seed has none)."""
    _fields_ = [("num_ferns", C.c_int32), ("cell", C.c_int32), ("channels", C.c_int32), ("depth_min_mm", C.c_int32),
                ("depth_max_mm", C.c_int32), ("seed", C.c_uint32)]

    def __init__(self, num_ferns=0, cell=0, channels=0, depth_min_mm=0, depth_max_mm=0, seed=0):
        super().__init__(num_ferns, cell, channels, depth_min_mm, depth_max_mm, seed)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FernMatch(C.Structure):
    """dslam_fern_match."""
    _fields_ = [("id", C.c_int32), ("dissimilarity", C.c_int32)]


FERN_MATCH_DTYPE = np.dtype([("id", "<i4"), ("dissimilarity", "<i4")])
assert C.sizeof(FernParams) == 24 and C.sizeof(FernMatch) == 8 and FERN_MATCH_DTYPE.itemsize == 8  # the header's layouts


QUERY_MAX_ELEMENTS, QUERY_MAX_RAY_VOXELS = 1 << 24, 16384   # DSLAM_QUERY_MAX_ELEMENTS, DSLAM_QUERY_MAX_RAY_VOXELS
QUERY_SDF, QUERY_GRADIENT, QUERY_COLOUR = 1, 2, 4           # DSLAM_QUERY_SDF, _GRADIENT, _COLOUR
QUERY_ALL = QUERY_SDF | QUERY_GRADIENT | QUERY_COLOUR
QUERY_OUTSIDE = 1                                           # DSLAM_QUERY_OUTSIDE


class PointSample(C.Structure):
    """dslam_point_sample."""
    _fields_ = [("sdf", C.c_float), ("weight", C.c_float), ("grad", C.c_float * 3), ("colour", C.c_float * 3),
                ("found_lo", C.c_uint32), ("found_hi", C.c_uint32), ("status", C.c_int32), ("pad", C.c_int32)]


class RayHit(C.Structure):
    """dslam_ray_hit."""
    _fields_ = [("t", C.c_float), ("point", C.c_float * 3), ("normal", C.c_float * 3), ("colour", C.c_float * 3),
                ("status", C.c_int32), ("steps", C.c_int32)]


POINT_SAMPLE_DTYPE = np.dtype([("sdf", "<f4"), ("weight", "<f4"), ("grad", "<f4", (3,)), ("colour", "<f4", (3,)),
                               ("found_lo", "<u4"), ("found_hi", "<u4"), ("status", "<i4"), ("pad", "<i4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)), ("colour", "<f4", (3,)),
                          ("status", "<i4"), ("steps", "<i4")])
assert C.sizeof(PointSample) == C.sizeof(RayHit) == POINT_SAMPLE_DTYPE.itemsize == RAY_HIT_DTYPE.itemsize == 48  # the header's layouts


GRID_MAX_CELL, GRID_MAX_DIM, GRID_MAX_CELLS = 64, 1024, 1 << 26   # DSLAM_GRID_MAX_CELL, _MAX_DIM, _MAX_CELLS
CELL_OBSERVED, CELL_OCCUPIED = 1, 2                              # DSLAM_CELL_OBSERVED, _OCCUPIED
SEED_OCCUPIED, SEED_UNKNOWN = 1, 2                               # DSLAM_SEED_OCCUPIED, _UNKNOWN
DIST_SQUARED_CELLS, DIST_METRES = 0, 1                           # DSLAM_DIST_SQUARED_CELLS, _METRES
DIST_MAX_CELLS, DIST_FAR = 1774, 0x7FFFFFFF                      # DSLAM_DIST_MAX_CELLS, DSLAM_DIST_FAR


class Grid(C.Structure):
    """dslam_grid: a world-aligned box of cells in world voxel units."""
    _fields_ = [("origin", C.c_int32 * 3), ("cell", C.c_int32), ("dims", C.c_int32 * 3), ("pad", C.c_int32)]

    @classmethod
    def of(cls, origin, cell, dims, pad=0):
        return cls((C.c_int32 * 3)(*[int(v) for v in origin]), int(cell), (C.c_int32 * 3)(*[int(v) for v in dims]), int(pad))

    @property
    def cells(self):
        return int(self.dims[0]) * int(self.dims[1]) * int(self.dims[2])


GRID_DTYPE = np.dtype([("origin", "<i4", (3,)), ("cell", "<i4"), ("dims", "<i4", (3,)), ("pad", "<i4")])
assert C.sizeof(Grid) == GRID_DTYPE.itemsize == 32  # the header's layout


STEREO_INVALID, STEREO_COST_OUT, STEREO_MAX_SIZE, STEREO_MAX_P2 = 0xFFFF, 63, 4096, 192   # DSLAM_STEREO_INVALID, _COST_OUT, _MAX_SIZE, _MAX_P2
STEREO_CENSUS_LEFT, STEREO_CENSUS_RIGHT, STEREO_S = 0, 1, 2                              # DSLAM_STEREO_CENSUS_LEFT, _CENSUS_RIGHT, _S


class StereoParams(C.Structure):
    """dslam_stereo_params in the header's encoding: a field left at 0 selects its default; uniqueness -1 = off; lr_max -1 =
    check off, -2 = exact.  effective(): what the law takes (uniqueness 0 = off, lr_max -1 = off, 0 = exact)."""
    _fields_ = [("max_disparity", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness", C.c_int32),
                ("lr_max", C.c_int32), ("channels", C.c_int32), ("pad", C.c_int32 * 2)]

    def __init__(self, max_disparity=0, p1=0, p2=0, uniqueness=0, lr_max=0, channels=0):
        super().__init__(max_disparity, p1, p2, uniqueness, lr_max, channels)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}

    def effective(self):
        d = self.as_dict()
        d["uniqueness"] = max(d["uniqueness"], 0)
        d["lr_max"] = 0 if d["lr_max"] == -2 else d["lr_max"]
        return d


class StereoCalib(C.Structure):
    """dslam_stereo_calib."""
    _fields_ = [("focal_length_px", C.c_float), ("baseline_m", C.c_float), ("scale", C.c_float), ("min_depth_m", C.c_float),
                ("max_depth_m", C.c_float)]


STEREO_PARAMS_DTYPE = np.dtype([("max_disparity", "<i4"), ("p1", "<i4"), ("p2", "<i4"), ("uniqueness", "<i4"), ("lr_max", "<i4"),
                                ("channels", "<i4"), ("pad", "<i4", (2,))])
STEREO_CALIB_DTYPE = np.dtype([("focal_length_px", "<f4"), ("baseline_m", "<f4"), ("scale", "<f4"), ("min_depth_m", "<f4"),
                               ("max_depth_m", "<f4")])
assert C.sizeof(StereoParams) == STEREO_PARAMS_DTYPE.itemsize == 32 and C.sizeof(StereoCalib) == STEREO_CALIB_DTYPE.itemsize == 20


# DSLAM_SFLOW_MAX_SIZE, _MAX_NMS_N, _MAX_BINS, _MAX_FEATURES, _MARGIN, _MAX_COST, _SOBEL_BOUND, _CHECKER_BOUND
SFLOW_MAX_SIZE, SFLOW_MAX_NMS_N, SFLOW_MAX_BINS, SFLOW_MAX_FEATURES, SFLOW_MARGIN, SFLOW_MAX_COST = 4096, 32, 65536, 4194304, 9, 8160
SFLOW_SOBEL_BOUND, SFLOW_CHECKER_BOUND = 12240, 2040
SFLOW_FEATURE_BYTES, SFLOW_MATCH_WORDS = 48, 12                                  # DSLAM_SFLOW_FEATURE_BYTES, _MATCH_WORDS
SFLOW_IMAGE_1C, SFLOW_IMAGE_2C, SFLOW_IMAGE_1P, SFLOW_IMAGE_2P = 0, 1, 2, 3      # DSLAM_SFLOW_IMAGE_*
SFLOW_FILTER_DU, SFLOW_FILTER_DV, SFLOW_FILTER_F1, SFLOW_FILTER_F2 = 0, 1, 2, 3  # DSLAM_SFLOW_FILTER_*


class SflowParams(C.Structure):
    """dslam_sflow_params in the header's encoding: a field left at 0 selects its default; half_resolution -1 = off.
    effective(): what the law takes (half_resolution 0 = off)."""
    _fields_ = [("nms_n", C.c_int32), ("nms_tau", C.c_int32), ("match_binsize", C.c_int32), ("match_radius", C.c_int32),
                ("match_disp_tolerance", C.c_int32), ("half_resolution", C.c_int32), ("channels", C.c_int32), ("pad", C.c_int32)]

    def __init__(self, nms_n=0, nms_tau=0, match_binsize=0, match_radius=0, match_disp_tolerance=0, half_resolution=0, channels=0):
        super().__init__(nms_n, nms_tau, match_binsize, match_radius, match_disp_tolerance, half_resolution, channels)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}

    def effective(self):
        d = self.as_dict()
        d["half_resolution"] = max(d["half_resolution"], 0)
        return d


SFLOW_PARAMS_DTYPE = np.dtype([("nms_n", "<i4"), ("nms_tau", "<i4"), ("match_binsize", "<i4"), ("match_radius", "<i4"),
                               ("match_disp_tolerance", "<i4"), ("half_resolution", "<i4"), ("channels", "<i4"), ("pad", "<i4")])
assert C.sizeof(SflowParams) == SFLOW_PARAMS_DTYPE.itemsize == 32


class MergeParams(C.Structure):
    """dslam_merge_params; max_passes = 0 selects its default."""
    _fields_ = [("max_passes", C.c_int32), ("with_colour", C.c_int32)]

    def __init__(self, max_passes=0, with_colour=1):
        super().__init__(max_passes, with_colour)


class MergeResult(C.Structure):
    """dslam_merge_result."""
    _fields_ = [("passes", C.c_int32), ("exhausted", C.c_int32), ("src_blocks", C.c_int32),
                ("blocks_allocated", C.c_int32), ("blocks_touched", C.c_int32), ("requests_unserved", C.c_int32),
                ("src_candidates", C.c_int64), ("out_of_range", C.c_int64), ("voxels_changed", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(MergeParams) == 8 and C.sizeof(MergeResult) == 48  # the header's layouts


class UnmergeParams(C.Structure):
    """dslam_unmerge_params."""
    _fields_ = [("with_colour", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, with_colour=1):
        super().__init__(with_colour, 0)


class UnmergeResult(C.Structure):
    """dslam_unmerge_result."""
    _fields_ = [("src_blocks", C.c_int32), ("blocks_touched", C.c_int32), ("src_candidates", C.c_int64),
                ("out_of_range", C.c_int64), ("candidates_without_block", C.c_int64), ("voxels_changed", C.c_int64),
                ("depth_underweight", C.c_int64), ("colour_underweight", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(UnmergeParams) == 8 and C.sizeof(UnmergeResult) == 56  # the header's layouts


class PackInfo(C.Structure):
    """dslam_pack_info: the 64-byte header of a packed map, as it lies in the buffer."""
    _fields_ = [("magic", C.c_char * 4), ("version", C.c_uint32), ("num_buckets", C.c_int32), ("num_excess", C.c_int32),
                ("blocks", C.c_int32), ("free_excess", C.c_int32), ("voxel_size_bits", C.c_uint32), ("mu_bits", C.c_uint32),
                ("blocks_offset", C.c_int64), ("total_bytes", C.c_int64), ("bbox_min", C.c_int16 * 3),
                ("bbox_max", C.c_int16 * 3), ("reserved", C.c_uint32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["bbox_min"], d["bbox_max"] = list(self.bbox_min), list(self.bbox_max)
        return d


class WeightParams(C.Structure):
    _fields_ = [("depth_weighting", C.c_int32), ("max_new_w", C.c_int32), ("max_distance", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("num_allocated_blocks", C.c_int32), ("last_free_block_id", C.c_int32),
                ("last_free_excess_id", C.c_int32), ("no_visible_entries", C.c_int32),
                ("decayed_block_count", C.c_int64), ("slid_block_count", C.c_int64), ("frame_counter", C.c_int32),
                ("fusion_fifo_len", C.c_int32), ("defusion_fifo_len", C.c_int32), ("alloc_failures", C.c_int32),
                ("last_swapped_in", C.c_int32), ("last_swapped_out", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DslamError(RuntimeError):
    pass


def mat_to_abi(M):
    """4x4 math matrix (M[row, col]) -> column-major float32[16] as the ABI expects."""
    M = np.asarray(M, dtype=np.float32)
    if M.shape != (4, 4):
        raise ValueError("expected a 4x4 matrix")
    return np.ascontiguousarray(M.T).ravel()


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _vptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Handle:
    def __init__(self, api, ptr, destroy):
        self.api, self.ptr, self._destroy = api, ptr, destroy

    def close(self):
        if self.ptr:
            self._destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene(_Handle):
    pass


class RenderState(_Handle):
    width = 0
    height = 0


class View(_Handle):
    pass


class FrameStore(_Handle):
    pass


class FernIndex(_Handle):
    pass


class Stereo(_Handle):
    pass


class Sflow(_Handle):
    pass


class CApi:
    """One bound library.  Also plays the role of the engine handle (one engine per CApi instance)."""

    def __init__(self, path, prefix, has_engine_device=True, device=0):
        if not os.path.exists(path):
            raise DslamError(f"shared library not found: {path} (run __graft_entry__.build())")
        self.lib = C.CDLL(path)
        self.prefix = prefix
        self.path = path
        self._engine = C.c_void_p()
        self._pinned = {}
        if has_engine_device:
            self._check(self._fn("engine_create")(C.c_int(device), C.byref(self._engine)), "engine_create")
        else:
            self._check(self._fn("engine_create")(C.byref(self._engine)), "engine_create")

    # -- plumbing --------------------------------------------------------------------------------------
    def _fn(self, name):
        f = getattr(self.lib, self.prefix + name)
        f.restype = C.c_int
        return f

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    def _check(self, rc, what):
        if rc < 0:
            msg = ""
            if hasattr(self.lib, self.prefix + "last_error"):
                g = getattr(self.lib, self.prefix + "last_error")
                g.restype = C.c_char_p
                msg = (g() or b"").decode()
            raise DslamError(f"{self.prefix}{what} failed with status {rc} {msg}")
        return rc

    def _call(self, name, *args):
        return self._check(self._fn(name)(*args), name)

    def close(self):
        if self._engine:
            self._fn("engine_destroy")(self._engine)
            self._engine = C.c_void_p()

    # -- engine ----------------------------------------------------------------------------------------
    def set_async(self, flag):
        self._call("engine_set_async", self._engine, C.c_int(int(flag)))

    def device_numa_node(self, device=0):
        """NUMA node of the host the device hangs off (-1: unknown) -- HIP engine"""
        node = C.c_int(-1)
        self._call("device_numa_node", C.c_int(int(device)), C.byref(node))
        return node.value

    def selftest_division(self, samples):
        out = C.c_longlong(-1)
        self._call("selftest_division", self._engine, C.c_longlong(samples), C.byref(out))
        return out.value

    def debug_set_render_tile_budget(self, budget):
        self._call("debug_set_render_tile_budget", self._engine, C.c_int(budget))

    def synchronize(self):
        self._call("engine_synchronize", self._engine)

    # fences: markers in the engine's stream for callers that pipeline frames across PCIe (async mode)
    def fence_create(self):
        h = C.c_void_p()
        self._call("fence_create", self._engine, C.byref(h))
        return _Handle(self, h, self._fn("fence_destroy"))

    def fence_record(self, fence):
        self._call("fence_record", self._engine, fence.ptr)

    def fence_wait(self, fence):
        self._call("fence_wait", fence.ptr)

    def fence_query(self, fence):
        done = C.c_int(0)
        self._call("fence_query", fence.ptr, C.byref(done))
        return bool(done.value)

    def stream(self):
        f = getattr(self.lib, self.prefix + "engine_stream")
        f.restype = C.c_void_p
        return f(self._engine)

    def set_threads(self, n):  # oracle only
        self._call("engine_set_threads", self._engine, C.c_int(n))

    def max_threads(self):  # oracle only
        return self._fn("max_threads")()

    def set_fusion_weight_params(self, depth_weighting=False, max_new_w=1, max_distance=1.0):
        w = WeightParams(int(depth_weighting), int(max_new_w), float(max_distance))
        self._call("set_fusion_weight_params", self._engine, C.byref(w))

    # -- objects ---------------------------------------------------------------------------------------
    def create_scene(self, params, ext_voxel_blocks_dev=None):
        h = C.c_void_p()
        if self.prefix == "dslam_":
            self._call("scene_create", self._engine, C.byref(params), C.c_void_p(ext_voxel_blocks_dev or 0), C.byref(h))
        else:
            self._call("scene_create", self._engine, C.byref(params), C.byref(h))
        s = Scene(self, h, self._fn("scene_destroy"))
        p = SceneParams()
        self._call("scene_get_params", h, C.byref(p))
        s.params = p
        s.n_entries = p.num_buckets + p.num_excess
        return s

    def reset_scene(self, scene):
        self._call("scene_reset", self._engine, scene.ptr)

    def set_shard(self, scene, shard, num_shards, chunk_blocks=256):
        self._call("scene_set_shard", scene.ptr, C.c_int(shard), C.c_int(num_shards), C.c_int(chunk_blocks))

    def set_shard_range(self, scene, first_block, num_blocks):
        self._call("scene_set_shard_range", scene.ptr, C.c_int(first_block), C.c_int(num_blocks))

    def create_render_state(self, scene, width, height):
        h = C.c_void_p()
        self._call("render_state_create", self._engine, scene.ptr, C.c_int(width), C.c_int(height), C.byref(h))
        r = RenderState(self, h, self._fn("render_state_destroy"))
        r.width, r.height, r.n_entries, r.n_local = width, height, scene.n_entries, scene.params.num_local_blocks
        return r

    def create_view(self, width, height, width_d=None, height_d=None):
        h = C.c_void_p()
        width_d = width if width_d is None else width_d
        height_d = height if height_d is None else height_d
        self._call("view_create", self._engine, C.c_int(width), C.c_int(height), C.c_int(width_d), C.c_int(height_d),
                   C.byref(h))
        v = View(self, h, self._fn("view_destroy"))
        v.width, v.height, v.width_d, v.height_d = width, height, width_d, height_d
        return v

    # -- view ------------------------------------------------------------------------------------------
    def view_update(self, view, rgba, depth_mm, affine_a=1.0 / 1000.0, affine_b=0.0, timestamp=0.0, bilateral=False):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert rgba.size == view.width * view.height * 4 and depth_mm.size == view.width_d * view.height_d
        self._call("view_update", self._engine, view.ptr, _vptr(rgba), _vptr(depth_mm), C.c_float(affine_a),
                   C.c_float(affine_b), C.c_double(timestamp), C.c_int(int(bilateral)))

    def view_update_device(self, view, rgba_dev_ptr, depth_dev_ptr, affine_a=1.0 / 1000.0, affine_b=0.0,
                           timestamp=0.0, bilateral=False):
        self._call("view_update_device", self._engine, view.ptr, C.c_void_p(rgba_dev_ptr), C.c_void_p(depth_dev_ptr),
                   C.c_float(affine_a), C.c_float(affine_b), C.c_double(timestamp), C.c_int(int(bilateral)))

    def view_update_bgr(self, view, bgr, depth_mm, affine_a=1.0 / 1000.0, affine_b=0.0, timestamp=0.0, bilateral=False):
        """CvToItm + UpdateView: packed OpenCV BGR (H, W, 3) in, converted to RGBA on the device."""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert bgr.size == view.width * view.height * 3 and depth_mm.size == view.width_d * view.height_d
        self._call("view_update_bgr", self._engine, view.ptr, _vptr(bgr), _vptr(depth_mm), C.c_float(affine_a),
                   C.c_float(affine_b), C.c_double(timestamp), C.c_int(int(bilateral)))

    def view_update_bgr_device(self, view, bgr_dev_ptr, depth_dev_ptr, affine_a=1.0 / 1000.0, affine_b=0.0,
                               timestamp=0.0, bilateral=False):
        self._call("view_update_bgr_device", self._engine, view.ptr, C.c_void_p(bgr_dev_ptr), C.c_void_p(depth_dev_ptr),
                   C.c_float(affine_a), C.c_float(affine_b), C.c_double(timestamp), C.c_int(int(bilateral)))

    # -- keyframe store ----------------------------------------------------------------------------------
    def create_frame_store(self, width, height, capacity, width_d=None, height_d=None):
        h = C.c_void_p()
        width_d = width if width_d is None else width_d
        height_d = height if height_d is None else height_d
        self._call("frame_store_create", self._engine, C.c_int(width), C.c_int(height), C.c_int(width_d),
                   C.c_int(height_d), C.c_int(capacity), C.byref(h))
        fs = FrameStore(self, h, self._fn("frame_store_destroy"))
        fs.width, fs.height, fs.width_d, fs.height_d, fs.capacity = width, height, width_d, height_d, capacity
        return fs

    def frame_store_put(self, fs, slot, rgba, depth_mm):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert rgba.size == fs.width * fs.height * 4 and depth_mm.size == fs.width_d * fs.height_d
        self._call("frame_store_put", self._engine, fs.ptr, C.c_int(slot), _vptr(rgba), _vptr(depth_mm))

    def frame_store_put_bgr(self, fs, slot, bgr, depth_mm):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert bgr.size == fs.width * fs.height * 3 and depth_mm.size == fs.width_d * fs.height_d
        self._call("frame_store_put_bgr", self._engine, fs.ptr, C.c_int(slot), _vptr(bgr), _vptr(depth_mm))

    def frame_store_put_view(self, fs, slot, view):
        self._call("frame_store_put_view", self._engine, fs.ptr, C.c_int(slot), view.ptr)

    def frame_store_get(self, fs, slot):
        rgba = np.empty((fs.height, fs.width, 4), dtype=np.uint8)
        depth = np.empty((fs.height_d, fs.width_d), dtype=np.int16)
        self._call("frame_store_get", self._engine, fs.ptr, C.c_int(slot), _vptr(rgba), _vptr(depth))
        return rgba, depth

    def frame_store_enable_lists(self, fs, scene):
        self._call("frame_store_enable_lists", self._engine, fs.ptr, scene.ptr)

    def frame_store_put_visible_list(self, fs, slot, scene, rs):
        """Keep the render state's visible list (the blocks the keyframe was just fused into) with the keyframe."""
        self._call("frame_store_put_visible_list", self._engine, fs.ptr, C.c_int(slot), scene.ptr, rs.ptr)

    def deprocess_frame_stored(self, scene, view, fs, slot, M_d, intr, M_rgb=None, intr_rgb=None):
        """DeProcessFrame on exactly the blocks stored with the keyframe (no allocation pass; render state untouched)."""
        m, k = self._mi(M_d, intr)
        mr = mat_to_abi(M_rgb) if M_rgb is not None else None
        kr = np.ascontiguousarray(intr_rgb, dtype=np.float32) if intr_rgb is not None else None
        self._call("deprocess_frame_stored", self._engine, scene.ptr, view.ptr, fs.ptr, C.c_int(slot), _fptr(m), _fptr(k),
                   _fptr(mr), _fptr(kr))

    def reintegrate_batch(self, scene, view, rs, fs, slots, old_Ms, new_Ms, intr, affine_a=1.0 / 1000.0, affine_b=0.0):
        """DenseSlam::OnlineCorrection's loop (DenseSlam.cpp:389-403) over keyframes of a store as ONE call: equal to
        view_update_from_store + deprocess_frame_stored(old pose) + process_frame(new pose, is_defusion) +
        frame_store_put_visible_list per keyframe; the HIP engine runs it block-major (each touched block loaded once)."""
        n = len(slots)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        om = np.ascontiguousarray(np.stack([mat_to_abi(m) for m in old_Ms]) if n else np.zeros((0, 16)), dtype=np.float32)
        nm = np.ascontiguousarray(np.stack([mat_to_abi(m) for m in new_Ms]) if n else np.zeros((0, 16)), dtype=np.float32)
        k = np.ascontiguousarray(intr, dtype=np.float32)
        self._call("reintegrate_batch", self._engine, scene.ptr, view.ptr, rs.ptr, fs.ptr, C.c_int(n), _vptr(sl), _fptr(om), _fptr(nm),
                   _fptr(k), C.c_float(affine_a), C.c_float(affine_b))

    def debug_inject_device_error(self, scene, bits):
        self._call("debug_inject_device_error", self._engine, scene.ptr, C.c_int(int(bits)))

    def debug_set_push_job_min(self, n):
        self._call("debug_set_push_job_min", self._engine, C.c_int(int(n)))

    def debug_stream_launches(self):
        n = C.c_longlong(0)
        self._call("debug_stream_launches", self._engine, C.byref(n))
        return n.value

    def debug_front_end_counts(self):
        """(fusion launches that computed GetImage's front end, GetImage calls that took it)"""
        computed, adopted = C.c_longlong(0), C.c_longlong(0)
        self._call("debug_front_end_counts", self._engine, C.byref(computed), C.byref(adopted))
        return computed.value, adopted.value

    def debug_mark_overlap_counts(self):
        """(allocation passes whose k_mark ran beside the previous GetImage's march, passes whose k_mark ran in the stream)"""
        overlapped, in_stream = C.c_longlong(0), C.c_longlong(0)
        self._call("debug_mark_overlap_counts", self._engine, C.byref(overlapped), C.byref(in_stream))
        return overlapped.value, in_stream.value

    def debug_sweep_overlap_counts(self):
        """(allocation passes whose sweep ran on the auxiliary stream with its table writes published later, passes whose sweep
        ran in the stream)"""
        overlapped, in_stream = C.c_longlong(0), C.c_longlong(0)
        self._call("debug_sweep_overlap_counts", self._engine, C.byref(overlapped), C.byref(in_stream))
        return overlapped.value, in_stream.value

    def debug_front_overlap_counts(self):
        """(front ends computed on the auxiliary stream beside the fusion launch, front ends computed inside the fusion launch)"""
        on_aux, in_launch = C.c_longlong(0), C.c_longlong(0)
        self._call("debug_front_overlap_counts", self._engine, C.byref(on_aux), C.byref(in_launch))
        return on_aux.value, in_launch.value

    def reintegrate_batch_stats(self, scene):
        """(blocks the last batch loaded, its block-operations: (block, keyframe) pairs de-integrated or re-fused) -- HIP engine"""
        b, o = C.c_int32(0), C.c_int32(0)
        self._call("reintegrate_batch_stats", self._engine, scene.ptr, C.byref(b), C.byref(o))
        return b.value, o.value

    def scene_table_changed(self, scene):
        """after the hash table was written through dslam_scene_hash_table_dev: rebuild the allocation bitmap (HIP engine)"""
        self._call("scene_table_changed", self._engine, scene.ptr)

    def view_update_from_store(self, view, fs, slot, affine_a=1.0 / 1000.0, affine_b=0.0, timestamp=0.0, bilateral=False):
        self._call("view_update_from_store", self._engine, view.ptr, fs.ptr, C.c_int(slot), C.c_float(affine_a),
                   C.c_float(affine_b), C.c_double(timestamp), C.c_int(int(bilateral)))

    def view_update_dataset(self, view, colour, depth_raw, depth_format, max_depth_m, affine_a=1.0 / 1000.0, affine_b=0.0,
                            timestamp=0.0, bilateral=False):
        """Colour image (H, W, 4) RGBA or (H, W, 3) BGR plus the dataset's raw 16-bit depth image; depth_format:
        0 millimetres, 1 KITTI-style depth * 256, 2 TUM / ICL-NUIM (divide by 5)."""
        colour = np.ascontiguousarray(colour, dtype=np.uint8)
        ch = colour.shape[-1]
        raw = np.ascontiguousarray(depth_raw, dtype=np.int16)
        assert colour.size == view.width * view.height * ch and raw.size == view.width_d * view.height_d
        self._call("view_update_dataset", self._engine, view.ptr, _vptr(colour), C.c_int(ch), _vptr(raw),
                   C.c_int(depth_format), C.c_float(max_depth_m), C.c_float(affine_a), C.c_float(affine_b),
                   C.c_double(timestamp), C.c_int(int(bilateral)))

    def download_view_raw_depth(self, view):
        out = np.empty((view.height_d, view.width_d), dtype=np.int16)
        self._call("download_view_raw_depth", self._engine, view.ptr, _vptr(out))
        return out

    def get_depth_image_int16(self, scene, rs, M, intr, scale):
        """GetImage(FREECAMERA_DEPTH) as int16 = (int16)(metres * scale): scale 1000 -> mm, 256 -> the PNG format."""
        m, k = self._mi(M, intr)
        out = np.empty((rs.height, rs.width), dtype=np.int16)
        self._call("get_depth_image_int16", self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k), C.c_int(scale), _vptr(out))
        return out

    def download_view_rgba(self, view):
        out = np.empty((view.height, view.width, 4), dtype=np.uint8)
        self._call("download_view_rgba", self._engine, view.ptr, _vptr(out))
        return out

    def depth_post_processing(self, curr_depth_mm, prev_depth_mm, Tpc, intr, filter_threshold, filter_area):
        """DenseSlam::depthPostProcessing's pixel loop on host images; returns (filtered depth, count)."""
        curr = np.array(curr_depth_mm, dtype=np.int16, order="C")
        prev = np.ascontiguousarray(prev_depth_mm, dtype=np.int16)
        assert curr.ndim == 2 and curr.shape == prev.shape
        m, k = self._mi(Tpc, intr)
        count = C.c_int(0)
        self._call("depth_post_processing", self._engine, _vptr(curr), _vptr(prev), C.c_int(curr.shape[1]),
                   C.c_int(curr.shape[0]), _fptr(m), _fptr(k), C.c_float(filter_threshold), C.c_float(filter_area),
                   C.byref(count))
        return curr, count.value

    def depth_post_processing_device(self, curr_dev_ptr, prev_dev_ptr, width, height, Tpc, intr, filter_threshold,
                                     filter_area, want_count=True):
        m, k = self._mi(Tpc, intr)
        count = C.c_int(0)
        self._call("depth_post_processing_device", self._engine, C.c_void_p(curr_dev_ptr), C.c_void_p(prev_dev_ptr),
                   C.c_int(width), C.c_int(height), _fptr(m), _fptr(k), C.c_float(filter_threshold),
                   C.c_float(filter_area), C.byref(count) if want_count else None)
        return count.value

    # -- fusion ----------------------------------------------------------------------------------------
    @staticmethod
    def _mi(M, intr):
        return mat_to_abi(M), np.ascontiguousarray(intr, dtype=np.float32)

    def allocate_scene_from_depth(self, scene, view, rs, M_d, intr, only_update_visible_list=False):
        m, k = self._mi(M_d, intr)
        self._call("allocate_scene_from_depth", self._engine, scene.ptr, view.ptr, rs.ptr, _fptr(m), _fptr(k),
                   C.c_int(int(only_update_visible_list)))

    def integrate_into_scene(self, scene, view, rs, M_d, intr, M_rgb=None, intr_rgb=None):
        m, k = self._mi(M_d, intr)
        mr = mat_to_abi(M_rgb) if M_rgb is not None else None
        kr = np.ascontiguousarray(intr_rgb, dtype=np.float32) if intr_rgb is not None else None
        self._call("integrate_into_scene", self._engine, scene.ptr, view.ptr, rs.ptr, _fptr(m), _fptr(k), _fptr(mr),
                   _fptr(kr))

    def process_frame(self, scene, view, rs, M_d, intr, M_rgb=None, intr_rgb=None, only_update_visible_list=False,
                      is_defusion=False):
        m, k = self._mi(M_d, intr)
        mr = mat_to_abi(M_rgb) if M_rgb is not None else None
        kr = np.ascontiguousarray(intr_rgb, dtype=np.float32) if intr_rgb is not None else None
        self._call("process_frame", self._engine, scene.ptr, view.ptr, rs.ptr, _fptr(m), _fptr(k), _fptr(mr), _fptr(kr),
                   C.c_int(int(only_update_visible_list)), C.c_int(int(is_defusion)))

    def deprocess_frame(self, scene, view, rs, M_d, intr, M_rgb=None, intr_rgb=None):
        m, k = self._mi(M_d, intr)
        mr = mat_to_abi(M_rgb) if M_rgb is not None else None
        kr = np.ascontiguousarray(intr_rgb, dtype=np.float32) if intr_rgb is not None else None
        self._call("deprocess_frame", self._engine, scene.ptr, view.ptr, rs.ptr, _fptr(m), _fptr(k), _fptr(mr),
                   _fptr(kr))

    def decay(self, scene, rs, max_weight, min_age, force_all_voxels, defusion_part=False):
        name = "decay_defusion_part" if defusion_part else "decay"
        self._call(name, self._engine, scene.ptr, rs.ptr if rs is not None else None, C.c_int(max_weight),
                   C.c_int(min_age), C.c_int(int(force_all_voxels)))

    def slide_window(self, scene, rs, max_age):
        self._call("slide_window", self._engine, scene.ptr, rs.ptr if rs is not None else None, C.c_int(max_age))

    def slide_window_defusion_part(self, scene, rs, max_age, max_size):
        self._call("slide_window_defusion_part", self._engine, scene.ptr, rs.ptr if rs is not None else None,
                   C.c_int(max_age), C.c_int(max_size))

    def swap_in(self, scene, rs):
        self._call("swap_in", self._engine, scene.ptr, rs.ptr if rs is not None else None)

    def swap_out(self, scene, rs):
        self._call("swap_out", self._engine, scene.ptr, rs.ptr)

    def save_to_global_memory(self, scene):
        self._call("save_to_global_memory", self._engine, scene.ptr)

    # -- visualisation ---------------------------------------------------------------------------------
    def find_visible_blocks(self, scene, rs, M, intr):
        m, k = self._mi(M, intr)
        self._call("find_visible_blocks", self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k))

    def count_visible_blocks(self, scene, rs, min_id, max_id):
        out = C.c_int()
        self._call("count_visible_blocks", self._engine, scene.ptr, rs.ptr, C.c_int(min_id), C.c_int(max_id),
                   C.byref(out))
        return out.value

    def create_expected_depths(self, scene, rs, M, intr):
        m, k = self._mi(M, intr)
        self._call("create_expected_depths", self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k))

    def track_camera(self, view, rs, scene_pose_M, pose_M, intr, params=None):
        """ITMDepthTracker::TrackCamera; returns (tracked world->camera pose as a 4x4 row-major array, result)."""
        params = params or TrackerParams()
        sp, k = self._mi(scene_pose_M, intr)
        pose = mat_to_abi(pose_M).copy()
        res = TrackerResult()
        self._call("track_camera", self._engine, view.ptr, rs.ptr, _fptr(sp), _fptr(pose), _fptr(k), C.byref(params),
                   C.byref(res))
        return pose.reshape(4, 4).T.copy(), res

    def debug_icp_sums(self):
        """The 29 double sums of the tracker's most recent ComputeGandH evaluation: 21 Hessian (lower triangle, row by
        row), 6 gradient, sum of b^2, valid count."""
        out = np.empty(29, dtype=np.float64)
        self._call("debug_icp_sums", self._engine, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    @staticmethod
    def _map_list(scenes, map_poses, writable=False):
        """(scenes, map_poses) of a multi-map call as the ABI wants them: (N, the scene pointers, the N transforms as one
        column-major float32 array).  writable: an array of its own, for a call that writes its estimates into it."""
        scenes = list(scenes)
        T = np.asarray(map_poses, dtype=np.float32)
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError("map_poses must be N 4x4 matrices")
        if len(T) != len(scenes):
            raise ValueError(f"{len(scenes)} scenes but {len(T)} map poses")
        n = len(scenes)
        ptrs = (C.c_void_p * max(n, 1))(*[None if s is None else s.ptr for s in scenes])
        t_abi = np.ascontiguousarray(np.transpose(T, (0, 2, 1))).reshape(-1) if n else np.zeros(16, np.float32)
        return n, ptrs, (t_abi.copy() if writable else t_abi)

    def track_camera_sdf(self, view, scenes, map_poses, pose_M, intr, params=None):
        """dslam_track_camera_sdf: the camera of `view` tracked against the signed distance fields of several local maps.
        `scenes` / `map_poses` as get_image_multi; `pose_M`: the start, world -> camera (4x4, metres).  Returns (the
        estimate as a 4x4 float32 array -- the start's own bytes if no step was accepted --, TrackSdfResult)."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        pose, k = self._mi(pose_M, intr)
        pose = pose.copy()
        res = TrackSdfResult()
        self._call("track_camera_sdf", self._engine, view.ptr, ptrs, _fptr(t_abi), C.c_int(n), _fptr(pose), _fptr(k),
                   C.byref(params) if params is not None else None, C.byref(res))
        return pose.reshape(4, 4).T.copy(), res

    def debug_track_sdf_sums(self):
        """The 33 double sums of the most recent depth-to-SDF tracking evaluation (rows pivoted at the camera centre of the
        pose that was evaluated), laid out as debug_register_sums: 21 Hessian, 6 gradient, sum of b^2, valid count, 3 sum of
        p - t, candidate count."""
        out = np.empty(33, dtype=np.float64)
        self._call("debug_track_sdf_sums", self._engine, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def track_camera_sdf_rgb(self, view, scenes, map_poses, pose_M, intr, params=None):
        """dslam_track_camera_sdf_rgb: track_camera_sdf with a photometric term between the maps' colour field and the view's
        own colour image (which must have the depth image's size).  Arguments as track_camera_sdf, `params` a
        TrackSdfRgbParams.  Returns (the estimate as a 4x4 float32 array -- the start's own bytes if no step was accepted --,
        TrackSdfRgbResult)."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        pose, k = self._mi(pose_M, intr)
        pose = pose.copy()
        res = TrackSdfRgbResult()
        self._call("track_camera_sdf_rgb", self._engine, view.ptr, ptrs, _fptr(t_abi), C.c_int(n), _fptr(pose), _fptr(k),
                   C.byref(params) if params is not None else None, C.byref(res))
        return pose.reshape(4, 4).T.copy(), res

    def debug_track_sdf_rgb_sums(self):
        """The 35 double sums of the most recent track_camera_sdf_rgb evaluation: the 33 of debug_track_sdf_sums (depth and
        colour rows together in the first 27), the sum of e^2 over the colour-valid pixels, the colour-valid count."""
        out = np.empty(35, dtype=np.float64)
        self._call("debug_track_sdf_rgb_sums", self._engine, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def debug_track_sdf_rgb_grey(self, view, level):
        """Level `level` of the grey pyramid the most recent track_camera_sdf_rgb built on `view`: float32 [h >> level, w >> level]."""
        h, w = view.height >> level, view.width >> level
        out = np.empty((max(h, 0), max(w, 0)), dtype=np.float32)
        self._call("debug_track_sdf_rgb_grey", self._engine, view.ptr, C.c_int(level), _fptr(out.reshape(-1)))
        return out

    @staticmethod
    def _pose_list(poses_M):
        """[K] 4x4 world -> camera poses as one column-major float32 array of the caller's own."""
        P = np.asarray(poses_M, dtype=np.float32)
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("poses_M must be K 4x4 matrices")
        return len(P), np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1).copy()

    def score_camera_poses(self, view, scenes, map_poses, poses_M, intr, level=0, residual_gate=0.0):
        """dslam_score_camera_poses: one evaluation of dslam_track_camera_sdf's law per pose of `poses_M` ([K] 4x4, world ->
        camera) on `level` of the view's pyramid, all in one launch.  Returns a ctypes array of K PoseScore."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        k, poses = self._pose_list(poses_M)
        intr = np.ascontiguousarray(intr, dtype=np.float32)
        scores = (PoseScore * max(k, 1))()
        self._call("score_camera_poses", self._engine, view.ptr, ptrs, _fptr(t_abi), C.c_int(n), _fptr(poses), C.c_int(k),
                   _fptr(intr), C.c_int(level), C.c_float(residual_gate), scores)
        return scores

    def track_camera_sdf_starts(self, view, scenes, map_poses, poses_M, intr, params=None):
        """dslam_track_camera_sdf_starts: track_camera_sdf from every start of `poses_M` ([K] 4x4) in lock-step.  Returns (the
        estimates [K, 4, 4] float32 -- a start's own bytes where no step was accepted --, a ctypes array of K TrackSdfResult)."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        k, poses = self._pose_list(poses_M)
        intr = np.ascontiguousarray(intr, dtype=np.float32)
        res = (TrackSdfResult * max(k, 1))()
        self._call("track_camera_sdf_starts", self._engine, view.ptr, ptrs, _fptr(t_abi), C.c_int(n), _fptr(poses), C.c_int(k),
                   _fptr(intr), C.byref(params) if params is not None else None, res)
        return np.transpose(poses.reshape(k, 4, 4), (0, 2, 1)).copy(), res

    def debug_track_sdf_start_sums(self, start):
        """The 33 double sums of start `start`'s last evaluation in the most recent track_camera_sdf_starts."""
        out = np.empty(33, dtype=np.float64)
        self._call("debug_track_sdf_start_sums", self._engine, C.c_int(start), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def select_start_poses(self, scores, min_valid, max_keep):
        """dslam_select_start_poses (host only): the indices of the max_keep cheapest scores with valid >= min_valid."""
        num = len(scores)
        arr = scores if isinstance(scores, C.Array) else (PoseScore * max(num, 1))(*scores)
        kept = np.zeros(max(max_keep, 1), dtype=np.int32)
        count = C.c_int32(0)
        self._call("select_start_poses", arr, C.c_int(num), C.c_int(min_valid), C.c_int(max_keep),
                   kept.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(count))
        return kept[:count.value].copy()

    def camera_pose_lattice(self, pose_M, lattice):
        """dslam_camera_pose_lattice (host only): the lattice's poses around pose_M as [count, 4, 4] float32."""
        count = C.c_int32(0)
        cap = max(lattice.count, 1)
        out = np.zeros(cap * 16, dtype=np.float32)
        self._call("camera_pose_lattice", _fptr(mat_to_abi(pose_M)), C.byref(lattice), _fptr(out), C.c_int(cap), C.byref(count))
        return np.transpose(out[:16 * count.value].reshape(-1, 4, 4), (0, 2, 1)).copy()

    def _image_call(self, name, scene, rs, M, intr, image_type, download=True, out=None):
        """`out`: an existing (H, W) float32 / (H, W, 4) uint8 array to fill instead of a fresh one (e.g. a page-locked
        array from host_alloc, which the copy back DMAs into directly)."""
        m, k = self._mi(M, intr)
        out_rgba = out_f = None
        if download or out is not None:
            if image_type == IMAGE_DEPTH:
                out_f = out if out is not None else np.empty((rs.height, rs.width), dtype=np.float32)
                assert out_f.dtype == np.float32 and out_f.size == rs.height * rs.width and out_f.flags.c_contiguous
            else:
                out_rgba = out if out is not None else np.empty((rs.height, rs.width, 4), dtype=np.uint8)
                assert out_rgba.dtype == np.uint8 and out_rgba.size == rs.height * rs.width * 4 and out_rgba.flags.c_contiguous
        self._call(name, self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k), C.c_int(image_type), _vptr(out_rgba),
                   _fptr(out_f))
        return out_f if image_type == IMAGE_DEPTH else out_rgba

    def render_image(self, scene, rs, M, intr, image_type, download=True, out=None):
        return self._image_call("render_image", scene, rs, M, intr, image_type, download, out)

    def get_image(self, scene, rs, M, intr, image_type, download=True, out=None):
        return self._image_call("get_image", scene, rs, M, intr, image_type, download, out)

    def get_image_multi(self, scenes, map_poses, rs, M, intr, image_type, download=True, out=None):
        """dslam_get_image_multi: one raycast over several local maps.  `scenes`: 1 .. MAX_RENDER_MAPS scenes; `map_poses`:
        one 4x4 world -> map transform per scene (metres, estimatedGlobalPose.GetM()), as a list or an [N, 4, 4] array.
        Otherwise as get_image."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        m, k = self._mi(M, intr)
        out_rgba = out_f = None
        if download or out is not None:
            if image_type == IMAGE_DEPTH:
                out_f = out if out is not None else np.empty((rs.height, rs.width), dtype=np.float32)
                assert out_f.dtype == np.float32 and out_f.size == rs.height * rs.width and out_f.flags.c_contiguous
            else:
                out_rgba = out if out is not None else np.empty((rs.height, rs.width, 4), dtype=np.uint8)
                assert out_rgba.dtype == np.uint8 and out_rgba.size == rs.height * rs.width * 4 and out_rgba.flags.c_contiguous
        self._call("get_image_multi", self._engine, ptrs, _fptr(t_abi), C.c_int(n), rs.ptr, _fptr(m), _fptr(k),
                   C.c_int(image_type), _vptr(out_rgba), _fptr(out_f))
        return out_f if image_type == IMAGE_DEPTH else out_rgba

    def create_icp_maps(self, scene, rs, M, intr, download=True):
        """trackingController->Prepare.  download=False leaves the maps on the device (all the depth tracker needs)."""
        m, k = self._mi(M, intr)
        if not download:
            self._call("create_icp_maps", self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k), None, None)
            return None, None
        pts = np.empty((rs.height, rs.width, 4), dtype=np.float32)
        nrm = np.empty((rs.height, rs.width, 4), dtype=np.float32)
        self._call("create_icp_maps", self._engine, scene.ptr, rs.ptr, _fptr(m), _fptr(k), _fptr(pts), _fptr(nrm))
        return pts, nrm

    def download_icp_maps(self, rs):
        """The points / normals maps the last create_icp_maps left on the device."""
        pts = np.empty((rs.height, rs.width, 4), dtype=np.float32)
        nrm = np.empty((rs.height, rs.width, 4), dtype=np.float32)
        self._call("download_icp_maps", self._engine, rs.ptr, _fptr(pts), _fptr(nrm))
        return pts, nrm

    def download_raycast_image(self, rs):
        """renderState->raycastImage: the grey tracking raycast the last create_icp_maps drew (what
        ITMMainEngine::GetImage(InfiniTAM_IMAGE_SCENERAYCAST) copies out)."""
        out = np.empty((rs.height, rs.width, 4), dtype=np.uint8)
        self._call("download_raycast_image", self._engine, rs.ptr, _vptr(out))
        return out

    # -- meshing export --------------------------------------------------------------------------------
    def mesh_scene(self, scene, max_triangles=0, colour=False):
        """SaveCurrSceneToMesh's MeshScene: returns (positions [n, 3, 3] float32 in metres, colours [n, 3, 3] float32
        in [0, 1] or None), triangles in upstream's CPU-engine order."""
        n = C.c_int(0)
        self._call("mesh_scene", self._engine, scene.ptr, C.c_int(int(max_triangles)), C.c_int(int(colour)), C.byref(n))
        pos = np.empty((max(n.value, 1), 3, 3), dtype=np.float32)  # never a null pointer, even for an empty mesh
        col = np.empty((max(n.value, 1), 3, 3), dtype=np.float32) if colour else None
        self._call("mesh_download", self._engine, _fptr(pos), _fptr(col) if colour else None, C.c_int(n.value))
        return pos[:n.value], (col[:n.value] if colour else None)

    def mesh_scene_multi(self, scenes, map_poses, max_triangles=0, colour=False):
        """dslam_mesh_scene_multi: one mesh of several local maps in the world frame.  `scenes` / `map_poses` as
        get_image_multi.  Returns (positions [n, 3, 3] float32 in metres, colours [n, 3, 3] float32 in [0, 1] or None,
        per_map_counts [len(scenes)] int32): the triangles of map 0, then map 1, ..."""
        k, ptrs, t_abi = self._map_list(scenes, map_poses)
        n = C.c_int(0)
        counts = np.zeros(max(k, 1), dtype=np.int32)
        self._call("mesh_scene_multi", self._engine, ptrs, _fptr(t_abi), C.c_int(k), C.c_int(int(max_triangles)),
                   C.c_int(int(colour)), C.byref(n), counts.ctypes.data_as(C.POINTER(C.c_int32)))
        pos = np.empty((max(n.value, 1), 3, 3), dtype=np.float32)
        col = np.empty((max(n.value, 1), 3, 3), dtype=np.float32) if colour else None
        self._call("mesh_download", self._engine, _fptr(pos), _fptr(col) if colour else None, C.c_int(n.value))
        return pos[:n.value], (col[:n.value] if colour else None), counts[:k]

    # -- map registration ------------------------------------------------------------------------------
    def register_maps(self, src, dst, X0, params=None):
        """dslam_register_maps: the rigid transform from `src`'s frame to `dst`'s (4x4, metres), estimated from the two
        maps' voxels starting at X0.  Returns (X as a 4x4 float32 array, RegisterResult)."""
        X = mat_to_abi(X0).copy()
        res = RegisterResult()
        self._call("register_maps", self._engine, src.ptr, dst.ptr, _fptr(X), C.byref(params) if params is not None else None,
                   C.byref(res))
        return X.reshape(4, 4).T.copy(), res

    def debug_register_sums(self):
        """The 33 double sums of the most recent registration evaluation (pivot at the origin): 21 Hessian (lower
        triangle, row by row), 6 gradient, sum of b^2, valid count, 3 sum of q, candidate count."""
        out = np.empty(33, dtype=np.float64)
        self._call("debug_register_sums", self._engine, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def register_graph(self, scenes, map_poses, pairs, anchor, params=None):
        """dslam_register_graph: the poses of N local maps estimated jointly from the voxels of the listed overlapping pairs.
        `scenes` / `map_poses` as get_image_multi (the starts); `pairs`: (src, dst) indices into `scenes`; `anchor`: the map
        held fixed.  Returns (the estimates [N, 4, 4] float32, RegisterGraphResult, a list of RegisterPairResult)."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses, writable=True)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        res = RegisterGraphResult()
        pres = (RegisterPairResult * max(len(pr), 1))()
        self._call("register_graph", self._engine, ptrs, _fptr(t_abi), C.c_int(n), pr.ctypes.data_as(C.POINTER(C.c_int32)),
                   C.c_int(len(pr)), C.c_int(int(anchor)), C.byref(params) if params is not None else None, C.byref(res), pres)
        return np.transpose(t_abi.reshape(n, 4, 4), (0, 2, 1)).copy(), res, list(pres)[:len(pr)]

    def debug_register_graph_sums(self, pair):
        """The 33 double sums (as debug_register_sums) of pair `pair` at the most recent joint evaluation."""
        out = np.empty(33, dtype=np.float64)
        self._call("debug_register_graph_sums", self._engine, C.c_int(int(pair)), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    # -- overlap survey and pair selection ---------------------------------------------------------------
    def survey_overlaps(self, scenes, map_poses):
        """dslam_survey_overlaps: which of N local maps overlap, at block granularity.  `scenes` / `map_poses` as
        register_graph.  Returns (live [N], shared_blocks [N, N], shared_octants [N, N]), int32, row = source map."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        live = np.zeros(max(n, 1), dtype=np.int32)
        blocks = np.zeros((max(n, 1), max(n, 1)), dtype=np.int32)
        octants = np.zeros((max(n, 1), max(n, 1)), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._call("survey_overlaps", self._engine, ptrs, _fptr(t_abi), C.c_int(n), live.ctypes.data_as(i32),
                   blocks.ctypes.data_as(i32), octants.ctypes.data_as(i32))
        return live, blocks, octants

    def select_register_pairs(self, live, shared_octants, params=None):
        """dslam_select_register_pairs: the pair list for register_graph from a survey (host only).  Returns (pairs
        [selected, 2] int32 as (src, dst), component [N] int32, PairSelectResult)."""
        live = np.ascontiguousarray(np.asarray(live, dtype=np.int32))
        shared = np.ascontiguousarray(np.asarray(shared_octants, dtype=np.int32))
        n = len(live)
        if shared.shape != (n, n):
            raise ValueError("shared_octants must be N x N for N live counts")
        pairs = np.zeros((MAX_REGISTER_PAIRS, 2), dtype=np.int32)
        component = np.zeros(max(n, 1), dtype=np.int32)
        res = PairSelectResult()
        i32 = C.POINTER(C.c_int32)
        self._call("select_register_pairs", live.ctypes.data_as(i32), shared.ctypes.data_as(i32), C.c_int(n),
                   C.byref(params) if params is not None else None, pairs.ctypes.data_as(i32), component.ctypes.data_as(i32),
                   C.byref(res))
        return pairs[:res.selected].copy(), component[:n], res

    # -- view survey and map selection -------------------------------------------------------------------
    def view_frustum_planes(self, view, voxel_size):
        """dslam_view_frustum_planes (host only): the [7, 4] float32 rows of a SurveyView in the world frame, voxel units."""
        out = np.zeros((7, 4), dtype=np.float32)
        self._call("view_frustum_planes", C.byref(view), C.c_float(voxel_size), _fptr(out))
        return out

    def survey_views(self, scenes, map_poses, views, params=None):
        """dslam_survey_views: which of N local maps reach V camera views, at block granularity.  `scenes` / `map_poses` as
        register_graph (up to MAX_SURVEY_MAPS); `views`: SurveyView objects.  Returns (live [N], reach [V, N], nearest
        [V, N], farthest [V, N]), int32."""
        n, ptrs, t_abi = self._map_list(scenes, map_poses)
        views = list(views)
        nv = len(views)
        varr = (SurveyView * max(nv, 1))(*views)
        live = np.zeros(max(n, 1), dtype=np.int32)
        reach, nearest, farthest = (np.zeros((max(nv, 1), max(n, 1)), dtype=np.int32) for _ in range(3))
        i32 = C.POINTER(C.c_int32)
        self._call("survey_views", self._engine, ptrs, _fptr(t_abi), C.c_int(n), varr, C.c_int(nv),
                   C.byref(params) if params is not None else None, live.ctypes.data_as(i32), reach.ctypes.data_as(i32),
                   nearest.ctypes.data_as(i32), farthest.ctypes.data_as(i32))
        return live, reach, nearest, farthest

    def debug_survey_views_launches(self):
        n = C.c_longlong(0)
        self._call("debug_survey_views_launches", self._engine, C.byref(n))
        return n.value

    def select_view_maps(self, reach, nearest, params=None):
        """dslam_select_view_maps: the maps to list for a view from a survey (host only).  Returns (the kept map indices,
        ascending, int32, ViewSelectResult)."""
        reach = np.ascontiguousarray(np.asarray(reach, dtype=np.int32))
        nearest = np.ascontiguousarray(np.asarray(nearest, dtype=np.int32))
        if reach.ndim != 2 or nearest.shape != reach.shape:
            raise ValueError("reach and nearest must both be V x N")
        nv, n = reach.shape
        maps = np.zeros(MAX_RENDER_MAPS, dtype=np.int32)
        res = ViewSelectResult()
        i32 = C.POINTER(C.c_int32)
        self._call("select_view_maps", reach.ctypes.data_as(i32), nearest.ctypes.data_as(i32), C.c_int(nv), C.c_int(n),
                   C.byref(params) if params is not None else None, maps.ctypes.data_as(i32), C.byref(res))
        return maps[:res.selected].copy(), res

    # -- the maps at any point or along any ray --------------------------------------------------------
    def query_points(self, scenes, map_poses, points, what=QUERY_ALL):
        """dslam_query_points: the combined reads of `scenes` / `map_poses` (as track_camera_sdf) at world points [n, 3]
        (metres).  Returns a POINT_SAMPLE_DTYPE array [n]."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
        out = np.zeros(len(pts), dtype=POINT_SAMPLE_DTYPE)
        self._call("query_points", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), _fptr(pts), C.c_int(len(pts)),
                   C.c_int(what), _vptr(out))
        return out

    def query_points_device(self, scenes, map_poses, points_dev_ptr, n, out_dev_ptr, what=QUERY_ALL):
        """dslam_query_points_device: `points_dev_ptr` [n][3] float32 and `out_dev_ptr` [n] x 48 bytes are device addresses;
        enqueues on the engine's stream."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        self._call("query_points_device", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.c_void_p(points_dev_ptr),
                   C.c_int(n), C.c_int(what), C.c_void_p(out_dev_ptr))

    def cast_rays(self, scenes, map_poses, rays, max_range=0.0, what=QUERY_ALL):
        """dslam_cast_rays: `rays` [n, 8] float32 (origin, direction, t_min, t_max; metres); max_range 0: the limit.
        Returns a RAY_HIT_DTYPE array [n]."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        r = np.ascontiguousarray(np.asarray(rays, dtype=np.float32).reshape(-1, 8))
        out = np.zeros(len(r), dtype=RAY_HIT_DTYPE)
        self._call("cast_rays", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), _fptr(r), C.c_int(len(r)),
                   C.c_float(max_range), C.c_int(what), _vptr(out))
        return out

    def cast_rays_device(self, scenes, map_poses, rays_dev_ptr, n, out_dev_ptr, max_range=0.0, what=QUERY_ALL):
        """dslam_cast_rays_device: `rays_dev_ptr` [n][8] float32 and `out_dev_ptr` [n] x 48 bytes are device addresses;
        enqueues on the engine's stream."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        self._call("cast_rays_device", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.c_void_p(rays_dev_ptr), C.c_int(n),
                   C.c_float(max_range), C.c_int(what), C.c_void_p(out_dev_ptr))

    # -- occupancy and exact distance grids --------------------------------------------------------------
    def grid_from_box(self, lo_m, hi_m, voxel_size, cell):
        """dslam_grid_from_box: the Grid of cell edge `cell` (voxels) that covers the metric box lo_m .. hi_m."""
        lo, hi = np.asarray(lo_m, np.float32).reshape(3), np.asarray(hi_m, np.float32).reshape(3)
        g = Grid()
        self._call("grid_from_box", _fptr(lo), _fptr(hi), C.c_float(voxel_size), C.c_int(cell), C.byref(g))
        return g

    @staticmethod
    def _dist_dtype(fmt):
        return np.float32 if fmt == DIST_METRES else np.int32

    def mark_occupancy(self, scenes, map_poses, grid, min_weight=0, occupied_below=0.0, out=None):
        """dslam_mark_occupancy: one state byte per cell of `grid` (0 unknown, 1 observed free, 3 occupied) from `scenes` /
        `map_poses` (as query_points).  out: a uint8 array [cells] to write into."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        out = np.zeros(grid.cells, np.uint8) if out is None else out
        self._call("mark_occupancy", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.byref(grid), C.c_int(min_weight),
                   C.c_float(occupied_below), _vptr(out))
        return out

    def mark_occupancy_device(self, scenes, map_poses, grid, states_dev_ptr, min_weight=0, occupied_below=0.0):
        """dslam_mark_occupancy_device: `states_dev_ptr` [cells] bytes is a device address; enqueues on the engine's stream."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        self._call("mark_occupancy_device", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.byref(grid), C.c_int(min_weight),
                   C.c_float(occupied_below), C.c_void_p(states_dev_ptr))

    def distance_transform(self, grid, states, seeds=SEED_OCCUPIED, max_cells=0, fmt=DIST_SQUARED_CELLS, voxel_size=0.0, out=None):
        """dslam_distance_transform: the exact squared distance (int32, cells) or the distance in metres (float32) of every
        cell of `grid` to the nearest seed cell of `states` (uint8 [cells]); DIST_FAR / +inf beyond max_cells or without a seed."""
        states = None if states is None else np.ascontiguousarray(states, dtype=np.uint8)
        out = np.zeros(grid.cells, self._dist_dtype(fmt)) if out is None else out
        self._call("distance_transform", self._engine, C.byref(grid), _vptr(states), C.c_int(seeds), C.c_int(max_cells), C.c_int(fmt),
                   C.c_float(voxel_size), _vptr(out))
        return out

    def distance_transform_device(self, grid, states_dev_ptr, dist_dev_ptr, seeds=SEED_OCCUPIED, max_cells=0, fmt=DIST_SQUARED_CELLS,
                                  voxel_size=0.0):
        """dslam_distance_transform_device: `states_dev_ptr` [cells] bytes and `dist_dev_ptr` [cells] x 4 bytes are device addresses."""
        self._call("distance_transform_device", self._engine, C.byref(grid), C.c_void_p(states_dev_ptr), C.c_int(seeds),
                   C.c_int(max_cells), C.c_int(fmt), C.c_float(voxel_size), C.c_void_p(dist_dev_ptr))

    def distance_field(self, scenes, map_poses, grid, min_weight=0, occupied_below=0.0, seeds=SEED_OCCUPIED, max_cells=0,
                       fmt=DIST_SQUARED_CELLS, want_states=True, want_dist=True, states_out=None, dist_out=None):
        """dslam_distance_field: mark_occupancy, then distance_transform on its states, on the device.  Returns (states or
        None, distances or None)."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        if want_states and states_out is None:
            states_out = np.zeros(grid.cells, np.uint8)
        if want_dist and dist_out is None:
            dist_out = np.zeros(grid.cells, self._dist_dtype(fmt))
        self._call("distance_field", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.byref(grid), C.c_int(min_weight),
                   C.c_float(occupied_below), C.c_int(seeds), C.c_int(max_cells), C.c_int(fmt), _vptr(states_out), _vptr(dist_out))
        return states_out, dist_out

    def distance_field_device(self, scenes, map_poses, grid, states_dev_ptr, dist_dev_ptr, min_weight=0, occupied_below=0.0,
                              seeds=SEED_OCCUPIED, max_cells=0, fmt=DIST_SQUARED_CELLS):
        """dslam_distance_field_device: `states_dev_ptr` / `dist_dev_ptr` are device addresses, either may be 0 (not wanted)."""
        n_maps, ptrs, t_abi = self._map_list(scenes, map_poses)
        self._call("distance_field_device", self._engine, ptrs, _fptr(t_abi), C.c_int(n_maps), C.byref(grid), C.c_int(min_weight),
                   C.c_float(occupied_below), C.c_int(seeds), C.c_int(max_cells), C.c_int(fmt), C.c_void_p(states_dev_ptr or None),
                   C.c_void_p(dist_dev_ptr or None))

    def distance_field_phases(self, enable=-1, read=True):
        """dslam_debug_distance_field_phases (bench hook): [states, x pass, y pass, last pass] of the most recent call in ms."""
        ms = (C.c_float * 4)()
        self._call("debug_distance_field_phases", self._engine, C.c_int(enable), ms if read else None)
        return list(ms)

    # -- semi-global stereo matching -------------------------------------------------------------------
    def create_stereo(self, width, height, params=None):
        """dslam_stereo_create: a matcher for rectified pairs of width x height; .params: its StereoParams, defaults filled in."""
        h = C.c_void_p()
        self._call("stereo_create", self._engine, C.c_int(width), C.c_int(height), C.byref(params) if params is not None else None,
                   C.byref(h))
        st = Stereo(self, h, self._fn("stereo_destroy"))
        st.width, st.height, st.params = width, height, self.stereo_get_params(st)
        st.D, st.channels = st.params.max_disparity, st.params.channels
        return st

    def stereo_get_params(self, st):
        p = StereoParams()
        self._call("stereo_get_params", st.ptr, C.byref(p))
        return p

    @staticmethod
    def _stereo_image(st, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.size == st.width * st.height * st.channels
        return img

    @staticmethod
    def _stereo_calib(calib):
        return calib if isinstance(calib, StereoCalib) else StereoCalib(*[float(v) for v in calib])

    def stereo_match(self, st, left, right, out=None):
        """dslam_stereo_match: the left image's disparity, uint16 [H, W] in 1/16 pixel (STEREO_INVALID: none)."""
        left, right = self._stereo_image(st, left), self._stereo_image(st, right)
        out = np.zeros((st.height, st.width), np.uint16) if out is None else out
        self._call("stereo_match", self._engine, st.ptr, _vptr(left), _vptr(right), _vptr(out))
        return out

    def stereo_match_device(self, st, left_dev_ptr, right_dev_ptr, disp_dev_ptr):
        """dslam_stereo_match_device: device addresses; enqueues on the engine's stream."""
        self._call("stereo_match_device", self._engine, st.ptr, C.c_void_p(left_dev_ptr), C.c_void_p(right_dev_ptr),
                   C.c_void_p(disp_dev_ptr))

    def disparity_to_depth(self, st, disp, calib, out=None):
        """dslam_disparity_to_depth: int16 [H, W] millimetres from a uint16 disparity image; calib: a StereoCalib or its 5 values."""
        disp = np.ascontiguousarray(disp, dtype=np.uint16)
        assert disp.size == st.width * st.height
        out = np.zeros((st.height, st.width), np.int16) if out is None else out
        self._call("disparity_to_depth", self._engine, st.ptr, _vptr(disp), C.byref(self._stereo_calib(calib)), _vptr(out))
        return out

    def disparity_to_depth_device(self, st, disp_dev_ptr, calib, depth_dev_ptr):
        self._call("disparity_to_depth_device", self._engine, st.ptr, C.c_void_p(disp_dev_ptr), C.byref(self._stereo_calib(calib)),
                   C.c_void_p(depth_dev_ptr))

    def stereo_depth(self, st, left, right, calib, want_disp=True, depth_out=None, disp_out=None):
        """dslam_stereo_depth: (depth int16 [H, W] in millimetres, disparity uint16 [H, W] or None)."""
        left, right = self._stereo_image(st, left), self._stereo_image(st, right)
        depth_out = np.zeros((st.height, st.width), np.int16) if depth_out is None else depth_out
        if want_disp and disp_out is None:
            disp_out = np.zeros((st.height, st.width), np.uint16)
        self._call("stereo_depth", self._engine, st.ptr, _vptr(left), _vptr(right), C.byref(self._stereo_calib(calib)),
                   _vptr(depth_out), _vptr(disp_out))
        return depth_out, disp_out

    def stereo_depth_device(self, st, left_dev_ptr, right_dev_ptr, calib, depth_dev_ptr, disp_dev_ptr=None):
        """dslam_stereo_depth_device: device addresses (disp_dev_ptr may be None); the depth image is what view_update_device takes."""
        self._call("stereo_depth_device", self._engine, st.ptr, C.c_void_p(left_dev_ptr), C.c_void_p(right_dev_ptr),
                   C.byref(self._stereo_calib(calib)), C.c_void_p(depth_dev_ptr), C.c_void_p(disp_dev_ptr or None))

    def debug_stereo_download(self, st, what):
        """dslam_debug_stereo_download: STEREO_CENSUS_LEFT / _RIGHT uint64 [H, W], STEREO_S uint16 [H, W, D] of the last match."""
        out = np.zeros((st.height, st.width, st.D), np.uint16) if what == STEREO_S else np.zeros((st.height, st.width), np.uint64)
        self._call("debug_stereo_download", self._engine, st.ptr, C.c_int(what), _vptr(out))
        return out

    def debug_stereo_select(self, st, S, out=None):
        """dslam_debug_stereo_select: selection, left-right check and sub-pixel step on the caller's S uint16 [H, W, D]."""
        S = np.ascontiguousarray(S, dtype=np.uint16)
        assert S.size == st.width * st.height * st.D
        out = np.zeros((st.height, st.width), np.uint16) if out is None else out
        self._call("debug_stereo_select", self._engine, st.ptr, _vptr(S), _vptr(out))
        return out

    def stereo_phases(self, st, enable=-1, read=True):
        """dslam_debug_stereo_phases (bench hook): [census, aggregation, selection, left-right check, conversion alone] in ms."""
        ms = (C.c_float * 5)()
        self._call("debug_stereo_phases", self._engine, st.ptr, C.c_int(enable), ms if read else None)
        return list(ms)

    # -- sparse stereo scene flow ----------------------------------------------------------------------
    def create_sflow(self, width, height, params=None):
        """dslam_sflow_create: a scene-flow matcher for frames of width x height; .params: its SflowParams, defaults filled in."""
        h = C.c_void_p()
        self._call("sflow_create", self._engine, C.c_int(width), C.c_int(height), C.byref(params) if params is not None else None,
                   C.byref(h))
        sf = Sflow(self, h, self._fn("sflow_destroy"))
        sf.width, sf.height, sf.params = width, height, self.sflow_get_params(sf)
        sf.channels, sf.scale = sf.params.channels, 2 if sf.params.half_resolution == 1 else 1
        return sf

    def sflow_get_params(self, sf):
        p = SflowParams()
        self._call("sflow_get_params", sf.ptr, C.byref(p))
        return p

    @staticmethod
    def _sflow_image(sf, img):
        if img is None:
            return None
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.size == sf.width * sf.height * sf.channels
        return img

    def sflow_push(self, sf, left, right=None, replace=False):
        """dslam_sflow_push: a new current frame (right may be None); replace overwrites the current frame instead of rotating."""
        left, right = self._sflow_image(sf, left), self._sflow_image(sf, right)
        self._call("sflow_push", self._engine, sf.ptr, _vptr(left), _vptr(right), C.c_int(int(replace)))

    def sflow_push_device(self, sf, left_dev_ptr, right_dev_ptr=None, replace=False):
        self._call("sflow_push_device", self._engine, sf.ptr, C.c_void_p(left_dev_ptr), C.c_void_p(right_dev_ptr or None),
                   C.c_int(int(replace)))

    def sflow_match(self, sf, method, which=0, capacity=None, out=None):
        """dslam_sflow_match: (records int32 [min(count, capacity), 12], count).  capacity None: room for every match."""
        if capacity is None:
            count = C.c_int32(0)
            self._call("sflow_match", self._engine, sf.ptr, C.c_int(method), C.c_int(which), None, C.c_int(0), C.byref(count))
            capacity = count.value
        out = np.zeros((capacity, SFLOW_MATCH_WORDS), np.int32) if out is None else out
        count = C.c_int32(0)
        self._call("sflow_match", self._engine, sf.ptr, C.c_int(method), C.c_int(which), _vptr(out), C.c_int(capacity), C.byref(count))
        return out[:min(count.value, capacity)], count.value

    def sflow_match_device(self, sf, method, which, out_dev_ptr, capacity, count_dev_ptr):
        """dslam_sflow_match_device: records and count stay in device memory; enqueues on the engine's stream."""
        self._call("sflow_match_device", self._engine, sf.ptr, C.c_int(method), C.c_int(which), C.c_void_p(out_dev_ptr),
                   C.c_int(capacity), C.c_void_p(count_dev_ptr))

    def sflow_features(self, sf, image, which, capacity=None):
        """dslam_sflow_features: the records of one image (SFLOW_IMAGE_*) and set as int32 [n, 12] (12 words = 48 bytes)."""
        count = C.c_int32(0)
        if capacity is None:
            self._call("sflow_features", self._engine, sf.ptr, C.c_int(image), C.c_int(which), None, C.c_int(0), C.byref(count))
            capacity = count.value
        out = np.zeros((capacity, SFLOW_FEATURE_BYTES // 4), np.int32)
        self._call("sflow_features", self._engine, sf.ptr, C.c_int(image), C.c_int(which), _vptr(out), C.c_int(capacity), C.byref(count))
        return out[:min(count.value, capacity)], count.value

    def debug_sflow_download(self, sf, side, which):
        """dslam_debug_sflow_download: one filter image (SFLOW_FILTER_*) of the current frame's left (0) or right (1) image."""
        shape = (sf.height // sf.scale, sf.width // sf.scale)
        out = np.zeros(shape, np.uint8 if which <= SFLOW_FILTER_DV else np.int16)
        self._call("debug_sflow_download", self._engine, sf.ptr, C.c_int(side), C.c_int(which), _vptr(out))
        return out

    def sflow_phases(self, sf, enable=-1, read=True):
        """dslam_debug_sflow_phases (bench hook): [filters, suppression, compaction, bins, matching, match compaction] in ms."""
        ms = (C.c_float * 6)()
        self._call("debug_sflow_phases", self._engine, sf.ptr, C.c_int(enable), ms if read else None)
        return list(ms)

    # -- fern keyframe index ---------------------------------------------------------------------------
    def create_fern_index(self, width_d, height_d, capacity, params=None):
        """dslam_fern_index_create: an index of `capacity` codes for depth images of width_d x height_d."""
        h = C.c_void_p()
        self._call("fern_index_create", self._engine, C.c_int(width_d), C.c_int(height_d),
                   C.byref(params) if params is not None else None, C.c_int(capacity), C.byref(h))
        idx = FernIndex(self, h, self._fn("fern_index_destroy"))
        idx.width_d, idx.height_d, idx.capacity = width_d, height_d, capacity
        return idx

    def fern_index_count(self, idx):
        n = C.c_int32(-1)
        self._call("fern_index_count", idx.ptr, C.byref(n))
        return n.value

    def fern_index_table(self, idx):
        """dslam_fern_index_table: (the FernParams with defaults filled in, the table int32 [F, 4, 3])."""
        p = FernParams()
        self._call("fern_index_table", idx.ptr, C.byref(p), None)
        table = np.zeros((p.num_ferns, 4, 3), dtype=np.int32)
        self._call("fern_index_table", idx.ptr, None, table.ctypes.data_as(C.POINTER(C.c_int32)))
        return p, table

    def fern_index_reset(self, idx):
        self._call("fern_index_reset", self._engine, idx.ptr)

    def fern_encode(self, idx, view):
        """dslam_fern_encode: the view's code, uint32 [64]."""
        code = np.zeros(FERN_CODE_DWORDS, dtype=np.uint32)
        self._call("fern_encode", self._engine, idx.ptr, view.ptr, code.ctypes.data_as(C.POINTER(C.c_uint32)))
        return code

    def fern_query(self, idx, view, first_id, last_id, k):
        """dslam_fern_query: the first k candidates of the window as a FERN_MATCH_DTYPE array (id, dissimilarity)."""
        matches = np.zeros(max(k, 1), dtype=FERN_MATCH_DTYPE)
        n = C.c_int32(0)
        self._call("fern_query", self._engine, idx.ptr, view.ptr, C.c_int(first_id), C.c_int(last_id), C.c_int(k),
                   _vptr(matches), C.byref(n))
        return matches[:n.value].copy()

    def fern_process(self, idx, view, harvest_min_dissimilarity, first_id, last_id, k):
        """dslam_fern_process: (matches, the id the view's code was appended under or -1, full).  full: the code should have
        been appended but the index is full (DSLAM_ERR_UNSUPPORTED: the matches are delivered all the same)."""
        matches = np.zeros(max(k, 1), dtype=FERN_MATCH_DTYPE)
        n, added = C.c_int32(0), C.c_int32(-1)
        rc = self._fn("fern_process")(self._engine, idx.ptr, view.ptr, C.c_int(harvest_min_dissimilarity), C.c_int(first_id),
                                      C.c_int(last_id), C.c_int(k), _vptr(matches), C.byref(n), C.byref(added))
        full = rc == -3 and self.fern_index_count(idx) == idx.capacity
        if not full:
            self._check(rc, "fern_process")
        return matches[:n.value].copy(), added.value, full

    def fern_add_from_store(self, idx, fs, first_slot, num_slots):
        """dslam_fern_add_from_store: the id of the first of the num_slots codes appended."""
        first = C.c_int32(-1)
        self._call("fern_add_from_store", self._engine, idx.ptr, fs.ptr, C.c_int(first_slot), C.c_int(num_slots), C.byref(first))
        return first.value

    def fern_query_stored(self, idx, query_ids, first_id, last_id, k):
        """dslam_fern_query_stored: one list of matches (FERN_MATCH_DTYPE) per query id."""
        ids = np.ascontiguousarray(np.asarray(query_ids, dtype=np.int32))
        nq = len(ids)
        matches = np.zeros((max(nq, 1), max(k, 1)), dtype=FERN_MATCH_DTYPE)
        nums = np.zeros(max(nq, 1), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._call("fern_query_stored", self._engine, idx.ptr, ids.ctypes.data_as(i32), C.c_int(nq), C.c_int(first_id),
                   C.c_int(last_id), C.c_int(k), _vptr(matches), nums.ctypes.data_as(i32))
        return [matches[q, :nums[q]].copy() for q in range(nq)]

    # -- map merge -------------------------------------------------------------------------------------
    def merge_maps(self, src, dst, X, params=None):
        """dslam_merge_maps: fuse `src` into `dst` under X (source frame -> destination frame, 4x4, metres), on the
        device; `src` is only read.  Returns the MergeResult."""
        res = MergeResult()
        self._call("merge_maps", self._engine, src.ptr, dst.ptr, _fptr(mat_to_abi(X)),
                   C.byref(params) if params is not None else None, C.byref(res))
        return res

    def unmerge_maps(self, src, dst, X, params=None):
        """dslam_unmerge_maps: remove from `dst` what merge_maps(src, dst, X) added, on the device; `src` is only read.
        Returns the UnmergeResult."""
        res = UnmergeResult()
        self._call("unmerge_maps", self._engine, src.ptr, dst.ptr, _fptr(mat_to_abi(X)),
                   C.byref(params) if params is not None else None, C.byref(res))
        return res

    def remerge_maps(self, src, dst, X_old, X_new, params=None):
        """dslam_remerge_maps: unmerge_maps(src, dst, X_old), then merge_maps(src, dst, X_new, params), in one call.
        Returns (UnmergeResult, MergeResult); both zeroed when the two transforms are bit-identical."""
        un, re = UnmergeResult(), MergeResult()
        self._call("remerge_maps", self._engine, src.ptr, dst.ptr, _fptr(mat_to_abi(X_old)), _fptr(mat_to_abi(X_new)),
                   C.byref(params) if params is not None else None, C.byref(un), C.byref(re))
        return un, re

    def debug_merge_phases(self, enable):
        """The phase times (ms) of the last merge measured with the hook on; then turns the hook on or off."""
        out = np.zeros(5, dtype=np.float64)
        self._call("debug_merge_phases", self._engine, C.c_int(int(enable)), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    # -- packed maps: the host half ------------------------------------------------------------------------
    def pack_layout(self, blocks, free_excess):
        """dslam_pack_layout (host only): (blocks_offset, total_bytes) of a packed map of n blocks and f free excess slots."""
        off, total = C.c_int64(), C.c_int64()
        self._call("pack_layout", C.c_int32(blocks), C.c_int32(free_excess), C.byref(off), C.byref(total))
        return off.value, total.value

    def pack_header_read(self, first_64_bytes):
        """dslam_pack_header_read (host only): the PackInfo in the first 64 bytes of a packed map; raises if it is none."""
        raw = bytes(first_64_bytes)
        if len(raw) < C.sizeof(PackInfo):
            raise ValueError("a packed map's header is 64 bytes")
        info = PackInfo()
        self._call("pack_header_read", C.c_char_p(raw), C.byref(info))
        return info

    # -- packed maps: the device half ----------------------------------------------------------------------
    def pack_scene(self, scene, buf_ptr=None, capacity=0):
        """dslam_pack_scene: the map's packed image into `capacity` bytes at `buf_ptr` (an address in device or
        page-locked host memory, 16-byte aligned); buf_ptr None is the size query.  Returns the header as a PackInfo."""
        info = PackInfo()
        self._call("pack_scene", self._engine, scene.ptr, C.c_void_p(buf_ptr or 0), C.c_int64(int(capacity)), C.byref(info))
        return info

    def unpack_scene(self, scene, buf_ptr, nbytes):
        """dslam_unpack_scene: the packed image of `nbytes` bytes at `buf_ptr` into `scene`.  Returns its header."""
        info = PackInfo()
        self._call("unpack_scene", self._engine, scene.ptr, C.c_void_p(buf_ptr), C.c_int64(int(nbytes)), C.byref(info))
        return info

    def device_alloc(self, nbytes):
        """dslam_device_alloc: the address of `nbytes` of device memory on the engine's device; release with device_free."""
        p = C.c_void_p()
        self._call("device_alloc", self._engine, C.c_size_t(int(nbytes)), C.byref(p))
        return p.value

    def device_free(self, ptr):
        self._call("device_free", self._engine, C.c_void_p(ptr))

    def debug_live_engines(self):
        """dslam_debug_live_engines: engine objects of this process not yet freed (needs no engine)."""
        out = C.c_int(-1)
        self._call("debug_live_engines", C.byref(out))
        return out.value

    # -- page-locked host images -----------------------------------------------------------------------
    def host_alloc(self, shape, dtype):
        """A zero-filled numpy array over page-locked memory (dslam_host_alloc): view_update* in synchronous mode
        DMA straight out of such arrays.  Release with host_free(array) once nothing refers to it any more."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._call("host_alloc", C.c_size_t(n), C.byref(p))
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        self._call("host_free", C.c_void_p(self._pinned.pop(arr.ctypes.data)))

    # -- read-back -------------------------------------------------------------------------------------
    def stats(self, scene, rs=None):
        st = Stats()
        self._call("get_stats", self._engine, scene.ptr, rs.ptr if rs is not None else None, C.byref(st))
        return st.as_dict()

    def download_hash_table(self, scene):
        out = np.empty(scene.n_entries, dtype=HASH_ENTRY_DTYPE)
        self._call("download_hash_table", self._engine, scene.ptr, _vptr(out))
        return out

    def download_voxel_blocks(self, scene, first=0, count=None):
        count = scene.params.num_local_blocks - first if count is None else count
        out = np.empty((count, BLOCK_SIZE3), dtype=VOXEL_DTYPE)
        self._call("download_voxel_blocks", self._engine, scene.ptr, C.c_int(first), C.c_int(count), _vptr(out))
        return out

    def download_allocation_list(self, scene):
        out = np.empty(scene.params.num_local_blocks, dtype=np.int32)
        self._call("download_allocation_list", self._engine, scene.ptr, _vptr(out))
        return out

    def download_excess_list(self, scene):
        out = np.empty(scene.params.num_excess, dtype=np.int32)
        self._call("download_excess_list", self._engine, scene.ptr, _vptr(out))
        return out

    def download_visible_ids(self, rs):
        out = np.empty(rs.n_local, dtype=np.int32)
        n = C.c_int()
        self._call("download_visible_ids", self._engine, rs.ptr, _vptr(out), C.c_int(rs.n_local), C.byref(n))
        return out[:min(n.value, rs.n_local)].copy()

    def download_visible_types(self, rs):
        out = np.empty(rs.n_entries, dtype=np.uint8)
        self._call("download_visible_types", self._engine, rs.ptr, _vptr(out))
        return out

    def download_range_image(self, rs):
        out = np.empty((rs.height, rs.width, 2), dtype=np.float32)
        self._call("download_range_image", self._engine, rs.ptr, _fptr(out))
        return out

    def download_raycast_result(self, rs):
        out = np.empty((rs.height, rs.width, 4), dtype=np.float32)
        self._call("download_raycast_result", self._engine, rs.ptr, _fptr(out))
        return out

    def download_view_depth(self, view):
        out = np.empty((view.height_d, view.width_d), dtype=np.float32)
        self._call("download_view_depth", self._engine, view.ptr, _fptr(out))
        return out

    def download_swap_states(self, scene):
        out = np.empty(scene.n_entries, dtype=np.uint8)
        self._call("download_swap_states", self._engine, scene.ptr, _vptr(out))
        return out

    def download_alloc_scratch(self, scene):
        types = np.empty(scene.n_entries, dtype=np.uint8)
        coords = np.empty((scene.n_entries, 4), dtype=np.int16)
        self._call("download_alloc_scratch", self._engine, scene.ptr, _vptr(types), _vptr(coords))
        return types, coords

    def download_last_seen(self, scene):
        out = np.empty(scene.params.num_local_blocks, dtype=np.int32)
        self._call("download_last_seen", self._engine, scene.ptr, _vptr(out))
        return out

    def download_stored_block(self, scene, entry):
        out = np.empty(BLOCK_SIZE3, dtype=VOXEL_DTYPE)
        rc = self._call("download_stored_block", self._engine, scene.ptr, C.c_int(entry), _vptr(out))
        return bool(rc), out

    def upload_scene_state(self, scene, hash_table=None, allocation_list=None, last_free_block_id=0, excess_list=None,
                           last_free_excess_id=0):
        h = np.ascontiguousarray(hash_table, dtype=HASH_ENTRY_DTYPE) if hash_table is not None else None
        a = np.ascontiguousarray(allocation_list, dtype=np.int32) if allocation_list is not None else None
        x = np.ascontiguousarray(excess_list, dtype=np.int32) if excess_list is not None else None
        self._call("upload_scene_state", self._engine, scene.ptr, _vptr(h), _vptr(a), C.c_int(last_free_block_id),
                   _vptr(x), C.c_int(last_free_excess_id))

    def upload_voxel_blocks(self, scene, first, blocks):
        b = np.ascontiguousarray(blocks, dtype=VOXEL_DTYPE)
        self._call("upload_voxel_blocks", self._engine, scene.ptr, C.c_int(first), C.c_int(b.size // BLOCK_SIZE3),
                   _vptr(b))

    def track_dirty(self, scene, enable):
        self._call("scene_track_dirty", self._engine, scene.ptr, C.c_int(int(enable)))

    def shard_dirty_plan(self, scene, num_shards, chunk_blocks):
        counts = (C.c_int32 * num_shards)()
        self._call("shard_dirty_plan", self._engine, scene.ptr, C.c_int(num_shards), C.c_int(chunk_blocks), counts)
        return list(counts)

    def shard_dirty_pack(self, scene, shard, send_ptr, capacity_blocks):
        self._call("shard_dirty_pack", self._engine, scene.ptr, C.c_int(shard), C.c_void_p(send_ptr), C.c_int(capacity_blocks))

    def shard_dirty_unpack(self, scene, skip_shard, recv_ptr, stride_blocks):
        self._call("shard_dirty_unpack", self._engine, scene.ptr, C.c_int(skip_shard), C.c_void_p(recv_ptr), C.c_int(stride_blocks))

    def upload_visible_ids(self, rs, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        self._call("upload_visible_ids", self._engine, rs.ptr, _vptr(ids), C.c_int(ids.size))

    # -- instrumentation (product only) ----------------------------------------------------------------
    def time_integrate(self, scene, view, rs, M_d, intr, iterations):
        m, k = self._mi(M_d, intr)
        ms = C.c_float()
        nb = C.c_int()
        self._call("time_integrate", self._engine, scene.ptr, view.ptr, rs.ptr, _fptr(m), _fptr(k), C.c_int(iterations),
                   C.byref(ms), C.byref(nb))
        return ms.value, nb.value

    def kernel_timer_enable(self, flag):
        self._call("kernel_timer_enable", self._engine, C.c_int(int(flag)))

    def kernel_timer_read(self):
        ms = C.c_double()
        n = C.c_int64()
        nb = C.c_int64()
        self._call("kernel_timer_read", self._engine, C.byref(ms), C.byref(n), C.byref(nb))
        return ms.value, n.value, nb.value

    def scene_voxel_blocks_dev(self, scene):
        f = getattr(self.lib, self.prefix + "scene_voxel_blocks_dev")
        f.restype = C.c_void_p
        return f(scene.ptr)

    def render_state_image_dev(self, rs, want_float):
        f = getattr(self.lib, self.prefix + "render_state_image_dev")
        f.restype = C.c_void_p
        return f(rs.ptr, C.c_int(int(want_float)))
