"""What the five calls that take a list of maps -- (scenes[], T_map_from_world[], num_maps) -- reject, and where they
differ ("the multi-map calls' shared host code"):

    call               num_maps   a scene listed twice   a transform must be
    get_image_multi    1 .. MAX   allowed                invertible (the determinant test of invert_matrix)
    mesh_scene_multi   1 .. MAX   allowed                invertible
    register_graph     2 .. MAX   rejected               finite, rotation block orthonormal to 1e-4
    survey_overlaps    2 .. MAX   rejected               finite, rotation block orthonormal
    track_camera_sdf   1 .. MAX   rejected               finite, rotation block orthonormal

All five reject a count out of range, a NULL scene, a scene of another engine, a scene with another voxel_size and a
singular transform, with status -1.  A NaN has no determinant of zero, so the two calls that only ask for an invertible
transform let it through; the three others reject it as not finite.  The maps are empty and as small as a scene may be, so
an accepted call launches kernels over nothing and only has to return status 0."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 32, 24
CALLS = ("get_image_multi", "mesh_scene_multi", "register_graph", "survey_overlaps", "track_camera_sdf")
RIGID_ONLY = ("register_graph", "survey_overlaps", "track_camera_sdf")   # no scene twice, transforms finite and orthonormal


@pytest.fixture(scope="module")
def world(pkg, gpu):
    p = dict(num_local_blocks=64, num_buckets=256, num_excess=16)
    A, B = gpu.create_scene(pkg.SceneParams(**p)), gpu.create_scene(pkg.SceneParams(**p))
    other_vs = gpu.create_scene(pkg.SceneParams(voxel_size=0.006, **p))
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = second.create_scene(pkg.SceneParams(**p))
    view = gpu.create_view(W, H)
    gpu.view_update(view, np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.int16))
    rs = gpu.create_render_state(A, W, H)
    return dict(A=A, B=B, other_vs=other_vs, foreign=foreign, second=second, view=view, rs=rs)


def invoke(pkg, gpu, world, name, scenes, Ts, n=None):
    """The raw entry point `name` on (scenes, Ts) with everything else valid; returns the status or raises DslamError."""
    cap = pkg.MAX_RENDER_MAPS + 1   # (room for every count the test passes, whatever the call reads before it checks)
    ptrs = (C.c_void_p * cap)(*[None if s is None else s.ptr for s in scenes])
    t_abi = np.concatenate([pkg.mat_to_abi(t) for t in Ts] + [pkg.mat_to_abi(np.eye(4))] * (cap - len(Ts)))
    num = C.c_int(len(scenes) if n is None else n)
    fptr, i32 = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    T = t_abi.ctypes.data_as(fptr)
    I = pkg.mat_to_abi(np.eye(4))
    intr = np.array([30.0, 30.0, 16.0, 12.0], np.float32)
    if name == "get_image_multi":
        out = np.empty((H, W), np.float32)
        return gpu._call(name, gpu._engine, ptrs, T, num, world["rs"].ptr, I.ctypes.data_as(fptr), intr.ctypes.data_as(fptr),
                         C.c_int(pkg.IMAGE_DEPTH), None, out.ctypes.data_as(fptr))
    if name == "mesh_scene_multi":
        total, counts = C.c_int(0), np.zeros(cap, np.int32)
        return gpu._call(name, gpu._engine, ptrs, T, num, C.c_int(0), C.c_int(0), C.byref(total), counts.ctypes.data_as(i32))
    if name == "register_graph":
        pairs = np.array([0, 1], np.int32)
        res, pres = pkg.RegisterGraphResult(), (pkg.RegisterPairResult * 1)()
        return gpu._call(name, gpu._engine, ptrs, T, num, pairs.ctypes.data_as(i32), C.c_int(1), C.c_int(0), None, C.byref(res),
                         pres)
    if name == "survey_overlaps":
        live, blocks, octants = np.zeros(cap, np.int32), np.zeros(cap * cap, np.int32), np.zeros(cap * cap, np.int32)
        return gpu._call(name, gpu._engine, ptrs, T, num, live.ctypes.data_as(i32), blocks.ctypes.data_as(i32),
                         octants.ctypes.data_as(i32))
    assert name == "track_camera_sdf"
    res = pkg.TrackSdfResult()
    return gpu._call(name, gpu._engine, world["view"].ptr, ptrs, T, num, I.ctypes.data_as(fptr), intr.ctypes.data_as(fptr), None,
                     C.byref(res))


@pytest.mark.parametrize("name", CALLS)
def test_what_a_map_list_call_rejects(pkg, gpu, world, name):
    A, B = world["A"], world["B"]
    I4 = np.eye(4, dtype=np.float32)
    nan, singular, skew = I4.copy(), I4.copy(), I4.copy()
    nan[0, 0] = np.nan
    singular[1, 1] = 0.0
    skew[0, 1] += 0.01          # invertible, rows 0 and 1 no longer orthogonal (their product is 0.01 > 1e-4)
    rigid = name in RIGID_ONLY
    cases = [
        # what, scenes, transforms, num_maps (None: the list's length), rejected (a string: and the message says so)
        ("two maps", (A, B), (I4, I4), None, False),
        ("num_maps 0", (A, B), (I4, I4), 0, True),
        ("num_maps MAX + 1", (A, B), (I4, I4), pkg.MAX_RENDER_MAPS + 1, True),
        ("a NULL scene", (A, None), (I4, I4), None, True),
        ("a scene of another engine", (A, world["foreign"]), (I4, I4), None, True),
        ("another voxel_size", (A, world["other_vs"]), (I4, I4), None, True),
        ("a NaN in a transform", (A, B), (I4, nan), None, "not finite" if rigid else False),
        ("a singular transform", (A, B), (I4, singular), None, True),
        ("a skewed, invertible transform", (A, B), (I4, skew), None, "not orthonormal" if rigid else False),
        ("the same scene twice", (A, A), (I4, I4), None, rigid),
    ]
    for what, scenes, Ts, n, rejected in cases:
        try:
            outcome = invoke(pkg, gpu, world, name, scenes, Ts, n)
        except pkg.DslamError as err:
            outcome = str(err)
        if rejected:
            assert isinstance(outcome, str) and "status -1 " in outcome, f"{what}: {outcome!r}"
            assert rejected is True or rejected in outcome, f"{what}: {outcome!r}"
        else:
            assert outcome == 0, f"{what}: {outcome!r}"
