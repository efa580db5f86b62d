"""Inputs for the dslam_sflow_* tests: seeded textured frame pairs with a known disparity and motion, the golden cases
recorded from libviso2 itself (tests/golden/sflow_*.npz, written by tests/golden/make_sflow_golden.py), crafted cases for
the law's corners, and references computed once and shared read-only."""
import functools
import os

import numpy as np

import ref_sflow as rf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (W, H, half_resolution, disparity, (mx, my), method, seed, dense)
CASES = {
    "quad_160x96": (160, 96, 0, 7, (3, 2), 2, 1, False),
    "quad_96x64": (96, 64, 0, 5, (2, 1), 2, 2, False),
    "quad_131x77": (131, 77, 0, 6, (2, 1), 2, 3, False),
    "quad_320x128_half": (320, 128, 1, 8, (4, 2), 2, 4, False),
    "stereo_160x96": (160, 96, 0, 7, (3, 2), 1, 1, False),
    "flow_160x96": (160, 96, 0, 7, (3, 2), 0, 1, False),
    "quad_30x30": (30, 30, 0, 2, (1, 1), 2, 5, False),
    "quad_40x40": (40, 40, 0, 2, (1, 1), 2, 5, False),
    "dense_160x96": (160, 96, 0, 7, (3, 2), 2, 1, True),
}
IMAGES = ("1p", "2p", "1c", "2c")
# the library's eight feature arrays: (image, set)
SETS = {"m1p1": (rf.IMAGE_1P, 0), "m2p1": (rf.IMAGE_2P, 0), "m1c1": (rf.IMAGE_1C, 0), "m2c1": (rf.IMAGE_2C, 0),
        "m1p2": (rf.IMAGE_1P, 1), "m2p2": (rf.IMAGE_2P, 1), "m1c2": (rf.IMAGE_1C, 1), "m2c2": (rf.IMAGE_2C, 1)}
IMAGE_ID = {"1c": rf.IMAGE_1C, "2c": rf.IMAGE_2C, "1p": rf.IMAGE_1P, "2p": rf.IMAGE_2P}


def texture(w, h, seed, cell=5):
    """Cells of cell x cell pixels of uniform random grey from a 32-bit linear congruential generator."""
    cw, ch = -(-w // cell), -(-h // cell)
    x, vals = (seed * 2654435761 + 12345) & 0xFFFFFFFF, []
    for _ in range(cw * ch):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        vals.append(x >> 24)
    t = np.array(vals, np.uint8).reshape(ch, cw)
    return np.repeat(np.repeat(t, cell, axis=0), cell, axis=1)[:h, :w]


def frames(W, H, disparity, motion, seed):
    """{'1p', '2p', '1c', '2c'}: crops of one texture.  A point at u in the left image is at u - disparity in the right one,
    and a point at (u, v) in the previous frame is at (u + mx, v + my) in the current one."""
    mx, my = motion
    pad = 16
    t = texture(W + 2 * pad + disparity, H + 2 * pad, seed)

    def crop(x0, y0):
        return np.ascontiguousarray(t[y0:y0 + H, x0:x0 + W])
    return {"1p": crop(pad, pad), "2p": crop(pad + disparity, pad),
            "1c": crop(pad - mx, pad - my), "2c": crop(pad + disparity - mx, pad - my)}


def case_frames(name):
    W, H, half, d, motion, method, seed, dense = CASES[name]
    return frames(W, H, d, motion, seed)


def case_params(name):
    return rf.encode(half_resolution=CASES[name][2])


@functools.lru_cache(maxsize=None)
def golden(name):
    z = np.load(os.path.join(GOLDEN, "sflow_%s.npz" % name))
    return {k: z[k] for k in z.files}


def read_only(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(name):
    """The law on a golden case's inputs: {'filters': {side: 4 images}, 'features': {(image, set): records}, 'matches':
    {(method, set): records}}; computed once."""
    W, H, half, d, motion, method, seed, dense = CASES[name]
    g = golden(name)
    return reference_of(W, H, case_params(name), [(g["img_1p"], g["img_2p"]), (g["img_1c"], g["img_2c"])])


def reference_of(W, H, encoded, pushes, methods=(0, 1, 2)):
    m = rf.Matcher(W, H, encoded)
    for left, right in pushes:
        m.push(left, right)
    out = {"filters": {s: [read_only(a) for a in m.filter_images(s)] for s in (0, 1) if m.cur[s]["filters"] is not None},
           "features": {(i, s): read_only(m.features(i, s).copy()) for i in range(4) for s in (0, 1)},
           "matches": {(k, s): read_only(m.match(k, s)) for k in methods for s in (0, 1)}}
    return out


@functools.lru_cache(maxsize=None)
def size_reference(W, H, half):
    """A textured two-frame sequence of any size (disparity 4, motion (2, 1))."""
    f = frames(W, H, 4, (2, 1), 7)
    enc = rf.encode(half_resolution=half)
    return f, reference_of(W, H, enc, [(f["1p"], f["2p"]), (f["1c"], f["2c"])])


# ---------------------------------------------------------------------------------------------------------------------
# crafted cases: flat images with single pixels set.  A pixel of contrast 40 gives |f1| = 320 at itself and 40 around it, and
# |f2| = 40: with nms_tau = 50 it is exactly one feature, of class 1 (bright) or 0 (dark).  Full resolution, default parameters
# otherwise; every case says which property it puts on the table, and test_sflow_ref.py checks that it does.
# ---------------------------------------------------------------------------------------------------------------------
LEVEL, CONTRAST = 100, 40
FULL = rf.encode(half_resolution=0)


def flat(W, H, dots=()):
    img = np.full((H, W), LEVEL, np.uint8)
    for u, v, delta in dots:
        img[v, u] = LEVEL + delta
    return img


def crafted(name):
    """dict(W, H, pushes, method, set) of a crafted case."""
    b, d = CONTRAST, -CONTRAST
    if name == "plateau":
        # two equal blob maxima in the dense cell 16 .. 19 x 16 .. 19: the scan goes down column 17 before it reaches column 19,
        # so (17, 18) is the feature although (19, 16) comes first in row-major order
        img = flat(64, 48, [(17, 18, b), (19, 16, b)])
        return dict(W=64, H=48, pushes=[(img, img), (img, img)], method=2, set=1)
    if name == "clamped_hood":
        # w = 65: the last dense cell column is 52 .. 55 and w - 10 = 55.  The feature at (55, 20) has a better pixel at (57, 20)
        # inside u + 3, but the clamped bound stops at 55 and never sees it
        img = flat(65, 48, [(55, 20, b), (57, 20, b + 5)])
        return dict(W=65, H=48, pushes=[(img, img), (img, img)], method=2, set=1)
    if name == "tie":
        # flow: the current feature has two partners of equal cost in the previous image, A = (20, 60) in bin (0, 1) with the
        # lower index (its cell column comes first) and B = (30, 30) in bin (0, 0), which the bin walk meets first: B wins
        prev, cur = flat(64, 96, [(20, 60, b), (30, 30, b)]), flat(64, 96, [(25, 45, b)])
        return dict(W=64, H=96, pushes=[(prev, prev), (cur, cur)], method=0, set=1)
    if name in ("lonely_closes", "lonely_open"):
        # quad: the dark feature of 1p has no partner of its class anywhere, so every leg that asks for one answers feature 0.
        # closes: 1p holds nothing else, so the way back from 1c (a bright feature) finds no partner either and answers 0 = i1p.
        # open: 1p also holds a bright feature with the lower index; the dark one is i1p = 1, the way back answers 0
        bright = flat(96, 64, [(30, 30, b)])
        dark = flat(96, 64, [(40, 30, d)] + ([(20, 30, b)] if name == "lonely_open" else []))
        return dict(W=96, H=64, pushes=[(dark, bright), (bright, bright)], method=2, set=1)
    if name in ("two_classes_flow", "two_classes_stereo"):
        # a bright pixel in the middle of a faint checkerboard of 2 x 2 blocks: the blob maximum and the checkerboard maximum
        # are the same pixel, so two features (classes 1 and 3) share it; both match, and only the first is kept
        img = flat(64, 48)
        a = 10
        img[18:20, 18:20] += a
        img[21:23, 21:23] += a
        img[18:20, 21:23] -= a
        img[21:23, 18:20] -= a
        img[20, 20] += b
        return dict(W=64, H=48, pushes=[(img, img), (img, img)], method=0 if name.endswith("flow") else 1, set=1)
    raise KeyError(name)


CRAFTED = ("plateau", "clamped_hood", "tie", "lonely_closes", "lonely_open", "two_classes_flow", "two_classes_stereo")


@functools.lru_cache(maxsize=None)
def crafted_reference(name):
    c = crafted(name)
    return c, reference_of(c["W"], c["H"], FULL, c["pushes"], methods=(c["method"],))
