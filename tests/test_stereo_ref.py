"""tests/ref_stereo.py is a stereo matcher and not merely a law: on the random-dot stereogram it recovers the surfaces,
rejects most of what the right image does not see, and is rarely wrong where it accepts.  The conditions keep later edits of
the law honest; they are not tolerances for the GPU, which is held to the reference bit for bit (test_gpu_stereo.py).  Also
here: the bounds the device code rests on, and that the crafted S volumes produce the corners they are named for."""
import numpy as np
import pytest

import ref_stereo as rs
import stereo_fixtures as sf

CASES = [(160, 60, 64), (288, 60, 128)]
SEEDS = range(5)


def shares(W, H, D, seed, **encoded):
    left, right, disp, visible = sf.stereogram(W, H, D, seed)
    d16 = rs.match(left, right, rs.resolve(dict(encoded, max_disparity=D)))["disp"].astype(np.int64)
    accepted = d16 != rs.INVALID
    good = accepted & (np.abs(d16 - 16 * disp) <= 8)
    return good[visible].mean(), accepted[~visible].mean(), (accepted & ~good).sum() / accepted.sum(), visible


@pytest.mark.parametrize("W,H,D", CASES, ids=lambda v: str(v))
def test_the_reference_recovers_the_stereogram(W, H, D):
    for seed in SEEDS:
        recovered, hidden_accepted, accepted_wrong, visible = shares(W, H, D, seed)
        print(f"{W}x{H} D={D} seed {seed}: recovered {recovered:.4f} hidden accepted {hidden_accepted:.4f} accepted wrong {accepted_wrong:.4f}")
        assert 0.05 < (~visible).mean() < 0.5          # the scene has occlusions and a left border to speak of
        assert recovered >= 0.95
        assert hidden_accepted <= 0.30
        assert accepted_wrong <= 0.04


@pytest.mark.parametrize("W,H,D", CASES, ids=lambda v: str(v))
def test_with_both_filters_off_every_pixel_inside_is_accepted(W, H, D):
    left, right, _, _ = sf.stereogram(W, H, D, 0)
    out = rs.match(left, right, rs.resolve(rs.encode(max_disparity=D, uniqueness=0, lr_max=-1)))
    ds = out["S"].astype(np.int64).argmin(axis=2)
    inside = np.arange(W)[None, :] - ds >= 0
    assert np.array_equal(out["disp"] != rs.INVALID, inside) and inside.mean() > 0.99   # (outside: the crafted left_of_image)


@pytest.mark.parametrize("p1,p2", [(10, 120), (1, 1), (192, 192), (1, 192)])
def test_path_costs_fit_a_byte_and_their_sum_its_bound(p1, p2):
    left, right = sf.random_pair(48, 16, seed=3)
    out = rs.match(left, right, rs.resolve(dict(max_disparity=64, p1=p1, p2=p2)), each=True)
    assert len(out["L"]) == 8
    for L in out["L"]:
        assert L.min() >= 0 and L.max() <= rs.COST_OUT + p2 <= 255
    S = sum(out["L"])
    assert np.array_equal(S, out["S"]) and S.max() <= 8 * (rs.COST_OUT + p2)
    if p1 == 192:
        assert max(L.max() for L in out["L"]) == 255    # the byte's last value is reached


def test_census_and_cost_by_hand():
    g = np.arange(7 * 9, dtype=np.int32).reshape(7, 9)
    c = rs.census(g)
    # the centre pixel: the 31 neighbours before it in row-major order are smaller, the 31 after it are not
    assert int(c[3, 4]) == ((1 << 31) - 1) << 31
    assert int(c[0, 0]) == 0 and int(c[6, 8]) == (1 << 62) - 1 - sum(1 << (61 - i) for i in clamped_equal(6, 8))
    one = np.array([[5]], dtype=np.uint8)
    assert int(rs.census(rs.grey(one, 1))[0, 0]) == 0
    cl = np.array([[0, 0b1011, (1 << 62) - 1]], dtype=np.uint64)
    C = rs.cost(cl, np.zeros_like(cl), 64)
    assert C[0, 1, 0] == 3 and C[0, 1, 1] == 3 and C[0, 1, 2] == rs.COST_OUT and C[0, 2, 2] == 62 and (C[0, 2, 3:] == rs.COST_OUT).all()
    rgba = np.array([[[1, 2, 3, 200], [255, 255, 255, 0], [0, 1, 0, 9]]], dtype=np.uint8)
    assert rs.grey(rgba, 4).tolist() == [[2, 255, 0]]


def clamped_equal(y, x, H=7, W=9):
    """The neighbour indices (row-major, centre skipped) whose clamped coordinate is the pixel itself: not smaller."""
    out, i = [], 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            if (min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)) == (y, x):
                out.append(i)
            i += 1
    return out


@pytest.mark.parametrize("D", [64, 128])
def test_the_crafted_volumes_produce_their_corners(D):
    cr = sf.crafted(D)
    X = D + 4
    sel = {name: rs.select(S, u, lr).astype(np.int64) for name, (S, u, lr) in cr.items()}
    for a in (0, D // 2, D - 2):
        assert sel[f"tie_{a}_{a + 1}"][0, X] // 16 == a
    assert sel["end_0"][0, X] == 0 and sel["end_last"][0, X] == 16 * (D - 1)
    # den == 0 needs S(d* - 1) == s0, which the smallest-d rule excludes for d* > 0; a plateau to the right is the nearest
    # case, and the largest step: sm > s0 == sp gives num = 17 den, delta = +8
    assert sel["plateau"][0, X] == 16 * 9 + 8
    # the floor division: negative numerators with and without remainder, and C's truncation would differ
    S = cr["floor_residues"][0].astype(np.int64)
    at = S[:, :, 11] == 100
    sm, sp = S[:, :, 10][at], S[:, :, 12][at]
    num, den2 = 16 * (sm - sp) + (sm + sp - 200), 2 * (sm + sp - 200)
    assert at.sum() >= 70 and (num < 0).sum() >= 60
    assert ((num < 0) & (num % den2 == 0)).sum() >= 2 and ((num < 0) & (num % den2 != 0)).sum() >= 50
    truncated = np.trunc(num / den2).astype(np.int64)
    assert (truncated != num // den2).sum() >= 50
    assert np.array_equal(sel["floor_residues"][at], 16 * 11 + num // den2)
    assert (np.abs(num // den2) <= 8).all()
    for d in sorted(set(den2.tolist()))[:6]:
        # every residue this denominator admits occurs: num = 16 k + den with k = sm - sp in -den .. -1 of den's parity
        den = d // 2
        k = np.arange(-den, 0, 2)
        assert set(((16 * k + den) % d).tolist()) == set((num[den2 == d] % d).tolist()), d
    u = sel["uniqueness_edge"][0]
    assert [u[X], u[X - 3], u[X - 6]] == [16 * 30, rs.INVALID, 16 * 30]
    assert sel["left_of_image"][0, 5] == rs.INVALID and rs.select(np.roll(cr["left_of_image"][0], 5, axis=1), 0, -1)[0, 10] != rs.INVALID
    assert rs.right_disparity(cr["right_tie"][0])[0, 40] == 3
    assert [sel["right_tie"][0, 43], sel["right_tie"][0, 47]] == [48, rs.INVALID]
    assert [sel["right_tie_exact"][0, 43], sel["right_tie_exact"][0, 47]] == [48, rs.INVALID]
    assert [sel["right_tie_wide"][0, 43], sel["right_tie_wide"][0, 47]] == [48, 112]


def test_depth_by_hand():
    d16 = np.array([0, 1, 16, 160, 16 * 63, rs.INVALID], dtype=np.uint16)
    mm = rs.depth_mm(d16, 480.0, 0.54, 1.0, 0.5, 30.0)
    # 480 * 0.54 = 259.2 m px: d = 1/16 -> 4147 m (beyond), d = 1 -> 259 m (beyond), d = 10 -> 25.92 m, d = 63 -> 4.114 m
    assert mm.tolist() == [0, 0, 0, 25920, 4114, 0] or mm.tolist() == [0, 0, 0, 25919, 4114, 0]
    assert rs.depth_mm(np.array([16 * 100], np.uint16), 48.0, 0.5, 1.0, 0.5, 30.0).tolist() == [0]   # 0.24 m: nearer than min
    with pytest.raises(ValueError):
        rs.depth_mm(d16, 480.0, 0.54, 1.0, 0.5, 32.8)
