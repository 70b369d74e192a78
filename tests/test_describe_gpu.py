"""describe alone (ORBextractor.debug_describe) on planted keypoints against the CPU oracle: every keypoint
record as float bits and all 32 descriptor bytes of every planted point, no tolerance.  The images and
positions (tests/describe_ref.py) reach what FAST corners on natural scenes reach only by luck: reflected
borders, both sides of every edge of the interior predicate, every (base & 3) realignment, the odd level-0
row step, the fast_atan2 corner inputs, saturated patches and exact ties, the score field and the level
scale up to the top level -- under both trig modes, the three launch grids and several frames.
test_planted_inputs_are_sharp asserts, from the plain numpy reference, that the inputs do reach them."""
import os

import numpy as np
import pytest

import describe_ref as R
from orb_slam2_refactored_amd import ORBextractor
from orb_slam2_refactored_amd._lib import OrbError

pytestmark = pytest.mark.gpu

GRIDS = {"table": {}, "dense": {"ORBX_DESC_DENSE": "1"}, "overflow": {"ORBX_DESC_DENSE": "1", "ORBX_DESC_C": "64"}}


def make(grid="table", trig="double"):
    env = GRIDS[grid]
    os.environ.update(env)
    try:
        ex = ORBextractor(ORBextractor.Parameters(R.NFEATURES, R.SCALE, R.NLEVELS))
    finally:
        for k in env:
            del os.environ[k]
    ex.set_opencv_compat(trig=trig)
    return ex


@pytest.fixture(scope="module")
def ex():
    return make()


def expected(oracle, name, W=R.W0, trig="double"):
    _, img, pts = R.case(name, W, R.H0)
    with oracle.compat(trig=trig):
        return oracle.describe(R.params(oracle), img, pts)


def test_planted_inputs_are_sharp():
    odd = set()
    for W in (321, 323):
        for n in R.VARIANT_CASES:
            odd |= set(R.reference(n, W, R.H0)["path"])
    R.assert_sharp(R.sharpness(), odd)


@pytest.mark.parametrize("name", [c[0] for c in R.cases()])
def test_family_exact(oracle, ex, name):
    _, img, pts = R.case(name)
    kps, desc = ex.debug_describe(img, pts)
    okps, odesc = expected(oracle, name)
    R.same_records(kps, okps, desc, odesc)


@pytest.mark.parametrize("trig", ["double", "float"])
@pytest.mark.parametrize("W", [321, 323])
def test_odd_level0_step_exact(oracle, W, trig):
    e = make(trig=trig)
    for name in R.VARIANT_CASES:
        _, img, pts = R.case(name, W, R.H0)
        kps, desc = e.debug_describe(img, pts)
        okps, odesc = expected(oracle, name, W, trig)
        R.same_records(kps, okps, desc, odesc)


@pytest.mark.parametrize("trig", ["double", "float"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_trig_modes_and_grids_exact(oracle, grid, trig):
    """The slot-table grid, the dense grid (its C from the call before) and a forced C = 64 that sends most
    of the 464 rows through describe_overflow_kernel; two calls per image so the dense grid runs with both
    its first C (every row) and the one sized from the previous call."""
    e = make(grid, trig)
    for name in R.VARIANT_CASES:
        _, img, pts = R.case(name)
        okps, odesc = expected(oracle, name, trig=trig)
        for _ in range(2):
            kps, desc = e.debug_describe(img, pts)
            R.same_records(kps, okps, desc, odesc)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_three_frames_equal_their_single_frame_results(oracle, grid):
    """F = 3 different images in one call (the dense grid's frame divide, the overflow kernel's frame loop):
    every frame equals its own single-frame call and the oracle; the same call three times is
    byte-identical."""
    e = make(grid)
    pts = R.positions(R.W0, R.H0)
    frames = np.stack([R.case(n)[1] for n in R.VARIANT_CASES])
    outs = [e.debug_describe(frames, pts) for _ in range(3)]
    for k, d in outs[1:]:
        assert k.tobytes() == outs[0][0].tobytes() and d.tobytes() == outs[0][1].tobytes()
    kps, desc = outs[0]
    assert kps.shape == (3, len(pts)) and desc.shape == (3, len(pts), 32)
    for f, name in enumerate(R.VARIANT_CASES):
        k1, d1 = e.debug_describe(frames[f], pts)
        R.same_records(kps[f], k1, desc[f], d1)
        okps, odesc = expected(oracle, name)
        R.same_records(kps[f], okps, desc[f], odesc)


def test_pyramid_is_extracts(ex):
    """The planted call builds the pyramid Extract builds."""
    _, img, pts = R.case("synth")
    ex.debug_describe(img, pts)
    planted = ex.GetImagePyramid()
    other = make()
    other.Extract(img)
    for a, b in zip(planted, other.GetImagePyramid()):
        assert np.array_equal(a, b)


def test_rejects_points_extract_cannot_produce(oracle, ex):
    _, img, pts = R.case("noise")
    dims = R.level_dims(R.W0, R.H0)
    w7, h7 = dims[7]
    bad = [(8, 30, 30, 1), (-1, 30, 30, 1), (0, 18, 30, 1), (0, R.W0 - 19, 30, 1), (0, 30, 18, 1),
           (0, 30, R.H0 - 19, 1), (7, w7 - 19, 30, 1), (7, 30, h7 - 19, 1), (0, 30, 30, 256), (0, 30, 30, -1)]
    for b in bad:
        with pytest.raises(OrbError, match="planted point"):
            ex.debug_describe(img, np.concatenate([pts[:5], np.array([b], np.int32)]))
    # more points on the top level than its selection capacity (the level's share of max_keypoints)
    cap7 = max(int(ex.FeaturesPerLevel()[7]) + 3, 4 * 2) + 1   # 89 x 67: two quadtree roots
    many = np.array([(7, 30, 30, 1)] * (cap7 + 1), np.int32)
    with pytest.raises(OrbError, match="selection capacity"):
        ex.debug_describe(img, many)
    k, d = ex.debug_describe(img, many[:cap7])   # exactly the capacity is accepted
    assert (d == d[0]).all() and len(k) == cap7
    # a level too low for one 30-row FAST cell takes no keypoints, though FAST's range is not empty on it
    small = ORBextractor(ORBextractor.Parameters(500, 1.2, 8))
    assert R.level_dims(160, 120)[4] == (77, 58)
    flat = np.zeros((120, 160), np.uint8)
    with pytest.raises(OrbError, match="takes no keypoints"):
        small.debug_describe(flat, np.array([(4, 30, 25, 1)], np.int32))
    assert (small.debug_describe(flat, np.array([(3, 30, 25, 1)], np.int32))[1] == 0).all()
    # the handle still works after the refusals
    kps, desc = ex.debug_describe(img, pts)
    okps, odesc = expected(oracle, "noise")
    R.same_records(kps, okps, desc, odesc)
