"""tests/frame_ref.py, the restatement the frame builder is compared with, pinned on hand cases: the k1 == 0 rule, the
principal point, five iterations written out in Python scalars, 4 against 5 coefficients, the forward model on a TUM1 grid
(which cross-checks the recalled formula; it does not prove OpenCV parity), the iteration count, the TUM1 bounds, the
depth rule and the truncation of (int)pt.  CPU only."""
import numpy as np

import frame_ref as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def tum1_grid():
    xs, ys = np.linspace(0, 640, 41), np.linspace(0, 480, 31)   # edges included
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(f32)


def test_k1_zero_returns_the_input_bits_and_the_plain_bounds():
    rng = np.random.default_rng(0)
    xy = rng.uniform(-5, 700, (50, 2)).astype(f32)
    xy[0] = (-0.0, np.nan)
    for k1 in (0.0, -0.0):
        dist = np.array([k1, 0.3, 0.01, -0.02, 0.5], f32)   # the other coefficients do not matter
        assert np.array_equal(bits(R.keypoint_xy(R.TUM1_CAMERA, dist, xy)), bits(xy))
        assert np.array_equal(bits(R.image_bounds(480, 640, R.TUM1_CAMERA, dist)), bits([0, 640, 0, 480]))
    assert not np.array_equal(bits(R.keypoint_xy(R.TUM1_CAMERA, R.TUM1_DIST, xy[1:])), bits(xy[1:]))


def test_the_principal_point_maps_to_itself():
    for cam, dist in ((R.TUM1_CAMERA, R.TUM1_DIST), (R.TUM2_CAMERA, R.TUM2_DIST)):
        got = R.undistort(cam, dist, cam[2:4].reshape(1, 2))
        assert np.array_equal(bits(got), bits(cam[2:4].reshape(1, 2)))


def test_pure_k1_against_five_iterations_in_python_scalars():
    cam = np.array([500, 510, 320, 240, 40], f32)
    k1 = float(f32(0.2))
    for u, v in ((20.0, 30.0), (611.5, 402.25)):
        x0 = (float(f32(u)) - 320.0) * (1.0 / 500.0)
        y0 = (float(f32(v)) - 240.0) * (1.0 / 510.0)
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1 + ((0.0 * r2 + 0.0) * r2 + k1) * r2)
            x, y = (x0 - 0.0) * icdist, (y0 - 0.0) * icdist
        want = [f32(500.0 * x + 0.0 * y + 320.0), f32(0.0 * x + 510.0 * y + 240.0)]
        got = R.undistort(cam, np.array([k1, 0, 0, 0, 0], f32), np.array([[u, v]], f32))
        assert np.array_equal(bits(got[0]), bits(want)), (u, v)
        assert abs(float(got[0, 0]) - u) > 0.5   # the distortion is not a no-op here


def test_four_coefficients_are_five_with_k3_zero():
    xy = tum1_grid()
    assert np.array_equal(bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST[:4], xy)),
                          bits(R.undistort(R.TUM1_CAMERA, np.append(R.TUM1_DIST[:4], f32(0)), xy)))
    assert not np.array_equal(bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST[:4], xy)), bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST, xy)))


def forward_miss(cam, dist, xy, iters):
    return np.abs(R.distort(cam, dist, R.undistort(cam, dist, xy, iters)) - xy.astype(np.float64)).max()


def test_the_forward_model_returns_the_input_on_the_tum1_grid():
    xy = tum1_grid()
    assert len(xy) == 41 * 31
    m5, m10 = forward_miss(R.TUM1_CAMERA, R.TUM1_DIST, xy, 5), forward_miss(R.TUM1_CAMERA, R.TUM1_DIST, xy, 10)
    print("TUM1 forward miss, 5 iterations", m5, "10 iterations", m10)
    assert m5 < 0.2      # measured 0.110 px: a wrong formula misses by pixels
    assert m10 < 1e-3    # measured 4e-4 px
    assert m5 > 10 * m10   # five iterations are not converged: the count is observable


def test_the_fifth_and_sixth_iteration_differ_in_bits():
    xy = tum1_grid()
    assert not np.array_equal(bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST, xy, 5)), bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST, xy, 6)))
    assert np.array_equal(bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST, xy)), bits(R.undistort(R.TUM1_CAMERA, R.TUM1_DIST, xy, 5)))


def test_the_tum1_bounds():
    b = R.image_bounds(480, 640, R.TUM1_CAMERA, R.TUM1_DIST)
    assert np.abs(b.astype(np.float64) - [10.801, 626.048, 14.669, 473.312]).max() < 1e-3, b


def test_a_negative_icdist_leaves_the_loop_with_the_first_guess():
    """The chosen behaviour (newer OpenCV's; parity unpinned): the point comes back where it was."""
    cam = np.array([500, 500, 320, 240, 40], f32)
    dist = np.array([-5.0, 0, 0, 0, 0], f32)   # 1 + k1 * r2 < 0 for r2 > 0.2
    xy = np.array([[640, 480], [330, 250]], f32)
    got = R.undistort(cam, dist, xy)
    assert np.array_equal(bits(got[0]), bits(f32([640, 480])))     # left at the first iteration: x0 * fx + cx
    assert not np.array_equal(bits(got[1]), bits(xy[1]))           # r2 small: iterates as usual


def test_the_depth_rule():
    bf, x = f32(40), f32(100.5)
    for d in (0.0, -0.0, -3.0, np.nan):
        ur, dp = R.rgbd(f32(d), x, bf)
        assert ur == -1 and dp == -1, d
    ur, dp = R.rgbd(f32(np.inf), x, bf)
    assert dp == np.inf and ur == x   # bf / inf = 0
    sub = f32(1e-42)
    assert sub > 0 and sub < np.finfo(f32).tiny
    ur, dp = R.rgbd(sub, x, bf)
    assert bits(dp) == bits(sub) and ur == -np.inf   # 40 / 1e-42 overflows
    ur, dp = R.rgbd(f32(2.5), x, bf)
    assert bits(dp) == bits(f32(2.5)) and bits(ur) == bits(f32(100.5 - 16.0))
    factor = f32(1.0 / 5000.0)
    assert R.depth_value(np.uint16(0), factor) == 0 and R.rgbd(R.depth_value(np.uint16(0), factor), x, bf)[1] == -1
    assert bits(R.depth_value(np.uint16(1), factor)) == bits(factor)
    assert bits(R.depth_value(np.uint16(65535), factor)) == bits(f32(65535) * factor)
    assert R.rgbd(R.depth_value(np.uint16(65535), factor), x, bf)[1] > 13.1
    assert bits(R.depth_value(f32(5000), factor)) == bits(f32(5000) * factor)


def test_the_pixel_is_truncated():
    assert R.pixel(f32(3.99), f32(7.99), 480, 640) == (3, 7)
    assert R.pixel(f32(639.99), f32(479.99), 480, 640) == (639, 479)
    assert R.pixel(f32(-0.5), f32(0.0), 480, 640) == (0, 0)     # (int)-0.5 = 0
    assert R.pixel(f32(640.0), f32(0.0), 480, 640) is None
    assert R.pixel(f32(0.0), f32(-1.0), 480, 640) is None
    assert R.pixel(f32(np.nan), f32(5.0), 480, 640) is None
    depth = np.zeros((480, 640), f32)
    depth[7, 3], depth[8, 4] = 2.0, 9.0
    xy = np.array([[3.99, 7.99]], f32)
    ur, dp = R.stereo_from_rgbd(xy, xy, depth, 1.0, 40.0)
    assert dp[0] == 2.0 and ur[0] == f32(3.99) - f32(20)


def test_build_leaves_the_padding_and_the_stereo_arrays():
    rng = np.random.default_rng(3)
    kps = np.zeros((2, 5), R.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, (2, 5)), rng.uniform(0, 480, (2, 5))
    kps["octave"], kps["angle"] = rng.integers(0, 8, (2, 5)), rng.uniform(0, 360, (2, 5))
    cam, dist = np.stack([R.TUM1_CAMERA] * 2), np.stack([R.TUM1_DIST, np.zeros(5, f32)])
    out = dict(frame_n=np.full(2, 9, np.int32), kp_xy=np.full((2, 5, 2), 77, f32), kp_uright=np.full((2, 5), 55, f32),
               kp_depth=np.full((2, 5), 55, f32), kp_begin=np.zeros(3, np.int32), kp_un=np.full((2, 5, 7), 9, np.int32))
    R.build(kps, np.array([3, 7], np.int32), cam, dist, 480, 640, R.STEREO, out=out)
    assert out["frame_n"].tolist() == [3, 5] and out["kp_begin"].tolist() == [0, 5, 10]
    assert (out["kp_xy"][0, 3:] == 77).all() and (out["kp_xy"][0, :3] != 77).all() and (out["kp_uright"] == 55).all()
    assert np.array_equal(bits(out["kp_xy"][1, :, 0]), bits(kps["x"][1])) and (out["kp_un"][0, 3:] == 9).all()
    assert np.array_equal(out["kp_un"][1].view(R.KP_DTYPE).reshape(-1), kps[1])
    R.build(kps, np.array([3, -2], np.int32), cam, dist, 480, 640, R.MONO, out=out)
    assert (out["kp_uright"][0, :3] == -1).all() and (out["kp_uright"][0, 3:] == 55).all() and (out["kp_depth"][1] == 55).all()
