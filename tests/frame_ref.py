"""Frame construction restated sequentially in numpy (src/System.cc:153-219): cv::undistortPoints with float K and 4 or 5
float coefficients in float64 (restated from recall: exactly five fixed-point iterations, K applied again as a 3x3 product,
one rounding to float32), the k1 == 0 rule, ComputeImageBounds, depth.convertTo folded into ComputeStereoFromRGBD's lookup in
float32, and the split into the arrays the library's frame tables hold.  Nothing is imported from the library."""
import numpy as np

MONO, STEREO, RGBD = 0, 1, 2
ITERS = 5
f32, f64 = np.float32, np.float64

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])

TUM1_CAMERA = np.array([517.306408, 516.469215, 318.643040, 255.313989, 40.0], f32)
TUM1_DIST = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], f32)
TUM2_CAMERA = np.array([520.908620, 521.007327, 325.141442, 249.701764, 40.0], f32)
TUM2_DIST = np.array([0.231222, -0.784899, -0.003257, -0.000105, 0.917205], f32)


def coefficients(dist):
    """k1, k2, p1, p2, k3 as float64 scalars; four coefficients are five with k3 = 0."""
    d = [f64(f32(v)) for v in np.asarray(dist).reshape(-1)]
    assert len(d) in (4, 5)
    return d + [f64(0.0)] * (5 - len(d))


def undistort_double(camera, dist, xy, iters=ITERS):
    """The normalised undistorted points (x, y) in float64 after `iters` iterations, point by point elementwise.  A point
    whose icdist turns negative leaves the loop with its first guess (newer OpenCV; parity unpinned)."""
    fx, fy, cx, cy = (f64(f32(v)) for v in np.asarray(camera).reshape(-1)[:4])
    k1, k2, p1, p2, k3 = coefficients(dist)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    u, v = xy[:, 0].astype(f64), xy[:, 1].astype(f64)
    with np.errstate(all="ignore"):
        x0 = (u - cx) * (f64(1.0) / fx)
        y0 = (v - cy) * (f64(1.0) / fy)
        x, y = x0.copy(), y0.copy()
        live = np.ones(len(x), bool)
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = f64(1.0) / (f64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2)
            left = live & (icdist < 0)
            x[left], y[left] = x0[left], y0[left]
            live &= ~left
            dx = f64(2.0) * p1 * x * y + p2 * (r2 + f64(2.0) * x * x)
            dy = p1 * (r2 + f64(2.0) * y * y) + f64(2.0) * p2 * x * y
            nx, ny = (x0 - dx) * icdist, (y0 - dy) * icdist
            x, y = np.where(live, nx, x), np.where(live, ny, y)
    return x, y


def undistort(camera, dist, xy, iters=ITERS):
    """cv::undistortPoints(points, points, K, distCoeffs, cv::Mat(), K): (n, 2) float32."""
    fx, fy, cx, cy = (f64(f32(v)) for v in np.asarray(camera).reshape(-1)[:4])
    x, y = undistort_double(camera, dist, xy, iters)
    with np.errstate(all="ignore"):
        xx = fx * x + f64(0.0) * y + cx
        yy = f64(0.0) * x + fy * y + cy
        ww = f64(1.0) / (f64(0.0) * x + f64(0.0) * y + f64(1.0))
        return np.stack([(xx * ww).astype(f32), (yy * ww).astype(f32)], 1)


def distort(camera, dist, xy_un):
    """The forward model: the pixel a camera with these coefficients puts the undistorted pixel xy_un at (float64)."""
    fx, fy, cx, cy = (f64(f32(v)) for v in np.asarray(camera).reshape(-1)[:4])
    k1, k2, p1, p2, k3 = coefficients(dist)
    xy_un = np.asarray(xy_un, f64).reshape(-1, 2)
    x, y = (xy_un[:, 0] - cx) / fx, (xy_un[:, 1] - cy) / fy
    r2 = x * x + y * y
    c = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * c + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * c + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], 1)


def undistorted(dist):
    """UndistortKeyPoints' early return (:155): distCoeffs(0) == 0.f"""
    return f32(np.asarray(dist).reshape(-1)[0]) == f32(0.0)


def keypoint_xy(camera, dist, xy):
    xy = np.asarray(xy, f32).reshape(-1, 2)
    return xy.copy() if undistorted(dist) else undistort(camera, dist, xy)


def image_bounds(rows, cols, camera, dist):
    """ComputeImageBounds (:177-194): minx, maxx, miny, maxy."""
    h, w = f32(rows), f32(cols)
    if undistorted(dist):
        return np.array([0, w, 0, h], f32)
    c = undistort(camera, dist, np.array([[0, 0], [w, 0], [0, h], [w, h]], f32))
    smin = lambda a, b: b if b < a else a   # std::min   # noqa: E731
    smax = lambda a, b: b if a < b else a   # std::max   # noqa: E731
    return np.array([smin(c[0, 0], c[2, 0]), smax(c[1, 0], c[3, 0]), smin(c[0, 1], c[1, 1]), smax(c[2, 1], c[3, 1])], f32)


def depth_value(raw, depth_factor):
    """depth.convertTo(CV_32F, depthFactor) of one element: uint16 -> (float)raw * factor, float -> raw * factor."""
    with np.errstate(all="ignore"):
        return f32(f32(raw) * f32(depth_factor))


def pixel(x, y, rows, cols):
    """(u, v) = ((int)pt.x, (int)pt.y), or None when that is outside the image or a coordinate is NaN (the departure)."""
    x, y = f32(x), f32(y)
    if not (x > f32(-1) and x < f32(cols) and y > f32(-1) and y < f32(rows)):
        return None
    return int(np.trunc(x)), int(np.trunc(y))


def rgbd(d, x_un, bf):
    """ComputeStereoFromRGBD for one keypoint: (uright, depth)."""
    d = f32(d)
    if d > 0:   # NaN, zeros and negatives are out; +inf and denormals are in
        with np.errstate(all="ignore"):
            return f32(f32(x_un) - f32(bf) / d), d
    return f32(-1), f32(-1)


def stereo_from_rgbd(kps_xy, xy_un, depth_image, depth_factor, bf):
    """(uright, depth) float32 (n,) for one frame: kps_xy the distorted points, depth_image (rows, cols) uint16 or float32."""
    n = len(kps_xy)
    ur, dp = np.full(n, -1, f32), np.full(n, -1, f32)
    rows, cols = depth_image.shape
    for i in range(n):
        p = pixel(kps_xy[i, 0], kps_xy[i, 1], rows, cols)
        if p is not None:
            ur[i], dp[i] = rgbd(depth_value(depth_image[p[1], p[0]], depth_factor), xy_un[i, 0], bf)
    return ur, dp


OUT_KEYS = ("frame_n", "kp_xy", "kp_octave", "kp_angle", "kp_un", "kp_uright", "kp_depth", "bounds", "frame_mappoint",
            "frame_outlier", "kp_begin")


def build(kps, counts, camera, dist, rows, cols, mode, depth=None, depth_factor=1.0, out=None):
    """The whole step on kps (F, cap) KP_DTYPE: updates the arrays of `out` that are present (rows from the clamped count up
    are left as they are; STEREO leaves kp_uright / kp_depth alone) and returns it."""
    F, cap = kps.shape
    out = {} if out is None else out
    has = lambda k: out.get(k) is not None   # noqa: E731
    for f in range(F):
        n = min(max(int(counts[f]), 0), cap)
        if has("frame_n"):
            out["frame_n"][f] = n
        if has("bounds"):
            out["bounds"][f] = image_bounds(rows, cols, camera[f], dist[f])
        k = kps[f, :n]
        xy = np.stack([k["x"], k["y"]], 1).astype(f32).reshape(n, 2)
        un = keypoint_xy(camera[f], dist[f], xy)
        if has("kp_xy"):
            out["kp_xy"][f, :n] = un
        if has("kp_octave"):
            out["kp_octave"][f, :n] = k["octave"]
        if has("kp_angle"):
            out["kp_angle"][f, :n] = k["angle"]
        if has("kp_un"):
            ku = k.copy()
            ku["x"], ku["y"] = un[:, 0], un[:, 1]
            out["kp_un"][f, :n] = ku.view(np.int32).reshape(n, 7)
        if mode != STEREO:
            if mode == RGBD:
                ur, dp = stereo_from_rgbd(xy, un, depth[f], depth_factor, camera[f][4])
            else:
                ur, dp = np.full(n, -1, f32), np.full(n, -1, f32)
            if has("kp_uright"):
                out["kp_uright"][f, :n] = ur
            if has("kp_depth"):
                out["kp_depth"][f, :n] = dp
        if has("frame_mappoint"):
            out["frame_mappoint"][f, :n] = -1
        if has("frame_outlier"):
            out["frame_outlier"][f, :n] = 0
    if has("kp_begin"):
        out["kp_begin"][:] = np.arange(F + 1) * cap
    return out
