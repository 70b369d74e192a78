"""One build_device launch against the path it replaces, 256 frames x 2000 keypoints at 640 x 480 with uint16 depth (TUM1
camera): the resident form timed with device events over windows of 500 calls (the Python call included), and what the
parent commit needs for the same arrays: the keypoints copied back, the undistortion on one CPU thread
(orbfr_undistort_points, the same header at -O3), the depth lookup and the split in vectorised numpy, five uploads.  Both
give the same bits.  `--trace` only launches 100 times, for `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/time_frame.py --trace`.  DESIGN.md section 4, "Frame construction", records one run.

The keypoint dtype and the camera come from tests/frame_ref.py: run it from a checkout that has the tests."""
import sys, time
from pathlib import Path
import numpy as np
import torch
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import frame_ref as R
from orb_slam2_refactored_amd import frame as FR

F, cap, rows, cols = 256, 2000, 480, 640
rng = np.random.default_rng(0)
kps = np.zeros((F, cap), R.KP_DTYPE)
kps["x"], kps["y"] = rng.uniform(19, cols - 19, (F, cap)), rng.uniform(19, rows - 19, (F, cap))
kps["octave"], kps["angle"] = rng.integers(0, 8, (F, cap)), rng.uniform(0, 360, (F, cap))
counts = np.full(F, cap, np.int32)
camera, dist = np.stack([R.TUM1_CAMERA] * F), np.stack([R.TUM1_DIST] * F)
depth = rng.integers(0, 40000, (F, rows, cols)).astype(np.uint16)
factor = 1.0 / 5000.0
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
d_kps, d_counts, d_cam, d_dist, d_depth = up(kps.view(np.int32).reshape(F, cap, 7)), up(counts), up(camera), up(dist), up(depth)
out = FR.build_device(d_kps, d_counts, d_cam, d_dist, rows, cols, FR.RGBD, depth=d_depth, depth_factor=factor)
torch.cuda.synchronize()
if "--trace" in sys.argv:
    for _ in range(100):
        FR.build_device(d_kps, d_counts, d_cam, d_dist, rows, cols, FR.RGBD, depth=d_depth, depth_factor=factor, out=out)
    torch.cuda.synchronize()
    sys.exit(0)

def window(n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        FR.build_device(d_kps, d_counts, d_cam, d_dist, rows, cols, FR.RGBD, depth=d_depth, depth_factor=factor, out=out)
    b.record(); b.synchronize()
    return a.elapsed_time(b) / n

window(50)
res = sorted(window(500) for _ in range(7))
print("resident ms per call (7 windows of 500):", res)

# ---- what the parent commit needs for the same arrays
def parent():
    t = [time.perf_counter()]
    hk = d_kps.cpu().numpy(); t.append(time.perf_counter())                       # 1 keypoints back
    k = hk.view(R.KP_DTYPE).reshape(F, cap)
    xy = np.ascontiguousarray(np.stack([k["x"], k["y"]], -1).reshape(-1, 2))
    un = FR.undistort_points(camera[0], dist[0], xy).reshape(F, cap, 2); t.append(time.perf_counter())   # 2 undistortion in C
    u, v = xy[:, 0].astype(np.int32).reshape(F, cap), xy[:, 1].astype(np.int32).reshape(F, cap)
    d = depth[np.arange(F)[:, None], v, u].astype(np.float32) * np.float32(factor)
    ok = d > 0
    dp = np.where(ok, d, np.float32(-1)).astype(np.float32)
    with np.errstate(all="ignore"):
        ur = np.where(ok, un[..., 0] - np.float32(camera[0, 4]) / d, np.float32(-1)).astype(np.float32)
    octv, ang = np.ascontiguousarray(k["octave"]), np.ascontiguousarray(k["angle"]); t.append(time.perf_counter())   # 3 depth + split
    dev = [up(a) for a in (un, octv, ang, ur, dp)]
    torch.cuda.synchronize(); t.append(time.perf_counter())                      # 4 five uploads
    return np.diff(t) * 1e3, (un, ur, dp)

parent()
runs = np.array([parent()[0] for _ in range(5)])
print("parent ms [copy back, undistort (C, one thread), depth + split (numpy), upload x5]: median", np.median(runs, 0), "total", np.median(runs.sum(1)))
_, (un, ur, dp) = parent()
g = {k: v.cpu().numpy() for k, v in out.items()}
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
print("round trip equals resident:", same(g["kp_xy"], un), same(g["kp_uright"], ur), same(g["kp_depth"], dp))
