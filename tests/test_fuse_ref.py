"""tests/fuse_ref.py (the restatement the Fuse / Sim3 GPU tests compare against) pinned by hand-built
known-answer cases, one per gate sitting exactly on its boundary, and make_fuse_batch shown not to be
vacuous under the reference alone at the GPU tests' shapes.  Also the host-side validation of the Python
wrappers and a compile / link check of the C++ ones.  CPU only.

Camera of the hand-built cases: identity pose, fx = fy = 512, cx = 320, cy = 240, bf = 40, image
[0, 640) x [0, 480) (grid cells 10 x 10 px, boundaries at 10 c + 5), so every projection below is exact
in float32."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fuse_ref
from orb_slam2_refactored_amd import matcher as M
from orb_slam2_refactored_amd.synth import make_fuse_batch

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
SF = np.array([1.2 ** i for i in range(8)], F32)


def kat(points, kps, inv_sigma2=None, th=3.0, chi2=True):
    """points: (Xw, normal, maxDistance_); kps: (x, y, octave, uright, descriptor byte)."""
    P, K = len(points), len(kps)
    return {
        "kp_begin": np.array([0, K], np.int32), "mp_begin": np.array([0, P], np.int32),
        "kp_xy": np.array([[k[0], k[1]] for k in kps], F32).reshape(K, 2),
        "kp_octave": np.array([k[2] for k in kps], np.int32), "kp_uright": np.array([k[3] for k in kps], F32),
        "kp_desc": np.array([[k[4]] * 32 for k in kps], np.uint8).reshape(K, 32),
        "bounds": np.array([[0, 640, 0, 480]], F32),
        "pose": np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F32),
        "camera": np.array([[512, 512, 320, 240, 40]], F32),
        "mp_valid": np.ones(P, np.uint8), "mp_xw": np.array([p[0] for p in points], F32).reshape(P, 3),
        "mp_normal": np.array([p[1] for p in points], F32).reshape(P, 3),
        "mp_max_min": np.array([[p[2], p[2] / 3.0] for p in points], F32).reshape(P, 2),
        "mp_desc": np.zeros((P, 32), np.uint8),
        "scale_factors": SF, "inv_sigma2": np.ones(8, F32) if inv_sigma2 is None else np.asarray(inv_sigma2, F32),
        "log_scale_factor": float(F32(np.log(np.float64(F32(1.2))))), "th": th, "chi2_gate": chi2,
    }


Z = (0.0, 0.0, 1.0)                # a normal along the viewing ray of a point on the optical axis
CENTRE = ((0.0, 0.0, 4.0), Z, 4.0)   # projects to (320, 240), ur = 310, dist3D = 4 = maxDistance_: scale 0


def _causes(b):
    st = {}
    out = fuse_ref.fuse(b, st)
    return out, {k: v for k, v in st["causes"].items() if v}


def test_depth_gate_is_strict():
    kp = [(320, 240, 0, -1, 0)]
    # z == 0 and z == -0 pass `Xc.z < 0` and die on the image test (u, v are inf / nan)
    (bi, bd, nf), c = _causes(kat([((1.0, 0.0, 0.0), Z, 4.0), ((0.0, 0.0, -0.0), Z, 4.0)], kp))
    assert c == {"image": 2} and (bi == -1).all() and (bd == 256).all() and nf[0] == 0
    _, c = _causes(kat([((0.0, 0.0, -2.0 ** -20), Z, 4.0)], kp))
    assert c == {"depth": 1}


def test_image_bounds_are_half_open():
    # (keypoints right of x = 635 fall off the grid: cell 64; so a window of 6 px and no chi2 gate)
    kp = [(1, 240, 0, -1, 0), (634, 240, 0, -1, 0)]
    # z = 1: u = 320 + 512 x exactly; the normal along the ray; maxDistance_ = 1 < dist3D = 1.18 < 1.2: scale 0
    for x, cause, idx in ((-0.625, {}, 0),                      # u = 0 = minx is inside
                          (0.625, {"image": 1}, -1),            # u = 640 = maxx is outside
                          (0.625 - 2.0 ** -20, {}, 1)):         # the float below it is inside
        (bi, _, _), c = _causes(kat([((x, 0.0, 1.0), (x, 0.0, 1.0), 1.0)], kp, th=6.0, chi2=False))
        assert c == cause and bi[0] == idx, x


def test_viewing_angle_boundary():
    kp = [(320, 240, 0, -1, 0)]
    # PO = (0, 0, 4), dist3D = 4: dot = 4 * nz against 0.5 * 4
    (bi, _, nf), c = _causes(kat([((0.0, 0.0, 4.0), (0.8, 0.0, 0.5), 4.0)], kp))
    assert c == {} and bi[0] == 0 and nf[0] == 1          # dot == 0.5 * dist is not `<`
    below = float(np.nextafter(F32(0.5), F32(0)))
    _, c = _causes(kat([((0.0, 0.0, 4.0), (0.8, 0.0, below), 4.0)], kp))
    assert c == {"angle": 1}


def test_chi2_thresholds_compare_in_double():
    up, dn = (lambda x: float(np.nextafter(F32(x), F32(np.inf)))), (lambda x: float(np.nextafter(F32(x), F32(0))))
    mono, stereo = [(319, 240, 0, -1, 0)], [(319, 240, 0, 310, 0)]   # dx = 1, dy = 0 (dz = 0): NormSq = 1
    for kps, s2, fused in ((mono, 5.99, True),          # float32(5.99) = 5.98999977 < 5.99
                           (mono, up(5.99), False),
                           (stereo, 7.8, False),        # float32(7.8) = 7.80000019 > 7.8: a float compare would pass
                           (stereo, dn(7.8), True)):
        (bi, bd, nf), c = _causes(kat([CENTRE], kps, inv_sigma2=[s2] * 8))
        assert (bi[0] == 0 and bd[0] == 0 and nf[0] == 1) if fused else (bi[0] == -1 and bd[0] == 256 and nf[0] == 0), s2
        assert fused or list(c) == ["chi2_stereo" if kps is stereo else "chi2_mono"]
    # the Sim3 overload has no chi2 gate
    (bi, _, _), c = _causes(kat([CENTRE], mono, inv_sigma2=[100.0] * 8, chi2=False))
    assert bi[0] == 0 and c == {}


def test_uright_zero_is_a_stereo_keypoint():
    # on the projection itself: the monocular gate would pass it, the stereo gate sees dz = 310
    (bi, bd, _), c = _causes(kat([CENTRE], [(320, 240, 0, 0.0, 0)]))
    assert bi[0] == -1 and bd[0] == 256 and c == {"chi2_stereo": 1}
    (bi, _, _), _ = _causes(kat([CENTRE], [(320, 240, 0, -1.0, 0)]))
    assert bi[0] == 0


def test_tie_keeps_the_lower_scan_position():
    # u = 325: keypoint 0 at x = 326 lies in column 33, keypoint 1 at x = 324 in column 32 (scanned first)
    p = ((5.0 * 4.0 / 512.0, 0.0, 4.0), Z, float(np.sqrt(16 + (20.0 / 512) ** 2)))
    b = kat([p], [(326, 240, 0, -1, 0), (324, 240, 0, -1, 0)])
    st = {}
    bi, bd, nf = fuse_ref.fuse(b, st)
    assert bi[0] == 1 and bd[0] == 0 and st["scan_order_ties"] == 1
    km, nm = fuse_ref.search_by_projection_sim3(b)
    assert km.tolist() == [-1, 0] and nm[0] == 1
    # level window [ps - 1, ps] and TH_LOW
    b = kat([CENTRE], [(320, 240, 1, -1, 0), (321, 240, 0, -1, 0x0F)])   # octave 1 > ps = 0; 128 bits away
    (bi, bd, _), c = _causes(b)
    assert bi[0] == -1 and bd[0] == 128 and c == {"level": 1, "th_low": 1}


def test_sim3_claims_in_list_order():
    # two points on one keypoint: the first takes it, the second falls back to the farther descriptor
    b = kat([CENTRE, CENTRE], [(320, 240, 0, -1, 0), (321, 240, 0, -1, 1)], chi2=False)
    km, nm = fuse_ref.search_by_projection_sim3(b)
    assert km.tolist() == [0, 1] and nm[0] == 2
    km, nm = fuse_ref.search_by_projection_sim3(dict(b, kp_claimed=np.array([1, 0], np.uint8)))
    assert km.tolist() == [-1, 0] and nm[0] == 1


GPU_N_KP = [600, 400, 900, 64, 600, 0]
GPU_N_MP = [300, 500, 200, 40, 0, 100]


def gpu_batch(th, chi2):
    """The batch tests/test_fuse_gpu.py runs for (th, chi2_gate); the seeds are fixed."""
    return make_fuse_batch(100 + int(th) * 10 + int(chi2), n_items=6, n_kp=GPU_N_KP, n_mp=GPU_N_MP, th=th, chi2_gate=chi2)


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("chi2", [True, False])
def test_generator_is_not_vacuous(th, chi2):
    """The batches of tests/test_fuse_gpu.py under the reference alone: every rejection cause at least 5
    times, at least 30 % of the mp_valid points of every item with keypoints and points fused, at least
    3 ties that scan order decides against index order, both kinds of uright."""
    b = gpu_batch(th, chi2)
    st = {}
    fuse_ref.fuse(b, st)
    want = ["depth", "image", "distance", "angle", "level", "th_low"] + (["chi2_mono", "chi2_stereo"] if chi2 else [])
    for cause in want:
        assert st["causes"][cause] >= 5, (cause, st["causes"])
    assert st["scan_order_ties"] >= 3
    checked = 0
    for (valid, _searched, fused), n_kp in zip(st["per_item"], GPU_N_KP):
        if n_kp and valid:
            assert fused >= 0.3 * valid, (valid, fused)
            checked += 1
    assert checked == 4
    assert (b["kp_uright"] >= 0).sum() > 50 and (b["kp_uright"] < 0).sum() > 50 and (b["kp_uright"] == 0).sum() >= 1


# ---------------------------------------------------------------- Python wrapper validation (no GPU)
def _small():
    return make_fuse_batch(1, n_items=1, n_kp=6, n_mp=3)


@pytest.mark.parametrize("key,bad", [("mp_normal", np.zeros((3, 2), np.float32)), ("camera", np.zeros((1, 4), np.float32)),
                                     ("kp_uright", np.zeros(5, np.float32)), ("mp_desc", np.zeros((2, 32), np.uint8))])
def test_fuse_refuses_short_arrays(key, bad):
    b = _small()
    b[key] = bad
    with pytest.raises(ValueError, match=key):
        M.Fuse(b)
    if key != "kp_uright":
        with pytest.raises(ValueError, match=key):
            M.SearchByProjectionSim3(b)


def test_fuse_refuses_missing_arrays():
    for key in ("mp_normal", "kp_uright", "inv_sigma2"):
        b = _small()
        b[key] = None
        with pytest.raises(ValueError, match=key):
            M.Fuse(b)
    b = _small()
    b["mp_normal"] = None
    with pytest.raises(ValueError, match="mp_normal"):
        M.SearchByProjectionSim3(b)
    b = _small()
    b["kp_claimed"] = np.zeros(5, np.uint8)
    with pytest.raises(ValueError, match="kp_claimed"):
        M.SearchByProjectionSim3(b)


def test_device_wrappers_refuse_wrong_dtype_and_rows():
    import torch
    b = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) and k not in ("scale_factors", "inv_sigma2") else v)
         for k, v in _small().items()}
    for fn in (M.fuse_device, M.search_by_projection_sim3_device):
        with pytest.raises(ValueError, match="mp_normal"):
            fn(dict(b, mp_normal=b["mp_normal"].double()))
        with pytest.raises(ValueError, match="mp_normal"):
            fn(dict(b, mp_normal=b["mp_normal"][:2].contiguous()))
        with pytest.raises(ValueError, match="mp_normal"):
            fn(dict(b, mp_normal=None))
    with pytest.raises(ValueError, match="kp_claimed"):
        M.search_by_projection_sim3_device(dict(b, kp_claimed=b["kp_claimed"].int()))


# ---------------------------------------------------------------- C++ wrappers
def _compile_wrapper_use(tmp_path):
    src = ROOT / "tests" / "native" / "fuse_wrapper_use.cpp"
    obj = tmp_path / "f.o"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o", str(obj)],
                   check=True)
    return obj


def test_fuse_cpp_wrapper_compiles(tmp_path):
    _compile_wrapper_use(tmp_path)


def test_fuse_cpp_wrapper_links_and_runs(tmp_path):
    lib = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    if not lib.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    obj = _compile_wrapper_use(tmp_path)
    main = tmp_path / "main.cpp"
    main.write_text("int use_fuse_empty(); int main() { return use_fuse_empty(); }\n")
    exe = tmp_path / "f"
    subprocess.run(["g++", str(main), str(obj), "-o", str(exe), f"-L{lib.parent}", "-lorbslam2_amd",
                    f"-Wl,-rpath,{lib.parent}"], check=True)
    # empty batches return before any device call: both host entries answer ORB_OK without a GPU
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
