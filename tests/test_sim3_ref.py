"""tests/sim3_ref.py (the restatement the SearchBySim3 / ComputeDistinctiveDescriptors GPU tests compare
against) pinned by hand-built known-answer cases, one per gate sitting exactly on its boundary, and
make_sim3_batch shown not to be vacuous under the reference alone at the GPU tests' shapes.  Also the
host-side validation of the Python wrappers and a compile / link check of the C++ ones.  CPU only.

Cameras of the hand-built cases: identity poses, fx = fy = 512, cx = 320, cy = 240, image [0, 640) x
[0, 480) (grid cells 10 x 10 px, boundaries at 10 c + 5), S12 = (I, 0, s) unless a case says otherwise, so
every projection below is exact in float32."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_ref
from orb_slam2_refactored_amd import matcher as M
from orb_slam2_refactored_amd.synth import make_observation_sets, make_sim3_batch

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
SF = np.array([1.2 ** i for i in range(8)], F32)


def bits(n, at=0):
    """A descriptor with the n bits [at, at + n) set."""
    d = np.zeros(256, np.uint8)
    d[at:at + n] = 1
    return np.packbits(d, bitorder="little")


def _desc(v):
    return np.full(32, v, np.uint8) if np.isscalar(v) else np.asarray(v, np.uint8)


def kat(side1, side2, s=1.0, t12=(0.0, 0.0, 0.0), th=7.5):
    """side: one (point, keypoint) per slot; point = None (no map point, or matched on entry) or (Xw,
    maxDistance_, minDistance_, descriptor); keypoint = (x, y, octave, descriptor); descriptor = one byte
    value for all 32, or the 32 bytes."""
    b = {"s12": np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, *t12, s]], F32), "scale_factors": SF,
         "log_scale_factor": float(F32(np.log(np.float64(F32(1.2))))), "th": th}
    for tag, side in (("1", side1), ("2", side2)):
        n = len(side)
        pts = [p if p is not None else ((0, 0, 0), 0, 0, 0) for p, _ in side]
        b[f"kp{tag}_begin"] = np.array([0, n], np.int32)
        b[f"kp{tag}_xy"] = np.array([[k[0], k[1]] for _, k in side], F32).reshape(n, 2)
        b[f"kp{tag}_octave"] = np.array([k[2] for _, k in side], np.int32)
        b[f"kp{tag}_desc"] = np.array([_desc(k[3]) for _, k in side], np.uint8).reshape(n, 32)
        b[f"mp{tag}_valid"] = np.array([p is not None for p, _ in side], np.uint8)
        b[f"mp{tag}_xw"] = np.array([p[0] for p in pts], F32).reshape(n, 3)
        b[f"mp{tag}_max_min"] = np.array([[p[1], p[2]] for p in pts], F32).reshape(n, 2)
        b[f"mp{tag}_desc"] = np.array([_desc(p[3]) for p in pts], np.uint8).reshape(n, 32)
        b["bounds" + tag] = np.array([[0, 640, 0, 480]], F32)
        b["pose" + tag] = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F32)
        b["camera" + tag] = np.array([[512, 512, 320, 240]], F32)
    return b


def pt(X, maxd=None, mind=0.01, desc=0):
    """A map point; maxDistance_ defaults to |X| (predicted scale 0 at s = 1)."""
    return (X, float(np.sqrt(np.sum(np.square(np.asarray(X, np.float64))))) if maxd is None else maxd, mind, desc)


CENTRE = pt((0.0, 0.0, 4.0))          # projects to (320, 240), dist3D = 4 = maxDistance_: scale 0, radius 7.5
KP_C = (320, 240, 0, 0)               # the keypoint on that projection


def run(b):
    st = {}
    out = sim3_ref.search_by_sim3(b, st)
    return out, {k: v for k, v in st["causes"].items() if v}, st


def one_to_two(point, kps2, **kw):
    """Keyframe 1 holds `point` alone; keyframe 2 holds keypoints without map points."""
    return kat([(point, (5, 5, 0, 0xFF))], [(None, k) for k in kps2], **kw)


def test_depth_gate_is_strict():
    # z == 0 and z == -0 pass `Xc2.z < 0` and die on the image test (u, v are inf / nan)
    for X in ((1.0, 0.0, 0.0), (0.0, 0.0, -0.0)):
        (m12, m1, m2, nf), c, _ = run(one_to_two(pt(X, 4.0), [KP_C]))
        assert c == {"invalid": 1, "image": 1} and m1[0] == -1 and nf[0] == 0, X
    _, c, _ = run(one_to_two(pt((0.0, 0.0, -2.0 ** -20), 4.0), [KP_C]))
    assert c == {"invalid": 1, "depth": 1}


def test_image_bounds_are_half_open():
    # z = 1: u = 320 + 512 x exactly; maxDistance_ = 1 < dist3D = 1.18 < 1.2: scale 0, radius 7.5
    kps = [(1, 240, 0, 0), (634, 240, 0, 0)]   # (keypoints right of x = 635 fall off the grid: cell 64)
    for x, cause, idx in ((-0.625, {}, 0),                      # u = 0 = minx is inside
                          (0.625, {"image": 1}, -1),            # u = 640 = maxx is outside
                          (0.625 - 2.0 ** -20, {}, 1)):         # the float below it is inside
        (_, m1, _, _), c, _ = run(one_to_two(pt((x, 0.0, 1.0), 1.0), kps))
        c.pop("invalid")
        assert c == cause and m1[0] == idx, x


def test_distance_gate_boundaries():
    # 0.8f * 5 == 4 and 1.2f * 5 == 6 exactly in float32
    assert F32(0.8) * F32(5) == F32(4) and F32(1.2) * F32(5) == F32(6)
    kp7 = [(320, 240, 7, 0)]   # maxDistance_ = 40 at dist 4: the predicted scale clamps to 7
    (_, m1, _, _), c, _ = run(one_to_two(pt((0.0, 0.0, 4.0), 40.0, 5.0), kp7))
    assert "distance" not in c and m1[0] == 0            # dist3D == 0.8f * minDistance_ is not `<`
    below = float(np.nextafter(F32(4), F32(0)))
    (_, m1, _, _), c, _ = run(one_to_two(pt((0.0, 0.0, below), 40.0, 5.0), kp7))
    assert c.get("distance") == 1 and m1[0] == -1
    (_, m1, _, _), c, _ = run(one_to_two(pt((0.0, 0.0, 6.0), 5.0, 0.01), [KP_C]))
    assert "distance" not in c and m1[0] == 0            # dist3D == 1.2f * maxDistance_ is not `>`
    above = float(np.nextafter(F32(6), F32(np.inf)))
    (_, m1, _, _), c, _ = run(one_to_two(pt((0.0, 0.0, above), 5.0, 0.01), [KP_C]))
    assert c.get("distance") == 1 and m1[0] == -1


def test_distance_is_the_norm_of_the_mapped_point():
    # Xw = (0, 0, 8) in camera 1, s = 2: Xc2 = (0, 0, 4); the gate and PredictScale see 4, not 8
    (_, m1, _, _), c, _ = run(one_to_two(pt((0.0, 0.0, 8.0), 4.0, 4.5), [KP_C], s=2.0))
    assert "distance" not in c and m1[0] == 0            # 0.8f * 4.5 = 3.6 <= 4 <= 4.8; dist 8 would fail
    # and no viewing-angle or chi2 gate exists: nothing else can refuse the centre point
    assert c == {"invalid": 1}


def test_th_high_is_100():
    (_, m1, _, _), c, _ = run(one_to_two(CENTRE, [(320, 240, 0, bits(100))]))
    assert m1[0] == 0 and "th_high" not in c
    (_, m1, _, _), c, _ = run(one_to_two(CENTRE, [(320, 240, 0, bits(101))]))
    assert m1[0] == -1 and c.get("th_high") == 1


def test_level_window():
    # maxDistance_ = 4 * 1.2^2 * 0.99 at dist 4: predicted scale 2, levels [1, 2]
    p = pt((0.0, 0.0, 4.0), 4.0 * 1.44 * 0.99)
    (_, m1, _, _), c, _ = run(one_to_two(p, [(320, 240, 3, 0), (321, 240, 0, 0)]))   # ps + 1 and ps - 2
    assert m1[0] == -1 and c.get("level") == 2 and "th_high" not in c
    (_, m1, _, _), c, _ = run(one_to_two(p, [(320, 240, 3, 0), (321, 240, 0, 0), (322, 240, 1, 3), (323, 240, 2, 1)]))
    assert m1[0] == 3 and c.get("level") == 2


def test_tie_keeps_the_lower_scan_position():
    # u = 325: keypoint 0 at x = 326 lies in column 33, keypoint 1 at x = 324 in column 32 (scanned first)
    p = pt((5.0 * 4.0 / 512.0, 0.0, 4.0))
    (_, m1, _, _), _, st = run(one_to_two(p, [(326, 240, 0, 0), (324, 240, 0, 0)]))
    assert m1[0] == 1 and st["scan_order_ties"] == 1


def test_one_way_match_is_not_agreed():
    # 1 -> 2: slot 0 of keyframe 1 finds keypoint 0 of keyframe 2.  2 -> 1: that slot's own map point
    # (descriptor 0xFF) prefers keypoint 1 of keyframe 1
    b = kat([(CENTRE, (320, 240, 0, 0x0F)), (None, (321, 240, 0, 0xFF))], [(pt((0.0, 0.0, 4.0), desc=0xFF), KP_C)])
    (m12, m1, m2, nf), _, st = run(b)
    assert m1.tolist() == [0, -1] and m2.tolist() == [1] and m12.tolist() == [-1, -1] and nf[0] == 0
    assert st["one_way_only"] == 1
    # with the partner agreeing
    b = kat([(CENTRE, (320, 240, 0, 0xFF)), (None, (321, 240, 0, 0x0F))], [(pt((0.0, 0.0, 4.0), desc=0xFF), KP_C)])
    (m12, m1, m2, nf), _, _ = run(b)
    assert m12.tolist() == [0, -1] and m2.tolist() == [0] and nf[0] == 1


def test_already_matched_slots_do_not_search():
    full = kat([(CENTRE, KP_C)], [(CENTRE, KP_C)])
    (m12, _, _, nf), c, _ = run(full)
    assert m12.tolist() == [0] and nf[0] == 1 and c == {}
    for tag in "12":   # mp_valid = 0: matches12[i1] set on entry / alreadyMatched2[i2]
        b = dict(full)
        b[f"mp{tag}_valid"] = np.zeros(1, np.uint8)
        (m12, m1, m2, nf), c, _ = run(b)
        assert c == {"invalid": 1} and nf[0] == 0 and m12[0] == -1
        assert (m1[0], m2[0]) == ((-1, 0) if tag == "1" else (0, -1))


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_inverse_composed_with_map_is_exact_on_powers_of_two(s):
    S = [1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0, -2.0, 0.5, s]
    x = [F32(0.25), F32(-0.5), F32(4.0)]
    y = sim3_ref.sim3_map(S, x)
    assert [float(v) for v in y] == [s * 0.25 + 1.0, s * -0.5 - 2.0, s * 4.0 + 0.5]
    inv = sim3_ref.sim3_inverse(S)
    assert [float(v) for v in inv[9:]] == [-1.0 / s, 2.0 / s, -0.5 / s, 1.0 / s]
    assert [float(v) for v in sim3_ref.sim3_map(inv, y)] == [0.25, -0.5, 4.0]
    # the search across the scale: Xw1 = (0, 0, 4 s) lands on (0, 0, 4) in camera 2 and back
    b = kat([(pt((0.0, 0.0, 4.0 * s), 4.0), KP_C)], [(pt((0.0, 0.0, 4.0), 4.0 * s), KP_C)], s=s)
    (m12, m1, m2, nf), c, _ = run(b)
    assert c == {} and m12.tolist() == [0] and m2.tolist() == [0] and nf[0] == 1


def boundary_cases():
    """The hand-built cases above as batches, for tests/test_sim3_gpu.py."""
    below4, above6 = float(np.nextafter(F32(4), F32(0))), float(np.nextafter(F32(6), F32(np.inf)))
    p2 = pt((0.0, 0.0, 4.0), 4.0 * 1.44 * 0.99)
    edge = [pt((1.0, 0.0, 0.0), 4.0), pt((0.0, 0.0, -0.0), 4.0), pt((0.0, 0.0, -2.0 ** -20), 4.0),
            pt((-0.625, 0.0, 1.0), 1.0), pt((0.625, 0.0, 1.0), 1.0), pt((0.625 - 2.0 ** -20, 0.0, 1.0), 1.0)]
    cases = [kat([(p, (5, 5, 0, 0xFF)) for p in edge], [(None, KP_C), (None, (1, 240, 0, 0)), (None, (634, 240, 0, 0))])]
    for z, maxd, mind, kp in ((4.0, 40.0, 5.0, (320, 240, 7, 0)), (below4, 40.0, 5.0, (320, 240, 7, 0)),
                              (6.0, 5.0, 0.01, KP_C), (above6, 5.0, 0.01, KP_C)):
        cases.append(one_to_two(pt((0.0, 0.0, z), maxd, mind), [kp]))
    cases += [one_to_two(pt((0.0, 0.0, 8.0), 4.0, 4.5), [KP_C], s=2.0),
              one_to_two(CENTRE, [(320, 240, 0, bits(100))]), one_to_two(CENTRE, [(320, 240, 0, bits(101))]),
              one_to_two(p2, [(320, 240, 3, 0), (321, 240, 0, 0)]),
              one_to_two(p2, [(320, 240, 3, 0), (321, 240, 0, 0), (322, 240, 1, 3), (323, 240, 2, 1)]),
              one_to_two(pt((5.0 * 4.0 / 512.0, 0.0, 4.0)), [(326, 240, 0, 0), (324, 240, 0, 0)]),
              kat([(CENTRE, (320, 240, 0, 0x0F)), (None, (321, 240, 0, 0xFF))], [(pt((0.0, 0.0, 4.0), desc=0xFF), KP_C)]),
              kat([(CENTRE, (320, 240, 0, 0xFF)), (None, (321, 240, 0, 0x0F))], [(pt((0.0, 0.0, 4.0), desc=0xFF), KP_C)])]
    full = kat([(CENTRE, KP_C)], [(CENTRE, KP_C)])
    cases += [full, dict(full, mp1_valid=np.zeros(1, np.uint8)), dict(full, mp2_valid=np.zeros(1, np.uint8))]
    for s in (0.5, 1.0, 2.0):
        cases.append(kat([(pt((0.0, 0.0, 4.0 * s), 4.0), KP_C)], [(pt((0.0, 0.0, 4.0), 4.0 * s), KP_C)], s=s))
    return cases


# ---------------------------------------------------------------- ComputeDistinctiveDescriptors
def sets(*points):
    rows = [r for p in points for r in p]
    return (np.array(rows, np.uint8).reshape(len(rows), 32),
            np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int32))


# rows bits(k): the distance between two of them is |k_i - k_j|
FOUR = [bits(0), bits(10), bits(16), bits(40)]
# rows 2 and 5 are one descriptor; every other row differs from it in its own 20 bits
C7 = bits(100, 150)
TIE = [C7 ^ bits(20, 0), C7 ^ bits(20, 20), C7, C7 ^ bits(20, 40), C7 ^ bits(20, 60), C7, C7 ^ bits(20, 80)]


def distinct_cases():
    """(desc, begin, best, best_median) worked out by hand."""
    return [
        (*sets(FOUR[:1]), [0], [0]),                 # N = 1, 2: the median position is the self-distance
        (*sets(FOUR[2:4]), [0], [0]),
        (*sets(FOUR[:3]), [1], [6]),                 # N = 3, position 1: medians 10, 6, 6 -> the lower row of the tie
        (*sets(FOUR), [1], [6]),                     # N = 4, position 1: medians 10, 6, 6, 24
        (*sets([bits(77)] * 5), [0], [0]),           # all rows equal
        (*sets(TIE), [2], [20]),                     # N = 7, position 3: rows 2 and 5 at 20, the others at 40
        (*sets(FOUR[:3], [], FOUR), [1, -1, 1], [6, -1, 6]),   # an empty point between two full ones
    ]


def test_distinctive_descriptors_by_hand():
    for desc, begin, best, med in distinct_cases():
        gb, gm = sim3_ref.distinctive_descriptors(desc, begin)
        assert gb.tolist() == best and gm.tolist() == med


GPU_N_KP1 = [600, 64, 900, 0, 300, 40]
GPU_N_KP2 = [400, 900, 64, 300, 0, 40]
GPU_N_OBS = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 200, 1024]


def gpu_batch(th):
    """The batch tests/test_sim3_gpu.py runs at `th`; the seeds are fixed."""
    return make_sim3_batch(300 + int(th), n_pairs=6, n_kp1=GPU_N_KP1, n_kp2=GPU_N_KP2, th=th)


def gpu_observation_sets():
    return make_observation_sets(5, len(GPU_N_OBS), GPU_N_OBS)


@pytest.mark.parametrize("th", [7.5, 3.0])
def test_generator_is_not_vacuous(th):
    """The batches of tests/test_sim3_gpu.py under the reference alone: every pair with keypoints on both
    sides finds matches, every rejection cause occurs, some matches are one-way only, scan order decides
    at least one tie against index order, and the scales differ from 1."""
    b = gpu_batch(th)
    st = {}
    _, _, _, nf = sim3_ref.search_by_sim3(b, st)
    for p, (n1, n2) in enumerate(zip(GPU_N_KP1, GPU_N_KP2)):
        assert (nf[p] > 0) == (n1 > 0 and n2 > 0), (p, nf)
    for cause in ("invalid", "depth", "image", "distance", "level", "th_high"):
        assert st["causes"][cause] > 0, (cause, st["causes"])
    assert st["one_way_only"] > 0 and st["scan_order_ties"] >= 1
    assert (np.abs(b["s12"][:, 12] - 1) > 0.04).all()


def test_observation_sets_are_not_vacuous():
    o = gpu_observation_sets()
    assert np.diff(o["begin"]).tolist() == GPU_N_OBS
    best, med = sim3_ref.distinctive_descriptors(o["desc"], o["begin"])
    assert best[0] == -1 and (best[1:] >= 0).all() and (best[1:] < np.array(GPU_N_OBS[1:])).all()
    assert (best[3:] > 0).any() and (med[5:] > 0).all()   # (a small point may hold a repeated row: median 0)


# ---------------------------------------------------------------- Python wrapper validation (no GPU)
def _small():
    return make_sim3_batch(1, n_pairs=1, n_kp1=6, n_kp2=5)


@pytest.mark.parametrize("key,bad", [("mp1_xw", np.zeros((6, 2), np.float32)), ("camera2", np.zeros((1, 3), np.float32)),
                                     ("s12", np.zeros((1, 12), np.float32)), ("mp2_desc", np.zeros((4, 32), np.uint8)),
                                     ("kp2_octave", np.zeros(4, np.int32)), ("kp2_begin", np.zeros(1, np.int32))])
def test_sim3_refuses_short_arrays(key, bad):
    b = _small()
    b[key] = bad
    with pytest.raises(ValueError, match=key):
        M.SearchBySim3(b)


def test_sim3_refuses_missing_arrays():
    for key in ("mp1_valid", "pose2", "s12", "kp1_begin"):
        b = _small()
        b[key] = None
        with pytest.raises(ValueError, match=key):
            M.SearchBySim3(b)


def test_sim3_device_wrapper_refuses_wrong_dtype_and_rows():
    import torch
    b = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) and k != "scale_factors" else v) for k, v in _small().items()}
    with pytest.raises(ValueError, match="mp2_xw"):
        M.search_by_sim3_device(dict(b, mp2_xw=b["mp2_xw"].double()))
    with pytest.raises(ValueError, match="mp2_xw"):
        M.search_by_sim3_device(dict(b, mp2_xw=b["mp2_xw"][:2].contiguous()))
    with pytest.raises(ValueError, match="mp2_xw"):
        M.search_by_sim3_device(dict(b, mp2_xw=None))
    with pytest.raises(ValueError, match="s12"):
        M.search_by_sim3_device(dict(b, s12=b["s12"][:, :12].contiguous()))
    with pytest.raises(ValueError, match="mp1_valid"):
        M.search_by_sim3_device(dict(b, mp1_valid=b["mp1_valid"].int()))


def test_distinct_wrappers_refuse_bad_arrays():
    import torch
    desc, begin = sets(FOUR, FOUR[:2])
    with pytest.raises(ValueError, match="desc"):
        M.ComputeDistinctiveDescriptors(desc[:5], begin)
    with pytest.raises(ValueError, match="desc"):
        M.ComputeDistinctiveDescriptors(None, begin)
    with pytest.raises(ValueError, match="begin"):
        M.ComputeDistinctiveDescriptors(desc, None)
    with pytest.raises(ValueError, match="out_desc"):
        M.ComputeDistinctiveDescriptors(desc, begin, out_desc=np.zeros((1, 32), np.uint8))
    with pytest.raises(ValueError, match="out_desc"):
        M.ComputeDistinctiveDescriptors(desc, begin, out_desc=np.zeros((2, 32), np.int32))
    td, tb = torch.from_numpy(desc), torch.from_numpy(begin)
    with pytest.raises(ValueError, match="desc"):
        M.compute_distinctive_descriptors_device(td.int(), tb)
    with pytest.raises(ValueError, match="begin"):
        M.compute_distinctive_descriptors_device(td, tb.long())
    with pytest.raises(ValueError, match="begin"):
        M.compute_distinctive_descriptors_device(td, None)
    with pytest.raises(ValueError, match="out_desc"):
        M.compute_distinctive_descriptors_device(td, tb, out_desc=torch.zeros((1, 32), dtype=torch.uint8))
    with pytest.raises(ValueError, match="best"):
        M.compute_distinctive_descriptors_device(td, tb, best=torch.zeros(1, dtype=torch.int32))


# ---------------------------------------------------------------- C++ wrappers
def _compile_wrapper_use(tmp_path):
    src = ROOT / "tests" / "native" / "sim3_wrapper_use.cpp"
    obj = tmp_path / "s.o"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o", str(obj)],
                   check=True)
    return obj


def test_sim3_cpp_wrapper_compiles(tmp_path):
    _compile_wrapper_use(tmp_path)


def test_sim3_cpp_wrapper_links_and_runs(tmp_path):
    lib = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    if not lib.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    obj = _compile_wrapper_use(tmp_path)
    main = tmp_path / "main.cpp"
    main.write_text("int use_sim3_empty(); int main() { return use_sim3_empty(); }\n")
    exe = tmp_path / "s"
    subprocess.run(["g++", str(main), str(obj), "-o", str(exe), f"-L{lib.parent}", "-lorbslam2_amd",
                    f"-Wl,-rpath,{lib.parent}"], check=True)
    # empty batches return, and an over-limit point is refused, before any device call: no GPU needed
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
