"""Argument validation of the observation edits: every ORB_EINVAL path of the host entries orbmm_add_keyframe_observations /
orbmm_fuse_apply / orbmm_grow_observations (all of them precede the first device call, so they run without a GPU), the
shared checks of the device entries, ValueError from the Python wrapper, and the C-ABI exports."""
import ctypes as C

import numpy as np
import pytest

import observe_cases as OC
from orb_slam2_refactored_amd import observations as OB
from orb_slam2_refactored_amd._lib import OrbError, OrbmmApply, OrbmmObserve, lib

EXPORTS = ("orbmm_add_keyframe_observations", "orbmm_fuse_apply", "orbmm_grow_observations")
KEYFRAME = ("kf_n", "kf_mappoint", "kf_uright")
POINT = ("mp_bad", "mp_nobs", "mp_obs_off", "mp_obs_kf", "mp_obs_idx")
REPLACE = ("mp_found", "mp_visible", "mp_replaced")


def last_error():
    return lib().orb_last_error().decode()


def poke(a, idx, v):
    a = a.copy()
    a[idx] = v
    return a


def refused(fn, text):
    with pytest.raises(OrbError, match="status -1") as e:
        fn()
    assert text in str(e.value), str(e.value)


def apply(t, c=None, mode=OB.APPLY_FUSE, state=None, **over):
    c = dict(OC.apply_of(c or OC.case("main")), **over)
    return OB.FuseApply(t, mode, c["item_kf"], c["mp_begin"], c["point"], c["best_idx"], state=state)


def test_the_c_abi_exports_are_present():
    so = C.CDLL(lib()._name)
    for name in EXPORTS:
        assert getattr(so, name) and getattr(so, name + "_device")


def test_null_arguments_sizes_and_modes_are_refused_by_both_forms():
    L = lib()
    one = C.c_void_p(8)   # never dereferenced: the checks below come first
    ap_ok = OrbmmApply(0, 1, 1, *([one] * 10))
    for rc in (L.orbmm_fuse_apply(None, C.byref(ap_ok), 0), L.orbmm_fuse_apply_device(None, C.byref(ap_ok), None),
               L.orbmm_add_keyframe_observations(None, 0, one, one, one, one, 0),
               L.orbmm_add_keyframe_observations_device(None, 0, one, one, one, one, None)):
        assert rc == -1 and "null observation tables" in last_error()
    ok = dict(n_keyframes=2, n_mappoints=2, kf_cap=4, n_obs=2)
    kf, pt = {k: one for k in KEYFRAME}, {k: one for k in POINT}
    for bad, text in ((dict(n_keyframes=-1), "negative sizes"), (dict(n_mappoints=-1), "negative sizes"), (dict(n_obs=-1), "negative sizes"),
                      (dict(kf_cap=0), "kf_cap must be at least 1"), (dict(n_keyframes=1 << 20, kf_cap=1 << 11), "2^31"),
                      (dict(n_obs=1 << 30), "2^31"), (pt, "null keyframe table"), (kf, "null map-point table")):
        o = OrbmmObserve(**dict(ok, **bad))
        for rc in (L.orbmm_add_keyframe_observations(C.byref(o), 0, one, one, one, one, 0),
                   L.orbmm_add_keyframe_observations_device(C.byref(o), 0, one, one, one, one, None),
                   L.orbmm_fuse_apply(C.byref(o), C.byref(ap_ok), 0), L.orbmm_fuse_apply_device(C.byref(o), C.byref(ap_ok), None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    o = OrbmmObserve(**dict(ok, **kf, **pt))                 # enough for the new keyframe's loop, not for Replace
    for rc in (L.orbmm_add_keyframe_observations(C.byref(o), 0, one, None, one, one, 0),
               L.orbmm_add_keyframe_observations_device(C.byref(o), 0, one, one, one, None, None)):
        assert rc == -1 and "null output" in last_error()
    for rc in (L.orbmm_fuse_apply(C.byref(o), C.byref(ap_ok), 0), L.orbmm_fuse_apply_device(C.byref(o), C.byref(ap_ok), None)):
        assert rc == -1 and "null map-point table" in last_error()
    o = OrbmmObserve(**dict(ok, **kf, **pt, **{k: one for k in REPLACE}))
    names = [f[0] for f in OrbmmApply._fields_]
    for bad, text in ((None, "null apply list"), (dict(mode=3), "unknown apply mode"), (dict(mode=-1), "unknown apply mode"),
                      (dict(n_items=-1), "negative sizes"), (dict(n_entries=-1), "negative sizes"), (dict(mp_begin=None), "null item array"),
                      (dict(item_kf=None), "null item array"), (dict(n_fused=None), "null item array"), (dict(point=None), "null entry array"),
                      (dict(best_idx=None), "null entry array"), (dict(mode=1, replace_point=None), "null replace_point"),
                      (dict(touched=None), "null output"), (dict(n_touched=None), "null output"), (dict(progress=None), "null output"),
                      (dict(status=None), "null output")):
        ap = None if bad is None else OrbmmApply(**dict(dict(zip(names, [0, 1, 1] + [one] * 10)), **bad))
        for rc in (L.orbmm_fuse_apply(C.byref(o), C.byref(ap) if ap else None, 0),
                   L.orbmm_fuse_apply_device(C.byref(o), C.byref(ap) if ap else None, None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    for args, text in (((-1, 0, one, one, one, 0, None, 0, one, one, one, one), "negative sizes"),
                       ((2, 2, one, one, one, -1, None, 4, one, one, one, one), "negative sizes"),
                       ((2, 2, one, one, one, 0, None, -4, one, one, one, one), "negative sizes"),
                       ((2, 1 << 30, one, one, one, 0, None, 1 << 30, one, one, one, one), "2^31"),
                       ((2, 2, None, one, one, 0, None, 4, one, one, one, one), "null observation array"),
                       ((2, 2, one, one, one, 0, None, 4, one, None, one, one), "null observation array"),
                       ((2, 2, one, one, one, 0, None, 4, one, one, one, None), "null observation array")):
        for rc in (L.orbmm_grow_observations(*args, 0), L.orbmm_grow_observations_device(*args, None)):
            assert rc == -1 and text in last_error(), (args, last_error())


def ascending_pair(t):
    """The entries of the first two live observations of a point that has two."""
    for p in range(OC.M):
        e = [e for e in range(t["mp_obs_off"][p], t["mp_obs_off"][p + 1]) if t["mp_obs_kf"][e] >= 0]
        if len(e) >= 2:
            return e[0], e[1]
    raise AssertionError


@pytest.mark.parametrize("key,idx,value,text", [
    ("mp_obs_off", 0, 1, "mp_obs: offsets must start at 0"), ("mp_obs_off", 100, 0, "mp_obs: offsets must not decrease"),
    ("mp_obs_off", -1, 1 << 20, "mp_obs: offsets end past n_obs"),
    ("mp_obs_kf", "live", OC.K, "mp_obs_kf entry outside"), ("mp_obs_kf", "live", -2, "mp_obs_kf entry outside"),
    ("mp_obs_idx", "live", OC.KF_CAP, "mp_obs_idx entry outside"), ("mp_obs_idx", "live", -1, "mp_obs_idx entry outside"),
    ("kf_mappoint", (11, 63), OC.M, "kf_mappoint entry outside"), ("kf_mappoint", (0, 0), -2, "kf_mappoint entry outside"),
    ("kf_n", 7, OC.KF_CAP + 1, "kf_n outside"), ("kf_n", 7, -1, "kf_n outside"),
])
def test_the_tables_are_validated_before_any_copy(key, idx, value, text):
    t = OC.tables(OC.case("main"))
    if idx == "live":
        idx = ascending_pair(t)[0]
    t[key] = poke(t[key], idx, value)
    refused(lambda: apply(t), text)
    refused(lambda: OB.AddKeyFrameObservations({k: t[k] for k in OB.NEW_KEYFRAME_KEYS}, 0), text)


def test_rows_that_do_not_ascend_and_duplicates_are_refused_and_the_slack_is_accepted():
    t = OC.tables(OC.case("main"))
    assert (t["mp_obs_kf"] == -1).any()                      # the slack itself passes (the walk below is refused later)
    e0, e1 = ascending_pair(t)
    new = {k: t[k] for k in OB.NEW_KEYFRAME_KEYS}
    swapped = poke(poke(t["mp_obs_kf"], e0, t["mp_obs_kf"][e1]), e1, t["mp_obs_kf"][e0])
    for text, kf in (("do not ascend in keyframe slot", swapped), ("a keyframe twice in a map point's observations", poke(t["mp_obs_kf"], e1, t["mp_obs_kf"][e0]))):
        refused(lambda: apply(dict(t, mp_obs_kf=kf)), text)
        refused(lambda: OB.AddKeyFrameObservations(dict(new, mp_obs_kf=kf), 0), text)
    p = t["kf_mappoint"][5, :t["kf_n"][5]]
    i, j = np.flatnonzero(p >= 0)[:2]
    twice = poke(t["kf_mappoint"], (5, j), p[i])
    refused(lambda: apply(dict(t, kf_mappoint=twice)), "a map point twice in a keyframe's row")
    refused(lambda: OB.AddKeyFrameObservations(dict(new, kf_mappoint=twice), 0), "a map point twice in a keyframe's row")
    refused(lambda: apply(dict(t, mp_replaced=poke(t["mp_replaced"], 3, OC.M))), "mp_replaced outside")
    refused(lambda: apply(dict(t, mp_replaced=poke(t["mp_replaced"], 3, -2))), "mp_replaced outside")


def test_slots_lists_progress_and_modes_out_of_range_are_refused():
    c = OC.case("main")
    t = OC.tables(c)
    new = {k: t[k] for k in OB.NEW_KEYFRAME_KEYS}
    refused(lambda: OB.AddKeyFrameObservations(new, OC.K), "cur outside")
    refused(lambda: OB.AddKeyFrameObservations(new, -1), "cur outside")
    refused(lambda: apply(t, mode=3), "unknown apply mode")
    refused(lambda: apply(t, item_kf=poke(c["item_kf"], 1, OC.K)), "item_kf outside")
    refused(lambda: apply(t, item_kf=poke(c["item_kf"], 1, -1)), "item_kf outside")
    refused(lambda: apply(t, mp_begin=poke(c["mp_begin"], 0, 1)), "mp_begin: offsets must start at 0")
    refused(lambda: apply(t, mp_begin=poke(c["mp_begin"], 2, 0)), "mp_begin: offsets must not decrease")
    refused(lambda: apply(t, mp_begin=poke(c["mp_begin"], -1, len(c["point"]) + 1)), "mp_begin: offsets end past")
    refused(lambda: apply(t, point=poke(c["point"], 4, OC.M)), "point outside")
    refused(lambda: apply(t, point=poke(c["point"], 4, -2)), "point outside")
    refused(lambda: apply(t, best_idx=poke(c["best_idx"], 4, OC.KF_CAP)), "best_idx outside")
    refused(lambda: apply(t, best_idx=poke(c["best_idx"], 4, -2)), "best_idx outside")
    n, items = len(c["point"]), len(c["item_kf"])
    fresh = dict(replace_point=np.full(n, -1, np.int32), n_fused=np.zeros(items, np.int32), touched=np.zeros(OC.M, np.int32),
                 n_touched=np.zeros(1, np.int32), progress=np.zeros(4, np.int32), status=np.zeros(1, np.int32))
    for prog in ((items + 1, 0, 0, 0), (-1, 0, 0, 0), (0, 2, 0, 0), (0, -1, 0, 0), (0, 0, OC.PER_ITEM + 1, 0), (0, 0, -1, 0), (items, 0, 1, 0)):
        refused(lambda: apply(t, mode=OB.APPLY_FUSE_SIM3, state=dict(fresh, progress=np.array(prog, np.int32))), "progress outside the list")
    refused(lambda: apply(t, state=dict(fresh, progress=np.array((0, 1, 0, 0), np.int32))), "progress outside the list")   # one phase
    refused(lambda: apply(t, mode=OB.APPLY_FUSE_SIM3, state=dict(fresh, replace_point=poke(fresh["replace_point"], 0, OC.M))),
            "replace_point outside")
    resumed = dict(fresh, progress=np.array((1, 0, 0, 0), np.int32))
    refused(lambda: apply(t, state=dict(resumed, n_touched=np.array([OC.M + 1], np.int32))), "n_touched outside")
    refused(lambda: apply(t, state=dict(resumed, n_touched=np.array([1], np.int32), touched=poke(fresh["touched"], 0, OC.M))),
            "touched entry outside")
    off, kf, idx = c["mp_obs_off"], c["mp_obs_kf"], c["mp_obs_idx"]
    refused(lambda: OB.GrowObservations(poke(off, 100, 0), kf, idx, 1), "offsets must not decrease")
    refused(lambda: OB.GrowObservations(poke(off, -1, 1 << 20), kf, idx, 1), "offsets end past n_obs")
    refused(lambda: OB.GrowObservations(off, kf, idx, 0, poke(np.zeros(OC.M, np.int32), 9, -1), len(kf)), "extra must not be negative")


def test_the_dirty_case_is_refused():
    c = OC.case("dirty")
    with pytest.raises(OrbError, match="status -1"):
        apply(OC.tables(c), c)


def test_the_python_wrapper_raises_on_dtype_shape_and_device():
    c = OC.case("main")
    t = OC.tables(c)
    with pytest.raises(ValueError, match="kf_uright must be float32"):
        apply(dict(t, kf_uright=t["kf_uright"].astype(np.float64)))
    with pytest.raises(ValueError, match="mp_bad must be uint8"):
        apply(dict(t, mp_bad=t["mp_bad"].astype(np.int32)))
    with pytest.raises(ValueError, match="mp_replaced must have shape"):
        apply(dict(t, mp_replaced=t["mp_replaced"][:-1]))
    with pytest.raises(ValueError, match="mp_found is required"):
        apply(dict(t, mp_found=None))
    with pytest.raises(ValueError, match="one length"):
        apply(dict(t, mp_obs_idx=t["mp_obs_idx"][:-1]))
    with pytest.raises(ValueError, match="best_idx must have shape"):
        apply(t, best_idx=c["best_idx"][:-1])
    with pytest.raises(ValueError, match="mp_begin must have shape"):
        apply(t, mp_begin=c["mp_begin"][:-1])
    with pytest.raises(ValueError, match="point must be int32"):
        apply(t, point=c["point"].astype(np.int64))
    with pytest.raises(ValueError, match="extra must have shape"):
        OB.GrowObservations(c["mp_obs_off"], c["mp_obs_kf"], c["mp_obs_idx"], 0, np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="GPU tensor"):
        OB.fuse_apply_device(t, OB.APPLY_FUSE, c["item_kf"], c["mp_begin"], c["point"], c["best_idx"])
    with pytest.raises(ValueError, match="GPU tensor"):
        OB.add_keyframe_observations_device({k: t[k] for k in OB.NEW_KEYFRAME_KEYS}, 0)
    with pytest.raises(ValueError, match="GPU tensor"):
        OB.grow_observations_device(c["mp_obs_off"], c["mp_obs_kf"], c["mp_obs_idx"], 10)


def test_the_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    libso = root / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text('#include "orbslam2_amd.hpp"\n'
                    "int main() {\n"
                    "    orbmm_observe t = {};\n"
                    "    t.kf_cap = 0;                                   // refused before anything is dereferenced\n"
                    "    ORB_SLAM2_AMD::Observations obs(t);\n"
                    "    orbmm_apply a = {};\n"
                    "    int refused = 0;\n"
                    "    try { obs.FuseApply(a); } catch (const std::exception&) { refused++; }\n"
                    "    try { obs.AddKeyFrameObservations(0, nullptr, nullptr, nullptr, nullptr); } catch (const std::exception&) { refused++; }\n"
                    "    try { obs.Grow(-1, nullptr, 0, nullptr, nullptr, nullptr, nullptr); } catch (const std::exception&) { refused++; }\n"
                    "    return refused == 3 ? 0 : 1;\n"
                    "}\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{root / 'include'}", str(main), "-o", str(exe), f"-L{libso.parent}",
                    "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
