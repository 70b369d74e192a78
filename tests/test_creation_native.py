"""csrc/mk_create.h on the CPU against tests/creation_ref.py: tests/native/creation_check.cpp is compiled stand-alone twice,
plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on the generated cases, those with entries outside
their tables among them.  Every array is equal, floats as bits.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import creation_cases as CC
import creation_ref as CR
from test_map_maintenance_native import dump

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("creation") / f"creation_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Werror", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "creation_check.cpp"), "-o", str(out)], check=True)
    return out


def run(exe, mode, tables):
    out = subprocess.run([str(exe), mode], input=dump(tables), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    got = {}
    for line in out.stdout.strip().split("\n"):
        name, n, *vals = line.split()
        got[name] = np.array(vals, np.int64).astype(np.int32)
        assert len(vals) == int(n)
    return got


def flat(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)).reshape(-1)


def create(exe, t, ls, alloc, by_keypoint=False, recent=None, n_recent=0):
    extra = dict(list_cap=np.array([ls["idx1"].shape[1]], np.int32), by_keypoint=np.array([int(by_keypoint)], np.int32),
                 alloc=np.array([alloc], np.int32))
    if "frame_mappoint" in ls:
        extra["kp_cap"] = np.array([ls["frame_mappoint"].shape[1]], np.int32)
    if recent is not None:
        extra.update(recent=recent, n_recent=np.array([n_recent], np.int32))
    got = run(exe, "create", {**t, **ls, **extra})
    upd, out = CR.create_points(t, ls, alloc, by_keypoint, recent, n_recent)
    for k, v in {**upd, **out}.items():
        assert np.array_equal(got[k], flat(v)), k
    return out


@pytest.mark.parametrize("two,by_keypoint", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("sizes", [(0,), (1,), (63, 0, 64, 65, 5)])
def test_the_created_points_are_equal_on_the_generated_cases(exe, sizes, two, by_keypoint):
    t = CC.make_map(K=6, kf_cap=160, M=260, alloc=9, seed=len(sizes))
    ls = CC.make_lists(t, sizes, 160, two=two, by_keypoint=by_keypoint, drops=3, frames=(2, 100))
    out = create(exe, t, ls, 9, by_keypoint, recent=np.full(300, -2, np.int32), n_recent=4)
    assert out["status"][0] == CR.OK and out["alloc"][0] == 9 + CC.n_valid(t, ls)


def test_a_list_of_257_crosses_a_chunk_and_values_may_be_left_out(exe):
    t = CC.make_map(K=3, kf_cap=600, M=600, alloc=0, seed=5, short_last_kf=False)
    for k in ("mp_normal", "mp_max_min", "mp_desc", "kf_desc", "kf_bad"):
        del t[k]
    ls = CC.make_lists(t, (257, 257), 300, two=True, values=False, drops=2)
    assert create(exe, t, ls, 0)["n_created"].sum() == CC.n_valid(t, ls) >= 500


def test_entries_outside_their_tables_are_dropped_and_nothing_is_touched_outside(exe):
    t = CC.make_map(K=4, kf_cap=96, M=120, alloc=3, seed=7)
    ls = CC.make_lists(t, (20, 20, 20, 20, 20), 64, two=True, frames=(2, 16))
    ls["n_list"][0] = 1000                                   # clamped to list_cap: the tail holds -7
    ls["kf1"][1] = 4
    ls["kf2"][2] = -5
    ls["kf2"][3] = ls["kf1"][3]                              # kf1 == kf2
    ls["idx1"][4, 3], ls["idx2"][4, 5], ls["idx1"][4, 7] = 1 << 30, -(1 << 31), 96
    ls["item_frame"][:] = (0, 9, -4, 1, 1)                   # idx1 >= kp_cap = 16 of the frame is not written either
    out = create(exe, t, ls, 3)
    assert out["status"][0] == CR.OK and list(out["n_created"]) == [20, 0, 0, 0, 17]
    out = create(exe, t, ls, -50)                            # alloc is clamped into the table
    assert out["alloc"][0] == 37
    bad = dict(t, mp_obs_off=np.where(np.arange(121) % 2 == 0, t["mp_obs_off"], -9).astype(np.int32))
    assert create(exe, bad, ls, 3)["status"][0] == CR.OVERFLOW   # rows of clamped offsets hold nothing


@pytest.mark.parametrize("room", [0, -1])
def test_overflow_of_slots_rows_and_recent_leaves_everything_as_it_was(exe, room):
    t = CC.make_map(K=5, kf_cap=64, M=80, alloc=11, seed=9, rows=(2, 3))
    ls = CC.make_lists(t, (30, 0, 39), 64, two=True)
    assert create(exe, t, ls, 11 + room * -1)["status"][0] == (CR.OK if room == 0 else CR.OVERFLOW)   # 69 points, 69 or 68 slots
    short = dict(t, mp_obs_off=t["mp_obs_off"].copy())
    short["mp_obs_off"][41:] -= short["mp_obs_off"][41] - short["mp_obs_off"][40] - 2 - room   # slot 40's row: 2 or 1 entries
    out = create(exe, short, ls, 11)
    assert list(out["needed"]) == ([80, -1] if room == 0 else [80, 40])
    recent = np.full(75 + room, -2, np.int32)
    assert create(exe, t, ls, 11, recent=recent, n_recent=6)["status"][0] == (CR.OK if room == 0 else CR.OVERFLOW)


def test_the_keyframe_rows_are_equal(exe):
    fr, kf = CC.make_frames(F=3, kp_cap=40), CC.make_keyframes(K=5, kf_cap=44, conn_cap=6)
    items = dict(item_frame=np.array([1, 0, 7, 2, -1], np.int32), item_kf=np.array([3, 0, 1, 9, 2], np.int32),
                 item_id=np.array([21, 22, 23, 24, 25], np.int32), item_baseline=np.array([.1, .2, .3, .4, .5], np.float32))
    fr["frame_n"][0] = 1000                                  # clamped to kp_cap
    sizes = dict(kp_cap=np.array([40], np.int32), kf_cap=np.array([44], np.int32), conn_cap=np.array([6], np.int32),
                 n_keyframes=np.array([5], np.int32))
    got = run(exe, "insert", {**fr, **kf, **items, **sizes})
    ref_fr = dict(fr, frame_n=np.minimum(fr["frame_n"], 40))
    want = CR.insert_keyframes(ref_fr, kf, **items)
    for k, v in want.items():
        assert np.array_equal(got[k], flat(v)), k
    assert np.array_equal(want["kf_mappoint"][1], kf["kf_mappoint"][1]) and want["kf_n"][3] == 40 and want["kf_id"][0] == 22
    few = {k: kf[k] for k in ("kf_n", "kf_desc", "ord_slot")}   # every output is optional
    got = run(exe, "insert", {**fr, **few, **items, **sizes})
    want = CR.insert_keyframes(ref_fr, few, **items)
    assert set(got) == set(few) and all(np.array_equal(got[k], flat(v)) for k, v in want.items())
