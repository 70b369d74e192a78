"""csrc/mm_observe.h on the CPU against tests/observe_ref.py: tests/native/observe_check.cpp is compiled stand-alone twice,
plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on the generated cases, the one with entries
outside their tables among them, in all three modes.  Every array is equal.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import culling_ref as CR
import observe_cases as OC
import observe_ref as OR
from test_map_maintenance_native import dump

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("observe") / f"observe_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "observe_check.cpp"), "-o", str(out)], check=True)
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


def walk(exe, tables, c, mode, state=None):
    """One call of the walk on `tables`; state: replace_point, n_fused, touched, progress of an interrupted one."""
    n, items = len(c["point"]), len(c["item_kf"])
    s = state or dict(replace_point=np.full(n, -1, np.int32), n_fused=np.zeros(items, np.int32), touched=np.zeros(0, np.int32),
                      progress=np.zeros(4, np.int32))
    got = run(exe, "apply", dict(tables, **OC.apply_of(c), mode=np.array([mode], np.int32), replace_point=s["replace_point"],
                                 n_fused=s["n_fused"], touched=s["touched"], n_touched=np.array([len(s["touched"])], np.int32),
                                 progress=s["progress"]))
    got["touched"] = got["touched"][:got["n_touched"][0]]
    return got


def assert_walk(got, want):
    for k in OR.UPDATED + ("n_fused", "replace_point", "touched", "progress"):
        assert np.array_equal(got[k], flat(want[k])), k
    assert got["status"][0] == want["status"]


@pytest.mark.parametrize("mode", OC.MODES)
@pytest.mark.parametrize("name", ["main", "dirty", "wide"])
def test_the_walk_is_equal_on_the_generated_cases(exe, name, mode):
    c = OC.case(name)
    assert_walk(walk(exe, OC.tables(c), c, mode), OC.expected(name, mode))


@pytest.mark.parametrize("mode", OC.MODES)
def test_a_walk_resumed_after_every_overflow_equals_the_uninterrupted_one(exe, mode):
    c = OC.make_main(slack=0)
    roomy = OC.make_main()
    want = OR.fuse_apply(OC.tables(roomy), mode, **OC.apply_of(roomy))
    t, state, stops = OC.tables(c), None, 0
    for _ in range(40):
        got = walk(exe, t, c, mode, state)
        ref = OR.fuse_apply(t, mode, **OC.apply_of(c), **({} if state is None else state))
        assert_walk(got, ref)
        t.update({k: got[k].reshape(t[k].shape).astype(t[k].dtype) for k in OR.UPDATED})
        if got["status"][0] == OR.OK:
            break
        stops += 1
        state = {k: got[k] for k in ("replace_point", "n_fused", "touched", "progress")}
        extra = np.full(OC.M, 2 * stops, np.int32)
        extra[got["progress"][3]] = OC.K                    # room for the point that was full, a little for the others
        off, kf, idx, st = OR.grow_observations(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"], 0, extra, len(t["mp_obs_kf"]) + 2 * stops * OC.M + OC.K)
        assert st == OR.OK
        t.update(mp_obs_off=off, mp_obs_kf=kf, mp_obs_idx=idx)
    assert got["status"][0] == OR.OK and stops >= 2
    a, b = OC.canonical(t), OC.canonical({k: want[k] for k in OR.UPDATED} | {"mp_obs_off": roomy["mp_obs_off"]})
    for k in OR.UPDATED + ("mp_obs_off",):
        assert np.array_equal(flat(a[k]), flat(b[k])), k
    for k in ("n_fused", "replace_point", "touched"):
        assert np.array_equal(got[k], flat(want[k])), k


def test_the_new_keyframe_loop_is_equal_with_a_full_row(exe):
    t, cur, full = OC.new_keyframe()
    want, added, recent, status = OR.add_keyframe_observations(t, cur)
    got = run(exe, "new", dict(t, cur=np.array([cur], np.int32)))
    for k in OR.NEW_KEYFRAME_UPDATED:
        assert np.array_equal(got[k], flat(want[k])), k
    assert np.array_equal(got["counts"], [len(added), len(recent)]) and np.array_equal(got["status"], status)
    assert np.array_equal(got["added"][:len(added)], added) and np.array_equal(got["recent_out"][:len(recent)], recent)
    assert len(added) >= 20 and len(recent) >= 3 and (status == OR.OBS_OVERFLOW).sum() == 1 and full not in added


@pytest.mark.parametrize("slack,per_point,room", [(0, False, 0), (2, False, 0), (0, True, 0), (4, False, -40)])
def test_the_grown_csr_is_equal(exe, slack, per_point, room):
    c = OC.case("dirty")
    t = {k: OC.expected("dirty", OR.FUSE)[k] for k in ("mp_obs_kf", "mp_obs_idx")}
    off = c["mp_obs_off"]
    extra = np.random.default_rng(2).integers(-1, 4, OC.M).astype(np.int32) if per_point else None
    n_out = int((t["mp_obs_kf"][:off[-1]] != -1).sum()) + 4 * OC.M + room
    w_off, w_kf, w_idx, w_st = OR.grow_observations(off, t["mp_obs_kf"], t["mp_obs_idx"], slack, extra, n_out)
    tabs = dict(mp_obs_off=off, mp_obs_kf=t["mp_obs_kf"], mp_obs_idx=t["mp_obs_idx"], slack=np.array([slack], np.int32),
                n_obs_out=np.array([n_out], np.int32))
    got = run(exe, "grow", dict(tabs, extra=extra) if per_point else tabs)
    assert np.array_equal(got["mp_obs_off"], w_off) and got["status"][0] == w_st
    assert np.array_equal(got["mp_obs_kf"], w_kf) and np.array_equal(got["mp_obs_idx"], w_idx)
    assert (w_st == OR.OBS_OVERFLOW) == (room < 0)
    if slack == 0 and not per_point:                        # slack 0 is the culls' compaction
        c_off, c_kf, c_idx = CR.compact_observations(off, t["mp_obs_kf"], t["mp_obs_idx"])
        assert np.array_equal(w_off, c_off) and np.array_equal(w_kf[:w_off[-1]], c_kf[:w_off[-1]]) and np.array_equal(w_idx[:w_off[-1]], c_idx[:w_off[-1]])
