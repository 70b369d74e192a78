"""Times one keyframe_culling_device call, one map_point_culling_device call and one compact_observations_device call at the
shape of tools/time_map_maintenance.py (512 keyframes, 2000 slots each), with a target list of 100 keyframes and a recent
list of 4000 points, and the same calls through tests/native/culling_check.cpp at -O2 on one core of the CPU.  The keyframe
cull is timed twice: on a map where no target is redundant (the common case) and on one where every tenth target is.  Device
times are medians of HIP-event intervals around a single call after warm-up, the state restored outside the interval.
Prints one JSON line."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import culling_ref as CR  # noqa: E402
from test_map_maintenance_native import dump  # noqa: E402
from time_map_maintenance import CONN_CAP, K, KF_CAP, make  # noqa: E402

CUR, TARGETS, RECENT, REPS, TH_DEPTH = 256, 100, 4000, 30, 3.5
KEYS = ("kf_id", "kf_n", "kf_mappoint", "kf_kp_octave", "kf_uright", "kf_depth", "kf_pose", "kf_bad", "kf_not_erase",
        "kf_to_be_erased", "kf_tcp", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_first_kf_id", "mp_ref_kf", "mp_obs_off",
        "mp_obs_kf", "mp_obs_idx", "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent", "kf_covis")


def make_cull(hot):
    """time_map_maintenance's map with the tables the culls read.  The rows connect every keyframe with the 50 on each side
    of it (weights falling with the distance), so CUR has 100 targets; the targets in `hot` sit at the top octave, the
    others at random ones, and a hot target's thinly observed points fail the depth gate, so that it is redundant."""
    m = make()
    rng = np.random.default_rng(1)
    M = len(m["mp_bad"])
    m["kf_id"] = m["kf_id"] + 1
    m["kf_kp_octave"][hot] = 7
    m["kf_kp_octave"][[k for k in range(K) if k not in hot]] //= 2
    m.update(kf_uright=np.where(rng.random((K, KF_CAP)) < 0.5, 1, -1).astype(np.float32),
             kf_depth=(rng.random((K, KF_CAP)) * 4).astype(np.float32), kf_bad=np.zeros(K, np.uint8),
             kf_not_erase=np.zeros(K, np.uint8), kf_to_be_erased=np.zeros(K, np.uint8), kf_tcp=np.zeros((K, 12), np.float32),
             mp_visible=rng.integers(1, 40, M).astype(np.int32), mp_first_kf_id=rng.integers(250, 256, M).astype(np.int32),
             kf_parent=np.arange(-1, K - 1).astype(np.int32))
    thin = np.diff(m["mp_obs_off"]) < 5
    for k in hot:                                          # a hot keyframe's thinly observed points fail the depth gate
        row = m["kf_mappoint"][k, :m["kf_n"][k]]
        m["kf_depth"][k, :m["kf_n"][k]][thin[row]] = -1
    m["mp_found"] = np.minimum(rng.integers(0, 40, M), m["mp_visible"]).astype(np.int32)
    stereo = m["kf_uright"][m["mp_obs_kf"], m["mp_obs_idx"]] >= 0
    m["mp_nobs"] = np.add.reduceat(np.append(1 + stereo, 0), m["mp_obs_off"][:-1]).astype(np.int32) * (np.diff(m["mp_obs_off"]) > 0)
    m["mp_nobs"] = m["mp_nobs"].astype(np.int32)
    G = CR.Connections(m, K)
    for k in range(K):
        G.write(k, {s: 60 - abs(s - k) for s in range(max(k - TARGETS // 2, 0), min(k + TARGETS // 2 + 1, K)) if s != k})
    return {k: m[k] for k in KEYS}


def main():
    quiet, busy = make_cull([]), make_cull(list(range(CUR - 50, CUR + 51, 10)))
    recent = np.random.default_rng(2).permutation(len(quiet["mp_bad"]))[:RECENT].astype(np.int32)
    res = dict(keyframes=K, kf_cap=KF_CAP, targets=int(quiet["n_ord"][CUR]), recent=RECENT, points=int(len(quiet["mp_bad"])),
               observations=int(len(quiet["mp_obs_kf"])))
    scal = lambda **kw: {k: np.array([v], np.float32 if isinstance(v, float) else np.int32) for k, v in kw.items()}  # noqa: E731
    want = {name: CR.keyframe_culling(t, CUR, False, TH_DEPTH)[2] for name, t in (("quiet", quiet), ("busy", busy))}
    res["culled"] = want
    after = dict(busy, **CR.keyframe_culling(busy, CUR, False, TH_DEPTH)[0])
    with tempfile.TemporaryDirectory() as d:
        exe = Path(d) / "check"
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                        str(ROOT / "tests" / "native" / "culling_check.cpp"), "-o", str(exe)], check=True)
        for name, mode, tables in (("keyframes_quiet", "keyframes", dict(quiet, **scal(cur=CUR, monocular=0, th_depth=TH_DEPTH))),
                                   ("keyframes_busy", "keyframes", dict(busy, **scal(cur=CUR, monocular=0, th_depth=TH_DEPTH))),
                                   ("points", "points", dict(quiet, recent=recent, **scal(cur_kf_id=256, monocular=0))),
                                   ("compact", "compact", {k: after[k] for k in ("mp_obs_off", "mp_obs_kf", "mp_obs_idx")})):
            text = dump(tables)
            res[f"cpu_{name}_ms"] = min(float(subprocess.run([str(exe), mode, "time"], input=text, capture_output=True, text=True,
                                                             check=True).stdout) for _ in range(3))
    import torch
    if torch.cuda.is_available():
        from orb_slam2_refactored_amd import culling as CU
        cuda = lambda t: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in t.items()}  # noqa: E731
        d_recent, n_out = torch.from_numpy(recent).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")
        for name, src in (("keyframes_quiet", quiet), ("keyframes_busy", busy), ("points", quiet), ("compact", after)):
            t, saved = cuda(src), cuda(src)
            out = (torch.empty(CONN_CAP, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                   torch.zeros(1, dtype=torch.int32, device="cuda"))
            packed = tuple(torch.zeros_like(t[k]) for k in ("mp_obs_off", "mp_obs_kf", "mp_obs_idx"))
            call = {"keyframes_quiet": lambda: CU.keyframe_culling_device(t, CUR, False, TH_DEPTH, out),
                    "keyframes_busy": lambda: CU.keyframe_culling_device(t, CUR, False, TH_DEPTH, out),
                    "points": lambda: CU.map_point_culling_device(t, d_recent, 256, False, n_out),
                    "compact": lambda: CU.compact_observations_device(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"], packed)}[name]
            ms = []
            for r in range(REPS + 5):
                for k in CR.KEYFRAME_UPDATED:
                    t[k].copy_(saved[k])
                d_recent.copy_(torch.from_numpy(recent))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                call()
                b.record()
                torch.cuda.synchronize()
                if r >= 5:
                    ms.append(a.elapsed_time(b))
            res[f"gpu_{name}_ms"] = float(np.median(ms))
            res[f"gpu_{name}_ms_min_max"] = [float(min(ms)), float(max(ms))]
            if name.startswith("keyframes"):
                assert int(out[1].cpu()[0]) == want[name.split("_")[1]], (name, int(out[1].cpu()[0]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
