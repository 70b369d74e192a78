"""Times one update_connections_device call and one update_normal_depth_device call at a loop-closing shape (512 keyframes,
2000 slots each, a batch of 100 keyframes, all points), and the same cases through tests/native/map_maintenance_check.cpp at
-O2 on the CPU.  Device times are medians of HIP-event intervals around a single call after warm-up, the state restored
outside the interval.  Prints one JSON line."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import map_maintenance_cases as MC  # noqa: E402
from test_map_maintenance_native import dump  # noqa: E402

K, KF_CAP, CONN_CAP, B, REPS = 512, 2000, 512, 100, 30


def make(seed=0):
    rng = np.random.default_rng(seed)
    M = K * KF_CAP // 5
    centre, half = rng.integers(0, K, M), rng.integers(1, 5, M)
    kf_n = np.zeros(K, np.int32)
    kf_mappoint = np.full((K, KF_CAP), -1, np.int32)
    off, obs_kf, obs_idx = np.zeros(M + 1, np.int32), [], []
    for p in range(M):
        for k in range(max(centre[p] - half[p], 0), min(centre[p] + half[p] + 1, K)):
            if kf_n[k] < KF_CAP:
                kf_mappoint[k, kf_n[k]] = p
                obs_kf.append(k)
                obs_idx.append(kf_n[k])
                kf_n[k] += 1
        off[p + 1] = len(obs_kf)
    obs_kf = np.array(obs_kf, np.int32)
    m = dict(kf_id=np.arange(K, dtype=np.int32), kf_n=kf_n, kf_mappoint=kf_mappoint, mp_bad=np.zeros(M, np.uint8), mp_obs_off=off,
             mp_obs_kf=obs_kf, mp_obs_idx=np.array(obs_idx, np.int32),
             mp_ref_kf=np.where(off[1:] > off[:-1], obs_kf[np.minimum(off[:-1], len(obs_kf) - 1)], -1).astype(np.int32),
             mp_xw=rng.normal(size=(M, 3)).astype(np.float32), kf_pose=np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 5], np.float32), (K, 1)),
             kf_kp_octave=rng.integers(0, 8, (K, KF_CAP)).astype(np.int32), mp_normal=np.zeros((M, 3), np.float32),
             mp_max_min=np.zeros((M, 2), np.float32))
    m.update(MC.empty_state(K, CONN_CAP))
    return m


def main():
    m = make()
    items = np.arange(0, K, K // B, dtype=np.int32)[:B]
    res = dict(keyframes=K, kf_cap=KF_CAP, batch=int(len(items)), points=int(len(m["mp_bad"])), observations=int(len(m["mp_obs_kf"])))
    with tempfile.TemporaryDirectory() as d:
        exe = Path(d) / "check"
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                        str(ROOT / "tests" / "native" / "map_maintenance_check.cpp"), "-o", str(exe)], check=True)
        for mode, tables in (("connect", dict(MC.graph(m), item=items)), ("normal", dict(MC.points(m), scale=MC.SCALE))):
            text = dump(tables)
            res[f"cpu_{mode}_ms"] = min(float(subprocess.run([str(exe), mode, "time"], input=text, capture_output=True, text=True,
                                                             check=True).stdout) for _ in range(3))
    import torch
    if torch.cuda.is_available():
        from orb_slam2_refactored_amd import map_maintenance as MM
        cuda = lambda t: {k: torch.from_numpy(v).cuda() for k, v in t.items()}  # noqa: E731
        g, saved, pts, it = cuda(MC.graph(m)), cuda({k: m[k] for k in MC.R.STATE_KEYS}), cuda(MC.points(m)), torch.from_numpy(items).cuda()
        status = torch.empty(K, dtype=torch.int32, device="cuda")
        for name, call in (("connect", lambda: MM.update_connections_device(g, it, status)),
                           ("normal", lambda: MM.update_normal_depth_device(pts, MC.SCALE))):
            ms = []
            for r in range(REPS + 5):
                for k, v in saved.items():
                    g[k].copy_(v)
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
        assert int(status.sum()) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
