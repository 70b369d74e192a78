"""The device on every row of tests/pose_cases.py (each row's claim is witnessed on the oracle's trace by
tests/test_pose_cases_oracle.py): identical n_inliers and outlier flags, pose within test_pose_gpu.py's TOL,
through both the host entry and the device entry; and every row alone bit-equal to the same row inside one
shuffled ragged batch of all rows."""
import numpy as np
import pytest

from orb_slam2_refactored_amd.optimizer import PoseOptimization, pose_optimization_device
from pose_cases import BY_ID, CASE_IDS, CASES, build_case, concat, oracle_result, swap_cameras, take

pytestmark = pytest.mark.gpu
TOL = 1e-6
OUT = ("pose_R", "pose_t", "n_inliers", "outlier")

_host, _dev = {}, {}


def host_result(case):
    if case.id not in _host:
        _host[case.id] = PoseOptimization(build_case(case))
    return _host[case.id]


def run_device(batch):
    import torch
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
    d = pose_optimization_device(dev)
    torch.cuda.synchronize()
    E = int(batch["edge_begin"][-1])
    return {k: d[k].cpu().numpy()[:E] if k == "outlier" else d[k].cpu().numpy() for k in OUT}


def device_result(case):
    if case.id not in _dev:
        _dev[case.id] = run_device(build_case(case))
    return _dev[case.id]


def compare(g, o):
    print("pose difference R %.3e t %.3e" % (np.abs(g["pose_R"] - o["pose_R"]).max(),
                                             np.abs(g["pose_t"] - o["pose_t"]).max()))
    assert np.array_equal(g["n_inliers"], o["n_inliers"])
    assert np.array_equal(g["outlier"], o["outlier"])
    assert np.abs(g["pose_R"] - o["pose_R"]).max() < TOL
    assert np.abs(g["pose_t"] - o["pose_t"]).max() < TOL


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_entry_matches_oracle(oracle, case):
    g = host_result(case)
    if case.id.startswith("solve-fail"):
        assert all(np.isfinite(g[k]).all() for k in OUT)
    compare(g, oracle_result(oracle, case))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_entry_matches_oracle_and_host(oracle, case):
    d = device_result(case)
    compare(d, oracle_result(oracle, case))
    h = host_result(case)
    for k in OUT:
        assert np.array_equal(d[k], h[k]), k
    again = run_device(build_case(case))
    for k in OUT:
        assert np.array_equal(d[k], again[k]), k


def test_exact_fit_leaves_the_pose_untouched():
    b, g = build_case(BY_ID["exact-fit"]), host_result(BY_ID["exact-fit"])
    assert np.array_equal(g["pose_R"], b["pose_R"]) and np.array_equal(g["pose_t"], b["pose_t"])
    assert g["n_inliers"][0] == 24 and not g["outlier"].any()


def test_another_frames_camera_changes_the_result():
    g = host_result(BY_ID["cams"])
    other = PoseOptimization(swap_cameras(build_case(BY_ID["cams"])))
    assert (other["n_inliers"] != g["n_inliers"]).all()


def test_rows_alone_equal_rows_in_one_shuffled_batch():
    """A frame's result depends on nothing but the frame: all rows' frames in one ragged batch, in a shuffled
    order, give bit for bit what each row gives alone (edge_begin, the per-frame cam / pose rows, the LDS
    staging and the HBM tail of a 1025-edge frame beside a 12-edge one)."""
    whole = concat([build_case(c) for c in CASES])
    n = len(whole["edge_begin"]) - 1
    order = np.random.default_rng(5).permutation(n)
    shuffled = take(whole, order)
    for run in (PoseOptimization, run_device):
        g = run(shuffled)
        eb = shuffled["edge_begin"]
        pos = {int(f): i for i, f in enumerate(order)}
        f = 0
        for c in CASES:
            alone = host_result(c)
            ebc = build_case(c)["edge_begin"]
            for j in range(len(ebc) - 1):
                i = pos[f]
                assert np.array_equal(g["pose_R"][i], alone["pose_R"][j]), (c.id, j)
                assert np.array_equal(g["pose_t"][i], alone["pose_t"][j]), (c.id, j)
                assert g["n_inliers"][i] == alone["n_inliers"][j], (c.id, j)
                assert np.array_equal(g["outlier"][eb[i]:eb[i + 1]], alone["outlier"][ebc[j]:ebc[j + 1]]), (c.id, j)
                f += 1
        assert f == n
