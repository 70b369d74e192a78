"""csrc/eg_edge.h and csrc/sim3_g2o.h on the CPU against tests/essential_graph_ref.py:
tests/native/essential_graph_check.cpp is compiled stand-alone (under AddressSanitizer and UBSan) and fed the edges of
a test graph.  The float side (measurement, recovered pose, corrected point) is the same IEEE float expressions on
both sides and is bit-equal.  log, the error and the Jacobian are the same double expressions but for libm's and
numpy's exp / log / acos / sin / cos: a few ulp (8 eps relative per component of a chain of four Sim3 products), and
delta = 1e-9 magnifies that by 1 / (2 delta) in the Jacobian."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import essential_graph_ref as R
import optsim3_ref as S
from test_essential_graph_ref import case, reference

ROOT = Path(__file__).resolve().parents[1]
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("eg") / "essential_graph_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "native" / "essential_graph_check.cpp"), "-o", str(out)], check=True)
    return out


def run(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    rows = [np.array(l.split(), np.float64) for l in out.stdout.strip().split("\n")]
    assert len(rows) == len(lines)
    return rows


def fmt(*arrs):
    return " ".join(repr(float(v)) for a in arrs for v in np.asarray(a, np.float64).reshape(-1))


def test_float_side_is_bit_equal(exe):
    g, r = case("chain13"), reference("chain13")
    lines = []
    for e in range(len(g["edge_i"])):
        tb = g["edge_sim3"] if g["edge_table"][e] else g["vertex_sim3"]
        lines.append("M " + fmt(tb[g["edge_i"][e]], tb[g["edge_j"][e]]))
    for row, want in zip(run(exe, lines), r["measurement"]):
        assert row.tobytes() == want.tobytes()
    lines = ["R " + fmt(r["sim3_g2o"][k], g["vertex_sim3"][k], g["points"][p]) for p, k in enumerate(g["point_ref"])]
    for p, row in enumerate(run(exe, lines)):
        k = g["point_ref"][p]
        assert row[:12].astype(np.float32).tobytes() == r["pose"][k].tobytes()
        assert row[12:].astype(np.float32).tobytes() == r["points"][p].tobytes()


def test_log_error_and_jacobian_agree(exe):
    g = case("chain13_large_loop")
    G = R.Graph(g)
    us = [[3e-6, -2e-6, 1e-6, 0.3, -0.2, 0.1, 2e-6], [0.3, -0.5, 0.2, 0.3, -0.2, 0.1, -3e-6],
          [2e-6, 1e-6, -3e-6, 1.0, 2.0, -0.5, 0.4], [-0.7, 0.4, 1.1, 1.0, 2.0, -0.5, -0.6]]
    for u, row in zip(us, run(exe, ["L " + fmt(S.g2o_row(S.sim3_exp(u))) for u in us])):   # the four branches
        assert np.abs(row - np.array(R.sim3_log(S.sim3_exp(u)))).max() <= 64 * EPS * max(1.0, np.abs(u).max())
    for fix in (0, 1):
        G.fix_scale = bool(fix)
        J = G.jacobians()
        err = G.errors()
        lines = ["E " + fmt(G.meas_rows[e], S.g2o_row(G.est[G.ei[e]]), S.g2o_row(G.est[G.ej[e]])) + f" {fix}" for e in range(G.E)]
        worst = 0.0
        for e, row in enumerate(run(exe, lines)):
            scale = max(1.0, np.abs(err[e]).max(), np.abs(G.meas_rows[e]).max())
            assert np.abs(row[:7] - err[e]).max() <= 64 * EPS * scale
            d = np.abs(row[7:].reshape(2, 7, 7) - J[e]).max()
            worst = max(worst, d / (64 * EPS * scale / (2 * R.DELTA)))
            if fix:
                assert not row[7:].reshape(2, 7, 7)[:, :, 6].any()
        print("Jacobian difference / bound, largest:", worst)
        assert worst <= 1.0
