"""The pyramid kernels' tap-table rectangles (csrc/orbx_pyr_rect.h) on the GPU: every level of every frame
byte-identical to the oracle's ComputePyramid at shapes that stress the geometry.

64x48 and 97x75: level l+1 smaller than one tile, every clamp active.  333x251: odd sizes, partial tiles on
both edges, a right-edge rectangle that starts off a dword.  640x480, 1242x375: the C1 / C3 table strides.
1280x720 (2 frames).  770x500: level 1 is 642 columns, so its last tile is 2 columns wide.  Each shape runs
with ORBX_PYR_PAIR 2 and 1 (pairs from level 1 / from level 2) and with a level-0 view whose base is not
16-byte aligned (the level kernel builds level 1, pairs from level 2); every run is a batch of 3 frames
through extract_batch_device, so a wrong frame stride in a rectangle's writes shows in frames 1 and 2.  The
VResizeLinear tail modes 0 and 16 run at one shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from orb_slam2_refactored_amd import ORBextractor, _lib
from orb_slam2_refactored_amd.synth import synth_image, textured_image

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (97, 75), (333, 251), (640, 480), (1242, 375), (1280, 720), (770, 500)]
_frames, _expected = {}, {}


def frames_of(W, H, n):
    """n frames of W x H (computed once per shape and shared, never written)."""
    if (W, H) not in _frames:
        _frames[W, H] = np.stack([textured_image(100 + i, W, H) if i % 2 else synth_image(100 + i, W, H) for i in range(3)])
        _frames[W, H].setflags(write=False)
    return _frames[W, H][:n]


def expected_of(oracle, W, H, n, simd=0):
    """The oracle's pyramids of frames_of(W, H, n), computed once per (shape, tail mode)."""
    from oracle_api import compat
    key = (W, H, simd)
    if key not in _expected:
        with compat(resize_simd=simd):
            _expected[key] = [oracle.pyramid(oracle.params(1000), f) for f in frames_of(W, H, 3)]
    return _expected[key][:n]


def _hip():
    with open("/proc/self/maps") as m:
        for line in m:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("the HIP runtime is not loaded")


def device_pyramids(ex, t):
    """Extracts the batch t ([F, H, W] uint8 on the GPU, rows may be padded) and returns every frame's levels
    1.. as numpy arrays, read from the extractor's pyramid slab."""
    F, H, W = t.shape
    cap = max(ex.max_keypoints(H, W), 1)   # (an image too small for any FAST cell has no output rows)
    kps = torch.empty((F, cap, 7), dtype=torch.int32, device=t.device)
    desc = torch.empty((F, cap, 32), dtype=torch.uint8, device=t.device)
    cnt = torch.empty((F,), dtype=torch.int32, device=t.device)
    lib = _lib.lib()
    _lib.check(lib.orbx_extract_batch_device(ex._h, C.c_void_p(t.data_ptr()), F, H, W, C.c_size_t(t.stride(0)),
                                             C.c_size_t(t.stride(1)), C.c_void_p(kps.data_ptr()),
                                             C.c_void_p(desc.data_ptr()), C.c_void_p(cnt.data_ptr()), cap, None),
               "orbx_extract_batch_device")
    torch.cuda.synchronize()
    assert ex.batch_status() == 0
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for f in range(F):
        levels = []
        for l in range(1, ex.param.nlevels):
            p, r, c, st = C.c_void_p(), C.c_int(), C.c_int(), C.c_size_t()
            _lib.check(lib.orbx_pyramid_device(ex._h, f, l, C.byref(p), C.byref(r), C.byref(c), C.byref(st)),
                       "orbx_pyramid_device")
            buf = np.zeros((r.value, st.value), np.uint8)
            assert hip.hipMemcpy(buf.ctypes.data, p, (r.value - 1) * st.value + c.value, 2) == 0
            levels.append(buf[:, :c.value])
        out.append(levels)
    return out


def make():
    return ORBextractor(ORBextractor.Parameters(1000, 1.2, 8, 20, 7))


def assert_pyramids(got, exp):
    assert len(got) == len(exp)
    for f, (gl, el) in enumerate(zip(got, exp)):
        for l, (g, e) in enumerate(zip(gl, el[1:]), start=1):
            assert g.shape == e.shape, (f, l)
            assert np.array_equal(g, e), f"frame {f} level {l}: {np.count_nonzero(g != e)} px differ"


def upload(frames, aligned):
    """The frames on the GPU; aligned = False: a view whose base is 3 bytes past a 16-byte boundary (row step
    W + 3), so level 0 cannot be staged in 16-byte pieces."""
    F, H, W = frames.shape
    if aligned:
        return torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    wide = np.zeros((F, H, W + 3), np.uint8)
    wide[:, :, 3:] = frames
    t = torch.from_numpy(wide).cuda()[:, :, 3:]
    assert t.data_ptr() % 16 == 3
    return t


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("pair", [2, 1])
@pytest.mark.parametrize("W,H", SHAPES)
def test_levels_match_the_oracle(oracle, monkeypatch, W, H, pair, aligned):
    monkeypatch.setenv("ORBX_PYR_PAIR", str(pair))
    n = 2 if (W, H) == (1280, 720) else 3
    got = device_pyramids(make(), upload(frames_of(W, H, n), aligned))
    assert_pyramids(got, expected_of(oracle, W, H, n))


@pytest.mark.parametrize("simd", [0, 16])
def test_resize_tail_modes(oracle, simd):
    W, H = 333, 251
    ex = make()
    ex.set_opencv_compat(resize_simd=simd)
    got = device_pyramids(ex, upload(frames_of(W, H, 3), True))
    assert_pyramids(got, expected_of(oracle, W, H, 3, simd))
