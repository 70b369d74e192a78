"""Tables for the global BA map update tests (orbba_gba_map as a dict of numpy arrays)."""
import numpy as np

F32 = np.float32
RZ = [0, -1, 0, 1, 0, 0, 0, 0, 1]     # a quarter turn about z
RZT = [0, 1, 0, -1, 0, 0, 0, 0, 1]
EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def csr(children, K):
    off = np.zeros(K + 1, np.int32)
    for k in range(K):
        off[k + 1] = off[k] + len(children.get(k, ()))
    idx = np.array([c for k in range(K) for c in children.get(k, ())], np.int32)
    return off, idx


def hand_case():
    """Six keyframes and six points whose results can be written out (tests/test_global_ba_ref.py):
    chain 0 -> 1 -> 2 -> 3 with 1 and 3 outside the adjustment; 4 unreachable, flagged, with a stale bef row; 5
    unreachable and unflagged."""
    K = 6
    pose = np.array([RZ + [1, 2, 3], EYE + [4, 5, 6], EYE + [1, 1, 1], RZ + [0, 0, 0], EYE + [0, 0, 5], EYE + [3, 3, 3]], F32)
    gba = np.array([EYE + [10, 20, 30], EYE + [-1, -1, -1], EYE + [7, 8, 9], EYE + [-2, -2, -2], EYE + [9, 9, 9],
                    EYE + [8, 8, 8]], F32)
    bef = np.zeros((K, 12), F32)
    bef[4] = EYE + [1, 0, 0]
    off, idx = csr({0: [1], 1: [2], 2: [3]}, K)
    return dict(origins=np.array([0], np.int32), kf_child_off=off, kf_child_idx=idx,
                kf_in_gba=np.array([1, 0, 1, 0, 1, 0], np.uint8), kf_pose=pose, kf_pose_gba=gba, kf_pose_bef=bef,
                mp_bad=np.array([0, 0, 1, 0, 0, 0], np.uint8), mp_in_gba=np.array([0, 0, 0, 1, 0, 0], np.uint8),
                mp_pos_gba=np.array([[0, 0, 0]] * 3 + [[5, 6, 7]] + [[0, 0, 0]] * 2, F32),
                mp_ref_kf=np.array([4, 5, 0, 0, 1, 4], np.int32),
                mp_xw=np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4], [1, 0, 0], [0, 0, 0]], F32))


def random_pose(rng, n):
    """n poses [n, 12] f32: rotations by up to a radian about random axes, translations within 10."""
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    an = rng.uniform(-1, 1, n)
    out = np.zeros((n, 12), F32)
    for i in range(n):
        x, y, z = ax[i]
        Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        R = np.eye(3) + np.sin(an[i]) * Kx + (1 - np.cos(an[i])) * Kx @ Kx
        out[i, :9] = R.reshape(9)
        out[i, 9:] = rng.uniform(-10, 10, 3)
    return out


def big_case(seed=0, K=400, M=1000):
    """K = 400: a path of 70 keyframes from the origin (more levels than a wavefront has lanes), 300 children under
    the path's keyframe 10 (more than a workgroup's wavefronts can take one each), 10 more spread over the path, and
    20 unreachable slots (two of them parent and child).  About half the keyframes are in the adjustment.  M points
    over the four cases, some referring to unreachable slots."""
    rng = np.random.default_rng(seed)
    children = {k: [k + 1] for k in range(69)}
    children[10] = children[10] + list(range(70, 370))
    for j, c in enumerate(range(390, 400)):
        children[5 * j + 20] = children[5 * j + 20] + [c]
    children[370] = [371]
    off, idx = csr(children, K)
    flag = (rng.random(K) < 0.5).astype(np.uint8)
    flag[0] = 1
    m = dict(origins=np.array([0], np.int32), kf_child_off=off, kf_child_idx=idx, kf_in_gba=flag,
             kf_pose=random_pose(rng, K), kf_pose_gba=random_pose(rng, K), kf_pose_bef=random_pose(rng, K),
             mp_bad=(rng.random(M) < 0.15).astype(np.uint8), mp_in_gba=(rng.random(M) < 0.4).astype(np.uint8),
             mp_pos_gba=rng.uniform(-20, 20, (M, 3)).astype(F32), mp_ref_kf=rng.integers(0, K, M).astype(np.int32),
             mp_xw=rng.uniform(-20, 20, (M, 3)).astype(F32))
    m["mp_ref_kf"][:40] = rng.integers(370, 390, 40)
    return m


def tiny_case():
    """K = 1, M = 0."""
    z = lambda *s, dt=F32: np.zeros(s, dt)   # noqa: E731
    return dict(origins=np.array([0], np.int32), kf_child_off=np.zeros(2, np.int32), kf_child_idx=np.zeros(0, np.int32),
                kf_in_gba=np.array([1], np.uint8), kf_pose=np.array([RZ + [1, 2, 3]], F32),
                kf_pose_gba=np.array([EYE + [4, 5, 6]], F32), kf_pose_bef=z(1, 12), mp_bad=z(0, dt=np.uint8),
                mp_in_gba=z(0, dt=np.uint8), mp_pos_gba=z(0, 3), mp_ref_kf=z(0, dt=np.int32), mp_xw=z(0, 3))


UPDATED = ("kf_in_gba", "kf_pose", "kf_pose_gba", "kf_pose_bef", "mp_xw")


def same_bits(a, b):
    """The five updated arrays equal as bits."""
    for k in UPDATED:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return True
