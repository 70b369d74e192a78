"""KeyFrameDatabase mirror (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:34-265) over the gfx950 C-ABI
(orbdb_*, include/orbslam2_amd.h): a device-resident database of BowVectors on slots, add / erase / clear,
DetectLoopCandidates and DetectRelocalizationCandidates batched over query frames, and the minScore loop of
LoopDetector::Detect (src/LoopClosing.cc:170-178) as MinScore.

BowVectors travel in orbv_transform_batch_device's layout: bow_word (F, cap) int32 / uint32, bow_weight (F, cap)
float64, n_words (F,) int32.  The `_device` forms take and return CUDA tensors and only enqueue; the others take
numpy arrays and are synchronous."""
import ctypes as C

import numpy as np

from ._lib import OrbdbQueryBatch, OrbdbResult, check, lib, ptr, stream_ptr, tptr

COVIS = 10
_OUT = (("cand", np.int32), ("words", np.int32), ("scored", np.uint8), ("score", np.float32), ("acc", np.float32),
        ("bestk", np.int32))


def _host(a, dtype, name, shape=None):
    if a is None:
        raise ValueError(f"{name} is required")
    a = np.ascontiguousarray(a)
    if dtype == np.uint32 and a.dtype == np.int32:
        a = a.view(np.uint32)
    if a.dtype != dtype:
        raise ValueError(f"{name} must be {np.dtype(dtype).name}, not {a.dtype.name}")
    if shape is not None and (a.ndim != len(shape) or any(s is not None and s != t for s, t in zip(shape, a.shape))):
        raise ValueError(f"{name} must have shape {shape}, not {a.shape}")
    return a


def _dev(t, dtype, name, shape=None):
    import torch
    if t is None:
        raise ValueError(f"{name} is required")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor")
    if shape is not None and (t.dim() != len(shape) or any(s is not None and s != u for s, u in zip(shape, t.shape))):
        raise ValueError(f"{name} must have shape {shape}, not {tuple(t.shape)}")
    return t


def _idx_dev(t, name):
    """A CSR index tensor; an empty one still needs an address."""
    import torch
    t = _dev(t, torch.int32, name, (None,))
    return t if t.numel() else torch.zeros(1, dtype=torch.int32, device=t.device)


class KeyFrameDatabase:
    def __init__(self, vocabulary, max_keyframes: int, word_cap: int, device: int = None):
        self.device = vocabulary.device if device is None else device
        self.max_keyframes, self.word_cap = int(max_keyframes), int(word_cap)
        h = C.c_void_p()
        check(lib().orbdb_create(vocabulary._h, self.max_keyframes, self.word_cap, self.device, C.byref(h)), "orbdb_create")
        self._h = h
        self._voc = vocabulary   # the reference keeps a pointer to it

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orbdb_destroy(self._h)
            self._h = None

    # ---- host forms
    def _bow_host(self, bow_word, bow_weight, n_words):
        n_words = _host(n_words, np.int32, "n_words", (None,))
        F = len(n_words)
        bow_word = _host(bow_word, np.uint32, "bow_word", (F, None))
        bow_weight = _host(bow_weight, np.float64, "bow_weight", (F, bow_word.shape[1]))
        return bow_word, bow_weight, n_words, F, max(int(bow_word.shape[1]), 1)

    def add(self, slot, bow_word, bow_weight, n_words, frame=None):
        """add(KeyFrame*) for the keyframes `slot`: slot[i] takes the BowVector of frame frame[i] (None: i)."""
        slot = _host(slot, np.int32, "slot", (None,))
        bw, bv, nw, F, cap = self._bow_host(bow_word, bow_weight, n_words)
        fr = None if frame is None else _host(frame, np.int32, "frame", (len(slot),))
        check(lib().orbdb_add(self._h, len(slot), ptr(slot), None if fr is None else ptr(fr), ptr(bw), ptr(bv), ptr(nw), cap, F),
              "orbdb_add")

    def erase(self, slot):
        slot = np.atleast_1d(slot)
        slot = _host(slot.astype(np.int32) if slot.dtype.kind in "iu" else slot, np.int32, "slot", (None,))
        check(lib().orbdb_erase(self._h, len(slot), ptr(slot)), "orbdb_erase")

    def clear(self, stream=None):
        check(lib().orbdb_clear(self._h, stream_ptr(stream)), "orbdb_clear")

    def slots(self):
        """(live (K,) uint8, reloc_score (K,) float32), synchronous."""
        live, rs = np.zeros(self.max_keyframes, np.uint8), np.zeros(self.max_keyframes, np.float32)
        check(lib().orbdb_read_slots(self._h, ptr(live), ptr(rs)), "orbdb_read_slots")
        return live, rs

    def _query_host(self, q, keep, covis=True):
        bw, bv, nw, F, cap = self._bow_host(q["bow_word"], q["bow_weight"], q["n_words"])
        fr = q.get("frame")
        fr = None if fr is None else _host(fr, np.int32, "frame", (None,))
        Q = F if fr is None else len(fr)
        b = OrbdbQueryBatch(Q, cap, F, ptr(bw).value, ptr(bv).value, ptr(nw).value, None if fr is None else ptr(fr).value)
        keep += [bw, bv, nw, fr]
        if covis:
            cv = _host(q.get("covis"), np.int32, "covis", (self.max_keyframes, COVIS))
            keep.append(cv)
            b.covis = ptr(cv).value
        return b, Q

    def _csr_host(self, off, idx, Q, name, keep):
        off = _host(off, np.int32, name + "_off", (Q + 1,))
        idx = _host(np.zeros(0, np.int32) if idx is None else idx, np.int32, name + "_idx", (None,))
        if Q >= 0 and len(off) and int(off[-1]) > len(idx):
            raise ValueError(f"{name}_idx is shorter than {name}_off[-1]")
        keep += [off, idx]
        return ptr(off).value, ptr(idx).value if len(idx) else None

    def _result_host(self, Q):
        K = self.max_keyframes
        out = {k: np.zeros((Q, K), dt) for k, dt in _OUT}
        out["n_cand"] = np.zeros(Q, np.int32)
        r = OrbdbResult(*[ptr(out[k]).value if Q else None for k in ("cand", "n_cand", "words", "scored", "score", "acc", "bestk")])
        return out, r

    def DetectRelocalizationCandidates(self, query):
        """query: dict(bow_word, bow_weight, n_words, frame=None, covis).  Returns dict(cand (Q, K) ascending slots, -1 padded,
        n_cand (Q,), words, scored, score, acc, bestk (Q, K))."""
        keep = []
        b, Q = self._query_host(query, keep)
        out, r = self._result_host(Q)
        check(lib().orbdb_detect_reloc(self._h, C.byref(b), C.byref(r)), "orbdb_detect_reloc")
        return out

    def DetectLoopCandidates(self, query, min_score):
        """query as above plus conn_off (Q + 1,), conn_idx: GetConnectedKeyFrames() as slots; min_score (Q,) float32."""
        keep = []
        b, Q = self._query_host(query, keep)
        b.conn_off, b.conn_idx = self._csr_host(query.get("conn_off"), query.get("conn_idx"), Q, "conn", keep)
        ms = _host(min_score, np.float32, "min_score", (Q,))
        b.min_score = ptr(ms).value
        out, r = self._result_host(Q)
        check(lib().orbdb_detect_loop(self._h, C.byref(b), C.byref(r)), "orbdb_detect_loop")
        return out

    def MinScore(self, query, cov_off, cov_idx):
        """Detect's minScore per query over its covisible slots (CSR)."""
        keep = []
        b, Q = self._query_host(query, keep, covis=False)
        off, idx = self._csr_host(cov_off, cov_idx, Q, "cov", keep)
        ms = np.zeros(Q, np.float32)
        check(lib().orbdb_min_score(self._h, C.byref(b), off, idx, ptr(ms)), "orbdb_min_score")
        return ms

    # ---- device forms
    def _bow_device(self, bow_word, bow_weight, n_words):
        import torch
        n_words = _dev(n_words, torch.int32, "n_words", (None,))
        F = int(n_words.shape[0])
        bow_word = _dev(bow_word, torch.int32, "bow_word", (F, None))
        bow_weight = _dev(bow_weight, torch.float64, "bow_weight", (F, int(bow_word.shape[1])))
        return bow_word, bow_weight, n_words, F, max(int(bow_word.shape[1]), 1)

    def add_device(self, slot, bow_word, bow_weight, n_words, frame=None, stream=None):
        """slot (n,) int32 CUDA; the BoW arrays are an orbv_transform_batch_device output (used in place)."""
        import torch
        slot = _dev(slot, torch.int32, "slot", (None,))
        bw, bv, nw, F, cap = self._bow_device(bow_word, bow_weight, n_words)
        fr = None if frame is None else _dev(frame, torch.int32, "frame", (int(slot.shape[0]),))
        check(lib().orbdb_add_device(self._h, int(slot.shape[0]), tptr(slot), None if fr is None else tptr(fr), tptr(bw), tptr(bv),
                                     tptr(nw), cap, F, stream_ptr(stream)), "orbdb_add_device")

    def erase_device(self, slot, stream=None):
        import torch
        slot = _dev(slot, torch.int32, "slot", (None,))
        check(lib().orbdb_erase_device(self._h, int(slot.shape[0]), tptr(slot), stream_ptr(stream)), "orbdb_erase_device")

    def _query_device(self, q, covis=True):
        import torch
        bw, bv, nw, F, cap = self._bow_device(q["bow_word"], q["bow_weight"], q["n_words"])
        fr = q.get("frame")
        fr = None if fr is None else _dev(fr, torch.int32, "frame", (None,))
        Q = F if fr is None else int(fr.shape[0])
        b = OrbdbQueryBatch(Q, cap, F, bw.data_ptr(), bv.data_ptr(), nw.data_ptr(), None if fr is None else fr.data_ptr())
        if covis:
            b.covis = _dev(q.get("covis"), torch.int32, "covis", (self.max_keyframes, COVIS)).data_ptr()
        return b, Q, bw.device

    def _result_device(self, Q, dev, out, extras):
        import torch
        K = self.max_keyframes
        tt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
        if out is None:
            out = {k: torch.empty((Q, K), dtype=tt[dt], device=dev) for k, dt in _OUT if extras or k == "cand"}
            out["n_cand"] = torch.empty(Q, dtype=torch.int32, device=dev)
        r = OrbdbResult(*[out[k].data_ptr() if k in out else None for k in ("cand", "n_cand", "words", "scored", "score", "acc", "bestk")])
        return out, r

    def detect_relocalization_candidates_device(self, query, out=None, extras=True, stream=None):
        b, Q, dev = self._query_device(query)
        out, r = self._result_device(Q, dev, out, extras)
        check(lib().orbdb_detect_reloc_device(self._h, C.byref(b), C.byref(r), stream_ptr(stream)), "orbdb_detect_reloc_device")
        return out

    def detect_loop_candidates_device(self, query, min_score, out=None, extras=True, stream=None):
        import torch
        b, Q, dev = self._query_device(query)
        b.conn_off = _dev(query.get("conn_off"), torch.int32, "conn_off", (Q + 1,)).data_ptr()
        conn_idx = _idx_dev(query.get("conn_idx"), "conn_idx")
        b.conn_idx = conn_idx.data_ptr()
        b.min_score = _dev(min_score, torch.float32, "min_score", (Q,)).data_ptr()
        out, r = self._result_device(Q, dev, out, extras)
        check(lib().orbdb_detect_loop_device(self._h, C.byref(b), C.byref(r), stream_ptr(stream)), "orbdb_detect_loop_device")
        return out

    def min_score_device(self, query, cov_off, cov_idx, out=None, stream=None):
        import torch
        b, Q, dev = self._query_device(query, covis=False)
        off = _dev(cov_off, torch.int32, "cov_off", (Q + 1,))
        idx = _idx_dev(cov_idx, "cov_idx")
        if out is None:
            out = torch.empty(Q, dtype=torch.float32, device=dev)
        check(lib().orbdb_min_score_device(self._h, C.byref(b), tptr(off), tptr(idx), tptr(out), stream_ptr(stream)),
              "orbdb_min_score_device")
        return out
