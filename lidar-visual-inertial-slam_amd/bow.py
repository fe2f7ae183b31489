"""Python handle over include/lvi_bow.h: the pose graph's DBoW2 keyframe database on the GPU — db.query and db.add of
LoopDetector::detectLoop (pose_graph/src/loop_detector.cpp:56-139) over the keyframe store of kf.KeyframeDescriber; a
restatement of the reference's vendored DBoW2, DESIGN §15.

A separate ABI from include/lvi_hotpath.h and include/lvi_kf.h: only the product library exports it, so its signature
table lives here and is bound against ``liblvi_hip.so`` alone.

The vocabulary is the VINSLoop binary layout (ThirdParty/VocabularyBinary.hpp); no vocabulary ships with the project.
``read_vocab`` / ``write_vocab`` move it between bytes and numpy structured arrays."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

MAX_RESULTS = 32
L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3

HEADER_DTYPE = np.dtype([("k", "<i4"), ("L", "<i4"), ("scoringType", "<i4"), ("weightingType", "<i4"), ("nNodes", "<i4"), ("nWords", "<i4")])
NODE_DTYPE = np.dtype([("nodeId", "<i4"), ("parentId", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])
WORD_DTYPE = np.dtype([("nodeId", "<i4"), ("wordId", "<i4")])
RESULT_DTYPE = np.dtype([("entry_id", "<i4"), ("reserved", "<i4"), ("score", "<f8")])
assert (HEADER_DTYPE.itemsize, NODE_DTYPE.itemsize, WORD_DTYPE.itemsize, RESULT_DTYPE.itemsize) == (24, 48, 8, 16)

# name -> (restype, argtypes), one entry per function of include/lvi_bow.h
BOW_SIGNATURES = {
    "lvi_bow_abi_version": (_i32, []),
    "lvi_bow_create": (_i32, [_vp, _vp, _i64, _i32, _P(_vp)]),
    "lvi_bow_destroy": (None, [_vp]),
    "lvi_bow_size": (_i32, [_vp]),
    "lvi_bow_query": (_i32, [_vp, _i32, _i32, _i32, _vp, _P(_i32)]),
    "lvi_bow_add": (_i32, [_vp, _i32, _P(_i32)]),
    "lvi_bow_words": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "lvi_bow_get_entry": (_i32, [_vp, _i32, _P(_i32), _vp, _vp]),
}


def bind(lib):
    """set the database signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(BOW_SIGNATURES)


def write_vocab(k, L, nodes, words, scoring=L1_NORM, weighting=TF_IDF):
    """the file's bytes: nodes = NODE_DTYPE array in file order (it decides the children's order), words = WORD_DTYPE array"""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    words = np.ascontiguousarray(words, WORD_DTYPE)
    head = np.array([(k, L, scoring, weighting, len(nodes), len(words))], HEADER_DTYPE)
    return head.tobytes() + nodes.tobytes() + words.tobytes()


def read_vocab(src):
    """bytes or a path -> (header dict, nodes, words); checks the size only: the library validates the tree"""
    if not isinstance(src, (bytes, bytearray, memoryview)):
        with open(src, "rb") as f:
            src = f.read()
    src = bytes(src)
    if len(src) < HEADER_DTYPE.itemsize:
        raise ValueError("vocabulary shorter than its header")
    head = np.frombuffer(src, HEADER_DTYPE, 1)[0]
    nn, nw = int(head["nNodes"]), int(head["nWords"])
    if nn < 0 or nw < 0 or len(src) != 24 + 48 * nn + 8 * nw:
        raise ValueError("vocabulary size does not match its node and word counts")
    nodes = np.frombuffer(src, NODE_DTYPE, nn, 24).copy()
    words = np.frombuffer(src, WORD_DTYPE, nw, 24 + 48 * nn).copy()
    return {n: int(head[n]) for n in HEADER_DTYPE.names}, nodes, words


class BowDatabase(A.Owned):
    """BriefDatabase of the reference's LoopDetector on the GPU of `store` (a kf.KeyframeDescriber, which must outlive it).
    vocab = the file's bytes or its path."""
    _destroy = "lvi_bow_destroy"

    def __init__(self, lib, store, vocab, max_entries=4096):
        self.lib = bind(lib)
        self.store = store
        if not isinstance(vocab, (bytes, bytearray, memoryview)):
            with open(vocab, "rb") as f:
                vocab = f.read()
        buf = np.frombuffer(bytes(vocab), np.uint8)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_bow_create(store._h, C.c_void_p(buf.ctypes.data) if buf.size else None, buf.size, int(max_entries), C.byref(self._h)),
                  "lvi_bow_create")
        self.max_entries = int(max_entries)

    def __len__(self):
        return int(self.lib.dll.lvi_bow_size(self._h))

    def query(self, slot, max_results=4, max_id=-1):
        """db.query(kp descriptors of slot, ret, max_results, max_id) -> (entry ids int32 [n], scores float64 [n]), best first"""
        out = np.zeros(MAX_RESULTS, RESULT_DTYPE)
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_bow_query(self._h, int(slot), int(max_results), int(max_id), A._ptr(out), C.byref(n)), "lvi_bow_query")
        return out["entry_id"][:n.value].copy(), out["score"][:n.value].copy()

    def add(self, slot):
        """db.add(kp descriptors of slot) -> the entry id"""
        e = C.c_int32(-1)
        self.lib.check(self.lib.dll.lvi_bow_add(self._h, int(slot), C.byref(e)), "lvi_bow_add")
        return e.value

    def words(self, desc):
        """transform(feature, id, weight) per descriptor: desc [n, 4] uint64 -> (word ids int32 [n], weights float64 [n])"""
        d = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
        w = np.full(max(len(d), 1), -1, np.int32); v = np.zeros(max(len(d), 1), np.float64)
        self.lib.check(self.lib.dll.lvi_bow_words(self._h, A._ptr(d), len(d), A._ptr(w), A._ptr(v)), "lvi_bow_words")
        return w[:len(d)].copy(), v[:len(d)].copy()

    def entry(self, entry_id=-1):
        """the BowVector of an entry (-1: of the last query or add) -> (word ids int32 [m] ascending, values float64 [m])"""
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_bow_get_entry(self._h, int(entry_id), C.byref(n), None, None), "lvi_bow_get_entry")
        w = np.zeros(max(n.value, 1), np.int32); v = np.zeros(max(n.value, 1), np.float64)
        self.lib.check(self.lib.dll.lvi_bow_get_entry(self._h, int(entry_id), C.byref(n), A._ptr(w), A._ptr(v)), "lvi_bow_get_entry")
        return w[:n.value].copy(), v[:n.value].copy()
