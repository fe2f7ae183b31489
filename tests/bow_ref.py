"""Plain-Python restatement of the DBoW2 lines behind LoopDetector::detectLoop (pose_graph/src/loop_detector.cpp:56-139):
the parity target of include/lvi_bow.h.  Unlike the OpenCV and PCL restatements of this project it is read
off the reference's own vendored source, line by line:

    Vocabulary.__init__      TemplatedVocabulary::loadBin                  TemplatedVocabulary.h:1509-1561 (VocabularyBinary.hpp)
    Vocabulary.transform_one transform(feature, word_id, weight)           TemplatedVocabulary.h:1217-1258
    Vocabulary.transform     transform(features, v)                        TemplatedVocabulary.h:1065-1121
    add_weight, add_if_not_exist, normalize_l1                             BowVector.cpp:34-84
    Database.add             TemplatedDatabase::add                        TemplatedDatabase.h:408-475
    Database.query           TemplatedDatabase::query / queryL1            TemplatedDatabase.h:607-723
    detect_loop              LoopDetector::detectLoop                      loop_detector.cpp:56-139

std::map is a dict iterated in sorted key order, a double is a Python float, and every sum runs left to right as the
std::map loops do.  A descriptor is a Python int of 256 bits (word i of the [4] uint64 layout at bits 64 i ..).

std::sort of the results compares the score alone, so the order of equal scores is unspecified in the reference; here (and
in the library, which documents it) they come in ascending entry id.

Also here: the writer of the VINSLoop layout and the seeded generators of synthetic vocabularies and keyframe sequences
(no vocabulary file is committed: tests build theirs into tmp_path)."""
import struct

import numpy as np

L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3

NODE_DTYPE = np.dtype([("nodeId", "<i4"), ("parentId", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])
WORD_DTYPE = np.dtype([("nodeId", "<i4"), ("wordId", "<i4")])

_M64 = (1 << 64) - 1


def to_int(d):
    """[4] uint64 -> 256-bit int"""
    return int(d[0]) | (int(d[1]) << 64) | (int(d[2]) << 128) | (int(d[3]) << 192)


def to_words(v):
    return np.array([(v >> (64 * i)) & _M64 for i in range(4)], np.uint64)


def ints(desc):
    """[n, 4] uint64 -> list of 256-bit ints"""
    return [to_int(r) for r in np.asarray(desc, np.uint64).reshape(-1, 4)]


_bit_count = getattr(int, "bit_count", None) or (lambda v: bin(v).count("1"))


def hamming(a, b):
    return _bit_count(a ^ b)                                            # FBrief::distance: (a ^ b).count()


def to_bytes(k, L, nodes, words, scoring=L1_NORM, weighting=TF_IDF):
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    words = np.ascontiguousarray(words, WORD_DTYPE)
    return struct.pack("<6i", k, L, scoring, weighting, len(nodes), len(words)) + nodes.tobytes() + words.tobytes()


# ------------------------------------------------------------------------------------------------------------- BowVector.cpp:34-84
def add_weight(v, wid, w):
    if wid in v:
        v[wid] += w
    else:
        v[wid] = w


def add_if_not_exist(v, wid, w):
    if wid not in v:
        v[wid] = w


def normalize_l1(v):
    norm = 0.0
    for wid in sorted(v):
        norm += abs(v[wid])
    if norm > 0.0:
        for wid in v:
            v[wid] /= norm


# ------------------------------------------------------------------------------------------------------------- the vocabulary
class Vocabulary:
    """loadBin as the reference runs it: it trusts the file (the library validates; these tests feed both the same
    well-formed files)"""

    def __init__(self, data):
        self.k, self.L, self.scoring, self.weighting, nn, nw = struct.unpack_from("<6i", data, 0)
        nodes = np.frombuffer(data, NODE_DTYPE, nn, 24)
        words = np.frombuffer(data, WORD_DTYPE, nw, 24 + 48 * nn)
        self.children = [[] for _ in range(nn + 1)]                     # m_nodes[pid].children.push_back(nid): file order
        self.weight = [0.0] * (nn + 1)
        self.desc = [0] * (nn + 1)
        self.word_id = [-1] * (nn + 1)
        for r in nodes:
            nid, pid = int(r["nodeId"]), int(r["parentId"])
            self.weight[nid] = float(r["weight"])
            self.desc[nid] = to_int(r["descriptor"])
            self.children[pid].append(nid)
        self.n_words = nw
        for r in words:
            self.word_id[int(r["nodeId"])] = int(r["wordId"])

    def transform_one(self, feature):
        final_id = 0
        while True:
            nodes = self.children[final_id]
            final_id = nodes[0]
            best_d = hamming(feature, self.desc[final_id])
            for nid in nodes[1:]:
                d = hamming(feature, self.desc[nid])
                if d < best_d:
                    best_d = d
                    final_id = nid
            if not self.children[final_id]:                             # isLeaf
                break
        return self.word_id[final_id], self.weight[final_id]

    def transform(self, features):
        """-> the BowVector as a dict word id -> value.  With L1 scoring mustNormalize is always true, so the TF branch's
        division by v.size() never runs."""
        assert self.scoring == L1_NORM
        v = {}
        if self.weighting in (TF, TF_IDF):
            for f in features:
                wid, w = self.transform_one(f)
                if w > 0:
                    add_weight(v, wid, w)
        else:
            for f in features:
                wid, w = self.transform_one(f)
                if w > 0:
                    add_if_not_exist(v, wid, w)
        normalize_l1(v)
        return v


# ------------------------------------------------------------------------------------------------------------- the database
class Database:
    def __init__(self, voc):
        self.voc = voc
        self.ifile = [[] for _ in range(voc.n_words)]                   # m_ifile[word] = [(entry_id, word_weight)], ascending entry
        self.nentries = 0
        self.vectors = []                                               # not in the reference (use_di = false): kept for the tests

    def add(self, features):
        return self.add_vector(self.voc.transform(features))

    def add_vector(self, v):
        entry_id = self.nentries
        self.nentries += 1
        for wid in sorted(v):
            self.ifile[wid].append((entry_id, v[wid]))
        self.vectors.append(dict(v))
        return entry_id

    def query_vector_all(self, vec, max_id=-1):
        """queryL1 up to and including the sort, and the final scaling: every entry that shares a word, best first"""
        pairs = {}
        for wid in sorted(vec):
            qvalue = vec[wid]
            for entry_id, dvalue in self.ifile[wid]:
                if entry_id < max_id or max_id == -1 or entry_id == self.nentries - 1:
                    value = abs(qvalue - dvalue) - abs(qvalue) - abs(dvalue)
                    if entry_id in pairs:
                        pairs[entry_id] += value
                    else:
                        pairs[entry_id] = value
        ret = sorted(((pairs[e], e) for e in sorted(pairs)))              # ascending raw score (the lower the better), ties by id
        return [(e, -s / 2.0) for s, e in ret]

    def query_vector(self, vec, max_results, max_id=-1):
        ret = self.query_vector_all(vec, max_id)
        if max_results > 0 and len(ret) > max_results:
            ret = ret[:max_results]
        return ret

    def query(self, features, max_results, max_id=-1):
        """-> [(entry id, score)], best first"""
        return self.query_vector(self.voc.transform(features), max_results, max_id)


def detect_loop(db, features, frame_index):
    """LoopDetector::detectLoop without the DEBUG_IMAGE code -> (loop index or -1, the query's results)"""
    vec = db.voc.transform(features)
    ret = db.query_vector(vec, 4, frame_index - 200)
    db.add_vector(vec)                                                  # the reference transforms again: the same vector
    find_loop = False
    if len(ret) >= 1 and ret[0][1] > 0.05:
        for i in range(1, len(ret)):
            if ret[i][1] > 0.015:
                find_loop = True
    if find_loop and frame_index > 50:
        min_index = -1
        for e, s in ret:
            if min_index == -1 or (e < min_index and s > 0.015):
                min_index = e
        return min_index, ret
    return -1, ret


# ------------------------------------------------------------------------------------------------------------- tolerances
U = 2.0 ** -53


def value_bound(n):
    """relative bound on a normalised value when the sums of n words run in another order"""
    return n * U


def score_bound(n):
    """absolute bound on a score between vectors of at most n words"""
    return 8 * n * U


# ------------------------------------------------------------------------------------------------------------- the k=2, L=2 known-answer tree
# worked out in the comments of tests/test_bow_ref.py: (nodeId, parentId, weight, low 8 bits of descriptor word 0), (nodeId, wordId)
KAT_NODES = [(1, 0, 0.0, 0b00000000), (2, 0, 0.0, 0b11111111), (3, 1, 2.0, 0b00000001), (4, 1, 1.0, 0b00000110), (5, 2, 0.0, 0b01111111),
             (6, 2, 0.5, 0b11111100)]
KAT_WORDS = [(3, 2), (4, 0), (5, 3), (6, 1)]
KAT_FEATURES = [0b00000001, 0b00000011, 0b00000111, 0b00001111, 0b11111111, 0b11111110]
KAT_WORD_IDS = [2, 2, 0, 0, 3, 1]
KAT_WEIGHTS = [2.0, 2.0, 1.0, 1.0, 0.0, 0.5]


def kat_vocab(weighting=TF_IDF, scoring=L1_NORM):
    nodes = np.zeros(len(KAT_NODES), NODE_DTYPE)
    for i, (nid, pid, w, d) in enumerate(KAT_NODES):
        nodes[i] = (nid, pid, w, [d, 0, 0, 0])
    words = np.array(KAT_WORDS, WORD_DTYPE)
    return to_bytes(2, 2, nodes, words, scoring, weighting)


# ------------------------------------------------------------------------------------------------------------- generators
def flip(d, bits):
    for b in bits:
        d ^= 1 << int(b)
    return d


def make_vocab(seed, k, L, weighting=TF_IDF, irregular=False, dup=0.1, stopped=0.05):
    """A seeded synthetic vocabulary -> (file bytes, nodes, words).  A child is its parent with some bits flipped (the
    first level is random); `irregular` gives some nodes fewer children and turns some inner nodes into leaves above level
    L; a share `dup` of the children copy their previous sibling's descriptor, so that descents meet ties; a share
    `stopped` of the words has weight 0, the others positive reals.  Node ids, the file order of the node records (which
    is the children's order), word ids and the order of the word records are all shuffled."""
    rng = np.random.default_rng(seed)
    recs = []                                                           # (parent index in recs or -1, descriptor int, level)
    frontier = [(-1, 0, 0)]
    leaves = []
    while frontier:
        nxt = []
        for idx, desc, lvl in frontier:
            nch = k
            if irregular and idx >= 0:
                r = rng.random()
                if r < 0.15:
                    nch = 0
                elif r < 0.45:
                    nch = int(rng.integers(1, k + 1))
            if lvl == L or nch == 0:
                leaves.append(idx)
                continue
            prev = None
            for c in range(nch):
                if lvl == 0:
                    d = to_int(rng.integers(0, 2 ** 64, 4, dtype=np.uint64))
                else:
                    d = flip(desc, rng.choice(256, max(6, 64 >> lvl), replace=False))
                if prev is not None and rng.random() < dup:
                    d = prev
                prev = d
                recs.append((idx, d, lvl + 1))
                nxt.append((len(recs) - 1, d, lvl + 1))
        frontier = nxt
    nn = len(recs)
    node_id = rng.permutation(nn) + 1                                    # recs index -> nodeId
    nodes = np.zeros(nn, NODE_DTYPE)
    leaf_set = set(leaves)
    for i, (par, d, _lvl) in enumerate(recs):
        w = 0.0
        if i in leaf_set:
            w = 0.0 if rng.random() < stopped else float(rng.uniform(0.25, 9.0))
        nodes[i] = (node_id[i], 0 if par < 0 else node_id[par], w, to_words(d))
    nodes = nodes[rng.permutation(nn)]
    words = np.zeros(len(leaves), WORD_DTYPE)
    words["nodeId"] = node_id[np.array(leaves, np.int64)]
    words["wordId"] = rng.permutation(len(leaves))
    words = words[rng.permutation(len(leaves))]
    return to_bytes(k, L, nodes, words, L1_NORM, weighting), nodes, words


def leaf_descriptors(nodes, words):
    by_id = {int(r["nodeId"]): r["descriptor"] for r in nodes}
    return np.array([by_id[int(n)] for n in words["nodeId"]], np.uint64)


def make_descriptors(rng, leaf_desc, n, max_flips=6):
    """n descriptors [n, 4] uint64 near random leaves of the vocabulary"""
    out = np.zeros((n, 4), np.uint64)
    for i in range(n):
        d = to_int(leaf_desc[int(rng.integers(len(leaf_desc)))])
        out[i] = to_words(flip(d, rng.choice(256, int(rng.integers(0, max_flips + 1)), replace=False)))
    return out


def make_sequence(seed, leaf_desc, n_desc=200, n_places=230, shared=0.3, revisit=(5, 35), replaced=0.2, bits=4):
    """The keyframes of a loop: n_places places, each sharing a part of its descriptors with its predecessor, then revisits
    of places revisit[0] .. revisit[1]-1 with a share of the descriptors replaced and `bits` bits flipped in each
    -> list of [n_desc, 4] uint64"""
    rng = np.random.default_rng(seed)
    frames = []
    for p in range(n_places):
        d = make_descriptors(rng, leaf_desc, n_desc)
        if p > 0:
            keep = rng.choice(n_desc, int(shared * n_desc), replace=False)
            d[keep] = frames[-1][keep]
        frames.append(d)
    for p in range(*revisit):
        d = frames[p].copy()
        rep = rng.choice(n_desc, int(replaced * n_desc), replace=False)
        d[rep] = make_descriptors(rng, leaf_desc, len(rep))
        for i in range(n_desc):
            d[i] = to_words(flip(to_int(d[i]), rng.choice(256, bits, replace=False)))
        frames.append(d)
    return frames
