"""CPU tier of the DBoW2 database (include/lvi_bow.h): the plain-Python restatement tests/bow_ref.py against
hand-computed answers, the behaviours of queryL1 that the library keeps on purpose, the host-only vocabulary model
csrc/lvi_bow_vocab.hpp compiled alone (plain and under the address and undefined-behaviour sanitizers) against the
restatement and against malformed files, and the signature table of the Python binding."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bow_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------------------------- the k=2, L=2 KAT
# Descriptors use the low 8 bits of word 0 only.  File order = children order.
#
#   root ── A 00000000 ── A0 00000001  word 2, weight 2.0
#        │             └─ A1 00000110  word 0, weight 1.0
#        └─ B 11111111 ── B0 01111111  word 3, weight 0   (stopped)
#                      └─ B1 11111100  word 1, weight 0.5
#
#   f1 00000001: A 1, B 7 -> A;  A0 0, A1 3 -> A0  word 2
#   f2 00000011: A 2, B 6 -> A;  A0 1, A1 2 -> A0  word 2
#   f3 00000111: A 3, B 5 -> A;  A0 2, A1 1 -> A1  word 0
#   f4 00001111: A 4, B 4 -> A (a tie: the first child stays);  A0 3, A1 2 -> A1  word 0
#   f5 11111111: A 8, B 0 -> B;  B0 1, B1 2 -> B0  word 3, weight 0: dropped
#   f6 11111110: A 7, B 1 -> B;  B0 2, B1 1 -> B1  word 1
#
#   TF_IDF vector of f1..f6: word 0: 1 + 1 = 2, word 1: 0.5, word 2: 2 + 2 = 4; sum 6.5 -> {0: 4/13, 1: 1/13, 2: 8/13}
#   IDF    vector of f1..f6: word 0: 1, word 1: 0.5, word 2: 2;       sum 3.5 -> {0: 2/7, 1: 1/7, 2: 4/7}
#   entry D = (f1, f6), TF_IDF: word 1: 0.5, word 2: 2; sum 2.5 -> {1: 0.2, 2: 0.8}
#   (the tree and the features are bow_ref.KAT_NODES, KAT_WORDS and KAT_FEATURES)
#   score(Q, D): word 1: |1/13 - 0.2| - 1/13 - 0.2 = -2/13; word 2: |8/13 - 0.8| - 8/13 - 0.8 = -16/13;
#                -0.5 (-18/13) = 9/13   (= the sum of min(q, d) over the common words)
KAT_FEATURES, KAT_WORD_IDS, KAT_WEIGHTS, kat_vocab = B.KAT_FEATURES, B.KAT_WORD_IDS, B.KAT_WEIGHTS, B.kat_vocab


def test_kat_words():
    voc = B.Vocabulary(kat_vocab())
    got = [voc.transform_one(f) for f in KAT_FEATURES]
    assert [g[0] for g in got] == KAT_WORD_IDS and [g[1] for g in got] == KAT_WEIGHTS


@pytest.mark.parametrize("weighting,want", [(B.TF_IDF, {0: 4 / 13, 1: 1 / 13, 2: 8 / 13}), (B.TF, {0: 4 / 13, 1: 1 / 13, 2: 8 / 13}),
                                            (B.IDF, {0: 2 / 7, 1: 1 / 7, 2: 4 / 7}), (B.BINARY, {0: 2 / 7, 1: 1 / 7, 2: 4 / 7})])
def test_kat_vector(weighting, want):
    v = B.Vocabulary(kat_vocab(weighting)).transform(KAT_FEATURES)
    assert sorted(v) == sorted(want)
    for w in want:
        assert abs(v[w] - want[w]) <= 4 * B.U


def test_kat_score():
    voc = B.Vocabulary(kat_vocab())
    db = B.Database(voc)
    assert db.add([KAT_FEATURES[0], KAT_FEATURES[5]]) == 0
    assert db.vectors[0] == {1: 0.2, 2: 0.8}
    ret = db.query(KAT_FEATURES, 4)
    assert len(ret) == 1 and ret[0][0] == 0 and abs(ret[0][1] - 9 / 13) <= B.score_bound(3)


# ------------------------------------------------------------------------------------------------------------- queryL1
@pytest.fixture(scope="module")
def small():
    data, nodes, words = B.make_vocab(11, 10, 3)
    return B.Vocabulary(data), B.leaf_descriptors(nodes, words)


def test_identical_vectors_score_one(small):
    voc, leaf = small
    f = B.ints(B.make_descriptors(np.random.default_rng(1), leaf, 300))
    db = B.Database(voc)
    db.add(f)
    (e, s), = db.query(f, 4)
    assert e == 0 and abs(s - 1.0) <= B.score_bound(len(db.vectors[0])) and len(db.vectors[0]) > 100


def test_disjoint_vectors_are_absent():
    voc = B.Vocabulary(kat_vocab())
    db = B.Database(voc)
    db.add([KAT_FEATURES[2]])                                            # word 0 only
    db.add([KAT_FEATURES[5]])                                            # word 1 only
    assert [e for e, _ in db.query([KAT_FEATURES[0]], 4)] == []          # word 2: shares nothing
    assert [e for e, _ in db.query([KAT_FEATURES[3]], 4)] == [0]


def test_max_id_quirks(small):
    """entry e takes part iff e < max_id || max_id == -1 || e == size - 1"""
    voc, leaf = small
    rng = np.random.default_rng(2)
    f = B.ints(B.make_descriptors(rng, leaf, 200))
    db = B.Database(voc)
    for i in range(6):
        g = list(f)
        g[:20 * i] = B.ints(B.make_descriptors(rng, leaf, 20 * i))
        db.add(g)
    ids = lambda max_id: sorted(e for e, _ in db.query(f, 32, max_id))  # noqa: E731
    assert ids(-1) == [0, 1, 2, 3, 4, 5]                                 # no limit (frame_index - 200 == -1 at frame 199)
    assert ids(-2) == [5] and ids(-100) == [5]                           # any other negative value: the newest entry alone
    assert ids(0) == [5]
    assert ids(3) == [0, 1, 2, 5]                                        # the newest entry is always eligible
    assert ids(6) == ids(1000) == [0, 1, 2, 3, 4, 5]
    assert [e for e, _ in db.query(f, 2, -1)] == [0, 1]                  # best first, cut to max_results


def test_empty_vector_entries():
    voc = B.Vocabulary(kat_vocab())
    db = B.Database(voc)
    assert db.add([]) == 0                                               # no features
    assert db.add([KAT_FEATURES[4]]) == 1                                # a stopped word only
    assert db.add([KAT_FEATURES[0]]) == 2
    assert db.vectors[0] == {} and db.vectors[1] == {} and db.nentries == 3
    (e, s), = db.query(KAT_FEATURES, 4)                                  # entry 2 = {2: 1}: min(8/13, 1)
    assert e == 2 and abs(s - 8 / 13) <= B.score_bound(3)
    assert db.query([], 4) == [] and db.query([KAT_FEATURES[4]], 4) == []


def test_equal_scores_come_in_ascending_id(small):
    voc, leaf = small
    f = B.ints(B.make_descriptors(np.random.default_rng(3), leaf, 100))
    db = B.Database(voc)
    for _ in range(3):
        db.add(f)
    ret = db.query(f, 4)
    assert [e for e, _ in ret] == [0, 1, 2] and ret[0][1] == ret[1][1] == ret[2][1]


def test_detect_loop_gates():
    """ret[0] > 0.05 and a later result > 0.015, frame_index > 50, and the min-index scan that takes ret[0] unconditionally"""
    class Fake:
        def __init__(self, ret):
            self.ret, self.voc = ret, self
        def transform(self, f): return {}                                # noqa: E704
        def query_vector(self, v, n, max_id): return self.ret            # noqa: E704
        def add_vector(self, v): return 0                                # noqa: E704
    assert B.detect_loop(Fake([(7, 0.06), (3, 0.016)]), [], 51)[0] == 3
    assert B.detect_loop(Fake([(7, 0.06), (3, 0.016)]), [], 50)[0] == -1
    assert B.detect_loop(Fake([(7, 0.05), (3, 0.016)]), [], 51)[0] == -1
    assert B.detect_loop(Fake([(7, 0.06), (3, 0.015)]), [], 51)[0] == -1
    assert B.detect_loop(Fake([(7, 0.06)]), [], 51)[0] == -1
    assert B.detect_loop(Fake([(7, 0.06), (3, 0.01), (9, 0.02)]), [], 51)[0] == 7      # 3 is below 0.015, 9 is not smaller
    assert B.detect_loop(Fake([(7, 0.06), (9, 0.02), (2, 0.016)]), [], 51)[0] == 2


# ------------------------------------------------------------------------------------------------------------- lvi_bow_vocab.hpp alone
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "lvi_bow_vocab.hpp"

// usage: driver vocab.bin [descriptors.bin]; exit 0 = accepted, 3 = invalid, 4 = unsupported
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    lvi_bowvoc::FlatVocab v;
    std::string err;
    const int st = lvi_bowvoc::load_vocab_file(argv[1], v, err);
    if (st != lvi_bowvoc::VOCAB_OK) {
        std::printf("rejected %d %s\n", st, err.c_str());
        return st == lvi_bowvoc::VOCAB_UNSUPPORTED ? 4 : 3;
    }
    std::printf("ok %d %d %d %d %d %d %d %d\n", v.k, v.L, v.scoring, v.weighting, v.n_nodes, v.n_words, v.max_depth, v.accumulates() ? 1 : 0);
    for (int f = 0; f < v.n_nodes; f++)
        std::printf("node %d %d %d %d\n", v.node_id[f], v.child_begin[f], v.child_count[f], v.word_id[f]);
    if (argc > 2) {
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        uint64_t d[4];
        while (std::fread(d, 8, 4, f) == 4) {
            int32_t w; double wt;
            lvi_bowvoc::transform_one(v, d, w, wt);
            std::printf("word %d %a\n", w, wt);
        }
        std::fclose(f);
    }
    return 0;
}
"""


def _build_driver(pkg, d, flags):
    d.mkdir(exist_ok=True)
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", *flags, "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", str(exe), str(d / "driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def drivers(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("bow_vocab")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


GOOD = [("kat", lambda: (kat_vocab(), None)), ("regular", lambda: B.make_vocab(21, 10, 3)[0:3]), ("irregular", lambda: B.make_vocab(22, 10, 4, irregular=True)[0:3]),
        ("wide", lambda: B.make_vocab(23, 17, 2, weighting=B.IDF)[0:3]), ("chain", lambda: B.make_vocab(24, 1, 3, weighting=B.BINARY)[0:3])]


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("name,make", GOOD, ids=[g[0] for g in GOOD])
def test_vocab_header_equals_the_restatement(drivers, tmp_path, which, name, make):
    """header fields, the children of every node in file order, the leaves' word ids, and transform(feature) of 300
    descriptors through the flattened tree"""
    got = make()
    data = got[0]
    (tmp_path / "v.bin").write_bytes(data)
    voc = B.Vocabulary(data)
    rng = np.random.default_rng(5)
    if name == "kat":
        desc = np.array([[f, 0, 0, 0] for f in KAT_FEATURES], np.uint64)
    else:
        leaf = B.leaf_descriptors(got[1], got[2])
        desc = np.concatenate([B.make_descriptors(rng, leaf, 250, max_flips=40), rng.integers(0, 2 ** 64, (50, 4), dtype=np.uint64)])
    (tmp_path / "d.bin").write_bytes(desc.tobytes())
    r = subprocess.run([drivers[which], str(tmp_path / "v.bin"), str(tmp_path / "d.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    head = [int(x) for x in lines[0].split()[1:]]
    nn = len(voc.children)
    depth = {0: 0}
    order, q = [], [0]                                                   # the flat numbering: breadth first from the root
    while q:
        n = q.pop(0)
        order.append(n)
        for c in voc.children[n]:
            depth[c] = depth[n] + 1
            q.append(c)
    max_depth = max(depth[n] for n in order if not voc.children[n])
    assert head == [voc.k, voc.L, voc.scoring, voc.weighting, nn, voc.n_words, max_depth, 1 if voc.weighting in (B.TF_IDF, B.TF) else 0]
    flat = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("node ")]
    assert [f[0] for f in flat] == order                                 # breadth first, children in file order
    for i, (nid, begin, count, wid) in enumerate(flat):
        assert [flat[begin + c][0] for c in range(count)] == voc.children[nid]
        assert wid == voc.word_id[nid] and (wid >= 0) == (count == 0)
    words = [ln.split()[1:] for ln in lines if ln.startswith("word ")]
    want = [voc.transform_one(f) for f in B.ints(desc)]
    assert [(int(w), float.fromhex(x)) for w, x in words] == want


def _patched(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def _malformed():
    """name -> (bytes, expected exit code): every file differs from a good one in one place"""
    data, nodes, words = B.make_vocab(31, 4, 2)
    nn = len(nodes)
    node_at = lambda i: 24 + 48 * i                                      # noqa: E731
    word_at = lambda i: 24 + 48 * nn + 8 * i                             # noqa: E731
    id_of = {int(r["nodeId"]): i for i, r in enumerate(nodes)}
    inner = next(i for i, r in enumerate(nodes) if int(r["parentId"]) == 0)
    child = next(i for i, r in enumerate(nodes) if int(r["parentId"]) == int(nodes[inner]["nodeId"]))
    out = {
        "truncated": data[:-5],
        "truncated_header": data[:20],
        "one_word_short": data[:-8],
        "trailing_bytes": data + b"\0" * 8,
        "negative_nodes": _patched(data, 16, "<i", -1),
        "negative_words": _patched(data, 20, "<i", -3),
        "huge_counts": _patched(_patched(data, 16, "<i", 2 ** 31 - 1), 20, "<i", 2 ** 31 - 1),
        "parent_out_of_range": _patched(data, node_at(3) + 4, "<i", nn + 1),
        "parent_negative": _patched(data, node_at(3) + 4, "<i", -1),
        "node_id_zero": _patched(data, node_at(2), "<i", 0),
        "node_id_out_of_range": _patched(data, node_at(2), "<i", nn + 1),
        "node_id_duplicated": _patched(data, node_at(2), "<i", int(nodes[5]["nodeId"])),
        # an inner node becomes the child of its own child: neither reaches the root any more
        "cycle": _patched(data, node_at(inner) + 4, "<i", int(nodes[child]["nodeId"])),
        "self_parent": _patched(data, node_at(inner) + 4, "<i", int(nodes[inner]["nodeId"])),
        # the first word now names the node of the second: one leaf without a word, one with two
        "leaf_without_word": _patched(data, word_at(0), "<i", int(words[1]["nodeId"])),
        "word_on_inner_node": _patched(data, word_at(0), "<i", int(nodes[inner]["nodeId"])),
        "word_node_out_of_range": _patched(data, word_at(0), "<i", nn + 7),
        "word_id_duplicated": _patched(data, word_at(0) + 4, "<i", int(words[1]["wordId"])),
        "word_id_out_of_range": _patched(data, word_at(0) + 4, "<i", len(words)),
        "weight_nan": _patched(data, node_at(1) + 8, "<d", float("nan")),
        "weight_inf": _patched(data, node_at(1) + 8, "<d", float("inf")),
        "weighting_unknown": _patched(data, 12, "<i", 4),
        "no_nodes": struct.pack("<6i", 10, 6, 0, 0, 0, 0),
    }
    # a leaf's record removed: an id beyond the new nNodes remains, in a node record or in the word that named the leaf
    keep = np.ones(nn, bool)
    keep[id_of[int(words[0]["nodeId"])]] = False
    out["missing_leaf_record"] = B.to_bytes(4, 2, nodes[keep], words)
    # a word record removed: a leaf is left without a word (or a word id reaches nWords)
    out["word_dropped"] = B.to_bytes(4, 2, nodes, words[1:])
    res = {k: (v, 3) for k, v in out.items()}
    res["scoring_l2"] = (_patched(data, 8, "<i", 1), 4)
    res["scoring_dot"] = (_patched(data, 8, "<i", 5), 4)
    return res


MALFORMED = _malformed()


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_vocabularies_are_rejected(drivers, tmp_path, which, name):
    data, code = MALFORMED[name]
    (tmp_path / "v.bin").write_bytes(data)
    r = subprocess.run([drivers[which], str(tmp_path / "v.bin")], capture_output=True, text=True)
    assert r.returncode == code and r.stdout.startswith("rejected") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------------- the binding
def test_vocab_reader_and_writer(pkg):
    data, nodes, words = B.make_vocab(41, 5, 2, weighting=B.IDF)
    assert (pkg.bow.NODE_DTYPE, pkg.bow.WORD_DTYPE) == (B.NODE_DTYPE, B.WORD_DTYPE)
    assert pkg.bow.write_vocab(5, 2, nodes, words, weighting=pkg.bow.IDF) == data
    head, n2, w2 = pkg.bow.read_vocab(data)
    assert head == dict(k=5, L=2, scoringType=0, weightingType=2, nNodes=len(nodes), nWords=len(words))
    assert np.array_equal(n2, nodes) and np.array_equal(w2, words)
    with pytest.raises(ValueError):
        pkg.bow.read_vocab(data[:-1])


def test_signature_table(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvi_bow.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(lvi_bow_[a-z0-9_]+)\s*\(", txt))) == sorted(pkg.bow.BOW_SIGNATURES)
    assert not set(pkg.bow.BOW_SIGNATURES) & set(pkg._abi.SIGNATURES)
    assert not set(pkg.bow.BOW_SIGNATURES) & set(pkg.kf.KF_SIGNATURES)
    assert all(n.startswith("lvi_bow_") for n in pkg.bow.BOW_SIGNATURES)
    kf = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvi_kf.h")).read(), flags=re.S)
    assert "lvi_bow" not in kf
