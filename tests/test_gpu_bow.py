"""GPU tier of the DBoW2 database (include/lvi_bow.h) against the plain-Python restatement tests/bow_ref.py.

Word ids, counts, entry ids, result order and loop indices are compared exactly.  Values and scores are compared within
the bounds derived in DESIGN §15 (bow_ref.value_bound / score_bound): with u = 2^-53 and n the larger word count of the two
vectors, a differently ordered double sum moves a normalised value by at most n u relative and a score by at most 8 n u
absolute.  Because ids and decisions are compared exactly, the query and sequence tests first assert on the restatement
alone that no two adjacent scores among the first max_results + 1 come closer than 1e-9 and that no compared score lies
within 1e-9 of a threshold: a seed that violates this is a bug of the test's inputs.

Keyframes enter through lvi_kf_put with synthetic descriptors, so no images are involved."""
import ctypes as C
import os

import numpy as np
import pytest

import bow_ref as B
import kfdesc_ref as R
from bow_ref import KAT_FEATURES, KAT_WEIGHTS, KAT_WORD_IDS, kat_vocab

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = 1024                                                                 # max_keypoints of the shared store
GAP = 1e-9


@pytest.fixture(scope="module")
def pattern(pkg):
    return pkg.config.load_brief_pattern(os.path.join(HERE, "golden", "brief_pattern.yml"))


@pytest.fixture(scope="module")
def store(pkg, hip, pattern):
    h = pkg.KeyframeDescriber(hip, pattern, max_width=32, max_height=32, max_keypoints=K, max_window=8, max_keyframes=6)
    yield h
    h.close()


def _make(name):
    if name == "kat":
        return kat_vocab(), None, None
    if name == "regular":
        return B.make_vocab(21, 10, 3)
    if name == "irregular":
        return B.make_vocab(22, 10, 4, irregular=True)
    if name == "wide":                                                   # more children than the 16 lanes of a group
        return B.make_vocab(23, 17, 2)
    return B.make_vocab(24, 1, 3)                                        # "chain": one child per node


VOCABS = ["kat", "regular", "irregular", "wide", "chain"]


@pytest.fixture(scope="module")
def vocabs(pkg, hip, store):
    """name -> (restatement vocabulary, leaf descriptors, nodes, database handle), built once"""
    out = {}
    for name in VOCABS:
        data, nodes, words = _make(name)
        leaf = B.leaf_descriptors(nodes, words) if nodes is not None else None
        out[name] = (B.Vocabulary(data), leaf, nodes, pkg.BowDatabase(hip, store, data, max_entries=4))
    yield out
    for v in out.values():
        v[3].close()


def _tie_descriptors(voc, rng, n):
    """descriptors that meet a tie on their way down: copies of a child whose descriptor a sibling shares (distance 0 to
    both), and midpoints between two siblings (half of the differing bits taken from each)"""
    out = []
    for kids in voc.children:
        for a, b in zip(kids, kids[1:]):
            da, db = voc.desc[a], voc.desc[b]
            if da == db:
                out.append(da)
            else:
                diff = [i for i in range(256) if (da ^ db) >> i & 1]
                if len(diff) % 2 == 0:
                    out.append(B.flip(da, diff[:len(diff) // 2]))
    idx = rng.permutation(len(out))[:n]
    return np.array([B.to_words(out[i]) for i in idx], np.uint64).reshape(-1, 4)


def _descriptors(name, voc, leaf, n, seed):
    rng = np.random.default_rng(seed)
    if name == "kat":
        return np.array([[KAT_FEATURES[i % 6], 0, 0, 0] for i in range(n)], np.uint64).reshape(-1, 4)
    ties = _tie_descriptors(voc, rng, n // 4)
    rest = n - len(ties)
    near = B.make_descriptors(rng, leaf, rest - rest // 5, max_flips=40)
    noise = rng.integers(0, 2 ** 64, (rest // 5, 4), dtype=np.uint64)
    d = np.concatenate([ties, near, noise])
    return d[rng.permutation(len(d))]


# ------------------------------------------------------------------------------------------------------------- words
def test_vocabularies_have_ties(vocabs):
    for name in ("regular", "irregular", "wide"):
        voc = vocabs[name][0]
        assert any(voc.desc[a] == voc.desc[b] for kids in voc.children for a, b in zip(kids, kids[1:])), name
        assert len(_tie_descriptors(voc, np.random.default_rng(0), 10 ** 6)) > 20
    assert max(len(c) for c in vocabs["wide"][0].children) == 17 and max(len(c) for c in vocabs["chain"][0].children) == 1
    irr = vocabs["irregular"][0]
    assert len({len(c) for c in irr.children}) > 3 and irr.n_words < 10 ** 4


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", VOCABS)
def test_words_are_exact(vocabs, name, n):
    voc, leaf, _, db = vocabs[name]
    d = _descriptors(name, voc, leaf, n, 100 + n)
    assert len(d) == n
    wid, wt = db.words(d)
    want = [voc.transform_one(f) for f in B.ints(d)]
    assert wid.tolist() == [w for w, _ in want]
    assert wt.tolist() == [x for _, x in want]
    if name == "kat" and n >= 6:
        assert wid[:6].tolist() == KAT_WORD_IDS and wt[:6].tolist() == KAT_WEIGHTS


# ------------------------------------------------------------------------------------------------------------- vectors
def _check_vector(got, want):
    """word ids exact, values within n u relative"""
    gw, gv = got
    assert gw.tolist() == sorted(want)
    n = len(want)
    for w, v in zip(gw.tolist(), gv.tolist()):
        assert abs(v - want[w]) <= B.value_bound(n) * abs(want[w]), (w, v, want[w])


@pytest.mark.parametrize("weighting", [B.TF_IDF, B.TF, B.IDF, B.BINARY])
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_vectors(pkg, hip, store, weighting, n):
    data, nodes, words = B.make_vocab(21, 10, 3, weighting=weighting)
    voc = B.Vocabulary(data)
    rng = np.random.default_rng(7 + n)
    d = _descriptors("regular", voc, B.leaf_descriptors(nodes, words), n, 200 + n)
    if n > 10:
        d[rng.choice(n, n // 3, replace=False)] = d[rng.choice(n // 10, n // 3)]      # repeated descriptors: TF sums of up to tens of terms
    db = pkg.BowDatabase(hip, store, data, max_entries=2)
    try:
        store.put(0, kp_desc=d)
        want = voc.transform(B.ints(d))
        wid, _ = db.words(d)
        per_word = [voc.transform_one(f) for f in B.ints(d)]
        assert wid.tolist() == [w for w, _ in per_word]                  # the occurrence structure: which descriptor fell into which word
        if n == 1000:
            counts = np.bincount([w for w, x in per_word if x > 0])
            assert counts.max() > 5 and any(x == 0 for _, x in per_word)
        assert db.add(0) == 0
        _check_vector(db.entry(-1), want)
        _check_vector(db.entry(0), want)
        ids, sc = db.query(0, 4)
        if want:
            assert ids.tolist() == [0] and abs(sc[0] - 1.0) <= B.score_bound(len(want))       # identical vectors score 1
        else:
            assert len(ids) == 0
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------------------- query
SIZES = [0, 1, 2, 63, 64, 65, 300]
MAX_RESULTS = [1, 4, 32]
N_DESC = 150


def _max_ids(size):
    return [-1, -7, 0, size // 2, size + 10]


def _assert_conditions(full, max_results, thresholds=()):
    sc = [s for _, s in full[:max_results + 1]]
    for a, b in zip(sc, sc[1:]):
        assert a - b > GAP, "input condition: adjacent scores closer than 1e-9 (change the seed)"
    for s in sc[:max_results]:
        for t in thresholds:
            assert abs(s - t) > GAP, "input condition: a score within 1e-9 of a threshold (change the seed)"


@pytest.fixture(scope="module")
def grown(pkg, hip, store):
    """one database grown to 300 entries; at every size of SIZES the answers of the library and of the restatement to
    every (max_results, max_id) case, and to an empty query vector: {(size, max_results, max_id): (got, full reference list)}"""
    data, nodes, words = B.make_vocab(21, 10, 3)
    voc = B.Vocabulary(data)
    leaf = B.leaf_descriptors(nodes, words)
    rng = np.random.default_rng(55)
    query = B.make_descriptors(rng, leaf, N_DESC)
    stopped = np.array([B.to_words(voc.desc[n]) for n in range(len(voc.children)) if voc.word_id[n] >= 0 and voc.transform_one(voc.desc[n])[1] == 0][:5],
                       np.uint64)                                        # descriptors that fall into words of weight 0
    assert len(stopped) == 5 and voc.transform(B.ints(stopped)) == {}
    ref = B.Database(voc)
    db = pkg.BowDatabase(hip, store, data, max_entries=300)
    store.put(1, kp_desc=query)
    store.put(2, kp_desc=np.zeros((0, 4), np.uint64))
    store.put(3, kp_desc=stopped)
    qvec = voc.transform(B.ints(query))
    out, empty = {}, {}
    try:
        for size in range(301):
            if size in SIZES:
                assert len(db) == ref.nentries == size
                for mid in _max_ids(size):
                    full = ref.query_vector_all(qvec, mid)
                    for mr in MAX_RESULTS:
                        out[(size, mr, mid)] = (db.query(1, mr, mid), full)
                empty[size] = (db.query(2, 4, -1), db.query(3, 4, -1))
            if size == 300:
                break
            e = B.make_descriptors(rng, leaf, N_DESC)
            keep = rng.choice(N_DESC, int(rng.integers(0, N_DESC // 2)), replace=False)      # a varying share of the query's descriptors
            e[keep] = query[keep]
            store.put(0, kp_desc=e)
            assert db.add(0) == ref.add(B.ints(e)) == size
    finally:
        db.close()
    return out, empty, len(qvec), max(len(v) for v in ref.vectors)


@pytest.mark.parametrize("max_results", MAX_RESULTS)
@pytest.mark.parametrize("size", SIZES)
def test_query(grown, size, max_results):
    out, _, nq, nd = grown
    for mid in _max_ids(size):
        (ids, sc), full = out[(size, max_results, mid)]
        _assert_conditions(full, max_results)
        want = full[:max_results]
        assert ids.tolist() == [e for e, _ in want], (size, max_results, mid)
        for s, (_, w) in zip(sc.tolist(), want):
            assert abs(s - w) <= B.score_bound(max(nq, nd))
        # the eligibility rule, stated once more on the reference's answer
        assert all(e < mid or mid == -1 or e == size - 1 for e, _ in full)
    if size >= 2:
        assert len(out[(size, 32, -1)][1]) == size                      # every entry shares a word with the query
        assert [e for e, _ in out[(size, 32, -7)][1]] == [size - 1] == out[(size, 4, 0)][0][0].tolist()     # fewer eligible entries than max_results
        assert len(out[(size, 32, size // 2)][1]) == size // 2 + 1


@pytest.mark.parametrize("size", SIZES)
def test_query_with_an_empty_vector(grown, size):
    for ids, sc in grown[1][size]:
        assert len(ids) == 0 and len(sc) == 0


def test_equal_scores_come_back_in_ascending_id(pkg, hip, store, vocabs):
    voc, leaf, _, _ = vocabs["regular"]
    data = B.make_vocab(21, 10, 3)[0]
    rng = np.random.default_rng(66)
    a, b = B.make_descriptors(rng, leaf, 120), B.make_descriptors(rng, leaf, 120)
    b[:40] = a[:40]
    ref = B.Database(voc)
    db = pkg.BowDatabase(hip, store, data, max_entries=8)
    try:
        for d in (b, a, b, a, a):
            store.put(0, kp_desc=d)
            assert db.add(0) == ref.add(B.ints(d))
        store.put(1, kp_desc=a)
        full = ref.query(B.ints(a), 32)
        assert [e for e, _ in full] == [1, 3, 4, 0, 2]
        assert full[0][1] == full[1][1] == full[2][1] and full[3][1] == full[4][1] and full[2][1] - full[3][1] > GAP
        for mr in (1, 2, 4, 32):
            ids, sc = db.query(1, mr)
            assert ids.tolist() == [1, 3, 4, 0, 2][:mr]
            assert sc[0] == sc[min(mr, 3) - 1] and (mr < 5 or sc[3] == sc[4])          # identical entries: identical bits
            for s, (_, w) in zip(sc.tolist(), full):
                assert abs(s - w) <= B.score_bound(120)
        again = db.query(1, 32)
        assert again[0].tolist() == ids.tolist() and again[1].tobytes() == sc.tobytes()       # two runs: identical bits
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------------------- sequence
def test_sequence_through_the_loop_detector(pkg, hip, pattern, tmp_path):
    """260 keyframes through the C++ LoopDetector (host/lvi_bow_host.hpp): 230 places, then 30 revisits of places 5..34;
    result ids, scores and the loop index of every frame against detect_loop of the restatement.  Crosses frame 50 (the
    frame_index gate), 199 (max_id == -1) and 201 (the first frame whose max_id admits an old entry)."""
    data, nodes, words = B.make_vocab(7, 10, 3)
    voc = B.Vocabulary(data)
    frames = B.make_sequence(3, B.leaf_descriptors(nodes, words), n_desc=120)
    assert len(frames) == 260
    path = tmp_path / "brief_synthetic.bin"
    path.write_bytes(data)
    n_win = 40
    rng = np.random.default_rng(4)
    ref = B.Database(voc)
    want = [B.detect_loop(ref, B.ints(f), i) for i, f in enumerate(frames)]
    # the input conditions, on the restatement alone: detect_loop saw the first four of these lists
    check = B.Database(voc)
    for i, f in enumerate(frames):
        vec = voc.transform(B.ints(f))
        _assert_conditions(check.query_vector_all(vec, i - 200), 4, thresholds=(0.05, 0.015))
        check.add_vector(vec)
    loops = [w[0] for w in want]
    assert all(x == -1 for x in loops[:199]) and loops[199] != -1 and loops[200] == -1 and all(x != -1 for x in loops[201:])
    assert len(want[198][1]) == 1 and len(want[199][1]) == 4 and len(want[200][1]) == 1      # max_id == -1 at frame 199
    assert [w[1][0][0] for w in want[230:]] == list(range(5, 35))                          # a revisit's best match is its place

    ld = pkg.host_api.LoopDetector(pkg.load_host(), hip, pattern, max_entries=260, max_width=32, max_height=32, max_keypoints=128, max_window=64,
                                   max_keyframes=260)
    try:
        ld.loadVocabulary(path)
        connected = 0
        for i, f in enumerate(frames):
            xy = rng.uniform(0, 31, (len(f), 2)).astype(np.float32)
            nm = (xy / 32).astype(np.float32)
            ld.store.put(i, keypoints=xy, keypoints_norm=nm, kp_desc=f, window_xy=xy[:n_win], win_desc=f[:n_win])
            p3 = rng.uniform(-5, 5, (n_win, 3)).astype(np.float32)
            ids = np.arange(n_win, dtype=np.float64) + 1000 * i
            got = ld.addKeyFrame(i, i, True, p3, xy[:n_win], nm[:n_win], ids, xy, nm)
            loop, ret = want[i]
            assert got["ids"].tolist() == [e for e, _ in ret], i
            for s, (_, w) in zip(got["scores"].tolist(), ret):
                assert abs(s - w) <= B.score_bound(120), i
            assert got["loop_index"] == loop, i
            if loop != -1:
                st = R.match(f[:n_win], frames[loop])[0]
                assert got["connected"] == (int(st.sum()) > R.MIN_LOOP_NUM), i
                assert len(ld.connection()[2]) == int(st.sum())
                connected += got["connected"]
        assert connected >= 20                                           # the revisits do connect
    finally:
        ld.close()


# ------------------------------------------------------------------------------------------------------------- capacity and errors
def test_capacity_errors_and_entries_outlive_their_slot(pkg, hip, store, vocabs):
    voc, leaf, _, _ = vocabs["regular"]
    data = B.make_vocab(21, 10, 3)[0]
    INV, CAP = pkg._abi.LVI_ERR_INVALID_ARG, pkg._abi.LVI_ERR_CAPACITY
    rng = np.random.default_rng(9)
    a, b, c = (B.make_descriptors(rng, leaf, 100) for _ in range(3))
    b[:50] = a[:50]
    dll = hip.dll
    db = pkg.BowDatabase(hip, store, data, max_entries=2)
    try:
        store.put(0, kp_desc=a)
        store.put(1, kp_desc=b)
        store.release(4)
        # invalid arguments write nothing
        for slot, mr in ((4, 4), (5, 4), (6, 4), (-1, 4), (0, 0), (0, 33), (0, -1)):
            out = np.full(32, 7, pkg.bow.RESULT_DTYPE); n = C.c_int32(7)
            assert dll.lvi_bow_query(db._h, slot, mr, -1, out.ctypes.data_as(C.c_void_p), C.byref(n)) == INV
            assert n.value == 7 and np.all(out["entry_id"] == 7) and np.all(out["score"] == 7)
        e = C.c_int32(7)
        for slot in (4, 5, 6, -1):
            assert dll.lvi_bow_add(db._h, slot, C.byref(e)) == INV and e.value == 7
        assert len(db) == 0
        # query, then the slot changes, then add: the entry is the new content's vector, not the staged one
        db.query(0, 4)
        store.put(0, kp_desc=c)
        assert db.add(0) == 0
        _check_vector(db.entry(0), voc.transform(B.ints(c)))
        store.put(0, kp_desc=a)
        assert db.add(0) == 1
        before = db.query(1, 4)
        assert before[0].tolist() == [1, 0] or before[0].tolist() == [1]
        # capacity: nothing changes
        assert dll.lvi_bow_add(db._h, 1, C.byref(e)) == CAP and e.value == 7 and len(db) == 2
        with pytest.raises(pkg.LviError) as err:
            db.add(1)
        assert err.value.code == CAP
        kept = db.entry(1)
        # the entries survive the release and the reuse of their slot
        store.release(0)
        store.put(0, kp_desc=c)
        after = db.query(1, 4)
        assert after[0].tolist() == before[0].tolist() and after[1].tobytes() == before[1].tobytes()
        again = db.entry(1)
        assert again[0].tolist() == kept[0].tolist() and again[1].tobytes() == kept[1].tobytes()
        _check_vector(again, voc.transform(B.ints(a)))
    finally:
        db.close()


def test_create_rejects_bad_vocabularies(pkg, hip, store):
    INV, UNS = pkg._abi.LVI_ERR_INVALID_ARG, pkg._abi.LVI_ERR_UNSUPPORTED
    good = kat_vocab()
    l2 = kat_vocab(scoring=1)
    cyc = bytearray(good)
    cyc[24 + 4:24 + 8] = (3).to_bytes(4, "little")                      # node 1 becomes the child of its child 3
    for data, code, max_entries in ((good[:-3], INV, 4), (bytes(cyc), INV, 4), (l2, UNS, 4), (good, INV, 0), (good, INV, 2 ** 31 // K + 1)):
        with pytest.raises(pkg.LviError) as err:
            pkg.BowDatabase(hip, store, data, max_entries=max_entries)
        assert err.value.code == code
    h = C.c_void_p(7)
    buf = np.frombuffer(good, np.uint8)
    assert hip.dll.lvi_bow_create(None, C.c_void_p(buf.ctypes.data), len(good), 4, C.byref(h)) == INV and h.value is None


def test_abi_versions(pkg, hip):
    pkg.bow.bind(hip)
    assert hip.dll.lvi_bow_abi_version() == 1 and hip.dll.lvi_kf_abi_version() == 1 and hip.dll.lvi_abi_version() == 6
