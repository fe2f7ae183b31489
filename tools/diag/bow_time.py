"""Wall time of the DBoW2 database on the GPU (include/lvi_bow.h), host to host: one query + add (detectLoop's
db.query(.., 4, frame_index - 200) and db.add) of a keyframe with 1000 keypoint descriptors against a database of 1000
entries, and, on the same run, KeyFrameDescriber::descriptors of that slot (lvi_kf_get of the keypoint descriptors alone):
the download a host-side DBoW2 would need before it could start.

The vocabulary is a synthetic regular k=10, L=6 tree (1 111 110 nodes: 53 MB of node records and 8 MB of word records)
generated in memory from a seed; it is never written to disk.  The slot is uploaded again before every timed call (outside
the timed window), so that every query transforms its descriptors and every add reuses the vector its query staged, as in
detectLoop.  The database grows by one entry per call: from 1000 to 1000 + warmup + reps.  Checks the words of the first
descriptors against a numpy descent before timing.  There is no pass / fail threshold.

    python tools/diag/bow_time.py [--reps 100] [--warmup 10] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def flip_bits(rng, desc, nbits):
    """desc [n, 4] uint64 with nbits random bit positions toggled in each row (positions may repeat)"""
    out = desc.copy()
    rows = np.arange(len(out))
    for _ in range(nbits):
        b = rng.integers(0, 256, len(out))
        out[rows, b >> 6] ^= np.uint64(1) << (b & 63).astype(np.uint64)
    return out


def regular_vocab(pkg, k, L, seed):
    """breadth-first regular tree: node i (0 = the root) has the children k i + 1 .. k i + k; a child is its parent with
    64 >> level bits toggled, the first level is random -> (file bytes, nodes)"""
    rng = np.random.default_rng(seed)
    levels = [rng.integers(0, 2 ** 64, (k, 4), dtype=np.uint64)]
    for lvl in range(1, L):
        levels.append(flip_bits(rng, np.repeat(levels[-1], k, axis=0), max(6, 64 >> lvl)))
    desc = np.concatenate(levels)
    nn = len(desc)
    nodes = np.zeros(nn, pkg.bow.NODE_DTYPE)
    nodes["nodeId"] = np.arange(1, nn + 1)
    nodes["parentId"] = (np.arange(1, nn + 1) - 1) // k
    nodes["descriptor"] = desc
    n_leaf = len(levels[-1])
    nodes["weight"][nn - n_leaf:] = rng.uniform(0.25, 9.0, n_leaf)
    words = np.zeros(n_leaf, pkg.bow.WORD_DTYPE)
    words["nodeId"] = np.arange(nn - n_leaf + 1, nn + 1)
    words["wordId"] = np.arange(n_leaf)
    return pkg.bow.write_vocab(k, L, nodes, words), nodes


def numpy_word(nodes, k, L, d):
    """the descent of one descriptor on the regular tree: the first child of the smallest Hamming distance"""
    cur = 0
    for _ in range(L):
        kids = nodes["descriptor"][k * cur:k * cur + k]                  # ids k cur + 1 .. k cur + k are rows k cur .. k cur + k - 1
        dist = np.unpackbits((kids ^ d).view(np.uint8), axis=1).sum(axis=1)
        cur = k * cur + 1 + int(np.argmin(dist))
    return cur - (len(nodes) - k ** L) - 1


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), min_ms=float(ts.min()),
                max_ms=float(ts.max()), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--out", help="write the results as JSON here")
    a = ap.parse_args()
    pkg = graft.import_package()
    hip = pkg.load_hip()
    pattern = pkg.config.load_brief_pattern(os.path.join(ROOT, "tests", "golden", "brief_pattern.yml"))
    t0 = time.perf_counter()
    data, nodes = regular_vocab(pkg, a.k, a.levels, 2024)
    t_gen = time.perf_counter() - t0
    n_leaf = a.k ** a.levels
    leaf = nodes["descriptor"][len(nodes) - n_leaf:]
    rng = np.random.default_rng(7)
    kd = pkg.KeyframeDescriber(hip, pattern, max_width=32, max_height=32, max_keypoints=a.keypoints, max_window=8, max_keyframes=2)
    t0 = time.perf_counter()
    db = pkg.BowDatabase(hip, kd, data, max_entries=a.entries + a.warmup + a.reps)
    t_create = time.perf_counter() - t0

    def keyframe(base=None, share=0.0):
        d = flip_bits(rng, leaf[rng.integers(0, n_leaf, a.keypoints)], 3)
        if base is not None:
            keep = rng.random(a.keypoints) < share
            d[keep] = base[keep]
        return d

    probe = keyframe()
    wid, _ = db.words(probe)
    want = [numpy_word(nodes, a.k, a.levels, probe[i]) for i in range(32)]
    exact = wid[:32].tolist() == want
    for _ in range(a.entries):
        kd.put(0, kp_desc=keyframe(probe, 0.2))
        db.add(0)
    res = dict(k=a.k, L=a.levels, n_nodes=len(nodes), vocab_mb=len(data) / 1e6, vocab_generate_s=t_gen, create_s=t_create, keypoints=a.keypoints,
               entries_before=len(db), words_match_numpy_descent=bool(exact))
    cnt = (C.c_int32 * 2)()
    buf = np.zeros((a.keypoints, 4), np.uint64)
    dll = hip.dll

    def descriptors():                                                   # KeyFrameDescriber::descriptors (host/lvi_kf_host.hpp)
        dll.lvi_kf_get(kd._h, 1, cnt, None, None, None, None, None)
        dll.lvi_kf_get(kd._h, 1, cnt, None, None, buf.ctypes.data_as(C.c_void_p), None, None)

    t_qa, t_q, t_a, t_dl, n_res = [], [], [], [], []
    for i in range(a.warmup + a.reps):
        d = keyframe(probe, 0.2)
        kd.put(1, kp_desc=d)                                             # a fresh slot content: the query transforms it
        max_id = len(db) - 200
        t0 = time.perf_counter()
        ids, sc = db.query(1, 4, max_id)
        t1 = time.perf_counter()
        db.add(1)
        t2 = time.perf_counter()
        descriptors()
        t3 = time.perf_counter()
        if i >= a.warmup:
            t_qa.append(t2 - t0); t_q.append(t1 - t0); t_a.append(t2 - t1); t_dl.append(t3 - t2); n_res.append(len(ids))
    assert np.array_equal(buf, d)
    res.update(entries_after=len(db), results_per_query=float(np.mean(n_res)), words_in_last_vector=len(db.entry(-1)[0]), query_plus_add=stats(t_qa),
               query=stats(t_q), add=stats(t_a), descriptors_download=stats(t_dl))
    db.close(); kd.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not exact:
        raise SystemExit("the device words differ from the numpy descent")


if __name__ == "__main__":
    main()
