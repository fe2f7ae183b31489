"""GPU tier of LoopDetector::usePnP (host/lvi_bow_host.hpp, host/lvi_pnp_host.hpp): the keyframe sequence of
tests/test_gpu_bow.py's loop-detector test, once without the hook (today's answers) and once with it, where `connected`
must be KeyFrame::findConnection's boolean: the front gate and more than MIN_LOOP_NUM ones in the restatement's PnP
status (tests/pnp_ref.py) of the vectors PnPRANSAC received.

A revisit's point_3d is made consistent with the old keyframe's keypoints_norm (each window point is placed on the ray of
the old keypoint its descriptor matches, under one pose per frame), except on three frames whose point_3d is random: those
pass the first gate and must be rejected by PnP."""
import numpy as np
import pytest

import bow_ref as B
import kfdesc_ref as R
import pnp_ref as P

pytestmark = pytest.mark.gpu

N_WIN = 40
INCONSISTENT = (235, 245, 255)


@pytest.fixture(scope="module")
def pattern(pkg):
    import os
    return pkg.config.load_brief_pattern(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brief_pattern.yml"))


@pytest.fixture(scope="module")
def sequence():
    """the frames, the restatement's detect_loop answers, and every frame's host half"""
    data, nodes, words = B.make_vocab(7, 10, 3)
    voc = B.Vocabulary(data)
    frames = B.make_sequence(3, B.leaf_descriptors(nodes, words), n_desc=120)
    ref = B.Database(voc)
    want = [B.detect_loop(ref, B.ints(f), i) for i, f in enumerate(frames)]
    rng = np.random.default_rng(4)
    halves = []
    for i, f in enumerate(frames):
        xy = rng.uniform(0, 31, (len(f), 2)).astype(np.float32)
        nm = (xy / 32).astype(np.float32)
        p3 = rng.uniform(-5, 5, (N_WIN, 3)).astype(np.float32)
        loop = want[i][0]
        if loop != -1 and i not in INCONSISTENT:
            st, idx = R.match(f[:N_WIN], frames[loop])[:2]
            Rm, t = P.rodrigues(0.2 * rng.normal(0, 1, 3)), 0.5 * rng.normal(0, 1, 3)
            old_nm = halves[loop]["nm"]
            for j in np.nonzero(st)[0]:
                u, v = old_nm[idx[j]].astype(np.float64)
                z = rng.uniform(4, 12)
                p3[j] = (Rm.T @ (z * np.array([u, v, 1.0]) - t)).astype(np.float32)
        halves.append(dict(xy=xy, nm=nm, p3=p3, ids=np.arange(N_WIN, dtype=np.float64) + 1000 * i))
    return data, frames, want, halves


def _run(pkg, hip, pattern, sequence, tmp_path, with_pnp):
    data, frames, want, halves = sequence
    path = tmp_path / "brief_synthetic.bin"
    path.write_bytes(data)
    hl = pkg.load_host()
    ld = pkg.host_api.LoopDetector(hl, hip, pattern, max_entries=260, max_width=32, max_height=32, max_keypoints=128, max_window=64, max_keyframes=260)
    pnp = pkg.host_api.HostPnPRansac(hl, max_points=64) if with_pnp else None
    out = []
    try:
        ld.loadVocabulary(path)
        if with_pnp:
            ld.usePnP(pnp)
        for i, f in enumerate(frames):
            h = halves[i]
            ld.store.put(i, keypoints=h["xy"], keypoints_norm=h["nm"], kp_desc=f, window_xy=h["xy"][:N_WIN], win_desc=f[:N_WIN])
            got = ld.addKeyFrame(i, i, True, h["p3"], h["xy"][:N_WIN], h["nm"][:N_WIN], h["ids"], h["xy"], h["nm"])
            got["n_connection"] = len(ld.connection()[2]) if got["loop_index"] != -1 else 0
            got["pnp"] = ld.pnp_connection()
            out.append(got)
    finally:
        ld.close()
        if pnp is not None:
            pnp.close()
    return out


def test_loop_detector_with_and_without_the_pnp_hook(pkg, hip, pattern, sequence, tmp_path):
    data, frames, want, halves = sequence
    plain = _run(pkg, hip, pattern, sequence, tmp_path, False)
    hooked = _run(pkg, hip, pattern, sequence, tmp_path, True)
    confirmed = rejected = front_failed = 0
    for i, f in enumerate(frames):
        loop, ret = want[i]
        for got in (plain[i], hooked[i]):                                # the query and its gates: today's answers, hook or not
            assert got["ids"].tolist() == [e for e, _ in ret], i
            for s, (_, w) in zip(got["scores"].tolist(), ret):
                assert abs(s - w) <= B.score_bound(120), i
            assert got["loop_index"] == loop, i
        assert len(plain[i]["pnp"][2]) == 0                              # without the hook PnPRANSAC never runs
        if loop == -1:
            assert not plain[i]["connected"] and not hooked[i]["connected"] and len(hooked[i]["pnp"][2]) == 0
            continue
        st, idx = R.match(f[:N_WIN], frames[loop])[:2]
        front = int(st.sum()) > R.MIN_LOOP_NUM
        # without the hook: the front half, as before
        assert plain[i]["connected"] == front and plain[i]["n_connection"] == int(st.sum()), i
        # with it: findConnectionFront && popcount(pnp status) > MIN_LOOP_NUM, on the vectors PnPRANSAC received
        p3, p2, pst = hooked[i]["pnp"]
        if not front:
            assert not hooked[i]["connected"] and len(pst) == 0 and hooked[i]["n_connection"] == int(st.sum()), i
            front_failed += 1
            continue
        sel = np.nonzero(st)[0]
        np.testing.assert_array_equal(p3, halves[i]["p3"][sel])
        np.testing.assert_array_equal(p2, halves[loop]["nm"][idx[sel]])
        ref_st = P.solve(p3, p2)[0]
        np.testing.assert_array_equal(pst, ref_st, err_msg=str(i))
        assert hooked[i]["connected"] == (int(ref_st.sum()) > R.MIN_LOOP_NUM), i
        assert hooked[i]["n_connection"] == int(ref_st.sum()), i         # the six vectors were compacted by the PnP status
        if hooked[i]["connected"]:
            confirmed += 1
            assert i not in INCONSISTENT and ref_st.all()
        else:
            rejected += 1
            assert i in INCONSISTENT
    print("pnp loop:", dict(confirmed=confirmed, rejected=rejected, front_failed=front_failed))
    # every planted frame passes the first gate and is rejected by PnP; every other loop frame that passes it is confirmed
    assert rejected == len(INCONSISTENT) and confirmed >= 15 and front_failed + confirmed + rejected == sum(w[0] != -1 for w in want)


def test_host_pnp_status_is_the_reference_call(pkg, hip):
    """lvi_host::PnPRansac::status passes keyframe.cpp:163's arguments: (float)(10.0 / 460.0), 0.99, 100 iterations"""
    h = pkg.host_api.HostPnPRansac(pkg.load_host(), max_points=256)
    try:
        p3, p2, truth, _ = P.scene(150, 0.3, 1.0 / P.FOCAL_LENGTH, 31)
        st = h.status(p2, p3)
        np.testing.assert_array_equal(st, P.solve(p3, p2, P.THRESHOLD, 0.99, 100)[0])
        assert st[truth].mean() > 0.9 and not st[~truth].any()
        with pytest.raises(pkg.LviError):
            h.status(p2[:4], p3[:4])
    finally:
        h.close()
