"""rejectWithF without OpenCV: two TrackerNodes over the frames and stamps of test_gpu_tracker_node.py, one over the HIP
host library with the device RANSAC installed (TrackerNode.use_device_fundamental), one over the oracle-linked host
library with a hook that runs the host restatement tests/fmat_ref.py.  Every frame must agree as in
test_gpu_tracker_node.py, up to a status difference that test_gpu_fmat.py's classifier explains (after which the two runs
have different track sets and the comparison of that configuration stops)."""
import os

import numpy as np
import pytest

import fmat_ref as R
from helpers import bits
from test_gpu_tracker_node import CONFIGS, _camera, _sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_host(pkg, oracle, hip, tmp_path_factory):
    H = pkg.host_api
    out = tmp_path_factory.mktemp("hostlib_fmat") / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    return H.HostLibrary(str(out))


class RefReject:
    """the restatement as the oracle node's findFundamentalMat; also runs the device RANSAC on the same points to classify
    a status difference the moment it happens"""

    def __init__(self, dev):
        self.dev, self.calls, self.removed_frames, self.max_n = dev, [], 0, 0
        self.first_diff = None

    def __call__(self, un_cur, un_forw, thr):
        st, T = R.find(un_cur, un_forw, thr, 0.99)
        sd, info = self.dev.find(un_cur, un_forw, thr, with_info=True)
        k = len(self.calls)
        self.calls.append(len(un_cur))
        self.max_n = max(self.max_n, len(un_cur))
        self.removed_frames += int((st == 0).any())
        if self.first_diff is None and not (st == sd).all():
            self.first_diff = (k, self._classify(un_cur, un_forw, thr, st, sd, T, info))
        return st

    def _classify(self, p1, p2, thr, st, sd, T, info):
        tr = self.dev.trace()
        for h in range(min(len(T["nmodels"]), len(tr["nmodels"]))):
            if tr["nmodels"][h] != T["nmodels"][h]:
                return "F"
            for m in range(int(T["nmodels"][h])):
                d = np.abs(tr["F"][h, m].ravel() - T["F"][h, m].ravel()).max() / max(np.abs(T["F"][h, m]).max(), 1e-300)
                if d > 1e-9:
                    return "F"
        if R.lmeds_rounding_decided(T["path"], len(p1), (info["best_iter"], info["best_root"]), (T["best_iter"], T["best_root"]),
                                    tr["score"], T["score"]):
            return "lmeds_rounding"
        t = np.float32(thr * thr) if T["path"] != "lmeds" else np.float32(R.lmeds_sigma(len(p1), T["best_median"]) ** 2)
        e = R.errors(T["F_best"], p1, p2)[st != sd]
        lo, hi = t, t
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
        return "ulp" if ((e >= lo) & (e <= hi)).all() else "unexplained"


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_tracker_with_device_ransac_equals_the_restatement(pkg, oracle, hip, oracle_host, monkeypatch, cfg):
    name, (w, h), n, freq, equalize, _bound, max_cnt, min_dist, max_feat, radix = cfg
    frames, stamps, _ev = _sequence(pkg, w, h, n, seed=31 + len(name))
    tp = pkg.default_tracker_params(oracle, max_width=w, max_height=h, max_cnt=max_cnt, min_dist=min_dist, max_features=max_feat)
    cam = _camera(w, h)
    if radix:
        monkeypatch.setenv("LVI_GFTT_RADIX", "1")
    else:
        monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    H = pkg.host_api
    n_ora = H.TrackerNode(oracle_host, tp, h, w, freq, equalize=equalize, cam=cam)
    n_hip = H.TrackerNode(pkg.load_host(), tp, h, w, freq, equalize=equalize, cam=cam)
    monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    dev = pkg.FundamentalRansac(hip, max_points=max(max_cnt, 8), max_iters=1000)
    ref = RefReject(dev)
    n_ora.set_fundamental_hook(ref)
    n_hip.use_device_fundamental()
    try:
        # one node after the other (feature ids come from a static both host libraries share; see test_gpu_tracker_node.py)
        ro_all = [(n_ora.image(img, t), n_ora.points()) for img, t in zip(frames, stamps)]
        rg_all = [(n_hip.image(img, t), n_hip.points()) for img, t in zip(frames, stamps)]
    finally:
        n_ora.close(); n_hip.close(); dev.close()
    # a RANSAC status difference must be one the classifier explains; from the frame it reaches the track set on, the two
    # runs differ legitimately and the comparison stops
    diverged = ref.first_diff is not None
    if diverged:
        assert ref.first_diff[1] != "unexplained", (name, ref.first_diff)
    id_base = None
    compared = 0
    for k, ((ro, po), (rg, pg)) in enumerate(zip(ro_all, rg_all)):
        if diverged and not (po.shape == pg.shape and (bits(po[:, :2]) == bits(pg[:, :2])).all()):
            break                                                          # the explained difference reached the track set
        where = f"{name} frame {k}"
        assert ro["rejectWithF_skipped"] == 0 and rg["rejectWithF_skipped"] == 0, where
        for key in ("outcome", "pub_this_frame", "pub_count", "n_cur_pts"):
            assert ro[key] == rg[key], (where, key, ro[key], rg[key])
        assert po.shape == pg.shape, where
        np.testing.assert_array_equal(bits(po[:, :2]), bits(pg[:, :2]), err_msg=where)
        np.testing.assert_array_equal(po[:, 3], pg[:, 3], err_msg=where)
        if id_base is None and len(po):
            id_base = (po[:, 2].min(), pg[:, 2].min())
        if id_base is not None:
            np.testing.assert_array_equal(po[:, 2] - id_base[0], pg[:, 2] - id_base[1], err_msg=where)
        if ro["outcome"] in ("published", "first_publish_suppressed"):
            cho, chg = ro["channels"], rg["channels"]
            assert cho.shape == chg.shape, where
            np.testing.assert_array_equal(cho[0] - id_base[0], chg[0] - id_base[1], err_msg=where)
            np.testing.assert_array_equal(bits(cho[1:5]), bits(chg[1:5]), err_msg=where)
        compared += 1
    rep = dict(frames=len(frames), compared=compared, ransac_calls=len(ref.calls), frames_with_removals=ref.removed_frames, max_n=ref.max_n,
               first_diff=ref.first_diff)
    print(name, rep)
    assert len(ref.calls) > 10, rep
    assert ref.removed_frames >= 1, rep                                    # positive control: the RANSAC removes tracks
    if max_cnt >= 1000:
        assert ref.max_n >= 1000, rep
    if not diverged:
        assert compared == len(frames), rep
