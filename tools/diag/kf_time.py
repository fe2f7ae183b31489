"""Wall time of the keyframe describer (include/lvi_kf.h), host to host: describe (upload, blur, FAST, BRIEF, MEI lift, one
wait) of a 1024x576 frame with 150 window points, and match (one launch, one download, one wait) of those 150 window
descriptors against the keypoints that frame yields.  Checks the first call against tests/kfdesc_ref.py before timing.

    python tools/diag/kf_time.py [--reps 200] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return dict(median_ms=float(np.median(ts)) * 1e3, p90_ms=float(np.percentile(ts, 90)) * 1e3, min_ms=float(np.min(ts)) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--out", help="write the results as JSON here")
    a = ap.parse_args()
    import kfdesc_ref as R
    pkg = graft.import_package()
    hip = pkg.load_hip()
    S = pkg.synth
    w, h = a.width, a.height
    pattern = pkg.config.load_brief_pattern(os.path.join(ROOT, "tests", "golden", "brief_pattern.yml"))
    cam = pkg.config.load_camera_yaml(os.path.join(ROOT, "tests", "golden", "params_camera.yaml"))[1]
    img0 = S.make_texture(w, h, 4242)
    Hm = S.small_motion_homography(w, h, 100)
    img1 = S.warp_homography(img0, Hm)
    kp0 = R.fast(img0)
    sel = np.linspace(0, len(kp0) - 1, 150).astype(int)
    win = S.apply_homography(Hm, kp0[sel]).astype(np.float32)
    kd = pkg.KeyframeDescriber(hip, pattern, max_width=w, max_height=h, max_keypoints=16384, max_window=150, max_keyframes=2)
    i0 = kd.describe(0, img0, None, cam)
    i1 = kd.describe(1, img1, win, cam)
    st, ix, ds = kd.match(1, 0)
    ref0, ref1 = R.describe(img0, np.zeros((0, 2)), pattern), R.describe(img1, win, pattern)
    g0, g1 = kd.get(0), kd.get(1)
    rs, ri, rd = R.match(ref1["win_desc"], ref0["kp_desc"])
    exact = (np.array_equal(g0["keypoints"], ref0["keypoints"]) and np.array_equal(g0["kp_desc"], ref0["kp_desc"])
             and np.array_equal(g1["win_desc"], ref1["win_desc"]) and np.array_equal(st, rs) and np.array_equal(ix, ri) and np.array_equal(ds, rd))
    res = dict(width=w, height=h, n_window=len(win), n_keypoints_old=i0["n_keypoints_stored"], n_keypoints_cur=i1["n_keypoints_stored"],
               truncated=bool(i0["truncated"] or i1["truncated"]), n_matched=int(st.sum()), exact_against_restatement=bool(exact))
    res["describe"] = timed(lambda: kd.describe(1, img1, win, cam), a.reps, a.warmup)
    res["match"] = timed(lambda: kd.match(1, 0), a.reps, a.warmup)
    kd.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not exact:
        raise SystemExit("the device results differ from tests/kfdesc_ref.py")


if __name__ == "__main__":
    main()
