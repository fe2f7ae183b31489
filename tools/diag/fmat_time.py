"""Per-call cost of rejectWithF's RANSAC on one GPU (include/lvi_fmat.h): wall clock around lvi_fmat_find (one upload, two
kernels, one download, one wait), the host sample-stream part of it (lvi_fmat_info.stream_us), at n = 150 (the yaml
max_cnt) and 2500 and outlier fractions 0, 0.3 and 0.5 of tests/fmat_ref.two_view scenes (0.3 px noise, F_THRESHOLD 1);
then the per-frame node.image time of the 1024x576 tracker configuration of tests/test_gpu_tracker_node.py with and
without the device RANSAC.  Prints one JSON line.  Kernel times come from a separate rocprofv3 run of this script:

    timeout -k 10 300 python tools/diag/fmat_time.py
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d fmat_prof -o fmat -- python tools/diag/fmat_time.py --no-node --calls 50
"""
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


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 2), p99=round(float(np.percentile(v, 99)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--no-node", action="store_true")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import fmat_ref as R
    fr = pkg.FundamentalRansac(pkg.load_hip(), max_points=2500, max_iters=1000)
    out = {}
    for n in (150, 2500):
        for o in (0.0, 0.3, 0.5):
            p1, p2, _, _ = R.two_view(n, o, 0.3, seed=7 + n)
            for _ in range(5):
                fr.find(p1, p2, 1.0)
            wall, host, iters = [], [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                _, info = fr.find(p1, p2, 1.0, with_info=True)
                wall.append((time.perf_counter() - t0) * 1e6)
                host.append(info["stream_us"]); iters.append(info["iters"])
            out[f"n{n}_o{o}"] = dict(wall_us=_stats(wall), stream_us=_stats(host), walk_iters=int(iters[0]), hypotheses=info["n_subsets"])
    fr.close()
    if not a.no_node:
        from test_gpu_tracker_node import CONFIGS, _camera, _sequence
        from oracle import loader
        name, (w, h), n, freq, equalize, _b, max_cnt, min_dist, max_feat, _r = CONFIGS[0]
        frames, stamps, _ = _sequence(pkg, w, h, n, seed=31 + len(name))
        tp = pkg.default_tracker_params(loader.load(pkg), max_width=w, max_height=h, max_cnt=max_cnt, min_dist=min_dist, max_features=max_feat)
        for mode in ("no_hook", "device_ransac"):
            node = pkg.host_api.TrackerNode(pkg.load_host(), tp, h, w, freq, equalize=equalize, cam=_camera(w, h))
            if mode == "device_ransac":
                node.use_device_fundamental()
            ts = []
            for img, t in zip(frames, stamps):
                t0 = time.perf_counter()
                r = node.image(img, t)
                if r["pub_this_frame"]:
                    ts.append((time.perf_counter() - t0) * 1e6)
            node.close()
            out[f"node_image_pub_frames_{mode}"] = dict(us=_stats(ts[3:]), frames=len(ts) - 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
