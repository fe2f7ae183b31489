"""Per-call cost of the LiDAR depth association on one GPU (include/lvi_depth.h): lidar_callback and get_depth, wall
clock around each call (both end in one wait, so the wall time is the call's latency).  Input: clouds of
synth.make_scan(--points) along the loop trajectory, a window of --clouds clouds (LIDAR_SKIP 0, 0.1 s apart), --features
features in the image's field of view.  Prints one JSON line.

    timeout -k 10 300 python tools/diag/depth_time.py --points 100001 --clouds 12 --features 150
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100001)
    ap.add_argument("--clouds", type=int, default=12)
    ap.add_argument("--features", type=int, default=150)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    S = pkg.synth
    reg = pkg.DepthRegister(pkg.load_hip(), max_clouds=a.clouds + 1, max_cloud_points=a.points, max_features=a.features, lidar_skip=0,
                            window_s=0.1 * (a.clouds - 1) + 0.05)      # holds --clouds clouds 0.1 s apart once full
    scans = []
    for k in range(8):
        p = S.loop_pose(0.03 * k)
        s = S.make_scan(a.points, p, 40 + k)
        scans.append((np.stack([s["x"], s["y"], s["z"], s["reflectivity"].astype(np.float32)], 1).astype(np.float32), (p[3], p[4], p[5], p[0], p[1], p[2])))
    cb, gd = [], []
    rng = np.random.default_rng(1)
    f = np.stack([rng.uniform(-0.6, 0.6, a.features), rng.uniform(-0.45, 0.45, a.features), np.ones(a.features)], 1).astype(np.float32)
    n_cb = a.clouds + a.calls
    for k in range(n_cb):
        cloud, pose = scans[k % len(scans)]
        stamp = 0.1 * k
        t0 = time.perf_counter()
        reg.lidar_callback(cloud, pose, stamp)
        t1 = time.perf_counter()
        d = reg.get_depth(pose, f)
        t2 = time.perf_counter()
        if k >= a.clouds:
            cb.append(t1 - t0); gd.append(t2 - t1)
    st = reg.state()
    out = dict(points_per_cloud=a.points, clouds_in_window=st["n_clouds"], depth_cloud_points=st["n_depth_cloud"], features=a.features,
               with_depth=int((d > 0).sum()), calls=len(cb),
               lidar_callback_ms_median=1e3 * float(np.median(cb)), lidar_callback_ms_p90=1e3 * float(np.percentile(cb, 90)),
               get_depth_ms_median=1e3 * float(np.median(gd)), get_depth_ms_p90=1e3 * float(np.percentile(gd, 90)),
               method="wall clock per call (host to host, includes H2D of the cloud / features and the one wait)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
