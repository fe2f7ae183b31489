"""Per-call cost of the pose graph's loop confirmation on one GPU (include/lvi_pnp.h): wall clock around lvi_pnp_solve
(one upload, two kernels, one download, one wait) and the host sample-stream part of it (lvi_pnp_info.stream_us), at
n = 30 (just past findConnection's gate) and 150 and outlier fractions 0 and 0.3 of tests/pnp_ref.scene scenes (noise
0.5 / 460, the reference's threshold 10 / 460, 100 iterations).  Prints one JSON line.  OpenCV is not available to this
project, so there is no CPU solvePnPRansac to compare with.  Kernel times come from a separate rocprofv3 run:

    timeout -k 10 120 python tools/diag/pnp_time.py
    timeout -k 10 120 rocprofv3 --kernel-trace --stats -d pnp_prof -o pnp -- python tools/diag/pnp_time.py --calls 50
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
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import pnp_ref as P
    pr = pkg.PnPRansac(pkg.load_hip(), max_points=256, max_iters=100)
    out = {}
    for n in (30, 150):
        for o in (0.0, 0.3):
            p3, p2, _, _ = P.scene(n, o, 0.5 / P.FOCAL_LENGTH, seed=7 + n)
            for _ in range(5):
                pr.solve(p3, p2)
            wall, host, iters = [], [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                _, info = pr.solve(p3, p2, with_info=True)
                wall.append((time.perf_counter() - t0) * 1e6)
                host.append(info["stream_us"]); iters.append(info["iters"])
            out[f"n{n}_o{o}"] = dict(wall_us=_stats(wall), stream_us=_stats(host), walk_iters=int(iters[0]), hypotheses=info["n_subsets"],
                                     n_inliers=info["n_inliers"])
    pr.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
