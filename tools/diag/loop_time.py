"""Wall time of one loop-closure job on one GPU (include/lvi_loop.h): start -> result, i.e. the two submaps (fuse +
VoxelGrid), the nearest-neighbour index, every ICP iteration and the fitness pass behind ONE wait.  Input: 51 keyframes
of synth.make_scan(--points) along the loop (the target: 2 * 25 + 1 keys) and one more keyframe that revisits the middle of
the stretch with a drifted pose (0.3 m, 1 degree), the production leaf (mappingSurfLeafSize 0.4) and the production ICP
settings.  Prints one JSON line.  The per-kernel split comes from a run of its own:

    timeout -k 10 600 python tools/diag/loop_time.py --points 100001 --calls 20
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/loop_time.py --points 100001 --calls 3
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


def rpy_matrix(x, y, z, roll, pitch, yaw):
    A, B, Cc, D, E, F = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, :3] = [[A * Cc, A * D * F - B * E, B * F + A * D * E], [B * Cc, A * E + B * D * F, B * D * E - A * F], [-D, Cc * F, Cc * E]]
    T[:3, 3] = [x, y, z]
    return T


def drifted(pose, D):
    r, p, y, x, yy, z = [float(v) for v in pose]
    T = D @ rpy_matrix(x, yy, z, r, p, y)
    return np.array([np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0]), T[0, 3], T[1, 3], T[2, 3]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100001)
    ap.add_argument("--keys", type=int, default=51)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--leaf", type=float, default=0.4)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    S = pkg.synth
    hip = pkg.load_hip()
    P = dict(N_SCAN=4, Horizon_SCAN=32768, max_raw_points=a.points + 64, max_map_points=1 << 18, max_keyframes=a.keys + 8, max_keyframe_points=1 << 23)
    h = pkg.LidarHotpath(hip, **P)
    dev = "cuda" if "torch" in sys.modules and sys.modules["torch"].cuda.is_available() else None

    def keyframe(alpha, seed, D=None):
        pose = S.loop_pose(alpha, 0.01 * np.sin(seed), -0.01 * np.cos(seed)).astype(np.float32)
        h.scan_upload(S.make_scan(a.points, pose, seed, torch_device=dev)); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        h.keyframe_add_current(pose if D is None else drifted(pose, D))
    for k in range(a.keys):
        keyframe(0.2 + 0.04 * k, 900 + k)
    mid = a.keys // 2
    keyframe(0.2 + 0.04 * mid + 0.02, 1900, rpy_matrix(0.3, -0.2, 0.05, 0.004, -0.003, np.deg2rad(1.0)))
    n_kf, n_pts = h.keyframe_count()
    lp = pkg.LoopIcp(h)
    lp.reserve(1 << 18, min(1 << 24, n_pts + 64))
    params = lp.default_params(leaf=a.leaf)                               # search_num 25, max_corr_dist 30, 100 iterations, 1e-6 / 1e-6, 300 / 1000
    ts = []
    for k in range(a.calls + 2):
        t0 = time.perf_counter()
        lp.start(a.keys, mid, params)
        t1 = time.perf_counter()
        r = lp.result()
        t2 = time.perf_counter()
        if k >= 2:
            ts.append((t1 - t0, t2 - t0))
    ts = np.array(ts)
    iters = r["iterations"]
    out = dict(points_per_scan=a.points, keyframes=n_kf, keyframe_points=n_pts, leaf=a.leaf, n_source=r["n_source"], n_target=r["n_target"],
               n_target_fused=r["n_target_fused"], status=r["status"], converged=r["converged"], convergence_state=r["convergence_state"],
               iterations=iters, fitness=r["fitness"], calls=len(ts),
               start_ms_median=1e3 * float(np.median(ts[:, 0])), start_to_result_ms_median=1e3 * float(np.median(ts[:, 1])),
               start_to_result_ms_p90=1e3 * float(np.percentile(ts[:, 1], 90)), arena_bytes=lp.arena_bytes(),
               launches_per_job="1 fuse + 2 VoxelGrids (8 or 19 each) + 6 index + 2 * max_iters (= 200, all but 2 * iterations of them early exits) + 2",
               method="wall clock per job (host to host: the enqueue of every launch and the one wait in lvi_loop_result)")
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
