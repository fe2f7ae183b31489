"""Cost of the feature table's per-image operations on one GPU (include/lvi_fman.h) at the workload's size: a
300-feature table in an 11-frame window and a frame of 150 observations.  Wall clock, host clock around calls that end in
the call's one device synchronise, median and p99 over 200 frames, of add_frame, triangulate, projections and one slide
(removeBackShiftDepth).  Every timed call starts from the same table: it is rebuilt outside the timed window.  Beside it, the
upload of a whole hand-built feature list of that size through lvh_marg_set_features plus lvh_win_set_lidar_flags, which is
what a caller does today (a host-side copy; the list then travels inside the solve).  No threshold is set on any of the
numbers.  Prints one JSON line.

    timeout -k 10 300 python tools/diag/fman_time.py
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
    return dict(median=round(float(np.median(v)), 1), p99=round(float(np.percentile(v, 99)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--observations", type=int, default=150)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import fman_ref as R
    hip = pkg.load_hip()
    # the window: `features` features over frames 0..9; the timed frame is image 10 with `observations` ids, half of them known
    sc = R.window_scene(77, a.features)
    frames = [(ids, np.asarray(obs, np.float64).reshape(-1, 8)) for ids, obs in sc["frames"][:R.WINDOW]]
    known = [i for i in sc["frames"][R.WINDOW - 1][0]][:a.observations // 2]
    ids10 = sorted(known + list(range(10000, 10000 + a.observations - len(known))))
    rs = np.random.RandomState(5)
    obs10 = np.c_[rs.uniform(-0.4, 0.4, (len(ids10), 2)), np.ones(len(ids10)), rs.uniform(0, 600, (len(ids10), 2)), rs.normal(0, 0.1, (len(ids10), 2)), -np.ones(len(ids10))]
    tab = pkg.FeatureTable(hip, max_features=max(1024, 2 * a.features))

    def rebuild():
        tab.clear()
        for i, (ids, obs) in enumerate(frames):
            tab.add_frame(i, ids, obs, 0.0)

    I3 = np.eye(3)
    wall = dict(add_frame=[], triangulate=[], projections=[], slide=[])
    info = tri = proj = None
    for k in range(a.frames + 5):
        rebuild()
        t0 = time.perf_counter()
        info = tab.add_frame(R.WINDOW, ids10, obs10, 0.0)
        t1 = time.perf_counter()
        tri = tab.triangulate(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"])
        t2 = time.perf_counter()
        proj = tab.projections(R.MODE_WINDOW)
        t3 = time.perf_counter()
        tab.remove_back_shift_depth(I3, [0.0, 0.0, 0.0], I3, [0.08, 0.0, 0.0])
        t4 = time.perf_counter()
        if k >= 5:
            for name, dt in zip(("add_frame", "triangulate", "projections", "slide"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                wall[name].append(dt * 1e6)
    rebuild()
    tab.add_frame(R.WINDOW, ids10, obs10, 0.0)
    table = tab.download()
    out = dict(frames=a.frames, table=len(table), frame_observations=len(ids10), tracked=info["last_track_num"], triangulated=tri["triangulated"],
               max_sweeps=tri["max_sweeps"], records=len(proj["records"]), features_in_the_solve=len(proj["inv_dep"]),
               **{name + "_wall_us": _stats(v) for name, v in wall.items()},
               note="projections is two calls (sizes, then the one download); add_frame, triangulate and the slide are one call with one wait each")
    tab.close()
    # what a caller does today: the whole list, built by hand, handed to the host mirror for every image
    feats = [dict(start_frame=int(f["start_frame"]), inv_dep=0.2,
                  obs=[dict(point=o["point"], velocity=o["velocity"], cur_td=float(o["cur_td"]), uv_y=float(o["uv"][1])) for o in f["obs"][:int(f["n_obs"])]]) for f in table]
    hl = pkg.load_host()
    V = pkg.host_api.VinsMarginalizer(hl, hip, max_features=min(512 - 15, len(feats)), estimate_td=True)
    O = pkg.host_api.VinsWindowOptimizer(hl, hip, V, max_features=min(512 - 15, len(feats)))
    up = []
    for k in range(a.frames + 5):
        t0 = time.perf_counter()
        V.set_features(feats)
        O.set_lidar_flags(np.zeros(len(feats), np.int32))
        if k >= 5:
            up.append((time.perf_counter() - t0) * 1e6)
    O.close()
    V.close()
    out.update(hand_built_list_upload_us=_stats(up), hand_built_list_note="Python packs the list and the host mirror copies it; no device work")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
