"""Wall time of the global map (include/lvi_gmap.h): build + result + fetch of the filtered cloud at ~5 M fused points
(250 keyframes of synth.make_map, interleaved corner + surf, leaf 0.05) and at the largest size the reservation allows;
achieved GB/s against the compulsory bytes; the arena's bytes per point; the restatement's CPU time (oracle transform +
VoxelGrid) on the 5 M-point input; the sequential replay's per-scan latency with a build started every 5 s of replay time.

    python tools/diag/gmap_time.py [--reps 10] [--skip-oracle] [--skip-seq]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.percentile(ts, 90)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--skip-seq", action="store_true")
    ap.add_argument("--out", help="write the results as JSON here")
    a = ap.parse_args()
    pkg = graft.import_package()
    from oracle import loader
    hip, ora = pkg.load_hip(), loader.load(pkg)
    S = pkg.synth
    P = dict(N_SCAN=4, Horizon_SCAN=16384, max_raw_points=70000, max_map_points=1 << 18, max_keyframes=512, max_keyframe_points=1 << 23)
    o = pkg.LidarHotpath(ora, **dict(P, max_map_points=1 << 21))
    kfs = []
    S.make_map(o, 250, 64001, seed=4711, keyframes_out=kfs)
    h = pkg.LidarHotpath(hip, **P)
    for kf in kfs:
        h.keyframe_add(kf[0], kf[1], kf[2])
    g = pkg.GlobalMap(h)
    res = {}
    keys5 = list(range(len(kfs)))
    per = h.keyframe_count()[1]
    for name, keys in (("all_keys", keys5), ("max_reservation", keys5 * max(1, ((1 << 25) - 64) // per))):
        g.reserve(min(1 << 25, len(keys) * per // len(kfs) + 64))
        n = g.build(keys, pkg.gmap.CORNER_SURF, 0.05); r = g.result()

        def run():
            g.build(keys, pkg.gmap.CORNER_SURF, 0.05); g.fetch(pkg.gmap.FILTERED)
        med, p90 = timed(run, a.reps)
        byt = 16.0 * (3 * n + r["n_out"])                # keyframe read, fused write, the filter's read of the fused cloud, output
        res[name] = dict(n_fused=n, n_out=r["n_out"], overflow=r["overflow"], median_ms=med, p90_ms=p90,
                         gbps_compulsory=byt / (med * 1e-3) / 1e9, arena_bytes_per_point=g.arena_bytes() / max(n, 1))
        print(name, json.dumps(res[name]), flush=True)
    if not a.skip_oracle:
        t0 = time.perf_counter()
        parts = []
        for k in keys5:
            parts.append(o.transform_cloud(kfs[k][0], kfs[k][2])); parts.append(o.transform_cloud(kfs[k][1], kfs[k][2]))
        fused = np.concatenate(parts)
        t1 = time.perf_counter()
        o2 = pkg.LidarHotpath(ora, **dict(P, max_map_points=min(1 << 25, len(fused) + 64)))
        o2.voxel_downsample(fused, 0.05)
        t2 = time.perf_counter()
        res["restatement_cpu_ms"] = dict(transform=(t1 - t0) * 1e3, voxel=(t2 - t1) * 1e3, n=len(fused))
        print("restatement", json.dumps(res["restatement_cpu_ms"]), flush=True)
        o2.close()
    h.close()
    if not a.skip_seq:
        H = pkg.host_api
        SEQ = dict(N_SCAN=4, Horizon_SCAN=8192, max_raw_points=20000, max_map_points=600000, max_keyframes=512, max_keyframe_points=1 << 22)
        poses = [S.loop_pose(0.3 + 0.02 * k, 0.004 * np.sin(k), -0.004 * np.cos(k)) for k in range(200)]
        scans = [S.make_scan(16001, p, 3000 + k) for k, p in enumerate(poses)]
        for mode in ("none", "build_every_5s"):
            m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ), incremental_map=1)
            gm = pkg.GlobalMap(m.handle); gm.reserve(1 << 22)
            lat, last = [], -1e9
            for k, sc in enumerate(scans):
                stamp = 20.0 + 0.2 * k
                t0 = time.perf_counter(); r = m.scan(sc, stamp); lat.append(time.perf_counter() - t0)
                if mode != "none" and stamp - last >= 5.0 and r["n_keyframes"] > 0:
                    gm.build(list(range(r["n_keyframes"])), pkg.gmap.CORNER_SURF, 0.05); last = stamp
            lat = np.array(lat[10:]) * 1e3
            res["seq_" + mode] = dict(p50_ms=float(np.median(lat)), p99_ms=float(np.percentile(lat, 99)))
            print("seq", mode, json.dumps(res["seq_" + mode]), flush=True)
            m.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
