"""Cost of one MARGIN_OLD marginalisation on one GPU (include/lvi_marg.h) at 120 features x 10 frames (1200
projection factors with td), with the previous prior resident on the device and an IMU-like dense block: wall clock around
VinsMarginalizer.run (window upload, every launch, one wait, the address shift), and the m, n, rank and sweeps of the call.
Beside it, on the CPU, the numpy restatement of the same system (tests/marg_ref.py): the two LAPACK eigendecompositions,
the pseudo-inverse, the Schur complement and the factoring, from an already accumulated A and b.  That is numpy over
LAPACK, NOT the reference's Eigen code with its four accumulation threads; no threshold is set on either number.
Prints one JSON line.  Kernel times come from a separate rocprofv3 run:

    timeout -k 10 300 python tools/diag/marg_time.py
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d marg_prof -o marg -- python tools/diag/marg_time.py --calls 20 --no-cpu
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--features", type=int, default=120)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import marg_ref as R
    win, feats = R.make_window(41, a.features)                       # every feature starts in frame 0 and is seen from all 11 frames
    imu = R.imu_block(42, 1e6)
    V = pkg.host_api.VinsMarginalizer(pkg.load_host(), pkg.load_hip(), max_features=a.features, estimate_td=True)
    V.set_window(win["pose"], win["speed_bias"], win["ex"], win["td"])
    V.set_features(feats)
    V.set_imu(0.5, imu["residual"], imu["jacobians"])
    wall, info = [], None
    for k in range(a.calls + 3):                                     # the first call has no prior; every later one consumes the previous result
        t0 = time.perf_counter()
        info = V.run(V.MARGIN_OLD)
        if k >= 3:
            wall.append((time.perf_counter() - t0) * 1e6)
    V.close()
    out = dict(features=a.features, projection_factors=sum(len(f["obs"]) - 1 for f in feats), m=info["m"], n=info["n"], rank=info["rank"], status=info["status"],
               sweeps=[info["sweeps_mm"], info["sweeps_rr"]], marginalize_wall_us=_stats(wall))
    if not a.no_cpu:
        prior = R.vins_marginalize(R.F64, None, R.MARGIN_OLD, win, feats, imu)
        M = R.Marg(R.F64)
        R.declare_window(M, win)
        M.add_prior(prior, [R.ID_POSE, R.ID_SPEEDBIAS])
        M.add_dense([R.ID_POSE, R.ID_SPEEDBIAS, R.ID_POSE + 1, R.ID_SPEEDBIAS + 1], imu["residual"], imu["jacobians"], [1, 1, 0, 0])
        recs, fblocks = R.vins_projections(win, feats, True)
        for b, v in fblocks.items():
            M.set_block(b, [v])
        for rec in recs:
            M.add_projection(rec)
        A, b, m, n = M.system()
        cpu = []
        for _ in range(10):
            t0 = time.perf_counter()
            Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
            w, Q = np.linalg.eigh(Amm)
            Ai = (Q * np.where(w > R.EPS, 1.0 / np.where(w > R.EPS, w, 1.0), 0.0)) @ Q.T
            H = A[m:, m:] - A[m:, :m] @ Ai @ A[:m, m:]
            g = b[m:] - A[m:, :m] @ Ai @ b[:m]
            w2, Q2 = np.linalg.eigh(H)
            S = np.where(w2 > R.EPS, w2, 0.0)
            J = (Q2 * np.sqrt(S)).T
            r = np.sqrt(np.where(w2 > R.EPS, 1.0 / np.where(w2 > R.EPS, w2, 1.0), 0.0)) * (Q2.T @ g)
            cpu.append((time.perf_counter() - t0) * 1e6)
        out.update(numpy_eig_schur_us=_stats(cpu), numpy_note="numpy over LAPACK from an accumulated A, b: not the reference's Eigen code, and without its accumulation",
                   numpy_m=m, numpy_n=n, numpy_rank=int((w2 > R.EPS).sum()), numpy_check=float(np.abs(J.T @ r - g).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
