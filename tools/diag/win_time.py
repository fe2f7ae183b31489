"""Cost of one window solve on one GPU (include/lvi_win.h) at the workload's size: 11 frames, 120 features x 10
observations (1200 projection factors with td), a prior, 10 IMU factors, 10 iterations: wall clock around lvi_win_solve
(the upload, every launch, the downloads of the loop) and the iterations it took.  Beside it, on the CPU, numpy over LAPACK
forming and solving the same reduced system ten times from an already accumulated H, W and h (NOT Ceres, and without the
factor evaluation and the accumulation), and the wall clock of the lvi_marg_get_prior download the resident route removes.
No threshold is set on any of the numbers.  Prints one JSON line.

    timeout -k 10 300 python tools/diag/win_time.py
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--features", type=int, default=120)
    ap.add_argument("--iterations", type=int, default=10)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import marg_ref as M
    import win_ref as R
    import win_scenes as S
    sc = S.make_scene(51, 11, [11] * a.features)
    hip = pkg.load_hip()
    w = pkg.WindowSolver(hip, max_blocks=64 + a.features, max_projections=10 * a.features, max_eliminated=a.features, max_imu=10, max_prior_rows=64, max_dim=176)
    P = dict(R.DEFAULTS)
    P.update(sc["params"], max_iterations=a.iterations)
    w.set_params(**P)
    recs = [op[1] for op in sc["ops"] if op[0] == "proj"]
    rec_arr = np.zeros(len(recs), w.record_dtype)
    for k, r in enumerate(recs):
        for key, v in r.items():
            rec_arr[k][key] = v
    imus = [op[1] for op in sc["ops"] if op[0] == "imu"]
    imu_arr = np.zeros(len(imus), w.imu_dtype)
    for k, r in enumerate(imus):
        for key, v in r.items():
            imu_arr[k][key] = v
    prior = [op[1] for op in sc["ops"] if op[0] == "prior"][0]

    def declare():
        w.begin()
        for op in sc["ops"]:
            if op[0] == "block":
                w.set_block(op[1], op[2], op[3])
        w.add_projection(rec_arr)
        w.add_imu(imu_arr)
        w.set_prior(prior["J"], prior["r"], prior["ids"], prior["sizes"], prior["col"], prior["x0"])
    wall, info = [], None
    for k in range(a.calls + 3):
        declare()
        t0 = time.perf_counter()
        info = w.solve()
        if k >= 3:
            wall.append((time.perf_counter() - t0) * 1e6)
    log = w.log()
    declare()
    s = w.debug_system()
    w.close()
    out = dict(features=a.features, projection_factors=len(recs), imu_factors=len(imus), dim=info["dim"], eliminated=info["eliminated"], iterations=info["iterations"],
               termination=info["termination"], accepted=sum(e["accepted"] for e in log), initial_cost=info["initial_cost"], final_cost=info["final_cost"],
               solve_wall_us=_stats(wall), per_iteration_us=round(float(np.median(wall)) / max(1, info["iterations"]), 1))
    cpu = []
    H, W, h, g, gf = s["H"], s["W"], s["hdiag"], s["g"], s["gf"]
    for _ in range(10):
        t0 = time.perf_counter()
        for _ in range(a.iterations):
            Wh = W / h[:, None]
            Sm = H + 1e-8 * np.diag(np.diag(H)) - W.T @ Wh
            b = g - Wh.T @ gf
            L = np.linalg.cholesky(Sm)
            y = np.linalg.solve(L.T, np.linalg.solve(L, -b))
        cpu.append((time.perf_counter() - t0) * 1e6)
    out.update(numpy_schur_cholesky_us=_stats(cpu), numpy_check=float(np.abs(Sm @ y + b).max()),
               numpy_note=f"numpy over LAPACK, {a.iterations} reduced systems from an accumulated H, W, h: not Ceres, no factor evaluation, no accumulation")
    win0, feats = M.make_window(41, a.features)
    imu = M.imu_block(42, 1e6)
    V = pkg.host_api.VinsMarginalizer(pkg.load_host(), hip, max_features=a.features, estimate_td=True)
    V.set_window(win0["pose"], win0["speed_bias"], win0["ex"], win0["td"])
    V.set_features(feats)
    V.set_imu(0.5, imu["residual"], imu["jacobians"])
    n = V.run(V.MARGIN_OLD)["n"]
    dl = []
    for _ in range(a.calls + 3):
        t0 = time.perf_counter()
        V.marg.prior()
        dl.append((time.perf_counter() - t0) * 1e6)
    V.close()
    out.update(prior_n=n, get_prior_download_us=_stats(dl[3:]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
