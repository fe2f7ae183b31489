"""Cost of one pose-graph solve on one GPU (include/lvi_pgo.h) at N = 1024 keys and L = 16 loops of a tests/pgo_ref.scene
circuit: wall clock around lvi_pgo_solve (the whole Gauss-Newton run: every launch of max_iters steps is enqueued, the
steps behind the converged one return at once; one wait), with the graph rebuilt before every call so that each solve
starts from the odometry chain.  Beside it, on the CPU, the linear systems of the same Gauss-Newton run (the reference's
anchored normal equations, tests/pgo_ref.py) solved by scipy's sparse SuperLU without pivoting — the factor-and-solve
time alone, without the Python linearisation.  Two more measurements on the same circuit (include/lvi_pgo_gps.h): the wall
clock of one lvi_pgo_gps_marginal_covariance call at the newest key of the solved graph (what the node pays per keyframe
when GPS is in use), without GPS factors and with them, and one GPS-mode solve with a fix every --gps-every keys (the full
system: key 0 live).  Prints one JSON line.  Kernel times come from a separate rocprofv3 run:

    timeout -k 10 300 python tools/diag/pgo_time.py
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d pgo_prof -o pgo -- python tools/diag/pgo_time.py --calls 20 --no-cpu
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
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--loops", type=int, default=16)
    ap.add_argument("--gps-every", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import pgo_ref as R
    n, nl = a.keys, a.loops
    rs = np.random.RandomState(3)
    loops = [(n - 1, 0)] + [(int(f), int(t)) for f, t in zip(rs.randint(n // 2, n, nl - 1), rs.randint(0, n // 2 - 1, nl - 1))]
    sc = R.scene(n, loops, 21)
    g = pkg.PoseGraph(pkg.load_hip(), max_poses=n, max_loops=nl)
    wall, build, info = [], [], None
    for k in range(a.calls + 3):
        g.clear()
        t0 = time.perf_counter()
        R.build(sc, g)
        t1 = time.perf_counter()
        info = g.solve()
        t2 = time.perf_counter()
        if k >= 3:
            build.append((t1 - t0) * 1e6); wall.append((t2 - t1) * 1e6)
    # the covariance call at the newest key of the solved graph, without GPS factors (the gauge split)
    cov = []
    for k in range(a.calls + 3):
        t0 = time.perf_counter()
        g.marginal_covariance(n - 1)
        if k >= 3:
            cov.append((time.perf_counter() - t0) * 1e6)
    # GPS mode: a fix every gps_every keys (ground truth + N(0, 0.3 m), variances 1, 2, 1), the solve and the covariance call
    g.set_params(max_iters=30)
    fixes = [(k, (sc["gt"][k][:3, 3] + rs.normal(0, 0.3, 3)).astype(np.float32)) for k in range(0, n, a.gps_every)]
    gwall, gcov, ginfo = [], [], None
    for k in range(a.calls + 3):
        g.clear()
        R.build(sc, g)
        for key, z in fixes:
            g.add_gps(key, z, [1.0, 2.0, 1.0])
        t1 = time.perf_counter()
        ginfo = g.solve()
        t2 = time.perf_counter()
        g.marginal_covariance(n - 1)
        t3 = time.perf_counter()
        if k >= 3:
            gwall.append((t2 - t1) * 1e6); gcov.append((t3 - t2) * 1e6)
    g.close()
    gps = dict(fixes=len(fixes), max_iters=30, solve_wall_us=_stats(gwall), iterations=ginfo["iterations"], converged=ginfo["converged"],
               chi2_before=ginfo["chi2_before"], chi2_after=ginfo["chi2_after"], covariance_wall_us=_stats(gcov))
    out = dict(keys=n, loops=nl, covariance_wall_us=_stats(cov), gps=gps, solve_wall_us=_stats(wall), graph_build_python_us=_stats(build), iterations=info["iterations"], converged=info["converged"],
               max_iters=10, chi2_before=info["chi2_before"], chi2_after=info["chi2_after"])
    if not a.no_cpu:
        ref = R.build(sc, R.Graph(1))
        per_iter, its = [], 0
        for _ in range(R.MAX_ITERS):
            J, r = ref.linear_system(True)
            r0, B0 = R.prior_error(ref.X[0], ref.Zc[0], 1)
            d0 = np.linalg.solve(B0, -r0)
            Jr = J[6:, :].tocsc()
            rr = r[6:] + Jr[:, :6] @ d0
            Jc = Jr[:, 6:].tocsc()
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                d = R._solve_ls(Jc, rr, "chol", True)
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            per_iter.append(best)
            d = np.r_[d0, d]
            for k in range(n):
                ref.X[k] = ref.X[k] @ R.pose_exp(d[6 * k:6 * k + 6], 1)
            its += 1
            if np.abs(d).max() < R.CONV_EPS:
                break
        out.update(cpu_sparse_iterations=its, cpu_sparse_solve_us_per_iteration=round(float(np.median(per_iter)), 1), cpu_sparse_solve_us_total=round(float(np.sum(per_iter)), 1),
                   cpu_chi2_after=ref.chi2())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
