"""Cost of the initial two-view pose on one GPU (include/lvi_relpose.h) beside csrc/lvi_relpose_math.hpp compiled
for the host and run on one thread over the same points:

  recover   one lvi_relpose_recover at n = 150 and n = 2500 on a 7-point F: upload, two launches, download, wait
  solve     one lvi_relpose_solve at n = 150 with no outliers and with 0.3: the float rounding, lvi_fmat_find (its own upload,
            kernels, download and wait), then recover; the share of lvi_fmat_find is timed beside it on a handle of its own
  find      Estimator::relativePose on a 300-feature table whose first frame passes: one lvi_fman_corresponding, the host
            parallax, one solve

Wall clock around the Python calls, median and p99 over --rounds rounds.  The host column is the median of recover_serial
of the header in a stand-alone program (g++ -O2 -ffp-contract=off): the decomposition and 4 n null vectors one after the
other.  The RANSAC has no host column: the header does not hold it.  No threshold is set on any of the numbers.  Prints one
JSON line.

    timeout -k 10 300 python tools/diag/relpose_time.py
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

HOST = r"""
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvi_relpose_math.hpp"
using namespace lvi_relpose_math;
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int n = atoi(argv[2]), rounds = atoi(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    if (!f || n < 1) return 3;
    double E[9];
    std::vector<float> pts(4 * (size_t)n);
    std::vector<unsigned char> in(n), masks(4 * (size_t)n);
    if (fread(E, 8, 9, f) != 9 || fread(pts.data(), 4, pts.size(), f) != pts.size() || fread(in.data(), 1, in.size(), f) != in.size()) return 4;
    std::vector<double> us;
    long sink = 0;
    for (int r = 0; r < rounds + 5; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        Pose p;
        double cand[4][12];
        recover_serial(E, pts.data(), in.data(), n, 50.0, p, cand, masks.data());
        const auto t1 = std::chrono::steady_clock::now();
        sink += p.n_inliers;
        if (r >= 5) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("%.2f %ld\n", us[us.size() / 2], sink);
    return 0;
}
"""


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 1), p99=round(float(np.percentile(v, 99)), 1))


def _host(pkg, tmp, E, p1, p2, mask, rounds):
    src, exe, dat = os.path.join(tmp, "host.cpp"), os.path.join(tmp, "host"), os.path.join(tmp, f"s{len(p1)}.bin")
    if not os.path.exists(exe):
        open(src, "w").write(HOST)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", exe, src], check=True)
    open(dat, "wb").write(np.asarray(E, np.float64).tobytes() + np.c_[p1, p2].astype(np.float32).tobytes() + np.asarray(mask, np.uint8).tobytes())
    out = subprocess.run([exe, dat, str(len(p1)), str(rounds)], capture_output=True, text=True, check=True).stdout
    return float(out.split()[0])


def _timed(fn, rounds):
    t = []
    for k in range(rounds + 5):
        t0 = time.perf_counter()
        fn()
        if k >= 5:
            t.append((time.perf_counter() - t0) * 1e6)
    return _stats(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import fman_ref as FM
    import relpose_ref as R
    hip = pkg.load_hip()
    rp = pkg.RelativePose(hip, max_points=2500)
    fr = pkg.FundamentalRansac(hip, max_points=2500)
    out = dict(rounds=a.rounds, chunk=pkg.relpose.CHUNK)
    with tempfile.TemporaryDirectory() as tmp:
        for n in (150, 2500):
            p1, p2, *_ = R.two_view(900 + n, n, noise=0.1 / R.FOCAL)
            s = rp.solve(R.pairs_of(p1, p2))                       # a 7-point F and its status: what solveRelativeRT hands to recoverPose
            E, mask = s["info"]["F"], s["status"]
            out[f"recover_{n}_us"] = _timed(lambda: rp.recover(E, p1, p2, mask), a.rounds)
            out[f"recover_{n}_host_us"] = _host(pkg, tmp, E, p1, p2, mask, a.rounds)
            out[f"recover_{n}_inliers"] = int(s["pose"]["n_inliers"])
        for o in (0.0, 0.3):
            p1, p2, *_ = R.two_view(950, 150, noise=0.1 / R.FOCAL, outliers=o)
            pairs = R.pairs_of(p1, p2)
            s = rp.solve(pairs)
            out[f"solve_150_outliers_{o}_us"] = _timed(lambda: rp.solve(pairs), a.rounds)
            out[f"solve_150_outliers_{o}_fmat_find_us"] = _timed(lambda: fr.find(p1, p2, R.THRESHOLD), a.rounds)
            out[f"solve_150_outliers_{o}_iterations"] = int(s["info"]["iters"])
            out[f"solve_150_outliers_{o}_host_recover_us"] = _host(pkg, tmp, s["info"]["F"], p1, p2, s["status"], a.rounds)
        tab = pkg.FeatureTable(hip, max_features=512)
        FM.load(tab, R.window_frames("first", seed=9, n=300))
        ok, l, *_ = rp.find(tab)
        out.update(find_300_ok=bool(ok), find_300_l=int(l), find_300_us=_timed(lambda: rp.find(tab), a.rounds),
                   find_300_corresponding_us=_timed(lambda: tab.corresponding(0, 10), a.rounds))
        tab.close()
    rp.close()
    fr.close()
    out["note"] = "wall clock of the Python call; host = recover_serial of lvi_relpose_math.hpp on one thread, the RANSAC not included"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
