"""Cost of one visual-inertial alignment on one GPU (include/lvi_align.h) beside csrc/lvi_align_math.hpp compiled
for the host and run on one thread over the same frames:

  solve     one lvi_align_solve at F = 11, 30 and 100 frames with 20 samples a frame: one upload, gyro, repropagate, five
            times system and factor-solve, one download, one wait.  A solve repropagates every frame, so every round does
            the same work.
  host      gyro_bias, repropagate of every frame and linear_alignment of the header in a stand-alone program
            (g++ -O2 -ffp-contract=off), the three parts timed apart

Wall clock around the Python call, median and p99 over --rounds rounds.  No threshold is set on any of the numbers.  Prints one
JSON line.  The time of each launch comes from a kernel trace of a run of this tool:

    timeout -k 10 300 python tools/diag/align_time.py
    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d D -- python tools/diag/align_time.py --frames 30 --rounds 30 --no-host
    python tools/diag/align_time.py --trace D        # median microseconds per launch of every align_* kernel, by grid size

--lib PATH times another build of liblvi_hip.so (the parent commit's, say) in place of the tree's.
"""
import argparse
import csv
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
#include "lvi_align_math.hpp"
using namespace lvi_align_math;
typedef std::chrono::steady_clock clk;
static double med(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int rounds = atoi(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    double head[8];       // F, samples, TIC, G
    if (!f || fread(head, 8, 8, f) != 8) return 3;
    const int F = (int)head[0], S = (int)head[1];
    std::vector<Frame> fr((size_t)F);
    std::vector<pm::State> st((size_t)F);
    std::vector<std::vector<double>> jac((size_t)F, std::vector<double>(225)), smp((size_t)F, std::vector<double>((size_t)S * 7));
    std::vector<double> lin((size_t)F * 6), work(pm::WORK_DOUBLES);
    for (int i = 0; i < F; i++) {
        double pose[12];
        if (fread(pose, 8, 12, f) != 12 || fread(&lin[6 * i], 8, 6, f) != 6 || fread(smp[i].data(), 8, smp[i].size(), f) != smp[i].size()) return 4;
        for (int k = 0; k < 9; k++) fr[i].R[k] = pose[k];
        for (int k = 0; k < 3; k++) fr[i].T[k] = pose[9 + k];
        fr[i].jacobian = jac[i].data();
    }
    const int nd = 3 * F, stride = sys_doubles(nd, NB_LINEAR);
    std::vector<double> sys((size_t)stride * SYSTEMS), fw((size_t)BW * nd + 4 * (nd + 4)), tg, tr, tl;
    double bg[3] = {0., 0., 0.}, zero[3] = {0., 0., 0.}, sink = 0.;
    auto reprop = [&]() {
        for (int i = 1; i < F; i++) {
            repropagate(st[i], jac[i].data(), &lin[6 * i], &lin[6 * i + 3], zero, bg, S, smp[i].data(), work.data());
            fr[i].pre.sum_dt = st[i].sum_dt;
            for (int k = 0; k < 3; k++) { fr[i].pre.delta_p[k] = st[i].delta_p[k]; fr[i].pre.delta_v[k] = st[i].delta_v[k]; }
            for (int k = 0; k < 4; k++) fr[i].pre.delta_q[k] = st[i].delta_q[k];
        }
    };
    reprop();
    for (int r = 0; r < rounds + 3; r++) {
        Result res{};
        double dbg[3], mp;
        const auto t0 = clk::now();
        gyro_bias(fr.data(), F, dbg, &mp);
        const auto t1 = clk::now();
        for (int k = 0; k < 3; k++) bg[k] = dbg[k] * 0.5;
        reprop();
        const auto t2 = clk::now();
        linear_alignment(fr.data(), F, head + 2, head + 5, sys.data(), fw.data(), res);
        const auto t3 = clk::now();
        sink += res.s + dbg[0];
        if (r >= 3) {
            tg.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            tr.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
            tl.push_back(std::chrono::duration<double, std::micro>(t3 - t2).count());
        }
    }
    printf("%.2f %.2f %.2f %g\n", med(tg), med(tr), med(tl), sink);
    return 0;
}
"""


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 1), p99=round(float(np.percentile(v, 99)), 1))


def _host(pkg, tmp, sc, S, rounds):
    src, exe, dat = os.path.join(tmp, "host.cpp"), os.path.join(tmp, "host"), os.path.join(tmp, f"s{sc['F']}.bin")
    if not os.path.exists(exe):
        open(src, "w").write(HOST)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", exe, src], check=True)
    m = sc["motion"]
    v = [float(sc["F"]), float(S), *m.tic, 0.0, 0.0, 9.8]
    for i in range(sc["F"]):
        dt, acc, gyr = sc["imu"][i]
        prev = sc["imu"][i - 1] if i else sc["imu"][0]
        smp = np.c_[dt, acc, gyr] if i else np.zeros((S, 7))
        v += [*np.asarray(sc["poses"][i][0]).ravel(), *sc["poses"][i][1], *prev[1][-1], *prev[2][-1], *smp.ravel()]
    open(dat, "wb").write(np.array(v, np.float64).tobytes())
    out = subprocess.run([exe, dat, str(rounds)], capture_output=True, text=True, check=True).stdout.split()
    return dict(gyro_us=float(out[0]), repropagate_us=float(out[1]), linear_alignment_us=float(out[2]),
                total_us=round(float(out[0]) + float(out[1]) + float(out[2]), 1))


def _trace(d):
    """median duration of every align_* kernel of a rocprofv3 kernel trace, by grid size"""
    rows = {}
    for base, _, files in os.walk(d):
        for fn in files:
            if not fn.endswith("kernel_trace.csv"):
                continue
            for r in csv.DictReader(open(os.path.join(base, fn))):
                name = r.get("Kernel_Name", "")
                if "align_" not in name:
                    continue
                short = [t for t in ("align_repropagate", "align_gyro", "align_system", "align_factor_solve") if t in name][0]
                key = f"{short} grid {r.get('Grid_Size_X', r.get('Grid_Size', '?'))}"
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: dict(launches=len(v), median_us=round(float(np.median(v)), 1), p99_us=round(float(np.percentile(v, 99)), 1)) for k, v in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--frames", default="11,30,100")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--lib", default=None, help="another build of liblvi_hip.so to time instead of the tree's")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(_trace(a.trace)))
        return
    pkg = graft.import_package()
    import align_ref as R
    hip = pkg._abi.Library(a.lib) if a.lib else pkg.load_hip()
    out = dict(rounds=a.rounds, samples=a.samples)
    with tempfile.TemporaryDirectory() as tmp:
        for F in (int(t) for t in a.frames.split(",")):
            sc = R.imu_scene(500 + F, F, samples=a.samples)
            al = pkg.ImuAligner(hip, max_frames=F, max_samples=a.samples, TIC=tuple(float(t) for t in sc["motion"].tic))
            R.feed(al, sc)
            Bgs = np.zeros((11, 3))
            t, info = [], None
            for k in range(a.rounds + 5):
                t0 = time.perf_counter()
                _, info = al.solve(Bgs)
                if k >= 5:
                    t.append((time.perf_counter() - t0) * 1e6)
            out[f"solve_{F}_us"] = _stats(t)
            out[f"solve_{F}_reason"] = int(info["reason"])
            out[f"solve_{F}_scale_error"] = abs(info["s"] - sc["motion"].s) / sc["motion"].s
            if not a.no_host:
                out[f"solve_{F}_host"] = _host(pkg, tmp, sc, a.samples, a.rounds)
            al.close()
    out["note"] = "wall clock of the Python call; host = gyro_bias, repropagate and linear_alignment of lvi_align_math.hpp on one thread"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
