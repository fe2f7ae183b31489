"""Cost of the IMU preintegration on one GPU (include/lvi_preint.h) beside csrc/lvi_preint_math.hpp compiled for
the host and run on one thread over the same samples:

  flush          one push of 20 samples into slot 10: the call alone (it does not wait) and launch-to-ready (the call plus
                 the read of the navigation state, which waits)
  repropagate    all eleven slots with 20 and with 200 samples each, one launch, to ready
  slide_new      slot 10's 20 samples pushed onto slot 9, to ready

Wall clock around the Python calls, median and p99 over --rounds rounds; every timed call starts from the same state, which
is rebuilt outside the timed window.  The host column is the median of the same arithmetic in a stand-alone program (g++ -O2
-ffp-contract=off), the eleven chains one after the other.  No threshold is set on any of the numbers.  Prints one JSON line.

    timeout -k 10 300 python tools/diag/preint_time.py

--lib PATH times another build of liblvi_hip.so (the parent commit's, say) in place of the tree's.
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
#include "lvi_preint_math.hpp"
using namespace lvi_preint_math;
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const int n = atoi(argv[2]), chains = atoi(argv[3]), rounds = atoi(argv[4]);
    FILE* f = fopen(argv[1], "rb");
    if (!f || n < 1) return 3;
    std::vector<double> dt(n), acc(3 * (size_t)n), gyr(3 * (size_t)n), us;
    if (fread(dt.data(), 8, dt.size(), f) != dt.size() || fread(acc.data(), 8, acc.size(), f) != acc.size() || fread(gyr.data(), 8, gyr.size(), f) != gyr.size()) return 4;
    double q[NV], J[225], C[225], work[WORK_DOUBLES], sink = 0;
    noise_diag(0.08, 0.004, 0.00004, 2.0e-6, q);
    const double ba[3] = {0.01, -0.02, 0.015}, bg[3] = {0.001, 0.002, -0.0015};
    for (int r = 0; r < rounds + 5; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int c = 0; c < chains; c++) {
            State s;
            state_reset(s, acc.data(), gyr.data(), ba, bg);
            matrices_reset(J, C);
            integrate(s, J, C, q, n, dt.data(), acc.data(), gyr.data(), work);
            sink += C[0] + s.delta_p[0];
        }
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 5) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("%.2f %.17g\n", us[us.size() / 2], sink);
    return 0;
}
"""


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 1), p99=round(float(np.percentile(v, 99)), 1))


def _host(pkg, tmp, dt, acc, gyr, chains, rounds):
    src, exe, dat = os.path.join(tmp, "host.cpp"), os.path.join(tmp, "host"), os.path.join(tmp, f"s{len(dt)}.bin")
    if not os.path.exists(exe):
        open(src, "w").write(HOST)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", exe, src], check=True)
    open(dat, "wb").write(dt.tobytes() + acc.tobytes() + gyr.tobytes())
    out = subprocess.run([exe, dat, str(len(dt)), str(chains), str(rounds)], capture_output=True, text=True, check=True).stdout
    return float(out.split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--lib", default=None, help="another build of liblvi_hip.so to time instead of the tree's")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    import preint_ref as R
    hip = pkg._abi.Library(a.lib) if a.lib else pkg.load_hip()
    w = pkg.ImuWindow(hip, max_samples=512)
    nav = dict(P=np.zeros(3), R=np.eye(3), V=np.array([1.0, 0.0, 0.0]), Ba=np.array([0.01, -0.02, 0.015]), Bg=np.array([0.001, 0.002, -0.0015]))
    s20, s200 = R.samples(1, 20), R.samples(2, 200)
    Bas, Bgs = np.tile(nav["Ba"], (11, 1)), np.tile(nav["Bg"], (11, 1))
    out = dict(rounds=a.rounds, chunk=pkg.preint.CHUNK, barriers_per_step=2, barriers_per_chunk=3)
    with tempfile.TemporaryDirectory() as tmp:
        def fill(samples):
            w.clear()
            w.set_nav(**nav)
            for _ in range(11):
                w.push(10, *samples)
                w.slide_old()
            w.push(10, *samples)
            w.nav()

        # flush and slide_new: slots 9 and 10 hold 20 samples before the slide, slot 10 is fresh before the flush
        fill(s20)
        call, ready, slide = [], [], []
        for k in range(a.rounds + 5):
            w.slide_old()
            w.nav()
            t0 = time.perf_counter()
            w.push(10, *s20)
            t1 = time.perf_counter()
            w.nav()
            t2 = time.perf_counter()
            w.slide_old()
            w.push(10, *s20)
            w.nav()
            t3 = time.perf_counter()
            w.slide_new()
            w.nav()
            t4 = time.perf_counter()
            w.push(10, *s20)
            if k >= 5:
                call.append((t1 - t0) * 1e6)
                ready.append((t2 - t0) * 1e6)
                slide.append((t4 - t3) * 1e6)
        out.update(flush_20_call_us=_stats(call), flush_20_ready_us=_stats(ready), flush_20_host_us=_host(pkg, tmp, *s20, 1, a.rounds),
                   slide_new_20_ready_us=_stats(slide), slide_new_20_host_us=_host(pkg, tmp, *s20, 1, a.rounds))
        for name, smp in (("20", s20), ("200", s200)):
            fill(smp)
            t = []
            for k in range(a.rounds + 5):
                t0 = time.perf_counter()
                w.repropagate(Bas, Bgs)
                w.nav()
                if k >= 5:
                    t.append((time.perf_counter() - t0) * 1e6)
            out[f"repropagate_11x{name}_ready_us"] = _stats(t)
            out[f"repropagate_11x{name}_host_us"] = _host(pkg, tmp, *smp, 11, a.rounds)
        t = []
        for k in range(a.rounds + 5):
            t0 = time.perf_counter()
            w.nav()
            if k >= 5:
                t.append((time.perf_counter() - t0) * 1e6)
        out["read_nav_alone_us"] = _stats(t)
    w.close()
    out["note"] = "ready = the call plus the read of the navigation state (one 168-byte download and the wait); read_nav_alone is that read on an idle stream"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
