// Driver of tests/test_gpu_align.py::test_cpp_mirror_equals_the_python_class: lvi_host::ImageFrames and
// lvi_host::VisualIMUAlignment (host/lvi_align_host.hpp).
//
// input (doubles): max_frames, max_samples, TIC [3], G [3], Bgs [33], F; per frame: stamp, n, n x (dt, acc [3], gyr [3]); then
// per frame: R [9], T [3], is_key_frame.
// output (doubles): ok, reason, n_state, frames, excitation, Bgs [33], g [3], delta_bg [3], s, min_pivot [6], x [n_state].
#include <cstdio>
#include <vector>

#include "lvi_align_host.hpp"

using namespace lvi_host;

static bool rd(FILE* f, double* v, size_t n) { return fread(v, sizeof(double), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    try {
        double head[42];
        if (!rd(in, head, 42)) return 4;
        const int F = (int)head[41];
        if (F < 0 || F > head[0]) return 5;
        lvi_align_params p;
        lvi_align_params_default(&p);
        for (int k = 0; k < 3; k++) { p.TIC[k] = head[2 + k]; p.G[k] = head[5 + k]; }
        ImageFrames all_image_frame(0, (int)head[0], (int)head[1], &p);
        std::vector<double> stamps((size_t)F);
        const double zero[3] = {0., 0., 0.};
        for (int i = 0; i < F; i++) {
            double sn[2];
            if (!rd(in, sn, 2) || sn[1] < 0 || sn[1] > head[1]) return 6;
            const int n = (int)sn[1];
            std::vector<double> smp(7 * (size_t)n), dt((size_t)n), acc(3 * (size_t)n), gyr(3 * (size_t)n);
            if (!rd(in, smp.data(), smp.size())) return 7;
            for (int k = 0; k < n; k++) {
                dt[k] = smp[7 * k];
                for (int a = 0; a < 3; a++) { acc[3 * k + a] = smp[7 * k + 1 + a]; gyr[3 * k + a] = smp[7 * k + 4 + a]; }
            }
            all_image_frame.pushIMU(n, dt.data(), acc.data(), gyr.data());
            all_image_frame.insert(sn[0], zero, zero);
            stamps[i] = sn[0];
        }
        for (int i = 0; i < F; i++) {
            double pose[13];
            if (!rd(in, pose, 13)) return 8;
            all_image_frame.setPose(stamps[i], pose, pose + 9, pose[12] != 0.);
        }
        const double var = all_image_frame.excitation();
        double Bgs[33], g[3];
        for (int k = 0; k < 33; k++) Bgs[k] = head[8 + k];
        std::vector<double> x;
        const bool ok = VisualIMUAlignment(all_image_frame, Bgs, g, x);
        const lvi_align_info& li = all_image_frame.last;
        const double rec[5] = {ok ? 1. : 0., (double)li.reason, (double)li.n_state, (double)li.frames, var};
        fwrite(rec, sizeof(double), 5, out);
        fwrite(Bgs, sizeof(double), 33, out);
        fwrite(g, sizeof(double), 3, out);
        fwrite(li.delta_bg, sizeof(double), 3, out);
        fwrite(&li.s, sizeof(double), 1, out);
        fwrite(li.min_pivot, sizeof(double), 6, out);
        fwrite(x.data(), sizeof(double), x.size(), out);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 9;
    }
    fclose(in);
    fclose(out);
    return 0;
}
