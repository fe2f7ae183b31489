// Driver of tests/test_gpu_preint.py::test_cpp_mirror_equals_the_python_class: lvi_host::ImuPreintegrator
// (host/lvi_preint_host.hpp) over a 12-image sequence, beside a VinsWindowOptimizer and a VinsMarginalizer it fills.
//
// input (doubles): max_samples, images; per image: n, slide (0 none, 1 old, 2 new), n x (dt, acc [3], gyr [3]), and for an
// image with a slide the window arrays para_Pose [11][7], para_SpeedBias [11][9] and the navigation state (21).
// output (bytes), per image with a slide: preIntegrations [10] with hasImu [10] as doubles, imuSumDt, imuResidual [15],
// imuJacobians [480]; then the records of all eleven slots after the slide and the navigation state.
// After the images, input: mask, Bas [11][3], Bgs [11][3] for one repropagate (output: the eleven records); then T [11][3],
// R [11][9], Ba, Bg [11][3], gravity, ric [9] and three samples for lidarInitialise over an empty feature table, first with
// reset_id[4] = -1 (output: 0.0 and the eleven records, unchanged), then with equal ids (output: 1.0, params.G, the eleven
// records), and a flush of the three samples into slot 10 (output: its record and the navigation state, stepped with the new G).
#include <cstdio>
#include <vector>

#include "lvi_marg_host.hpp"
#include "lvi_preint_host.hpp"
#include "lvi_win_host.hpp"

using namespace lvi_host;

static bool rd(FILE* f, double* v, size_t n) { return fread(v, sizeof(double), n, f) == n; }
static void wr(FILE* f, const void* v, size_t bytes) { fwrite(v, 1, bytes, f); }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    try {
        double head[2];
        if (!rd(in, head, 2)) return 4;
        ImuPreintegrator pre(0, (int)head[0]);
        VinsMarginalizer marg(0, 16, true);
        VinsWindowOptimizer opt(marg, 0, 16);
        int frame_count = 0;
        for (int image = 0; image < (int)head[1]; image++) {
            double h2[2];
            if (!rd(in, h2, 2)) return 5;
            const int n = (int)h2[0], slide = (int)h2[1];
            for (int k = 0; k < n; k++) {
                double s[7];
                if (!rd(in, s, 7)) return 6;
                pre.processIMU(s[0], s + 1, s + 4);
            }
            pre.flush(frame_count);
            if (!slide) { frame_count++; continue; }
            lvi_preint_nav nav;
            if (!rd(in, &marg.paraPose[0][0], 77) || !rd(in, &marg.paraSpeedBias[0][0], 99) || !rd(in, nav.P, 21)) return 7;
            pre.fillWindow(opt);
            pre.fillMarginalizer(marg);
            wr(out, opt.preIntegrations, sizeof(opt.preIntegrations));
            for (int j = 0; j < 10; j++) { const double v = opt.hasImu[j] ? 1. : 0.; wr(out, &v, 8); }
            const double has = marg.hasImu ? 1. : 0.;
            wr(out, &has, 8); wr(out, &marg.imuSumDt, 8); wr(out, marg.imuResidual, sizeof(marg.imuResidual)); wr(out, marg.imuJacobians, sizeof(marg.imuJacobians));
            pre.setNav(nav.P, nav.R, nav.V, nav.Ba, nav.Bg);
            if (slide == 1) pre.slideWindowOld(); else pre.slideWindowNew();
            for (int j = 0; j <= 10; j++) { const lvi_win_imu r = pre.record(j); wr(out, &r, sizeof(r)); }
            nav = pre.nav();
            wr(out, &nav, sizeof(nav));
        }
        const auto records = [&]() { for (int j = 0; j <= 10; j++) { const lvi_win_imu r = pre.record(j); wr(out, &r, sizeof(r)); } };
        double tail[67];
        if (!rd(in, tail, 67)) return 9;
        pre.repropagate(tail + 1, tail + 34, (uint32_t)tail[0]);
        records();
        double T[33], R[99], Ba[33], Bg[33], gr[10], smp[21];
        if (!rd(in, T, 33) || !rd(in, R, 99) || !rd(in, Ba, 33) || !rd(in, Bg, 33) || !rd(in, gr, 10) || !rd(in, smp, 21)) return 10;
        FeatureManager fman(0, 8);
        int reset_id[11] = {3, 3, 3, 3, -1, 3, 3, 3, 3, 3, 3};
        double ok = pre.lidarInitialise(fman, reset_id, T, R, Ba, Bg, gr[0], gr + 1) ? 1. : 0.;
        wr(out, &ok, 8);
        records();
        reset_id[4] = 3;
        ok = pre.lidarInitialise(fman, reset_id, T, R, Ba, Bg, gr[0], gr + 1) ? 1. : 0.;
        wr(out, &ok, 8); wr(out, pre.params.G, sizeof(pre.params.G));
        records();
        for (int k = 0; k < 3; k++) pre.processIMU(smp[7 * k], smp + 7 * k + 1, smp + 7 * k + 4);
        pre.flush(10);
        const lvi_win_imu r10 = pre.record(10);
        const lvi_preint_nav n10 = pre.nav();
        wr(out, &r10, sizeof(r10)); wr(out, &n10, sizeof(n10));
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 8;
    }
    fclose(in);
    fclose(out);
    return 0;
}
