// Driver of tests/test_gpu_relpose.py::test_cpp_mirror_equals_the_python_class: lvi_host::MotionEstimator and
// lvi_host::relativePose (host/lvi_relpose_host.hpp) over lvi_host::FeatureManager.
//
// input (doubles): max_points, windows; per window eleven frames, each: n, then n x (id, obs [8]).
// output (doubles), per window: ok, l, relative_R [9], relative_T [3], and of the last solveRelativeRT the flags, the
// inlier count, the chosen candidate and the average parallax.
#include <cstdio>
#include <vector>

#include "lvi_relpose_host.hpp"

using namespace lvi_host;

static bool rd(FILE* f, double* v, size_t n) { return fread(v, sizeof(double), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    try {
        double head[2];
        if (!rd(in, head, 2)) return 4;
        MotionEstimator m_estimator(0, (int)head[0]);
        FeatureManager f_manager(0, (int)head[0]);
        for (int w = 0; w < (int)head[1]; w++) {
            f_manager.clearState();
            for (int frame = 0; frame <= FeatureManager::WINDOW_SIZE; frame++) {
                double n = 0;
                if (!rd(in, &n, 1) || n < 0 || n > head[0]) return 5;
                std::vector<int32_t> ids((size_t)n);
                std::vector<double> obs(8 * (size_t)n);
                for (size_t k = 0; k < (size_t)n; k++) {
                    double rec[9];
                    if (!rd(in, rec, 9)) return 6;
                    ids[k] = (int32_t)rec[0];
                    for (int c = 0; c < 8; c++) obs[8 * k + c] = rec[1 + c];
                }
                f_manager.addFeatureCheckParallax(frame, (int)n, ids.data(), obs.data(), 0.0);
            }
            double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};
            int l = -1;
            m_estimator.last = lvi_relpose_result{};
            const bool ok = relativePose(f_manager, m_estimator, R, T, l);
            const double rec[18] = {ok ? 1. : 0., (double)l, R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], T[0], T[1], T[2],
                                    (double)m_estimator.last.flags, (double)m_estimator.last.pose.n_inliers, (double)m_estimator.last.pose.chosen,
                                    m_estimator.last.average_parallax};
            fwrite(rec, sizeof(double), 18, out);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 8;
    }
    fclose(in);
    fclose(out);
    return 0;
}
