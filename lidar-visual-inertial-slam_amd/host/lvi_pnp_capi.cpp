// C entry points over the loop confirmation of the host mirror (lvi_pnp_host.hpp): PnPRansac and the LoopDetector's
// usePnP hook, for replay harnesses that are not C++.  include/lvi_pnp.h is exported by liblvi_hip.so only, so this file
// is linked into host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.

#include "lvi_bow_capi_detail.hpp"
#include "lvi_pnp_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;
using lvi_host_capi::Detector;

extern "C" {

const char* lvh_pnp_last_error(void) { return g_err.c_str(); }

void* lvh_pnp_create(int32_t device, int32_t max_points, int32_t max_iters)
{
    try { return new PnPRansac(device, max_points, max_iters); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_pnp_destroy(void* p) { delete static_cast<PnPRansac*>(p); }

lvi_pnp* lvh_pnp_handle(void* p) { return p ? static_cast<PnPRansac*>(p)->get() : nullptr; }

// PnPRansac::status: matched_2d_old_norm [n][2], matched_3d [n][3] -> status [n]
int32_t lvh_pnp_status(void* p, const float* matched_2d_old_norm, const float* matched_3d, int32_t n, uint8_t* status)
{
    if (!p || n < 0 || (n > 0 && (!matched_2d_old_norm || !matched_3d || !status))) return fail("bad arguments");
    return guarded([&]() -> int32_t {
        std::vector<Point2f> a(n);
        std::vector<Point3f> b(n);
        for (int i = 0; i < n; i++) {
            a[i] = Point2f{matched_2d_old_norm[2 * i], matched_2d_old_norm[2 * i + 1]};
            b[i] = Point3f{matched_3d[3 * i], matched_3d[3 * i + 1], matched_3d[3 * i + 2]};
        }
        const std::vector<uint8_t> st = static_cast<PnPRansac*>(p)->status(a, b);
        for (int i = 0; i < n; i++) status[i] = st[i];
        return LVI_OK;
    });
}

// LoopDetector::usePnP on the detector of lvh_bow_create; pnp = NULL removes the hook.  The PnPRansac must outlive its use.
int32_t lvh_bow_use_pnp(void* d, void* pnp)
{
    if (!d) return fail("null argument");
    static_cast<Detector*>(d)->ld.usePnP(static_cast<PnPRansac*>(pnp));
    return LVI_OK;
}

// what PnPRANSAC received and answered in the last addKeyFrame: matched_3d [n][3], matched_2d_old_norm [n][2],
// status [n] (any may be NULL); returns n, 0 when PnPRANSAC did not run
int32_t lvh_bow_pnp_connection(void* d, float* matched_3d, float* matched_2d_old_norm, uint8_t* status)
{
    if (!d) return fail("null argument");
    const Connection& c = static_cast<Detector*>(d)->last.connection;
    const size_t n = c.pnp_status.size();
    if (matched_3d) for (size_t i = 0; i < n; i++) { matched_3d[3 * i] = c.front_3d[i].x; matched_3d[3 * i + 1] = c.front_3d[i].y; matched_3d[3 * i + 2] = c.front_3d[i].z; }
    if (matched_2d_old_norm) for (size_t i = 0; i < n; i++) { matched_2d_old_norm[2 * i] = c.front_2d_old_norm[i].x; matched_2d_old_norm[2 * i + 1] = c.front_2d_old_norm[i].y; }
    if (status) for (size_t i = 0; i < n; i++) status[i] = c.pnp_status[i];
    return (int32_t)n;
}

}  // extern "C"
