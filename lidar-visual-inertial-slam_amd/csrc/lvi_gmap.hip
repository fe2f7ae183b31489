// C-ABI of the global map (include/lvi_gmap.h): publishGlobalMap's and save_map's fuse + VoxelGrid
// (mapOptimization.cpp:179-236, :460-510) over the device keyframe store, on a stream of its own.
//
// No kernel of its own: the fuse is kf_assemble_kernel (lvi_icp.hip) driven by a piece table whose two output
// pointers both address the arena's fused cloud — the pieces land one after the other in list order, which gives the
// interleaved corner_k, surf_k order of publishGlobalMap with no kernel change, and the host-computed kf_matrix keeps
// every point bit-identical to lvi_transform_cloud.  The filter is a Submap sized to the reservation: the same bbox,
// overflow-rule, binned / sorted and centroid kernels as every other VoxelGrid here.  The stream, the arena, the piece
// table and the fetch are the keyframe job of lvi_kfjob.hpp.
#include <cmath>

#include "../../include/lvi_gmap.h"
#include "lvi_lidar.hpp"

namespace lvi {

struct GmapDev : KfJob {
    int req = 0;                                           // the reservation asked for (the cloud's capacity is at least 64)
    Submap cloud;                                          // the fused cloud and its VoxelGrid
    VoxGrid* h_grid = nullptr; int* h_nout = nullptr;      // pinned: the last build's grid record and voxel count
    // last build (host)
    bool built = false;
    int n_fused = 0; float leaf = 0.f;
};

namespace {

void gm_destroy(GmapDev* g)
{
    if (!g) return;
    g->destroy();
    g->cloud.release();
    if (g->h_grid) (void)hipHostFree(g->h_grid);
    if (g->h_nout) (void)hipHostFree(g->h_nout);
    delete g;
}

}  // namespace

void gmap_join(LidarDev& d)
{
    if (d.gmap) d.gmap->wait();
}

void gmap_free(LidarDev& d)
{
    GmapDev* g = d.gmap;
    d.gmap = nullptr;
    gm_destroy(g);
}

}  // namespace lvi

using namespace lvi;

extern "C" {

int32_t lvi_gmap_abi_version(void) { return LVI_GMAP_ABI_VERSION; }

int32_t lvi_gmap_reserve(lvi_lidar* h, int32_t max_points)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (max_points < 1 || max_points > LVI_GMAP_MAX_POINTS) return fail(LVI_ERR_INVALID_ARG, "max_points must be 1..LVI_GMAP_MAX_POINTS");
    LidarDev& d = lidar_slot0(h);
    if (d.gmap && d.gmap->req >= max_points) return LVI_OK;
    return guarded(d.device, [&]() -> int32_t {
        gmap_join(d);
        GmapDev* g = new GmapDev();
        try {
            g->req = max_points;
            g->create(std::max(d.kf_seg_cap, 2));
            LVI_HIP(hipHostMalloc((void**)&g->h_grid, sizeof(VoxGrid), hipHostMallocDefault));
            LVI_HIP(hipHostMalloc((void**)&g->h_nout, sizeof(int) * 2, hipHostMallocDefault));
            g->init_arena([&](auto& ar) {
                g->cloud.layout(ar, std::max(max_points, 64));
                g->d_seg = ar.template alloc<KfSeg>((size_t)g->seg_cap);
            });
            g->cloud.vox.mode = d.P.voxel_mode;
            LVI_HIP(hipStreamSynchronize(g->ctx.stream));
        } catch (...) {
            gm_destroy(g);
            throw;
        }
        gmap_free(d);                                                  // the old arena (its build has finished)
        d.gmap = g;
        return LVI_OK;
    });
}

int32_t lvi_gmap_release(lvi_lidar* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t { gmap_free(d); return LVI_OK; });
}

int32_t lvi_gmap_arena_bytes(lvi_lidar* h, int64_t* bytes)
{
    if (!h || !bytes) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const GmapDev* g = lidar_slot0(h).gmap;
    *bytes = g ? (int64_t)g->arena.size : 0;
    return LVI_OK;
}

int32_t lvi_gmap_build(lvi_lidar* h, const int32_t* keys, int32_t n_keys, int32_t which, float leaf, int32_t* n_fused)
{
    if (!h || n_keys < 0 || (n_keys > 0 && !keys)) return fail(LVI_ERR_INVALID_ARG, "bad key list");
    if (which < LVI_GMAP_CORNER || which > LVI_GMAP_CORNER_SURF) return fail(LVI_ERR_INVALID_ARG, "which must be LVI_GMAP_CORNER, _SURF or _CORNER_SURF");
    if (!(leaf >= 0.f) || std::isinf(leaf)) return fail(LVI_ERR_INVALID_ARG, "leaf must be 0 (no filter) or a finite positive size");
    LidarDev& d = lidar_slot0(h);
    if (!d.gmap) return fail(LVI_ERR_STATE, "no global-map reservation (lvi_gmap_reserve)");
    GmapDev& g = *d.gmap;
    const int nkf = (int)d.kf_pose.size();
    long long total = 0;
    for (int i = 0; i < n_keys; i++) {
        const int k = keys[i];
        if (k < 0 || k >= nkf) return fail(LVI_ERR_INVALID_ARG, "key index out of range");
        if (which != LVI_GMAP_SURF) total += d.kf_n_c[k];
        if (which != LVI_GMAP_CORNER) total += d.kf_n_s[k];
    }
    const long long nseg = (long long)n_keys * (which == LVI_GMAP_CORNER_SURF ? 2 : 1);
    if (nseg > g.seg_cap) return fail(LVI_ERR_CAPACITY, "key list longer than the global map's segment table (2 * max_keyframes + 2048 clouds)");
    if (total > g.req) return fail(LVI_ERR_CAPACITY, "fused cloud exceeds the global-map reservation");
    return guarded(d.device, [&]() -> int32_t {
        g.wait();                                                      // the previous build still reads h_seg / writes the arena
        const int n = (int)total;
        const bool filter = leaf > 0.f && n > 0;
        Submap& c = g.cloud;
        if (filter) c.prepare(g.ctx, leaf);                            // (synchronises the build's stream: before the fork below is enqueued)
        // both outputs are the fused cloud: one sequence in list order
        KfPieces t{g.h_seg};
        for (int i = 0; i < n_keys; i++) kf_pieces_add(d, t, keys[i], which != LVI_GMAP_SURF ? 0 : -1, which != LVI_GMAP_CORNER ? 0 : -1);
        g.fork(d.ctx);
        if (t.n) {
            LVI_HIP(hipMemcpyAsync(g.d_seg, g.h_seg, sizeof(KfSeg) * (size_t)t.n, hipMemcpyHostToDevice, g.ctx.stream));
            kf_assemble_launch(g.ctx, g.d_seg, t.n, t.maxn, d.kfPool, c.fused, c.fused, (double)n);
        }
        if (filter) {
            c.filter(g.ctx, n, "gmap");
            LVI_HIP(hipMemcpyAsync(g.h_grid, c.vox.d_grid, sizeof(VoxGrid), hipMemcpyDeviceToHost, g.ctx.stream));
            LVI_HIP(hipMemcpyAsync(g.h_nout, c.vox.d_nout, sizeof(int), hipMemcpyDeviceToHost, g.ctx.stream));
        }
        g.mark_done();
        g.built = true;
        g.n_fused = n; g.leaf = filter ? leaf : 0.f;
        if (n_fused) *n_fused = n;
        return LVI_OK;
    });
}

}  // extern "C"

namespace {

int32_t gm_result(LidarDev& d, lvi_gmap_info* info)
{
    if (!d.gmap || !d.gmap->built) return fail(LVI_ERR_STATE, "no global map built");
    GmapDev& g = *d.gmap;
    LVI_HIP(hipEventSynchronize(g.evDone));                            // this build only: not the handle's other streams
    lvi_gmap_info r{};
    r.n_fused = g.n_fused;
    r.filtered = g.leaf > 0.f ? 1 : 0;
    r.overflow = r.filtered && g.h_grid->overflow ? 1 : 0;
    r.n_out = r.filtered && !r.overflow ? *g.h_nout : g.n_fused;
    *info = r;
    return LVI_OK;
}

}  // namespace

extern "C" {

int32_t lvi_gmap_result(lvi_lidar* h, lvi_gmap_info* info)
{
    if (!h || !info) return fail(LVI_ERR_INVALID_ARG, "null argument");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t { return gm_result(d, info); });
}

int32_t lvi_gmap_fetch(lvi_lidar* h, int32_t what, int32_t first, int32_t count, lvi_pt* out)
{
    if (!h || (count > 0 && !out) || first < 0 || count < 0) return fail(LVI_ERR_INVALID_ARG, "bad fetch arguments");
    if (what != LVI_GMAP_FUSED && what != LVI_GMAP_FILTERED) return fail(LVI_ERR_INVALID_ARG, "what must be LVI_GMAP_FUSED or LVI_GMAP_FILTERED");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t {
        lvi_gmap_info r;
        const int32_t st = gm_result(d, &r);
        if (st) return st;
        GmapDev& g = *d.gmap;
        // the overflow rule / no filter: the fused cloud is the result (PCL's output = input)
        const bool from_fused = what == LVI_GMAP_FUSED || !r.filtered || r.overflow;
        const int n = what == LVI_GMAP_FUSED ? r.n_fused : r.n_out;
        if ((long long)first + count > n) return fail(LVI_ERR_INVALID_ARG, "fetch range outside the cloud");
        g.fetch((from_fused ? g.cloud.fused : g.cloud.out) + first, count, out);
        return LVI_OK;
    });
}

int32_t lvi_gmap_debug_voxel(lvi_lidar* h, int32_t* cells, int32_t* counts, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out || cap < 0 || (cap > 0 && (!cells || !counts))) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t {
        lvi_gmap_info r;
        const int32_t st = gm_result(d, &r);
        if (st) return st;
        GmapDev& g = *d.gmap;
        std::vector<int32_t> keys, vc, vn;
        if (r.filtered && !r.overflow) {
            voxel_debug_fetch(g.ctx, g.cloud.vox, g.n_fused, keys, vc, vn);
            // NOT the realisation's own compaction tables: the per-point voxel idx that vox_keys_kernel recomputes on the
            // device (PCL's key expression for this grid), grouped on the host — distinct idx ascending (PCL's output order)
            // and the points of each.  The filter's own output is checked through its centroids and voxel count.
            std::sort(keys.begin(), keys.end());
            vc.clear(); vn.clear();
            for (size_t i = 0; i < keys.size(); i++) {
                if (i == 0 || keys[i] != keys[i - 1]) { vc.push_back(keys[i]); vn.push_back(0); }
                vn.back()++;
            }
        }
        *n_out = (int32_t)vc.size();
        const int m = std::min((int)vc.size(), cap);
        if (m > 0) { std::memcpy(cells, vc.data(), sizeof(int32_t) * m); std::memcpy(counts, vn.data(), sizeof(int32_t) * m); }
        return LVI_OK;
    });
}

}  // extern "C"
