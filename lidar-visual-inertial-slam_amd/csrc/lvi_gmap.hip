// C-ABI of the global map (include/lvi_gmap.h): publishGlobalMap's and save_map's fuse + VoxelGrid
// (mapOptimization.cpp:179-236, :460-510) over the device keyframe store, on a stream of its own.
//
// No kernel of its own: the fuse is kf_assemble_kernel (lvi_icp.hip) driven by a segment table whose two output
// pointers both address the arena's fused cloud — the pieces land one after the other in list order, which gives the
// interleaved corner_k, surf_k order of publishGlobalMap with no kernel change, and the host-computed kf_matrix keeps
// every point bit-identical to lvi_transform_cloud.  The filter is a VoxelPlan of one segment sized to the
// reservation: the same bbox, overflow-rule, binned / sorted and centroid kernels as every other VoxelGrid here.
#include <cmath>

#include "../../include/lvi_gmap.h"
#include "lvi_lidar.hpp"

namespace lvi {

LidarDev& lidar_slot0(lvi_lidar* h);                       // lvi_capi.hip
void voxel_debug_fetch(const Ctx& ctx, const VoxelPlan& p, int n_in, std::vector<int32_t>& keys, std::vector<int32_t>& cells, std::vector<int32_t>& counts);

constexpr int GMAP_FETCH_CHUNK = 1 << 16;                  // points per pinned staging buffer of lvi_gmap_fetch (1 MB)

struct GmapDev {
    int cap = 0, seg_cap = 0;                              // cap: the arena's points (>= 64); req: the reservation asked for
    int req = 0;
    Arena arena;
    Ctx ctx;                                               // own stream; prof = null: the build is never profiled (another thread may read results)
    hipEvent_t evMain = nullptr;                           // recorded on the handle's main stream at build: the build's stream waits for it
    hipEvent_t evDone = nullptr;                           // end of the last build
    hipEvent_t evBuf[2] = {nullptr, nullptr};              // fetch: staging buffer b may be read by the host
    lvi_pt* fused = nullptr;                               // [cap]
    lvi_pt* out = nullptr;                                 // [cap] the VoxelGrid's output
    VoxelPlan vox;                                         // 1 segment: fused -> out
    LidarDev::KfSeg* d_seg = nullptr; LidarDev::KfSeg* h_seg = nullptr;   // [seg_cap] device / pinned
    lvi_pt* h_buf[2] = {nullptr, nullptr};                 // pinned [GMAP_FETCH_CHUNK] each
    VoxGrid* h_grid = nullptr; int* h_nout = nullptr;      // pinned: the last build's grid record and voxel count
    bool static_set = false; float static_leaf = 0.f;      // the plan's segment table is for this leaf
    // last build (host)
    bool built = false, pending = false;
    int n_fused = 0; float leaf = 0.f;
};

namespace {

int32_t fail(int32_t code, const std::string& msg) { set_error(msg); return code; }

template <class F>
int32_t gm_guarded(LidarDev& d, F&& f)
{
    try {
        LVI_HIP(hipSetDevice(d.device));
        return f();
    } catch (const HipError& e) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", e.what, hipGetErrorString(e.e), e.file, e.line);
        return fail(LVI_ERR_HIP, buf);
    } catch (const std::exception& e) {
        return fail(LVI_ERR_HIP, e.what());
    }
}

void gm_destroy(GmapDev* g)
{
    if (!g) return;
    if (g->ctx.stream) (void)hipStreamSynchronize(g->ctx.stream);
    g->vox.release();
    g->arena.release();
    if (g->h_seg) (void)hipHostFree(g->h_seg);
    for (int b = 0; b < 2; b++) {
        if (g->h_buf[b]) (void)hipHostFree(g->h_buf[b]);
        if (g->evBuf[b]) (void)hipEventDestroy(g->evBuf[b]);
    }
    if (g->h_grid) (void)hipHostFree(g->h_grid);
    if (g->h_nout) (void)hipHostFree(g->h_nout);
    if (g->evMain) (void)hipEventDestroy(g->evMain);
    if (g->evDone) (void)hipEventDestroy(g->evDone);
    if (g->ctx.stream) (void)hipStreamDestroy(g->ctx.stream);
    delete g;
}

template <class AR>
void gm_layout(AR& ar, GmapDev& g)
{
    g.fused = ar.template alloc<lvi_pt>(g.cap);
    g.out = ar.template alloc<lvi_pt>(g.cap);
    g.vox.allocate(ar, 1, g.cap, false);
    g.d_seg = ar.template alloc<LidarDev::KfSeg>((size_t)g.seg_cap);
}

void gm_wait(GmapDev& g)
{
    if (g.pending) { LVI_HIP(hipEventSynchronize(g.evDone)); g.pending = false; }
}

}  // namespace

void gmap_join(LidarDev& d)
{
    if (d.gmap) gm_wait(*d.gmap);
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
    return gm_guarded(d, [&]() -> int32_t {
        if (d.gmap) gm_wait(*d.gmap);
        GmapDev* g = new GmapDev();
        try {
            g->cap = std::max(max_points, 64);
            g->req = max_points;
            g->seg_cap = std::max(d.kf_seg_cap, 2);
            LVI_HIP(hipStreamCreateWithFlags(&g->ctx.stream, hipStreamNonBlocking));
            LVI_HIP(hipEventCreateWithFlags(&g->evMain, hipEventDisableTiming));
            LVI_HIP(hipEventCreateWithFlags(&g->evDone, hipEventDisableTiming));
            for (int b = 0; b < 2; b++) {
                LVI_HIP(hipEventCreateWithFlags(&g->evBuf[b], hipEventDisableTiming));
                LVI_HIP(hipHostMalloc((void**)&g->h_buf[b], sizeof(lvi_pt) * GMAP_FETCH_CHUNK, hipHostMallocDefault));
            }
            LVI_HIP(hipHostMalloc((void**)&g->h_seg, sizeof(LidarDev::KfSeg) * (size_t)g->seg_cap, hipHostMallocDefault));
            LVI_HIP(hipHostMalloc((void**)&g->h_grid, sizeof(VoxGrid), hipHostMallocDefault));
            LVI_HIP(hipHostMalloc((void**)&g->h_nout, sizeof(int) * 2, hipHostMallocDefault));
            ArenaSizer sz;
            gm_layout(sz, *g);
            g->arena.init(sz.used + (1 << 20));
            gm_layout(g->arena, *g);
            LVI_HIP(hipMemsetAsync(g->arena.base, 0, g->arena.size, g->ctx.stream));   // the plan's counters start at zero
            g->vox.mode = d.P.voxel_mode;
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
    return gm_guarded(d, [&]() -> int32_t { gmap_free(d); return LVI_OK; });
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
    return gm_guarded(d, [&]() -> int32_t {
        gm_wait(g);                                                    // the previous build still reads h_seg / writes the arena
        const int n = (int)total;
        const bool filter = leaf > 0.f && n > 0;
        if (filter && (!g.static_set || g.static_leaf != leaf)) {      // (synchronises the build's stream: before the wait below is enqueued)
            VoxSegStatic st{g.fused, nullptr, g.out, leaf};
            g.vox.set_static(g.ctx, &st);
            g.static_set = true; g.static_leaf = leaf;
        }
        int ns = 0, off = 0, maxn = 1;
        for (int i = 0; i < n_keys; i++) {
            const int k = keys[i];
            float M[12];
            kf_matrix(d.kf_pose[k].data(), M);                         // the pose of the store NOW: later set_pose calls change later builds only
            for (int w = 0; w < 2; w++) {
                if ((w == 0 && which == LVI_GMAP_SURF) || (w == 1 && which == LVI_GMAP_CORNER)) continue;
                LidarDev::KfSeg& sg = g.h_seg[ns++];
                sg.which = 0;                                          // both outputs are the fused cloud: one sequence in list order
                sg.in_off = w ? d.kf_off_s[k] : d.kf_off_c[k];
                sg.n = w ? d.kf_n_s[k] : d.kf_n_c[k];
                sg.out_off = off;
                for (int q = 0; q < 12; q++) sg.A[q] = M[q];
                off += sg.n;
                maxn = std::max(maxn, sg.n);
            }
        }
        // everything enqueued on the main stream so far (keyframe copies into the store) before the fuse reads the pool
        LVI_HIP(hipEventRecord(g.evMain, d.ctx.stream));
        LVI_HIP(hipStreamWaitEvent(g.ctx.stream, g.evMain, 0));
        if (ns) {
            LVI_HIP(hipMemcpyAsync(g.d_seg, g.h_seg, sizeof(LidarDev::KfSeg) * (size_t)ns, hipMemcpyHostToDevice, g.ctx.stream));
            kf_assemble_launch(g.ctx, g.d_seg, ns, maxn, d.kfPool, g.fused, g.fused, (double)n);
        }
        if (filter) {
            g.vox.n_host[0] = n; g.vox.use_n_host = true;
            voxel_downsample_batch(g.ctx, g.vox, "gmap", n);
            LVI_HIP(hipMemcpyAsync(g.h_grid, g.vox.d_grid, sizeof(VoxGrid), hipMemcpyDeviceToHost, g.ctx.stream));
            LVI_HIP(hipMemcpyAsync(g.h_nout, g.vox.d_nout, sizeof(int), hipMemcpyDeviceToHost, g.ctx.stream));
        }
        LVI_HIP(hipEventRecord(g.evDone, g.ctx.stream));
        g.pending = true; g.built = true;
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
    return gm_guarded(d, [&]() -> int32_t { return gm_result(d, info); });
}

int32_t lvi_gmap_fetch(lvi_lidar* h, int32_t what, int32_t first, int32_t count, lvi_pt* out)
{
    if (!h || (count > 0 && !out) || first < 0 || count < 0) return fail(LVI_ERR_INVALID_ARG, "bad fetch arguments");
    if (what != LVI_GMAP_FUSED && what != LVI_GMAP_FILTERED) return fail(LVI_ERR_INVALID_ARG, "what must be LVI_GMAP_FUSED or LVI_GMAP_FILTERED");
    LidarDev& d = lidar_slot0(h);
    return gm_guarded(d, [&]() -> int32_t {
        lvi_gmap_info r;
        const int32_t st = gm_result(d, &r);
        if (st) return st;
        GmapDev& g = *d.gmap;
        // the overflow rule / no filter: the fused cloud is the result (PCL's output = input)
        const bool from_fused = what == LVI_GMAP_FUSED || !r.filtered || r.overflow;
        const int n = what == LVI_GMAP_FUSED ? r.n_fused : r.n_out;
        if ((long long)first + count > n) return fail(LVI_ERR_INVALID_ARG, "fetch range outside the cloud");
        const lvi_pt* src = (from_fused ? g.fused : g.out) + first;
        // double buffer: chunk c is copied into h_buf[c & 1] while the host copies chunk c - 1 out of the other one
        const int nch = (count + GMAP_FETCH_CHUNK - 1) / GMAP_FETCH_CHUNK;
        for (int c = 0; c <= nch; c++) {
            if (c < nch) {
                const int len = std::min(GMAP_FETCH_CHUNK, count - c * GMAP_FETCH_CHUNK);
                LVI_HIP(hipMemcpyAsync(g.h_buf[c & 1], src + (size_t)c * GMAP_FETCH_CHUNK, sizeof(lvi_pt) * (size_t)len, hipMemcpyDeviceToHost, g.ctx.stream));
                LVI_HIP(hipEventRecord(g.evBuf[c & 1], g.ctx.stream));
            }
            if (c > 0) {
                const int p = c - 1;
                const int len = std::min(GMAP_FETCH_CHUNK, count - p * GMAP_FETCH_CHUNK);
                LVI_HIP(hipEventSynchronize(g.evBuf[p & 1]));
                std::memcpy(out + (size_t)p * GMAP_FETCH_CHUNK, g.h_buf[p & 1], sizeof(lvi_pt) * (size_t)len);
            }
        }
        return LVI_OK;
    });
}

int32_t lvi_gmap_debug_voxel(lvi_lidar* h, int32_t* cells, int32_t* counts, int32_t cap, int32_t* n_out)
{
    if (!h || !n_out || cap < 0 || (cap > 0 && (!cells || !counts))) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    LidarDev& d = lidar_slot0(h);
    return gm_guarded(d, [&]() -> int32_t {
        lvi_gmap_info r;
        const int32_t st = gm_result(d, &r);
        if (st) return st;
        GmapDev& g = *d.gmap;
        std::vector<int32_t> keys, vc, vn;
        if (r.filtered && !r.overflow) {
            voxel_debug_fetch(g.ctx, g.vox, g.n_fused, keys, vc, vn);
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
