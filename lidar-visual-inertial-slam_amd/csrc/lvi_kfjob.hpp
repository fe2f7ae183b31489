// The scaffold shared by the consumers of the device keyframe store: the piece table of
// kf_assemble_kernel, one cloud with its VoxelGrid (Submap), and a job on a stream of its own (KfJob).
// The global map (lvi_gmap.hip) and loop closure (lvi_loop.hip) are a KfJob plus what is theirs alone.
#pragma once
#include "lvi_voxel.hpp"

namespace lvi {

struct KfSeg { int in_off, n, out_off, which; float A[12]; };   // one (keyframe, corner|surf) piece of an assembly
// host side of a piece table under construction (kf_pieces_add, lvi_lidar.hpp): n pieces, the longest, points per output
struct KfPieces { KfSeg* h; int n = 0; int maxn = 1; int off[2] = {0, 0}; };

constexpr int KF_FETCH_CHUNK = 1 << 16;                    // points per pinned staging buffer of KfJob::fetch (1 MB)

// One cloud and its VoxelGrid: a plan of one segment (fused -> out) whose length travels as a kernel argument and whose
// segment table is uploaded again only when the leaf size changes.
struct Submap {
    lvi_pt* fused = nullptr;                               // [cap] the input
    lvi_pt* out = nullptr;                                 // [cap] the VoxelGrid's output
    VoxelPlan vox;
    int cap = 0;
    bool static_set = false; float static_leaf = 0.f;      // the plan's segment table is for this leaf

    template <class AR> void layout(AR& ar, int cap_)
    {
        cap = cap_;
        fused = ar.template alloc<lvi_pt>(cap);
        out = ar.template alloc<lvi_pt>(cap);
        vox.allocate(ar, 1, cap, false);
    }
    void release() { vox.release(); }
    // set_static synchronises the stream: a job calls this before the wait for the main stream is enqueued
    void prepare(const Ctx& ctx, float leaf)
    {
        if (static_set && static_leaf == leaf) return;
        VoxSegStatic st{fused, nullptr, out, leaf};
        vox.set_static(ctx, &st);
        static_set = true; static_leaf = leaf;
    }
    void filter(const Ctx& ctx, int n, const char* tag)
    {
        vox.n_host[0] = n; vox.use_n_host = true;
        vox.last_mode = voxel_downsample_batch(ctx, vox, tag, n).mode;
    }
};

// A job over the keyframe store beside the handle's own streams: one is in flight at most, its results stay in the arena
// until the next one, and another host thread may wait for it and fetch them.
struct KfJob {
    Ctx ctx;                                               // own stream; prof = null: never profiled (another thread may read results)
    hipEvent_t evMain = nullptr;                           // recorded on the handle's main stream at enqueue: the job's stream waits for it
    hipEvent_t evDone = nullptr;                           // end of the last job
    hipEvent_t evBuf[2] = {nullptr, nullptr};              // fetch: staging buffer b may be read by the host
    lvi_pt* h_buf[2] = {nullptr, nullptr};                 // pinned [KF_FETCH_CHUNK] each
    KfSeg* d_seg = nullptr; KfSeg* h_seg = nullptr;        // [seg_cap] device (the owner's layout allocates it) / pinned
    int seg_cap = 0;
    Arena arena;
    bool pending = false;

    void create(int seg_cap_)
    {
        seg_cap = seg_cap_;
        LVI_HIP(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
        LVI_HIP(hipEventCreateWithFlags(&evMain, hipEventDisableTiming));
        LVI_HIP(hipEventCreateWithFlags(&evDone, hipEventDisableTiming));
        for (int b = 0; b < 2; b++) {
            LVI_HIP(hipEventCreateWithFlags(&evBuf[b], hipEventDisableTiming));
            LVI_HIP(hipHostMalloc((void**)&h_buf[b], sizeof(lvi_pt) * KF_FETCH_CHUNK, hipHostMallocDefault));
        }
        LVI_HIP(hipHostMalloc((void**)&h_seg, sizeof(KfSeg) * (size_t)seg_cap, hipHostMallocDefault));
    }
    // size the arena with a dry run of the owner's layout, lay it out, zero it (the plans' counters start at zero)
    template <class L> void init_arena(L&& layout)
    {
        ArenaSizer sz;
        layout(sz);
        arena.init(sz.used + (1 << 20));
        layout(arena);
        LVI_HIP(hipMemsetAsync(arena.base, 0, arena.size, ctx.stream));
    }
    void destroy()                                         // waits for the stream first: the owner frees its own parts after this
    {
        if (ctx.stream) (void)hipStreamSynchronize(ctx.stream);
        arena.release();
        if (h_seg) (void)hipHostFree(h_seg);
        for (int b = 0; b < 2; b++) {
            if (h_buf[b]) (void)hipHostFree(h_buf[b]);
            if (evBuf[b]) (void)hipEventDestroy(evBuf[b]);
        }
        if (evMain) (void)hipEventDestroy(evMain);
        if (evDone) (void)hipEventDestroy(evDone);
        if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
    }
    void wait()
    {
        if (pending) { LVI_HIP(hipEventSynchronize(evDone)); pending = false; }
    }
    // everything enqueued on the main stream so far (keyframe copies into the store) before the job reads the pool
    void fork(const Ctx& main)
    {
        LVI_HIP(hipEventRecord(evMain, main.stream));
        LVI_HIP(hipStreamWaitEvent(ctx.stream, evMain, 0));
    }
    void mark_done()
    {
        LVI_HIP(hipEventRecord(evDone, ctx.stream));
        pending = true;
    }
    // double buffer: chunk c is copied into h_buf[c & 1] while the host copies chunk c - 1 out of the other one
    void fetch(const lvi_pt* src, int count, lvi_pt* out)
    {
        const int nch = div_up(count, KF_FETCH_CHUNK);
        for (int c = 0; c <= nch; c++) {
            if (c < nch) {
                const int len = std::min(KF_FETCH_CHUNK, count - c * KF_FETCH_CHUNK);
                LVI_HIP(hipMemcpyAsync(h_buf[c & 1], src + (size_t)c * KF_FETCH_CHUNK, sizeof(lvi_pt) * (size_t)len, hipMemcpyDeviceToHost, ctx.stream));
                LVI_HIP(hipEventRecord(evBuf[c & 1], ctx.stream));
            }
            if (c > 0) {
                const int p = c - 1;
                const int len = std::min(KF_FETCH_CHUNK, count - p * KF_FETCH_CHUNK);
                LVI_HIP(hipEventSynchronize(evBuf[p & 1]));
                std::memcpy(out + (size_t)p * KF_FETCH_CHUNK, h_buf[p & 1], sizeof(lvi_pt) * (size_t)len);
            }
        }
    }
};

}  // namespace lvi
