// pcl::VoxelGrid<PointXYZI>::filter on the GPU, batched over independent segments
// (the 4 per-ring calls of featureExtraction.cpp:239-243, the corner+surf pair of
// mapOptimization.cpp:987-999 and the corner+surf pair of :958-965 are one batch each).
#pragma once
#include "lvi_sort.hpp"
#include "lvi_vox_schedule.hpp"

namespace lvi {

struct VoxSegStatic {            // filled on the host once per plan
    const lvi_pt* in;            // input array
    const uint8_t* mask;         // optional: only points with mask != 0 take part (indexed like `in`)
    lvi_pt* out;                 // output array
    float leaf;
};
struct VoxSegDyn { int in_off; int n; };   // device: where the segment's input starts and how long it is

struct VoxGrid {                 // device, per segment
    unsigned bb[6];              // order-encoded min xyz, max xyz
    int n_valid;
    float inv;                   // inverse_leaf_size_
    int min_b[3];
    int div_b[3];
    unsigned mul1, mul2;         // divb_mul_[1], divb_mul_[2]
    unsigned sentinel;           // key of masked-out points, larger than every real key
    int nbits;
    int overflow;                // PCL's "leaf size too small" rule hit: output = input
    int nvox;
    int out_off;
    // ---- centroid arithmetic (every realisation, the incremental map included).  Per voxel and coordinate, with
    //      cell = the voxel's ABSOLUTE integer coordinate floor(value * inv):
    //          q_i = RNE(2^fx_k * (v_i - cell * leaf))   (binary64 offset: exact unless |v_i| < 2^-28 leaf in cell -1)
    //          centroid = RNE_f32(cell * leaf + sum q_i / (cnt * 2^fx_k)), rounded once (fx_centroid)
    //      The origin of a voxel's sums is a property of the voxel, not of the bounding box, so the sums do not depend on which
    //      other points are in the cloud, nor on the order the points of a voxel are visited in.  Intensity: q_i = RNE(I_i * 2^fx_ki)
    //      (origin 0), RNE_f32(sum q_i / (cnt * 2^fx_ki)); fx_ki from the segment's largest |intensity| (29 on the incremental map,
    //      which takes intensities < 256 only).  Within 2^-(fx_k+1) of the true mean before the final half ulp; NOT the true
    //      mean rounded once for coordinates below ~2^(24 - fx_k), whose bits are finer than the grid.  Range: |cell| < 2^26
    //      (cell * leaf * 2^fx_k < 2^62 in the exact finalisation; 2000 m at a 0.02 m leaf is a cell of ~2^17).
    double leaf_d;               // (double)leaf
    int fx_k, fx_ki;             // scale exponents: |value - cell*leaf| < 2 leaf < 2^(37 - fx_k); |intensity| < 2^(37 - fx_ki), at least 2^8
    // ---- binned path: bin = idx >> bin_shift, nbins <= VB_NB
    int bin_shift, nbins;
    unsigned long long ncells;   // div_b product (0 when the overflow rule fired or the segment is empty)
    int plan_ok;                 // vb_plan's histogram (taken under the PREVIOUS run's geometry, in the pass that takes the bbox) is valid for this run's geometry
};

// ---- KNN grid index over a downsampled map (built in lvi_icp.hip).  Its first step — one counter per point's cell, one per
//      chunk of the cell scan — is taken by whoever writes the downsampled map last: vb_copy of the binned map rebuild through
//      the hook below, grid_count (lvi_icp.hip) for every other producer.  Both use the device code at the end of this file.
struct GridMeta { double origin[3]; double edge, inv_edge; int dim[3]; int ncells; int n; int ok; int R; };
constexpr int GRID_SCAN_BLOCKS = 1024;       // chunks of the cell scan: chunk = cell / ceil(ncells / GRID_SCAN_BLOCKS)
constexpr int GRID_ERR_TOO_LARGE = 2;        // status bit of a map no cell edge up to 2^19 m fits into max_cells (DEV_ERR_GRID_TOO_LARGE)
struct GridCountHook {                       // all null: the plan's output is not indexed where it is written
    GridMeta* meta[2];                       // per segment (corner, surf): the geometry, stored by the segment's first workgroup
    int* count[2];                           // [max_cells + 1] points per cell, zero between builds
    int* blockSum[2];                        // [GRID_SCAN_BLOCKS] points per chunk, zero between builds
    int* d_status;                           // [1] = the build's status word
    int max_cells;
};

constexpr int VOX_HT = 1024;     // keys per workgroup in the head (segment boundary) kernels
constexpr int VB_NB = 4096;      // binned path: bins per segment (LDS histogram of the partition kernels)
constexpr int VB_CL_LOG = 10;    // binned path: voxels accumulated in LDS per sweep = 1 << VB_CL_LOG
constexpr int VB_TILE = 4096;    // binned path: points per tile of the histogram kernel (grid-stride)
constexpr int VB_STILE = 4096;   // binned path: points per workgroup of the scatter kernel (2048: 62 us instead of 56 us for the 4.9 M-point map)
constexpr int VB_PAD = 1;        // binned path: stride of the global bin counters / cursors (one per 64-B line, VB_PAD = 16, measured SLOWER: hist 36 vs 29 us, scatter 67 vs 56 us)
constexpr int VB_WG = 512;       // deterministic partition: workgroups (= contiguous point ranges) per segment (256 / 512 / 1024: scatter 62 / 44 / 46 us on the 4.87 M-point map)
constexpr int VB_XCD = 8;        // workgroups VB_XCD apart in dispatch order run on the same XCD (slot-major order of the raw-map passes, vb_block)
constexpr int VB_WROW = VB_NB + 64;   // words per row of the per-(workgroup, bin) count table: NOT a power of two — vb_colscan walks columns, and rows 16 KB apart meet in the same memory channels
constexpr int VB_CH = 8192;       // binned path: points per accumulate workgroup (chunk of a bin); with 32 scans in flight 4096 / 8192 / 16384: 7 050 / 7 400 / 7 460 scans/s (one rebuild alone: accum 33 / ~40 / 50 us)
constexpr int VB_LIGHT = 256;     // binned path: a bin of at most this many points is accumulated by ONE wavefront (vb_light_kernel)
constexpr int VB_TAB = 1 << VB_CL_LOG;      // entries per compacted chunk table
constexpr int VB_TABC = VB_TAB + 32;         // u32 words per chunk table: entries, then the entry count
constexpr int VB_ACC_BLOCKS = 1024;

struct VoxelPlan {
    int nseg = 0, seg_cap = 0, nblk_h = 0;
    bool concat_out = false;     // outputs of the segments are concatenated in out[0]'s array
    int centroid_lanes = 8;      // lanes that share one output voxel (32 for plans with tens of points per voxel)
    SortPlan sort;
    VoxSegStatic* d_static = nullptr;
    VoxSegDyn* d_dyn = nullptr;
    VoxGrid* d_grid = nullptr;
    int *d_n = nullptr, *d_nbits = nullptr;
    int* d_blockHeads = nullptr;   // [nseg][nblk_h]
    int* d_starts = nullptr;       // [nseg][seg_cap + 1]  first sorted position of every output voxel
    int* d_nout = nullptr;         // [nseg + 1]  voxels per segment, [nseg] = total
    float* d_mmPartial = nullptr;  // [nseg][nblk_mm][12] per-workgroup bbox partials
    int nblk_mm = 0;
    // binned path
    int n_host[4] = {0, 0, 0, 0};     // plans whose segment lengths the host knows (the raw map): passed as kernel arguments
    bool use_n_host = false;          // instead of d_dyn[].n (in_off stays 0)
    const int* n_dev[4] = {nullptr, nullptr, nullptr, nullptr};   // or: device counters of the producer (scan grids), in_off 0
    int mode = VOX_AUTO;
    unsigned* d_binCount = nullptr;   // [nseg][VB_NB]    points per bin (zero between runs)
    int* d_binStart = nullptr;        // [nseg][VB_NB+1]  first bucketed position of every bin
    unsigned* d_cursor = nullptr;     // [nseg][VB_NB]    reservation cursor of the partition
    int* d_binVox = nullptr;          // [nseg][VB_NB]    occupied voxels per bin
    int* d_binOut = nullptr;          // [nseg][VB_NB]    exclusive scan of d_binVox
    lvi_pt* d_bucketed = nullptr;     // [nseg][seg_cap]  points grouped by bin
    lvi_pt* d_staging = nullptr;      // [nseg][seg_cap]  centroids of bin b at d_binStart[b]…
    uint2* d_stagingKC = nullptr;     // [nseg][seg_cap]  (voxel idx, point count) beside them
    int* d_chunkStart = nullptr;      // [nseg][VB_NB+1]  exclusive scan of the chunks per bin
    int* d_multiStart = nullptr;      // [nseg][VB_NB+1]  … of the chunks of bins with more than one chunk
    int* d_chunkBin = nullptr;        // [nseg][max_chunks] bin of every chunk (saves the accumulate kernel a 12-step search through L2)
    int* d_multiOwner = nullptr;      // [nseg][max_multi] first chunk-table slot of a multi-chunk bin -> the bin (else -1)
    int* d_lightBin = nullptr;        // [nseg][VB_NB + 1] bins of at most VB_LIGHT points (one wavefront each, vb_light_kernel); their number at [VB_NB]
    int max_chunks = 0;
    unsigned long long* d_chunkTabV = nullptr;   // [nseg][max_multi][4][VB_TAB] compacted chunk tables of multi-chunk bins (sums of the occupied cells)
    unsigned* d_chunkTabC = nullptr;             // [nseg][max_multi][VB_TABC]: (cell << 16 | count) per entry, entry count at [VB_TAB]
    int max_multi = 0;
    unsigned long long* h_ncells = nullptr;   // pinned host, [nseg]: div_b product of the latest run (AUTO's hint)
    int last_mode = VOX_SORTED;               // the realisation of the latest run, stored by callers that serve voxel_debug_fetch
    int bin_pts = 2048, bin_max = 1024;       // binned path: points aimed at per bin, most bins (<= VB_NB)
    // tables of the deterministic partition (the raw local map only).  Whether a run takes them itself or finds them valid is
    // not the plan's to know: the caller says so in the VoxPlanState it passes (lvi_vox_schedule.hpp)
    unsigned* d_wprefix = nullptr;            // [nseg][VB_WG][VB_WROW] per-(workgroup, bin) prefix
    unsigned* d_binCountCached = nullptr;     // [nseg][VB_NB] points per bin of the current input (vb_colscan)
    int* d_planMiss = nullptr;                // [nseg] a point fell outside the previous geometry (vb_plan)
    bool slot_major = true;                   // batch launches of the raw-map passes fold the slot into blockIdx.x (vb_block; LVI_VB_SLOT_ORDER=0: blockIdx.z = slot)
    GridCountHook index = {};                 // two-segment plans whose output gets a KNN index (the local map): vb_copy counts what it writes

    template <class AR> void allocate(AR& ar, int nseg_, int seg_cap_, bool concat)
    {
        nseg = nseg_; seg_cap = seg_cap_; concat_out = concat; nblk_h = div_up(seg_cap_, VOX_HT);
        sort.allocate(ar, nseg_, seg_cap_);
        const size_t tot = (size_t)nseg_ * seg_cap_;
        d_static = ar.template alloc<VoxSegStatic>(nseg_);
        d_dyn = ar.template alloc<VoxSegDyn>(nseg_);
        d_grid = ar.template alloc<VoxGrid>(nseg_);
        d_n = ar.template alloc<int>(nseg_);
        d_nbits = ar.template alloc<int>(nseg_);
        d_blockHeads = ar.template alloc<int>((size_t)nseg_ * nblk_h);
        d_starts = ar.template alloc<int>((size_t)nseg_ * ((size_t)seg_cap_ + 1));
        d_nout = ar.template alloc<int>(nseg_ + 1);
        nblk_mm = std::max(1, std::min(div_up(seg_cap_, 256 * 16), 1024));
        d_mmPartial = ar.template alloc<float>((size_t)nseg_ * nblk_mm * 12);
        d_binCount = ar.template alloc<unsigned>((size_t)nseg_ * VB_NB * VB_PAD);
        d_binStart = ar.template alloc<int>((size_t)nseg_ * (VB_NB + 1));
        d_cursor = ar.template alloc<unsigned>((size_t)nseg_ * VB_NB * VB_PAD);
        d_binVox = ar.template alloc<int>((size_t)nseg_ * VB_NB);
        d_binOut = ar.template alloc<int>((size_t)nseg_ * VB_NB);
        d_bucketed = ar.template alloc<lvi_pt>(tot);
        d_staging = ar.template alloc<lvi_pt>(tot);
        d_stagingKC = ar.template alloc<uint2>(tot);
        d_chunkStart = ar.template alloc<int>((size_t)nseg_ * (VB_NB + 1));
        d_multiStart = ar.template alloc<int>((size_t)nseg_ * (VB_NB + 1));
        max_chunks = div_up(seg_cap_, VB_CH) + VB_NB;
        d_chunkBin = ar.template alloc<int>((size_t)nseg_ * max_chunks);
        d_lightBin = ar.template alloc<int>((size_t)nseg_ * (VB_NB + 1));
        max_multi = 2 * div_up(seg_cap_, VB_CH) + 2;         // sum of ceil(cnt/CH) over bins with cnt > CH  <=  2 n / CH
        d_multiOwner = ar.template alloc<int>((size_t)nseg_ * max_multi);
        d_chunkTabV = ar.template alloc<unsigned long long>((size_t)nseg_ * max_multi * (4 * VB_TAB));
        d_chunkTabC = ar.template alloc<unsigned>((size_t)nseg_ * max_multi * VB_TABC);
        d_planMiss = ar.template alloc<int>(nseg_);
    }
    void release();                                                            // frees h_ncells
    void set_static(const Ctx& ctx, const VoxSegStatic* host_segs);           // H2D of the per-segment pointers (+ the pinned hint)
};

// ---------------------------------------------------------------------------------------------------------------------
// Incremental local map: the two VoxelGrids of extractCloud (mapOptimization.cpp:958-965) kept as
// persistent per-voxel sums.  A voxel's membership — floor(p * inv_leaf) per axis — and its sums — relative to the voxel's
// own origin — do not depend on the bounding box, so whole keyframes can be added to and taken from the sums; an emission
// computes PCL's linear idx of every live voxel for the CURRENT bounding box, sorts by it and writes the centroids: the same
// voxels, order and bits as filtering the fused cloud.  One open-addressing table per map kind (corner, surf).
struct IncPiece { int in_off, n, which, sign, kf; float A[12]; };      // one (keyframe, corner|surf) cloud to add (+1) or take out (-1)
enum { INC_ERR_RANGE = 1, INC_ERR_FULL = 2, INC_ERR_OVERFLOW = 4, INC_ERR_INTENSITY = 8 };
struct IncMap {
    int H = 0;                                // slots per table (power of two)
    int max_kf = 0;
    unsigned long long* key[2] = {nullptr, nullptr};       // [H] packed absolute voxel coordinates, ~0 = empty
    unsigned long long* sums[2] = {nullptr, nullptr};      // [H][4]
    int* cnt[2] = {nullptr, nullptr};                      // [H] points in the voxel (0: a voxel every keyframe has left)
    int* occ[2] = {nullptr, nullptr};                      // [H] slots in first-touch order
    int* d_nocc = nullptr;                                 // [2]
    unsigned* kfBox = nullptr;                             // [max_kf][2][8] map-frame bbox of a stored keyframe at the pose it was added with
    int* d_active = nullptr;                               // [max_active] key indices of the current list (bbox fold)
    int* h_active = nullptr;                               // pinned staging of the same
    int max_active = 0;
    IncPiece* d_pieces = nullptr; IncPiece* h_pieces = nullptr; int max_pieces = 0;
    SortPlan sort;                                         // (idx, slot) pairs of the live voxels, 2 segments
    int *d_n = nullptr, *d_nbits = nullptr;                // [2]
    int* d_status = nullptr;                               // INC_ERR_* (sticky until cleared)
    int* h_status = nullptr;                               // pinned: [0] status, [1..2] n_occ
    template <class AR> void allocate(AR& ar, int H_, int max_kf_, int max_active_)
    {
        H = H_; max_kf = max_kf_; max_active = max_active_; max_pieces = 4 * max_active_ + 16;
        for (int w = 0; w < 2; w++) {
            key[w] = ar.template alloc<unsigned long long>(H); sums[w] = ar.template alloc<unsigned long long>((size_t)H * 4);
            cnt[w] = ar.template alloc<int>(H); occ[w] = ar.template alloc<int>(H);
        }
        d_nocc = ar.template alloc<int>(2);
        kfBox = ar.template alloc<unsigned>((size_t)std::max(max_kf, 1) * 16);
        d_active = ar.template alloc<int>(std::max(max_active, 1));
        d_pieces = ar.template alloc<IncPiece>(max_pieces);
        sort.allocate(ar, 2, H / 2);
        d_n = ar.template alloc<int>(2); d_nbits = ar.template alloc<int>(2);
        d_status = ar.template alloc<int>(4);
    }
};
void incmap_clear(const Ctx& ctx, const IncMap& m);
// add / remove the listed keyframe clouds (pool = the keyframe store)
void incmap_apply(const Ctx& ctx, const IncMap& m, const lvi_pt* pool, int n_pieces, int max_n, const float leaf[2]);
// emit the live voxels of both tables as laserCloud{Corner,Surf}FromMapDS: fills grid[2] / nout[3] / out[2] exactly as
// voxel_downsample_batch of the fused cloud would (n_active unique keys of d_active give the bounding box)
void incmap_emit(const Ctx& ctx, const IncMap& m, int n_active, const float leaf[2], VoxGrid* grid, int* nout, lvi_pt* outC, lvi_pt* outS, int seg_cap);

// Enqueue the whole filter for every segment.  Two interchangeable realisations with bit-identical output:
//   SORTED  stable radix sort of (voxel idx, point index) + ordered head compaction + per-voxel sums; any grid.
//   BINNED  one partition of the points into <= VB_NB bins of consecutive voxel idx, then one workgroup per bin
//           accumulates its voxels in LDS; ~2.5x less HBM traffic and 8 launches instead of 19 when the grid is
//           compact (div_b product <= VB_NB << VB_CL_LOG); still correct, but sweeping each bin several times,
//           when it is not.
// AUTO resolves to BINNED when the previous run's grids (read from pinned host memory, no sync) had at most
// 16.8 M cells (four sweeps per bin), to SORTED for sparser ones (voxel_resolve_mode).  Where the bounding box comes from
// and which of the three partitions a BINNED run takes is vox_schedule's answer (lvi_vox_schedule.hpp) to the
// VoxPlanState of every slot; the schedule that was enqueued is returned.  d_dyn must have been written (on the same
// stream) by the producer.  n_hint: nominal total input points, for byte accounting only.
//   st = null: voxel_plan_state of every plan — MINMAX, then RESERVE or the sort (ring, scan, depth, Submap plans);
//   the raw local map passes its own states (stage_map_build): WITH_PLAN + DET_PER_RUN, or CACHED + DET_CACHED.
// S plans of identical shape (the same plan of S batch slots) are ONE launch sequence, blockIdx.z = slot (raw-map passes
// under VoxSchedule::fold_slots: the slot folded into blockIdx.x); n_hint = points of all slots.
VoxSchedule voxel_downsample_batch(const Ctx& ctx, const VoxelPlan* const* plans, const VoxPlanState* st, int S, const char* tag, double n_hint);
VoxSchedule voxel_downsample_batch(const Ctx& ctx, const VoxelPlan& plan, const char* tag, double n_hint);
// whether a run of `plan` under schedule `sc` leaves the count step of the KNN index done (GridCountHook): binned runs of a plan with the hook
inline bool voxel_run_indexed(const VoxelPlan& plan, const VoxSchedule& sc) { return sc.part != VOX_PART_NONE && plan.nseg == 2 && plan.index.count[0] != nullptr; }
// what the plan itself tells about its next run: the resolved mode, the tables it owns, its lengths' source; not per-run, nothing valid
VoxPlanState voxel_plan_state(const VoxelPlan& plan);
// the bbox partial records of the plan's current input as a pass of its own, and — when the plan resolves to BINNED and owns
// the tables — the per-bin counts of the deterministic partition.  Returns whether the counts were taken; the caller
// owns both validity bits and clears them whenever the input changes.
bool voxel_bbox_pass(const Ctx& ctx, const VoxelPlan& plan, const char* tag, double n_hint);
// the realisation the next voxel_downsample_batch of this plan will enqueue (AUTO resolved from the previous batch's hint)
int voxel_resolve_mode(const VoxelPlan& plan);
// a cloud of at most VOX_TINY points, one workgroup, one launch, pinned host memory in and out (the node's key-pose grid)
constexpr int VOX_TINY = 1024;
void voxel_tiny(const Ctx& ctx, const lvi_pt* in_pinned, int n, float leaf, int seg_cap, int bin_pts, int bin_max, lvi_pt* out_pinned, int* hdr_pinned,
                int* cells_pinned, int* counts_pinned, int* keys_pinned);
// debug views of the plan's latest run over n_in points: per-point voxel idx, the occupied voxels and their point counts
void voxel_debug_fetch(const Ctx& ctx, const VoxelPlan& p, int n_in, std::vector<int32_t>& keys, std::vector<int32_t>& cells, std::vector<int32_t>& counts);

#ifdef __HIPCC__
// Runs of equal consecutive values across the lanes of a wave (consecutive points of a cloud mostly share a
// bin / a voxel, and same-address atomics serialise).  head = first lane of its run; hpos = that lane;
// len (valid on head lanes) = lanes in the run.  Every lane of the wavefront calls it.
struct WaveRun { bool head; int hpos; int len; };
__device__ __forceinline__ WaveRun wave_runs(unsigned v)
{
    const int l = lane_id();
    const unsigned prev = __shfl_up(v, 1, 64);
    WaveRun r;
    r.head = l == 0 || prev != v;
    const uint64_t hm = __ballot(r.head);
    r.hpos = 63 - __clzll(hm & ((2ull << l) - 1ull));
    const uint64_t above = l == 63 ? 0ull : hm & ~((2ull << l) - 1ull);
    r.len = (above ? __ffsll((unsigned long long)above) - 1 : 64) - l;
    return r;
}

// ---- KNN grid index: geometry and the count step (GridMeta / GridCountHook above)
// The geometry of segment w's index follows from the bounding box of the raw map (vox[w].bb) and the size of the downsampled one
// (nout[w]): a hundred cycles for 0.5 m cells, so every thread that counts derives it itself from the (uniform) records — no
// one-thread kernel in front, no barrier.  Returns the segment's status bits.
__device__ inline int grid_meta_one(const VoxGrid* vox, const int* nout, int max_cells, int w, GridMeta& m)
{
    const int n = nout[w];
    m.n = n; m.ok = 0; m.R = 1; m.edge = 0.5; m.inv_edge = 2.0;
    m.dim[0] = m.dim[1] = m.dim[2] = 1; m.ncells = 1; m.origin[0] = m.origin[1] = m.origin[2] = 0.0;
    if (n <= 0 || vox[w].n_valid == 0) return 0;
    double lo[3], ext[3];
    for (int d = 0; d < 3; d++) {
        const double mn = floor((double)ord2f(vox[w].bb[d])), mx = floor((double)ord2f(vox[w].bb[3 + d]));
        lo[d] = mn - 1.0;                       // one cell of padding on every side
        ext[d] = mx - mn + 3.0;
    }
    int c = 1;                                  // cell edge in half metres, integer >= 1
    // c = 1, the cell every map of ordinary extent gets: ext / 0.5 is ext * 2 and 1 / 0.5 is 2, exactly — no f64 division
    // (tens of instructions each on gfx950) in front of the workgroup's first point
    double nx = ceil(ext[0] * 2.0), ny = ceil(ext[1] * 2.0), nz = ceil(ext[2] * 2.0);
    while (!(nx * ny * nz <= (double)max_cells)) {
        if (c > 1 << 20) return GRID_ERR_TOO_LARGE;
        c++;
        const double e = 0.5 * c;
        nx = ceil(ext[0] / e); ny = ceil(ext[1] / e); nz = ceil(ext[2] / e);
    }
    m.dim[0] = (int)nx; m.dim[1] = (int)ny; m.dim[2] = (int)nz;
    // cell = floor((p - lo) / edge); a neighbour within 1 m is at most R cells away on every axis
    m.origin[0] = lo[0]; m.origin[1] = lo[1]; m.origin[2] = lo[2];
    m.ncells = m.dim[0] * m.dim[1] * m.dim[2];
    m.edge = 0.5 * c; m.inv_edge = c == 1 ? 2.0 : 1.0 / m.edge; m.R = c == 1 ? 2 : 1;
    m.ok = 1;
    return 0;
}

__device__ __forceinline__ void cell_of(const GridMeta& m, float x, float y, float z, int c[3])
{
    // the same expression places the map points (grid_count_wave, grid_scatter) and the queries (knn5_search_acc)
    c[0] = (int)floor(((double)x - m.origin[0]) * m.inv_edge);
    c[1] = (int)floor(((double)y - m.origin[1]) * m.inv_edge);
    c[2] = (int)floor(((double)z - m.origin[2]) * m.inv_edge);
}

__device__ __forceinline__ int cell_id_of(const GridMeta& m, const lvi_pt& p)
{
    int c[3];
    cell_of(m, p.x, p.y, p.z, c);
#pragma unroll
    for (int d = 0; d < 3; d++) c[d] = min(max(c[d], 0), m.dim[d] - 1);
    return (c[2] * m.dim[1] + c[1]) * m.dim[0] + c[0];
}

// cells per chunk of the cell scan (grid_scan_apply)
__device__ __forceinline__ int grid_chunk_len(int ncells) { return (ncells + GRID_SCAN_BLOCKS - 1) / GRID_SCAN_BLOCKS; }

// One point per lane (act: the lane has one; p is a real point of the map on every lane): its cell's counter, and its chunk's
// total where the counts are taken instead of a pass over the whole count array behind them.  The downsampled map comes in
// voxel order, so the points of a wavefront fall into a few chunks: one atomic per run of equal chunks.  Every lane of the
// wavefront calls it; m and L live in registers (behind an atomic the compiler would read them again for every point).
__device__ __forceinline__ void grid_count_wave(const GridMeta& m, int L, int* __restrict__ count, int* __restrict__ blockSum, bool act, const lvi_pt& p)
{
    const int cell = cell_id_of(m, p);
    const unsigned chunk = act ? (unsigned)(cell / L) : ~0u;          // (< GRID_SCAN_BLOCKS: cell < ncells <= L * GRID_SCAN_BLOCKS)
    const WaveRun r = wave_runs(chunk);
    if (act) {
        atomicAdd(&count[cell], 1);
        if (r.head) atomicAdd(&blockSum[chunk], r.len);
    }
}
#endif

}  // namespace lvi
