// Which launches one run of the VoxelGrid (voxel_downsample_batch, lvi_voxel.hip) consists of: decided once, here, by a pure
// function of what the host knows about the plans of the batch.  Nothing from HIP: compiles with a plain C++ compiler
// (tests/test_vox_schedule.py enumerates every input).
#pragma once

namespace lvi {

enum VoxMode { VOX_AUTO = 0, VOX_SORTED = 1, VOX_BINNED = 2 };

// where the bounding box of the run comes from
enum VoxBbox {
    VOX_BBOX_MINMAX = 0,         // vox_minmax runs
    VOX_BBOX_CACHED = 1,         // the plan holds the partial records of its unchanged input (voxel_bbox_pass): no pass
    VOX_BBOX_WITH_PLAN = 2,      // vb_plan takes it, in the pass that takes the per-bin counts
};
// how the points are partitioned into bins
enum VoxPart {
    VOX_PART_NONE = 0,           // sorted realisation: no bins
    VOX_PART_RESERVE = 1,        // vb_hist + vb_scan + vb_scatter (one global reservation per occupied bin and tile)
    VOX_PART_DET_CACHED = 2,     // vb_scan + vb_scatter_det on the counts voxel_bbox_pass left
    VOX_PART_DET_PER_RUN = 3,    // vb_plan + vox_setup + vb_hist_w + vb_colscan + vb_scan + vb_scatter_det
};

// What the host knows about one plan before a run.  No pointers.
struct VoxPlanState {
    int mode;                    // VOX_SORTED | VOX_BINNED: AUTO already resolved (voxel_resolve_mode)
    bool det_tables;             // the plan owns the tables of the deterministic partition (the raw local map)
    bool per_run;                // policy: bbox and counts are taken inside every run (else: cached where the input is written)
    bool bbox_valid;             // the bbox partial records are those of the current input
    bool counts_valid;           // … and so are the per-bin counts and the per-workgroup prefixes
    bool n_host;                 // the host knows the segment lengths (kernel arguments)
    bool slot_major;             // raw-map passes of a batch fold the slot into blockIdx.x
};

struct VoxSchedule {
    int mode;                    // VOX_SORTED | VOX_BINNED, the same for every slot
    VoxBbox bbox;
    VoxPart part;
    bool fold_slots;             // passes over the raw map: slot-major block order (when the pass's grid allows, nx % VB_XCD == 0)
    bool slot_by_slot;           // S > 1 and sorted: the radix sort is not batched, every slot runs alone (and sorted)
    // everything above in one word (what a captured launch sequence froze)
    int key() const { return mode | (int)bbox << 2 | (int)part << 4 | (fold_slots ? 64 : 0) | (slot_by_slot ? 128 : 0); }
};

// The launch sequence of one run over S slots.  The cached forms need EVERY slot's records valid, the per-run form every
// slot per-run: a batch whose slots disagree (some per-run — which hold no valid records — some cached) takes
// MINMAX + RESERVE, which is correct for any state.  The library never builds such a batch (stage_map_build gives
// every slot the policy and the validity of the one raw map they all read); the flag arithmetic this function replaced
// would have let its per-run slots read counts that were stale for them.
inline VoxSchedule vox_schedule(const VoxPlanState* st, int S)
{
    bool sorted = false, per_run = true, bbox = true, counts = true, fold = S > 1;
    for (int z = 0; z < S; z++) {
        sorted = sorted || st[z].mode == VOX_SORTED;              // the realisation is one for the whole launch
        per_run = per_run && st[z].per_run && st[z].det_tables;
        bbox = bbox && st[z].bbox_valid;
        counts = counts && st[z].bbox_valid && st[z].counts_valid;
        fold = fold && st[z].slot_major && st[z].n_host;
    }
    VoxSchedule s;
    s.mode = sorted ? VOX_SORTED : VOX_BINNED;
    s.fold_slots = fold;
    s.slot_by_slot = sorted && S > 1;
    if (!sorted && per_run) { s.bbox = VOX_BBOX_WITH_PLAN; s.part = VOX_PART_DET_PER_RUN; return s; }
    s.bbox = bbox ? VOX_BBOX_CACHED : VOX_BBOX_MINMAX;
    s.part = sorted ? VOX_PART_NONE : (counts ? VOX_PART_DET_CACHED : VOX_PART_RESERVE);
    return s;
}

}  // namespace lvi
