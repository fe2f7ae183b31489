// Internal view of the keyframe store of lvi_kf.hip for the other files of liblvi_hip.so (lvi_bow.hip reads the keypoint
// descriptors of a slot where they lie).  Not part of include/lvi_kf.h and not exported from the library.
#pragma once
#include "lvi_dev.hpp"
#include "../../include/lvi_kf.h"

namespace lvi {

struct KfStoreView {
    int device = 0, max_keypoints = 0;
    hipStream_t stream = nullptr;              // every lvi_kf_* call works on it; work that reads a slot goes there too
};

struct KfSlotView {
    bool valid = false;
    int n_kp = 0;
    const ulonglong2* kp_desc = nullptr;       // [n_kp][2]
    uint64_t generation = 0;                   // changes whenever describe, put or release touch the slot
};

__attribute__((visibility("hidden"))) bool kf_store_view(lvi_kf* h, KfStoreView* out);
__attribute__((visibility("hidden"))) bool kf_slot_view(lvi_kf* h, int32_t slot, KfSlotView* out);

}  // namespace lvi
