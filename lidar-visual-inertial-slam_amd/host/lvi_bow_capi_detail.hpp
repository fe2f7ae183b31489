// Internal to the C flattenings of the loop detector (lvi_bow_capi.cpp) and of its PnP hook (lvi_pnp_capi.cpp): the
// object behind the void* of lvh_bow_create.  Not part of any exported interface.
#pragma once
#include "lvi_bow_host.hpp"

namespace lvi_host_capi {

struct Detector {
    lvi_host::KeyFrameDescriber kd;
    lvi_host::LoopDetector ld;
    lvi_host::LoopResult last;
    template <class... A> explicit Detector(int max_entries, A... a) : kd(a...), ld(kd, max_entries) {}
};

}  // namespace lvi_host_capi
