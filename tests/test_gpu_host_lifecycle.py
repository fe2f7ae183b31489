"""The one lifetime of the eleven HIP-only wrappers of the host mirror (host_api.py over _abi.Owned):
NodeDepthRegister, GlobalMapper, LoopCloser, KeyFrameMatcher, HostPnPRansac, LoopDetector, PoseGraphBackend,
VinsMarginalizer, VinsWindowOptimizer, FeatureManager, TrackerRig.

  close twice           each is created at the smallest legal capacities test_gpu_handle_lifecycle.py uses for the handle
                        underneath (a 64x48 image, a 4-ring scan where one is needed) and closed twice
  dropped               each is created once more and dropped without close(); after gc.collect() the free device memory
                        is within the allowance of test_gpu_handle_lifecycle.py: one arena per handle, bounded from below
  invalid capacity      an out-of-range capacity through a host wrapper: the error code and the create function's text

A dependant is closed before what it borrows: the detector before the PnP handle it calls, the window optimizer before
the marginaliser whose arrays it solves, the depth register before the node it is installed on.

The allowance.  GlobalMapper and LoopCloser allocate nothing when they are constructed (their arenas are the lidar
handle's, made by reserve()), so they add nothing.  A LoopDetector without a vocabulary holds its keyframe store only.
The camera rig is bounded by the previous and the current image of each slot.  The others are the arenas of
test_gpu_handle_lifecycle.py at the capacities lvi_marg_host.hpp and lvi_win_host.hpp derive from max_features.
"""
import gc

import pytest

import test_gpu_handle_lifecycle as L

pytestmark = pytest.mark.gpu

W, H = 64, 48
SEQ_P = dict(N_SCAN=4, Horizon_SCAN=4096, max_raw_points=16384, max_map_points=200000)
F = 1                                                    # max_features of the VINS wrappers (Fman.small)
WINDOW_SIZE = 10
KEEP = 15 * (WINDOW_SIZE + 1) + 7
MARG_CAPS = dict(max_blocks=2 * (WINDOW_SIZE + 1) + 2 + F, max_projections=max(1, F * WINDOW_SIZE), max_dense_factors=1, max_dense_rows=15,
                 max_drop_dim=15 + F, max_keep_dim=KEEP)                                         # VinsMarginalizer::caps
WIN_CAPS = dict(max_blocks=2 * (WINDOW_SIZE + 1) + 2 + F, max_projections=max(1, F * WINDOW_SIZE), max_eliminated=F, max_imu=WINDOW_SIZE,
                max_prior_rows=KEEP, max_dim=KEEP)                                               # VinsWindowOptimizer::caps
STORE = dict(max_width=16, max_height=16, max_keypoints=1, max_window=1)                         # Kf.small, Bow.make


def _all(pkg, hip, hl, mapper, node, tp):
    """the eleven wrappers in creation order, a dependant after what it borrows, each with the arena it may keep"""
    A = pkg.host_api
    pattern = L._pattern(pkg)
    arena = {k: L.KINDS[k](pkg, hip).arena for k in L.KINDS}
    out = [(A.NodeDepthRegister(hl, node, hip, **L.Depth.small), arena["depth"](**L.Depth.small)),
           (A.GlobalMapper(hl, mapper), 0),
           (A.LoopCloser(hl, mapper), 0),
           (A.KeyFrameMatcher(hl, pattern, max_keyframes=1, **STORE), arena["kf"](max_keyframes=1, **STORE)),
           (A.HostPnPRansac(hl, **L.Pnp.small), arena["pnp"](**L.Pnp.small))]
    det = A.LoopDetector(hl, hip, pattern, max_entries=1, max_keyframes=2, **STORE)
    det.usePnP(out[-1][0])
    out.append((det, arena["kf"](max_keyframes=2, **STORE)))
    out.append((A.PoseGraphBackend(hl, hip, **L.Pgo.small), arena["pgo"](**L.Pgo.small)))
    out.append((A.VinsMarginalizer(hl, hip, max_features=F), arena["marg"](**MARG_CAPS)))
    out.append((A.VinsWindowOptimizer(hl, hip, out[-1][0], max_features=F), arena["win"](**WIN_CAPS)))
    out.append((A.FeatureManager(hl, hip, max_features=F), arena["fman"](max_features=F)))
    out.append((A.TrackerRig(hl, tp, 1, H, W), 2 * W * H))
    assert [type(o).__name__ for o, _ in out] == ["NodeDepthRegister", "GlobalMapper", "LoopCloser", "KeyFrameMatcher", "HostPnPRansac", "LoopDetector",
                                                  "PoseGraphBackend", "VinsMarginalizer", "VinsWindowOptimizer", "FeatureManager", "TrackerRig"]
    return out


def test_host_wrappers_close_twice_and_are_finalised_when_dropped(pkg, hip):
    import torch
    A = pkg.host_api
    hl = pkg.load_host()
    tp = pkg.default_tracker_params(hip, max_width=W, max_height=H, max_features=64, max_cnt=20, min_dist=5.0)
    mapper = A.SequentialMapper(hl, hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
    node = A.TrackerNode(hl, tp, H, W, 10)
    try:
        made = _all(pkg, hip, hl, mapper, node, tp)
        while made:                                              # in reverse: a dependant before what it borrows
            obj, _ = made.pop()
            assert issubclass(type(obj), pkg._abi.Owned) and getattr(obj, obj._ptr)
            obj.close()
            assert not getattr(obj, obj._ptr)
            obj.close()
            del obj
        gc.collect()
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        made = _all(pkg, hip, hl, mapper, node, tp)
        allowance = sum(a for _, a in made)
        while made:
            made.pop()                                           # dropped without close()
        gc.collect()
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        print(f"free before {before}, after {after}, allowance {allowance}")
        assert allowance > 0 and after >= before - allowance, (before, after, allowance)
    finally:
        node.close()
        mapper.close()
    node.close()
    mapper.close()


def test_invalid_capacity_through_a_host_wrapper(pkg, hip):
    caps = dict(L.Pnp.caps)
    caps.update(L.Pnp.bad)
    with pytest.raises(pkg.LviError) as e:
        pkg.host_api.HostPnPRansac(pkg.load_host(), **caps)
    assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    assert f"({L.Pnp.bad_text})" in str(e.value)
