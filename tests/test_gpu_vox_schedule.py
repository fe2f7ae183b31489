"""GPU tier (-m gpu): the raw local map's VoxelGrid through every transition of its schedule (csrc/lvi_vox_schedule.hpp) that the
other tests do not reach, and the launches each schedule consists of.

Every expectation is the DS map of a fresh single-scan handle that takes the sorted realisation (voxel_mode=1) of the same raw
map, bit for bit.  A stale bounding box or stale per-bin counts — an invalidation that was lost — would place points in the
voxels of another grid: the moved map below is the same cloud half a metre further, another grid for the same sizes.

Map sizes as in test_gpu_map_slot_order.py: 3 x 4096 + 17 surf points are four ranges of the deterministic partition with a
ragged last tile, 8 x 4096 + 1 nine ranges (a second decode group); 100 corner points are one range."""
import numpy as np
import pytest

from helpers import small_params, xyzi

pytestmark = pytest.mark.gpu

SIZES = {"four_ranges_ragged": (100, 3 * 4096 + 17), "nine_ranges": (100, 8 * 4096 + 1)}
PARAMS = dict(max_map_points=40000)


def _map_ds_bits(g):
    return [xyzi(c).view(np.uint32).copy() for c in g.get_map_ds()]


def _cloud(rng, n):
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.normal(0, 6, (n, 3)) * [1, 1, 0.2]
    pts[:, 3] = rng.uniform(-5, 300, n)
    return pts


def _want(pkg, hip, c, s):
    fresh = pkg.LidarHotpath(hip, **small_params(voxel_mode=1, **PARAMS))
    fresh.map_set(c, s)
    want = _map_ds_bits(fresh)
    fresh.close()
    assert len(want[0]) > 0 and len(want[1]) > 100
    return want


@pytest.fixture(scope="module")
def maps(pkg, hip):
    """name -> [(corner, surf, wanted DS bits)] for the map as drawn and moved by 0.5 m"""
    rng = np.random.default_rng(11)
    out = {}
    for name, (nc, ns) in SIZES.items():
        c, s = _cloud(rng, nc), _cloud(rng, ns)
        sc, ss = c.copy(), s.copy()
        sc[:, 0] += 0.5; ss[:, 0] += 0.5
        out[name] = [(cc, cs, _want(pkg, hip, cc, cs)) for cc, cs in ((c, s), (sc, ss))]
    return out


def _assert_every_slot(g, slots, want, what):
    for z in range(slots):
        g.batch_select(z)
        for got, w, kind in zip(_map_ds_bits(g), want, ("corner", "surf")):
            np.testing.assert_array_equal(got, w, err_msg=f"{what}, slot {z}, {kind}")
    g.batch_select(0)


@pytest.mark.parametrize("slots", [1, 3])
def test_cached_plan_under_auto_takes_the_counts_on_the_second_build(pkg, hip, maps, slots):
    """voxel_mode=0: a plan's first build is sorted (no grid hint yet), so the bbox pass takes no counts; the second build is
    binned and the pass runs once more for them; the third re-takes nothing; an upload starts over (now binned at once)"""
    for name, ((c, s, want), (sc, ss, want_moved)) in maps.items():
        g = pkg.LidarHotpath(hip, **small_params(batch_scans=slots, voxel_mode=0, map_plan_cache=1, **PARAMS))
        g.map_upload(c, s)
        for build in ("first build (sorted)", "second build (binned, counts taken)", "third build (all cached)"):
            g.map_build()
            _assert_every_slot(g, slots, want, f"{name}: {build}")
        g.map_upload(sc, ss)
        g.map_build()
        _assert_every_slot(g, slots, want_moved, f"{name}: moved map")
        g.close()


def test_cached_plan_is_retaken_after_an_assembly_and_after_an_upload(pkg, hip, maps):
    A = pkg._abi
    c, s, _ = maps["four_ranges_ragged"][0]
    oc, osf, want_other = maps["nine_ranges"][1]
    g = pkg.LidarHotpath(hip, **small_params(voxel_mode=2, map_plan_cache=1, max_keyframes=8, max_keyframe_points=40000, **PARAMS))
    half = len(s) // 2
    g.keyframe_add(c[:40], s[:half], [0, 0, 0, 0, 0, 0])
    g.keyframe_add(c[40:], s[half:], [0.02, -0.01, 0.3, 1.5, -2.0, 0.25])

    def assembled(keys):
        g.map_assemble(keys)                                        # fuses the keyframes into the raw map and builds
        raw = [xyzi(g.debug_get(w, A.PT_DTYPE)).copy() for w in (A.DBG_MAP_CORNER_RAW, A.DBG_MAP_SURF_RAW)]
        assert len(raw[0]) == len(c) and len(raw[1]) == len(s)
        return _want(pkg, hip, raw[0], raw[1])

    want = assembled([0, 1])
    _assert_every_slot(g, 1, want, "assembled map, first build")
    for build in ("second build", "third build"):
        g.map_build()
        _assert_every_slot(g, 1, want, f"assembled map, {build}")
    g.map_upload(oc, osf)
    g.map_build()
    _assert_every_slot(g, 1, want_other, "uploaded map after the assembly")
    g.map_build()
    _assert_every_slot(g, 1, want_other, "uploaded map, second build")
    want = assembled([1, 0])                                        # the plan of the uploaded map is valid when the assembly rewrites the raw map
    _assert_every_slot(g, 1, want, "assembly after the upload")
    g.close()


def test_cached_plan_of_a_sharer_follows_the_map_it_reads(pkg, hip, maps):
    (c, s, want_a), (sc, ss, want_b) = maps["nine_ranges"]
    oc, osf, want_own = maps["four_ranges_ragged"][0]
    a = pkg.LidarHotpath(hip, **small_params(voxel_mode=2, **PARAMS))
    b = pkg.LidarHotpath(hip, **small_params(voxel_mode=2, **PARAMS))
    g = pkg.LidarHotpath(hip, **small_params(batch_scans=3, voxel_mode=2, map_plan_cache=1, **PARAMS))
    a.map_upload(c, s); b.map_upload(sc, ss)                        # same sizes, other points
    g.map_share(a)
    for build in ("first build", "second build"):
        g.map_build()
        _assert_every_slot(g, 3, want_a, f"owner A, {build}")
    g.map_share(b)
    g.map_build()
    _assert_every_slot(g, 3, want_b, "owner B")
    g.map_upload(oc, osf)
    g.map_build()
    _assert_every_slot(g, 3, want_own, "own map")
    g.close(); a.close(); b.close()


def _launches_of(g, fn):
    g.prof_reset()
    fn()
    return {r["name"]: r["launches"] for r in g.prof_read()}


@pytest.mark.parametrize("slots", [1, 3])
def test_launches_of_each_map_schedule(pkg, hip, maps, slots):
    """the counts follow from the schedule definitions (VoxBbox / VoxPart): they are not measurements"""
    c, s, want = maps["nine_ranges"][0]
    per = pkg.LidarHotpath(hip, **small_params(batch_scans=slots, voxel_mode=2, **PARAMS))
    cached = pkg.LidarHotpath(hip, **small_params(batch_scans=slots, voxel_mode=2, map_plan_cache=1, **PARAMS))
    for g in (per, cached):
        g.prof_enable(True)
        g.map_upload(c, s)
    # WITH_PLAN + DET_PER_RUN, on every build
    for build in range(2):
        n = _launches_of(per, per.map_build)
        assert n.get("vb_plan/map") == 1 and "vox_minmax/map" not in n and "vb_hist/map" not in n, n
        assert n.get("vox_setup/map") == 1 and n.get("vb_hist_w/map") == 1 and n.get("vb_colscan/map") == 1 and n.get("vb_scan/map") == 1 and n.get("vb_scatter/map") == 1, n
    # the bbox pass (vox_minmax, vox_setup, vb_hist_w under the name vb_hist, vb_colscan), then CACHED + DET_CACHED
    n = _launches_of(cached, cached.map_build)
    assert n.get("vox_minmax/map") == 1 and n.get("vb_hist/map") == 1 and n.get("vb_colscan/map") == 1 and "vb_plan/map" not in n, n
    assert n.get("vox_setup/map") == 2 and n.get("vb_scan/map") == 1 and n.get("vb_scatter/map") == 1 and "vb_hist_w/map" not in n, n
    # CACHED + DET_CACHED alone
    n = _launches_of(cached, cached.map_build)
    assert "vox_minmax/map" not in n and "vb_hist/map" not in n and "vb_plan/map" not in n and "vb_colscan/map" not in n, n
    assert n.get("vox_setup/map") == 1 and n.get("vb_scan/map") == 1 and n.get("vb_scatter/map") == 1, n
    for g in (per, cached):
        _assert_every_slot(g, slots, want, "profiled builds")
        g.close()


def test_ring_and_scan_plans_take_the_reserving_partition(pkg, hip):
    """generic plans: MINMAX + RESERVE; nothing of the deterministic partition"""
    S = pkg.synth
    g = pkg.LidarHotpath(hip, **small_params(voxel_mode=2, **PARAMS))
    g.prof_enable(True)
    scan = S.make_scan(20001, S.loop_pose(0.37, 0.01, -0.02), 12345)

    def stages():
        g.scan_upload(scan); g.scan_organize(); g.scan_extract(); g.scan_downsample()
    n = _launches_of(g, stages)
    assert not [k for k in n if k.startswith(("vb_plan", "vb_colscan", "vb_hist_w"))], n
    for tag in ("ring", "scan"):
        assert n.get(f"vox_minmax/{tag}") == 1 and n.get(f"vb_hist/{tag}") == 1 and n.get(f"vb_scatter/{tag}") == 1, n
    g.close()
