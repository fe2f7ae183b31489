"""GPU tier (-m gpu): block order of the batched passes over the raw local map (vb_plan, vb_hist_w, vb_scatter_det, and the bbox
pass of the cached plan).

A batch launch folds the slot into blockIdx.x so that the workgroups of all slots that own one point range run side by side
on one XCD (LVI_VB_SLOT_ORDER, default 1); LVI_VB_SLOT_ORDER=0 keeps the slot in blockIdx.z.  The order is a placement only:
every (range, segment, slot) must be decoded exactly once, so every slot's DS map has the bits of a fresh single-scan handle
that takes the sorted realisation — for 1, 3 (not a power of two, fewer than the argument blocks of a launch) and 8 slots, with
the plan taken per rebuild and cached, on the first build of an upload (vb_hist_w), the second (vb_plan's counts stand) and after
the map moved by half a metre (another grid).

Map sizes: a range is 4 096 points here, the decode walks ranges in groups of 8.  3 x 4096 + 17 surf points are four active
ranges with a ragged last tile and 508 empty ones, 100 corner points one active range and 511 empty ones; 8 x 4096 + 1 surf
points are nine ranges, one beyond the first group."""
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


@pytest.fixture(scope="module")
def maps(pkg, hip):
    """name -> [(corner, surf, wanted DS bits)] for the map as drawn and moved by 0.5 m; wanted = a fresh sorted-mode handle"""
    rng = np.random.default_rng(5)
    out = {}
    for name, (nc, ns) in SIZES.items():
        c, s = _cloud(rng, nc), _cloud(rng, ns)
        sc, ss = c.copy(), s.copy()
        sc[:, 0] += 0.5; ss[:, 0] += 0.5
        out[name] = []
        for cc, cs in ((c, s), (sc, ss)):
            fresh = pkg.LidarHotpath(hip, **small_params(voxel_mode=1, **PARAMS))
            fresh.map_set(cc, cs)
            want = _map_ds_bits(fresh)
            fresh.close()
            assert len(want[0]) > 0 and len(want[1]) > 100
            out[name].append((cc, cs, want))
    return out


def _assert_every_slot(g, slots, want, what):
    for z in range(slots):
        g.batch_select(z)
        for got, w, kind in zip(_map_ds_bits(g), want, ("corner", "surf")):
            np.testing.assert_array_equal(got, w, err_msg=f"{what}, slot {z}, {kind}")
    g.batch_select(0)


@pytest.mark.parametrize("cache", [0, 1], ids=["plan_per_rebuild", "plan_cached"])
@pytest.mark.parametrize("order", [0, 1], ids=["z_major", "slot_major"])
@pytest.mark.parametrize("slots", [1, 3, 8])
def test_every_slot_builds_the_same_ds_map_in_either_block_order(pkg, hip, maps, monkeypatch, slots, order, cache):
    monkeypatch.setenv("LVI_VB_SLOT_ORDER", str(order))            # read when the handle is created
    g = pkg.LidarHotpath(hip, **small_params(batch_scans=slots, voxel_mode=2, map_plan_cache=cache, **PARAMS))
    for name, ((c, s, want), (sc, ss, want_shifted)) in maps.items():
        g.map_upload(c, s)
        g.map_build()
        _assert_every_slot(g, slots, want, f"{name}: first build")
        g.map_build()                                               # the unchanged map again: plan_ok
        _assert_every_slot(g, slots, want, f"{name}: second build")
        g.map_upload(sc, ss)
        g.map_build()                                               # same size, another grid
        _assert_every_slot(g, slots, want_shifted, f"{name}: moved map")
    g.close()


@pytest.mark.parametrize("order", [0, 1], ids=["z_major", "slot_major"])
def test_a_sharing_batch_handle_built_beside_its_owner(pkg, hip, maps, monkeypatch, order):
    """lvi_map_share: the slots of the sharer and the owner read one raw map; both build it, twice"""
    monkeypatch.setenv("LVI_VB_SLOT_ORDER", str(order))
    c, s, want = maps["nine_ranges"][0]
    owner = pkg.LidarHotpath(hip, **small_params(batch_scans=3, voxel_mode=2, **PARAMS))
    sharer = pkg.LidarHotpath(hip, **small_params(batch_scans=8, voxel_mode=2, **PARAMS))
    owner.map_upload(c, s)
    sharer.map_share(owner)
    for build in ("first build", "second build"):
        owner.map_build(); sharer.map_build()
        _assert_every_slot(sharer, 8, want, f"sharer, {build}")
        _assert_every_slot(owner, 3, want, f"owner, {build}")
    sharer.close(); owner.close()
