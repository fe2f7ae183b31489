"""CPU tier: the numpy reference of the scan feature extraction (tests/feat_ref.py) on hand-worked cases, and the C++
oracle against it on every tie-free scene of tests/feat_scenes.py."""
import numpy as np
import pytest

import feat_scenes as S
from feat_ref import CORNER_CAP, FeatRef, sector_bounds


def _ring30(first_ring=0, n_scan=1):
    r = np.full(30, 10.0, np.float32)
    r[12], r[21] = 11.0, 10.5
    rings = [np.zeros(0, np.float32)] * first_ring + [r]
    cols = [None] * first_ring + [10 * np.arange(30)]
    return S.assemble(rings, cols, n_scan=n_scan)


def _extract(ref, info):
    return ref.extract(info["point_range"], info["point_col_ind"], info["start_ring_index"], info["end_ring_index"])


def _check_ring30_first_scan(res):
    np.testing.assert_array_equal(res["curv"][5:25], np.float32([0, 0, 0, 0, 0, 1, 1, 16, 1, 1, 0, 0, 0, 0, 0.25, 0.25, 4, 0.25, 0.25, 0]))
    assert not res["occl"][5:25].any()
    np.testing.assert_array_equal(res["corner_idx"], [13, 21])
    assert {int(k): int(v) for k, v in enumerate(res["label"]) if v} == {0: -1, 6: -1, 13: 1, 21: 1}
    assert res["picked"][5:25].all()


def test_hand_worked_ring_of_30():
    """One ring of 30 points, range 10 except r[12] = 11 and r[21] = 10.5, columns 0, 10, 20, … (a difference of 10 is
    neither "< 10" nor "> 10": no occlusion test, no break), edgeThreshold 0.5, surfThreshold 0.1, fresh state.

    start = 4, end = 24, sectors [sp, ep] = [4,6] [7,9] [10,13] [14,16] [17,19] [20,23].
    diffRange: -4 at 12, +1 at 10, 11, 13, 14; -2 at 21, +0.5 at 19, 20, 22, 23 -> curvature 16, 1, 4, 0.25, else 0.
    Parallel beam at 12: |diff| = 1 is not above 0.1 * 11 -> no mark anywhere.
    [4,6]   no corner.  Surf: slot 4 is the stale entry {0, ind 0}: label[0] = -1, picked[0..5]; 5 is picked; slot 6 (ep, last):
            label[6] = -1, picked[1..11].
    [7,9]   all picked.
    [10,13] sorted range [10,13) = (1,10) (1,11) (16,12).  Corner walk starts at the ep slot: ind 13, curvature 1 > 0.5, unpicked
            -> corner 13, picked[8..18]; 12, 11, 10 are picked by now -> the largest curvature of the ring is NOT a corner.
    [14,16] [17,19] all picked, or 0.25 which is neither above 0.5 nor below 0.1.
    [20,23] sorted (0.25,20) (0.25,22) (4,21); ep slot 23 (0.25) no; ind 21 -> corner 21, picked[16..26].
    corners [13, 21]; labels {0: -1, 6: -1, 13: 1, 21: 1}; picked is 1 on all of [5, 25)."""
    assert [sector_bounds(4, 24, j) for j in range(6)] == [(4, 6), (7, 9), (10, 13), (14, 16), (17, 19), (20, 23)]
    _check_ring30_first_scan(_extract(FeatRef(1, 64, 0.5, 0.1), _ring30()))


def test_stale_slot_belongs_to_the_first_populated_ring_and_fires_once():
    """With ring 0 empty (start 4, end -6: C division leaves it no sector) ring 1 starts at 4 as well and sorts the stale
    entry in: the same results as the single-ring case.  A second scan on the same state: picked[0] is still 1, so ind 0
    is not labelled again and does not mark point 5; point 5 (curvature 0, unpicked) is the first real element of the surf
    walk instead: label[5] = -1, picked[0..10], and 6 is no longer labelled."""
    info = _ring30(first_ring=1, n_scan=2)
    assert list(info["start_ring_index"]) == [4, 4] and list(info["end_ring_index"]) == [-6, 24]
    assert all(sp >= ep for sp, ep in (sector_bounds(4, -6, j) for j in range(6)))
    ref = FeatRef(2, 64, 0.5, 0.1)
    _check_ring30_first_scan(_extract(ref, info))
    res = _extract(ref, info)
    np.testing.assert_array_equal(res["corner_idx"], [13, 21])
    assert res["label"][5] == -1 and res["label"][6] == 0 and res["picked"][5:25].all()


def test_the_41st_eligible_point_breaks_without_a_mark():
    """2000 points, a spike of growing height every 7th point, column gaps of 10, surfThreshold 0 (no surf walk): every sector
    holds 47 or 48 independent corner candidates; the walk takes the 40 highest, in descending order, and breaks at the 41st
    without labelling or marking it."""
    m = 2000
    r = np.full(m, 20.0, np.float32)
    spikes = np.arange(0, m, 7)
    r[spikes] += (0.5 + spikes / 8192.0).astype(np.float32)           # below 1: a spike's neighbours (diffRange = height) are no candidates
    info = S.assemble([r], [10 * np.arange(m)])
    res = _extract(FeatRef(1, m, 1.0, 0.0), info)
    assert len(res["sectors"]) == 6
    for s in res["sectors"]:
        lo = max(s["sp"], 5)                                                  # slot 4 holds the stale entry, not point 4
        want = ([s["ep"]] if s["ep"] in spikes else []) + sorted((int(k) for k in spikes if lo <= k < s["ep"]), reverse=True)
        assert len(want) > CORNER_CAP and s["broke"]
        assert s["taken"] == want[:CORNER_CAP]
        for k in want[CORNER_CAP:]:
            assert res["label"][k] == 0 and not res["picked"][k - 1:k + 2].any()
    assert len(res["corner_idx"]) == 6 * CORNER_CAP


def test_scene_builders_hold_their_conditions():
    """building the scenes runs every builder's assertions (tie groups, cap batches, break positions, sector lengths)"""
    scenes = S.all_scenes()
    assert tuple(scenes) == S.SCENE_NAMES
    assert tuple(n for n, sc in scenes.items() if not sc["tie_free"]) == S.TIED_SCENES


@pytest.mark.parametrize("name", [n for n in S.SCENE_NAMES if n not in S.TIED_SCENES])
def test_oracle_equals_reference_on_tie_free_scenes(pkg, oracle, name):
    """curvature bits, occlusion flags, labels, final picked flags over [5, n-5) and the corner indices, exact, for every scan
    of the scene on one oracle handle (fresh, then reused).  The scenes with curvature ties are left out: the oracle sorts
    with std::sort, whose order among equal keys is unspecified, so its result there is one of several the reference node
    could produce, while feat_ref.py fixes one (ascending (value, ind)); on those scenes only feat_ref.py can judge."""
    sc = S.all_scenes()[name]
    assert sc["tie_free"]
    rows = S.run_scene(pkg, oracle, sc, sc["n_rings"])
    for q, (got, want) in enumerate(zip(rows, sc["ref"])):
        S.assert_same(got, want, f"{name} scan {q}")
