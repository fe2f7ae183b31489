"""GPU tier (-m gpu): feat_smooth / feat_sector / feat_sector_big / feat_finalize against the numpy reference
(tests/feat_ref.py) on the scenes of tests/feat_scenes.py — ties, column breaks inside sectors, the 40-corner cap, threshold
equalities, the smallest geometries and the LDS capacity boundary.  Everything is compared exactly; there is no tolerance.

Compared per scan: curvature bits, DBG_PICKED_OCCL, DBG_LABEL and DBG_PICKED_FINAL over the whole window [5, n-5) that a
scan rewrites (the last slot n-6 included: the reference resets it and every mark that reaches it is specified), and
DBG_CORNER_INDEX whole.

Forms: every scene runs on three handles, and every scan of it on each — fresh, then reused:
  pipelined   the scene's own ring count (at most 4): one workgroup per (ring, sector) for every ring whose six sectors are regular
  redo        the same with sector_handover_wait_us = -1: no workgroup waits, each walks its ring from sector 0 itself
  sequential  N_SCAN = 6 (two more, empty rings): one workgroup per ring walks the six sectors in order
A ring with a degenerate sector takes the sequential form on all three, a ring with an oversize sector the global-memory
kernel (big) on all three.  The three must agree with the reference and therefore bit for bit with each other; the test
also compares them directly so that a failure names the form."""
import numpy as np
import pytest

import feat_scenes as S
from feat_ref import FeatRef

pytestmark = pytest.mark.gpu

FORMS = (("pipelined", lambda sc: dict(n_scan=sc["n_rings"])),
         ("redo", lambda sc: dict(n_scan=sc["n_rings"], sector_handover_wait_us=-1)),
         ("sequential", lambda sc: dict(n_scan=6)))


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_hip_equals_reference_in_every_form(pkg, hip, name):
    sc = S.all_scenes()[name]
    assert sc["n_rings"] <= 4
    rows = {form: S.run_scene(pkg, hip, sc, **kw(sc)) for form, kw in FORMS}
    errors = []
    for form, got in rows.items():
        for q, (g, want) in enumerate(zip(got, sc["ref"])):
            try:
                S.assert_same(g, want, f"{name}, {form}{' (big kernel)' if sc['big'] else ''}, scan {q}")
            except AssertionError as e:
                errors.append(str(e).strip().splitlines())
    for form in ("redo", "sequential"):
        for q, (a, b) in enumerate(zip(rows["pipelined"], rows[form])):
            try:
                S.assert_same(b, a, f"{name}, {form} against pipelined, scan {q}")
            except AssertionError as e:
                errors.append(str(e).strip().splitlines())
    assert not errors, "\n".join("\n".join(e[:12]) for e in errors)


def test_staged_path_on_a_quantised_scan(pkg, hip):
    """scan_upload / scan_organize / scan_extract: Livox points on the x axis with x a multiple of 1/16, so that the range
    (sqrt(x*x)) equals x exactly and curvature ties survive the organise stage.  The organised scan is read back, checked
    to be the ranges that went in (ring by ring, dense column counters) and judged by the reference, fresh and reused."""
    A = pkg._abi
    sc = S.all_scenes()["ties"]
    g = pkg.LidarHotpath(hip, N_SCAN=4, Horizon_SCAN=4096, max_raw_points=16384, max_map_points=4096, edgeThreshold=sc["edge"], surfThreshold=sc["surf"])
    ref = FeatRef(4, 4096, sc["edge"], sc["surf"])
    for q, info in enumerate(sc["scans"]):
        n = info["n"]
        ring = np.repeat(np.arange(4), info["ring_sizes"])
        order = np.lexsort((np.arange(n), (np.arange(n) + q) % 97))                  # message order: the rings interleaved
        scan = np.zeros(n + 1, A.LIVOX_DTYPE)                                        # the last raw point is dropped
        scan["x"][:n] = info["point_range"][order]
        scan["line"][:n] = ring[order]
        scan["x"][n] = 9.0
        g.scan_upload(scan); g.scan_organize(); g.scan_extract()
        got = g.get_scan_info()
        assert got["n"] == n
        want_r = np.concatenate([info["point_range"][order][ring[order] == r] for r in range(4)])
        np.testing.assert_array_equal(got["point_range"].view(np.uint32), want_r.view(np.uint32))
        np.testing.assert_array_equal(got["point_col_ind"], np.concatenate([np.arange(m) for m in info["ring_sizes"]]))
        np.testing.assert_array_equal(got["start_ring_index"], info["start_ring_index"])
        want = ref.extract(got["point_range"], got["point_col_ind"], got["start_ring_index"], got["end_ring_index"])
        assert len(want["corner_idx"]) > 50 and (want["label"] == -1).sum() > 200
        row = dict(n=n, curv=g.debug_get(A.DBG_CURVATURE, np.float32)[:n], occl=g.debug_get(A.DBG_PICKED_OCCL, np.int32)[:n],
                   label=g.debug_get(A.DBG_LABEL, np.int32)[:n], picked=g.debug_get(A.DBG_PICKED_FINAL, np.int32)[:n],
                   corner_idx=g.debug_get(A.DBG_CORNER_INDEX, np.int32))
        S.assert_same(row, want, f"staged path, scan {q}")
    g.close()
