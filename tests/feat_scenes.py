"""Injected scenes for the scan feature extraction (tests/feat_ref.py is the judge).

A scene is a short sequence of scans for ONE handle, each a (point_range, point_col_ind, start_ring_index, end_ring_index)
record for `extract_features(info)`.  Every builder asserts, from the reference alone, that its scene holds what it is
for; `conditions` keeps the figures it found.  Scenes are built once per process (`all_scenes()`)."""
import functools

import numpy as np

from feat_ref import CORNER_CAP, FeatRef, curvature, sector_bounds

FEAT_SEG_CAP = 8192          # LDS-resident sector capacity of the HIP kernel (points incl. the two five-point halos)
PT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])


# ----------------------------------------------------------------------------- assembly
def assemble(ring_ranges, ring_cols=None, n_scan=None):
    """rings in order -> scan info; columns default to the dense per-ring counter"""
    n_scan = max(n_scan or 0, len(ring_ranges))
    rr = [np.asarray(r, np.float32) for r in ring_ranges] + [np.zeros(0, np.float32)] * (n_scan - len(ring_ranges))
    cc = [np.arange(len(r)) if ring_cols is None or q >= len(ring_cols) or ring_cols[q] is None else np.asarray(ring_cols[q])
          for q, r in enumerate(rr)]
    start, end, count = [], [], 0
    for r in rr:                                       # imageProjection: start = count - 1 + 5, end = count - 1 - 5
        start.append(count - 1 + 5)
        count += len(r)
        end.append(count - 1 - 5)
    rng = np.concatenate(rr) if rr else np.zeros(0, np.float32)
    col = np.concatenate(cc).astype(np.int32) if cc else np.zeros(0, np.int32)
    pts = np.zeros(len(rng), PT_DTYPE)
    pts["x"] = rng
    pts["y"] = np.concatenate([np.full(len(r), q, np.float32) for q, r in enumerate(rr)]) if rr else 0
    pts["intensity"] = np.arange(len(rng)) % 256
    return dict(n=len(rng), point_range=rng, point_col_ind=col, start_ring_index=np.asarray(start, np.int32),
                end_ring_index=np.asarray(end, np.int32), cloud_deskewed=pts, ring_sizes=[len(r) for r in rr])


def pad_rings(info, n_scan):
    """the same scan for a handle with more rings (the extra ones are empty)"""
    have = len(info["start_ring_index"])
    assert n_scan >= have
    out = dict(info)
    n = info["n"]
    out["start_ring_index"] = np.concatenate([info["start_ring_index"], np.full(n_scan - have, n + 4, np.int32)])
    out["end_ring_index"] = np.concatenate([info["end_ring_index"], np.full(n_scan - have, n - 6, np.int32)])
    return out


def sectors_of(info):
    for ring, (s, e) in enumerate(zip(info["start_ring_index"], info["end_ring_index"])):
        for j in range(6):
            sp, ep = sector_bounds(int(s), int(e), j)
            if sp < ep:
                yield ring, j, sp, ep


def longest_sector(info):
    return max((ep - sp + 11 for _, _, sp, ep in sectors_of(info)), default=0)


def tied_points(info, edge, surf):
    """indices of walk-eligible points (curvature above the edge or below the surf threshold) of a sorted range [sp, ep)
    that share their curvature with another such point of the range — or, in the range that starts at slot 4, with the
    stale entry {0, ind 0}.  Only among these can an unspecified sort order show."""
    n = info["n"]
    curv = np.zeros(n, np.float32)
    if n > 10:
        curv[5:n - 5] = curvature(info["point_range"])
    out = []
    for _, _, sp, ep in sectors_of(info):
        lo = max(sp, 5)
        c = curv[lo:ep]
        el = (c > np.float32(edge)) | (c < np.float32(surf))
        idx = np.arange(lo, ep)[el]
        v = c[el]
        if sp == 4 and np.float32(0) < np.float32(surf):
            out.append(idx[v == 0])
        u, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        out.append(idx[cnt[inv] > 1])
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


def make_tie_free(info, edge, surf, seed, amp=2e-3):
    """nudge the ranges of tied points until no eligible two of a sorted range share a curvature"""
    rs = np.random.RandomState(seed)
    r = info["point_range"].copy()
    for _ in range(200):
        info["point_range"] = r
        t = tied_points(info, edge, surf)
        if len(t) == 0:
            info["cloud_deskewed"]["x"] = r
            return info
        r = r.copy()
        r[t] = (r[t] + rs.uniform(-amp, amp, len(t))).astype(np.float32)
    raise AssertionError("could not make the scene tie-free")


def rough_ring(rs, m, base=9.0, noise=0.02, spike_every=0.04, flat=False):
    """a continuous ring: slow wave, a few steps, noise, isolated spikes (corners) — all well inside every range gate"""
    if m == 0:
        return np.zeros(0, np.float32)
    t = np.arange(m)
    r = base + 1.5 * np.sin(t * 0.021 + rs.uniform(0, 6)) + np.cumsum((rs.uniform(size=m) < 0.015) * rs.uniform(-1.2, 1.2, m))
    r = r + rs.uniform(-noise, noise, m)
    if not flat:
        sp = rs.uniform(size=m) < spike_every
        r = r + sp * rs.uniform(0.28, 1.4, m) * rs.choice([-1.0, 1.0], m)
    return np.maximum(r, 2.0).astype(np.float32)


def run_reference(scene):
    ref = FeatRef(len(scene["scans"][0]["start_ring_index"]), max(64, max(s["n"] for s in scene["scans"])), scene["edge"], scene["surf"])
    return [ref.extract(s["point_range"], s["point_col_ind"], s["start_ring_index"], s["end_ring_index"]) for s in scene["scans"]]


def finish(name, scans, edge=1.0, surf=0.1, tie_free=False, conditions=None, seed=0):
    if tie_free:
        scans = [make_tie_free(s, edge, surf, seed + 100 + q) for q, s in enumerate(scans)]
        for s in scans:
            assert len(tied_points(s, edge, surf)) == 0
    else:
        tie_free = all(len(tied_points(s, edge, surf)) == 0 for s in scans)
    scene = dict(name=name, scans=scans, edge=edge, surf=surf, tie_free=tie_free, conditions=dict(conditions or {}))
    scene["n_rings"] = len(scans[0]["start_ring_index"])
    assert all(len(s["start_ring_index"]) == scene["n_rings"] for s in scans)
    scene["big"] = any(longest_sector(s) > FEAT_SEG_CAP for s in scans)
    scene["ref"] = run_reference(scene)
    return scene


# ----------------------------------------------------------------------------- the families
def scene_tie_free():
    rs = np.random.RandomState(11)
    scans = [assemble([rough_ring(rs, m) for m in sizes]) for sizes in ((700, 431, 520, 613), (655, 702, 388, 540))]
    sc = finish("tie_free", scans, tie_free=True, seed=11)
    assert all(len(r["corner_idx"]) > 20 and (r["label"] == -1).sum() > 50 and r["occl"].sum() > 20 for r in sc["ref"])
    sc["conditions"].update(rings=[s["ring_sizes"] for s in scans], tied_eligible_points=0)
    return sc


def _quantised_ring(rs, m, gaps=(1, 10, 10, 10), spike_p=0.25):
    u = rs.randint(0, 5, m)
    s = (rs.uniform(size=m) < spike_p) * rs.randint(5, 9, m)
    r = (8.0 + (u + s) / 16.0).astype(np.float32)
    return r, rs.choice(gaps, m)


def _cols(gaps):
    return np.cumsum(gaps) - gaps[0] if len(gaps) else np.zeros(0, np.int64)


def _tie_groups(res, info, edge, surf):
    """per sector: (groups of equal curvature among corner-eligible points, same among surf-eligible points, tied pairs
    within 5 positions corner / surf, ep tied with a range point within 5 positions: corner / surf); eligibility as the
    sector walk first meets it: the occlusion marks"""
    rows = []
    curv, occl = res["curv"], res["occl"]
    for ring, j, sp, ep in sectors_of(info):
        lo = max(sp, 5)
        idx = np.arange(lo, ep)
        free = occl[lo:ep] == 0
        row = []
        near = []
        epn = []
        for sel in (curv[lo:ep] > np.float32(edge), curv[lo:ep] < np.float32(surf)):
            ii, v = idx[sel & free], curv[lo:ep][sel & free]
            u, cnt = np.unique(v, return_counts=True)
            row.append(int((cnt > 1).sum()))
            close = 0
            for d in range(1, 6):
                both = np.isin(ii + d, ii)
                close += int((curv[ii[both]] == curv[ii[both] + d]).sum())
            near.append(close)
            epn.append(bool(occl[ep] == 0 and any(q in ii and curv[q] == curv[ep] for q in range(ep - 5, ep))))
        rows.append(dict(ring=ring, sec=j, corner_groups=row[0], surf_groups=row[1], corner_near=near[0], surf_near=near[1],
                         ep_corner=epn[0], ep_surf=epn[1]))
    return rows


def scene_ties():
    """ranges are multiples of 1/16: curvature is exact and heavily tied.  edge = surf = 1.0 leaves sixteen distinct values
    below the surf threshold (|diffRange| = 0 … 15/16), enough for ten tie groups per sector"""
    rs = np.random.RandomState(23)
    edge = surf = 1.0
    scans = []
    for sizes in ((2100, 2060, 2210, 2140), (2080, 2130, 2105, 2200)):
        rr, gg = zip(*[_quantised_ring(rs, m) for m in sizes])
        rr, gg = [r.copy() for r in rr], [g.copy() for g in gg]
        info0 = assemble(rr)
        for ring, j, sp, ep in sectors_of(info0):
            base = int(info0["start_ring_index"][ring]) - 4
            e = ep - base                                           # ring-local index of the ep slot
            if (ring + j) % 2 == 0:                                 # period-3 spike pattern: curvature[ep] == curvature[ep - 3], both corners
                rr[ring][e - 7:e + 3] = np.float32(8.0)
                rr[ring][[e - 6, e - 3, e]] = np.float32(8.0 + 6 / 16.0)
                gg[ring][e - 9:e + 5] = 10                          # gaps of 10 here: no occlusion marks, no break
            else:                                                   # flat: zero curvature at ep and before it
                rr[ring][e - 7:e + 3] = np.float32(8.0)
        rr[0][10:30] = np.float32(8.25)                             # ring 0, sector 0: zero curvature beside the stale entry {0, ind 0}
        scans.append(assemble(rr, [_cols(g) for g in gg]))
    sc = finish("ties", scans, edge=edge, surf=surf)
    assert not sc["tie_free"]
    for info, res in zip(sc["scans"], sc["ref"]):
        assert np.all(info["point_range"] * 16 == np.round(info["point_range"] * 16))
        rows = _tie_groups(res, info, edge, surf)
        assert len(rows) == 24
        assert min(r["corner_groups"] for r in rows) >= 10 and min(r["surf_groups"] for r in rows) >= 10, rows
        assert sum(r["corner_near"] for r in rows) >= 10 and sum(r["surf_near"] for r in rows) >= 10
        assert any(r["ep_corner"] for r in rows) and any(r["ep_surf"] for r in rows)
        _, _, sp0, ep0 = next(sectors_of(info))
        assert sp0 == 4 and ((res["curv"][5:ep0] == 0) & (res["occl"][5:ep0] == 0)).sum() >= 2
    rows = _tie_groups(sc["ref"][0], sc["scans"][0], edge, surf)
    sc["conditions"].update(min_corner_groups=min(r["corner_groups"] for r in rows), min_surf_groups=min(r["surf_groups"] for r in rows),
                            corner_pairs_within_5=sum(r["corner_near"] for r in rows), surf_pairs_within_5=sum(r["surf_near"] for r in rows),
                            sectors_with_ep_tie=(sum(r["ep_corner"] for r in rows), sum(r["ep_surf"] for r in rows)))
    return sc


def _break_distances(res, col):
    n = len(col)
    brk = np.zeros(n + 1, bool)
    brk[1:n] = np.abs(np.diff(col.astype(np.int64))) > 10       # brk[k]: jump between k-1 and k
    fwd, bwd = set(), set()
    for c in res["corner_idx"]:
        for d in range(1, 6):
            if c + d < n and brk[c + d]:
                fwd.add(d)
                break
        for d in range(1, 6):
            if c - d + 1 >= 1 and brk[c - d + 1]:
                bwd.add(d)
                break
    return fwd, bwd


def scene_column_breaks():
    """columns are per-ring cumulative sums of gaps from {1, 9, 10, 11}: 9 keeps the occlusion test (< 10), 10 neither, 11 breaks
    the neighbour marks (> 10).  Breaks are planted where the kernel's bitmaps change word and at a sector's rims"""
    rs = np.random.RandomState(37)
    scans = []
    for sizes in ((1000, 960, 1100, 1210), (1180, 1000, 990, 1050)):
        rr = [rough_ring(rs, m) for m in sizes]
        gaps = [rs.choice([1, 9, 10, 11], m, p=[0.82, 0.08, 0.07, 0.03]) for m in sizes]
        info0 = assemble(rr)
        planted = 0
        for ring, j, sp, ep in sectors_of(info0):
            base = int(info0["start_ring_index"][ring]) - 4
            k0 = sp - 5
            want = {0: (64, 128), 1: (63, 127), 2: (65, 129), 3: (64, 65), 4: (127, 128, 129), 5: (63, 64)}[j]
            want = [k0 + w for w in want]
            want += [sp + 1 + (ring + j) % 4, ep - (ring + j) % 4]                # inside the first / last five points of the sector
            for k in want:
                gaps[ring][k - base] = 11
            # corners with a break at distance d on one side: a spike with gaps of 10 around it (no occlusion mark)
            d = 1 + (ring * 6 + j) % 5
            c = sp + 30 - base
            rr[ring][c - 8:c + 9] = rr[ring][c - 8]
            rr[ring][c] += np.float32(2.0)
            gaps[ring][c - 7:c + 9] = 10
            if (ring + j) % 2 == 0:
                gaps[ring][c + d] = 11                                            # between c+d-1 and c+d
            else:
                gaps[ring][c - d + 1] = 11                                        # between c-d and c-d+1
            planted += 1
        scans.append(assemble(rr, [_cols(g) for g in gaps]))
    sc = finish("column_breaks", scans, tie_free=True, seed=37)
    for info, res in zip(sc["scans"], sc["ref"]):
        col = info["point_col_ind"].astype(np.int64)
        jump = np.abs(np.diff(col)) > 10
        local = set()
        rim = 0
        for ring, j, sp, ep in sectors_of(info):
            base = int(info["start_ring_index"][ring]) - 4
            ks = np.flatnonzero(jump[sp - 1:ep]) + sp                             # jump between k-1 and k, sp <= k <= ep
            ks = ks[ks > base]                                                    # not the ring boundary itself
            local |= {int(k - (sp - 5)) for k in ks}
            rim += int(np.any(ks <= sp + 4)) + int(np.any(ks >= ep - 3))
        assert {63, 64, 65, 127, 128, 129} <= local
        assert rim >= 24
        fwd, bwd = _break_distances(res, col)
        assert fwd == {1, 2, 3, 4, 5} and bwd == {1, 2, 3, 4, 5}, (fwd, bwd)
        assert set(np.unique(np.diff(col)[np.diff(col) > 0])) >= {1, 9, 10, 11}
    sc["conditions"].update(break_local_positions=[63, 64, 65, 127, 128, 129], break_distance_from_a_taken_corner="1..5 on both sides",
                            sectors_with_rim_breaks=24)
    return sc


def scene_cap():
    """two spiky rings with gaps of 10 between columns (no occlusion marks, no breaks): ring 0 has a spike every 7th point — more
    than 40 independent corners per sector, the cap falls in the first batch of 64 candidates; ring 1 has plateaus of three
    raised points whose candidates block each other, so that 64 candidates yield far fewer than 40 takes"""
    rs = np.random.RandomState(41)
    scans = []
    for rep in range(2):
        m0, m1 = 4000, 5600
        r0 = 20.0 + rs.uniform(-0.01, 0.01, m0)
        r0[::7] += 0.9
        r1 = 20.0 + rs.uniform(-0.01, 0.01, m1)
        h = rs.uniform(0.6, 3.0, m1 // 14 + 1)
        for q in range(3):
            r1[q::14] += h[:len(r1[q::14])]
        scans.append(assemble([r0.astype(np.float32), r1.astype(np.float32)], [10 * np.arange(m0), 10 * np.arange(m1)]))
    sc = finish("cap", scans, tie_free=True, seed=41)
    for res in sc["ref"]:
        full = [s for s in res["sectors"] if len(s["taken"]) == CORNER_CAP]
        # ranks are positions in the descending candidate list as the sequential walk meets the sector; the pipelined form
        # compacts its list before the predecessor's five hand-over marks arrive, so a batch boundary may sit up to 5 later
        first = [s for s in full if s["broke"] and max(s["ranks"]) < 64 - 5]
        later = [s for s in full if s["broke"] and s["ranks"][-1] >= 64 + 5]
        assert first and later, [(s["ring"], s["sec"], len(s["taken"]), s["ranks"][-1] if s["ranks"] else None) for s in res["sectors"]]
        assert res["occl"][5:].sum() == 0
    res = sc["ref"][0]
    sc["conditions"].update(sectors_at_cap=sum(len(s["taken"]) == CORNER_CAP for s in res["sectors"]),
                            rank_of_40th_take=[s["ranks"][-1] for s in res["sectors"] if len(s["taken"]) == CORNER_CAP],
                            sectors_with_a_41st_candidate=sum(s["broke"] for s in res["sectors"]))
    return sc


def scene_equalities():
    """edgeThreshold = 1.0, surfThreshold = 0.0625: curvature equal to either threshold (diffRange +-1, +-0.25), range steps
    of the float nearest 0.3 (above 0.3 as a double: marks) and of the float below (marks nothing), parallel-beam
    differences equal to 0.1 * range in double (range 5 and 10: no mark; one float above: mark)"""
    edge, surf = 1.0, 0.0625
    m = 240
    # ring 0 (gaps of 10 between columns as well): bumps of +-0.25 on a flat range: diffRange = -+1 at the bump, +-0.25 at its four neighbours
    r0 = np.full(m, 8.0, np.float32)
    ups, downs = [30, 75, 120, 170], [50, 95, 145, 200]
    r0[ups] += np.float32(0.25)
    r0[downs] -= np.float32(0.25)
    r0[[60, 110]] += np.float32(0.5)                  # controls: curvature 4 (a corner)
    # ring 1: steps of f = float32(0.3) and g = the float below, down and up
    f = np.float32(0.3)
    g = np.nextafter(f, np.float32(0))
    assert float(f) > 0.3 > float(g)
    seg = lambda v: [v] * 20
    r1 = np.array(seg(2 * f) + seg(f) + seg(2 * f) + seg(2 * g) + seg(g) + seg(2 * g) + seg(2 * g), np.float32)
    assert np.float32(r1[19] - r1[20]) == f and np.float32(r1[40] - r1[39]) == f
    assert np.float32(r1[79] - r1[80]) == g and np.float32(r1[100] - r1[99]) == g
    # ring 2: parallel beam; gaps of 10 between columns so that no occlusion mark interferes
    r2 = np.full(m, 7.0, np.float32)
    pb = {}
    for q, (rng, d) in enumerate(((5.0, 0.5), (10.0, 1.0))):
        assert 0.1 * float(np.float32(rng)) == d                                   # the double product is exactly the difference
        for w, (lo, hi) in enumerate(((rng + d, rng + d), (rng - d, rng + d), (np.nextafter(np.float32(rng + d), np.float32(99)),) * 2)):
            i = 20 + 60 * q + 20 * w
            r2[i - 4:i + 5] = np.float32(rng)
            r2[i - 1], r2[i + 1] = np.float32(lo), np.float32(hi)
            pb[i] = w == 2
    info = assemble([r0, r1, r2], [10 * np.arange(m), None, 10 * np.arange(m)])
    sc = finish("equalities", [info, info], edge=edge, surf=surf)
    b1, b2 = m, m + len(r1)
    for res in sc["ref"]:
        c, lab = res["curv"], res["label"]
        at_edge, at_surf = np.flatnonzero(c == np.float32(edge)), np.flatnonzero(c == np.float32(surf))
        assert set(ups + downs) <= set(at_edge) and len(at_surf) >= 4 * len(ups + downs) - 4
        assert np.all(lab[at_edge] != 1) and np.all(lab[at_surf] != -1)          # equality takes neither walk
        assert lab[60] == 1 and lab[110] == 1
        o = res["occl"]
        assert o[b1 + 18] == 1 and o[b1 + 19] == 1 and o[b1 + 17] == 0            # step down by f at i = 19: marks i-1, i
        assert o[b1 + 40] == 1 and o[b1 + 41] == 1 and o[b1 + 42] == 0            # step up by f at i = 39: marks i+1, i+2
        assert not o[b1 + 70:b1 + 110].any()                                     # steps of g: nothing
        for i, marked in pb.items():
            assert o[b2 + i] == int(marked), (i, marked)
    sc["conditions"].update(points_at_edge_threshold=int((sc["ref"][0]["curv"] == np.float32(edge)).sum()),
                            points_at_surf_threshold=int((sc["ref"][0]["curv"] == np.float32(surf)).sum()),
                            occlusion_steps=[float(f), float(g)], parallel_beam_equalities=[(5.0, 0.5), (10.0, 1.0)])
    return sc


def _small(name, size_lists, seed, expect_label0_after=None):
    rs = np.random.RandomState(seed)
    scans = []
    for sizes in size_lists:
        rr = [rough_ring(rs, m, noise=0.05, spike_every=0.15) for m in sizes]
        first = next((r for r in rr if len(r)), None)
        if first is not None:                          # a smooth start: no corner at point 5 whose backward marks would reach ind 0
            first[:9] = first[0] + np.float32(1e-3) * np.arange(len(first[:9]), dtype=np.float32)
        scans.append(assemble(rr, n_scan=4))
    sc = finish(name, scans, tie_free=True, seed=seed)
    # the stale entry {0, ind 0}: ind 0 is labelled in the first scan whose slot 4 opens a sector (4 = sp < ep) — unless an
    # earlier walk has already marked picked[0]: point 5, taken or labelled with five free steps backwards, reaches ind 0
    fired = [q for q, res in enumerate(sc["ref"]) if res["n"] > 0 and res["label"][0] == -1]
    assert (fired[0] if fired else None) == expect_label0_after, (name, fired)
    if expect_label0_after is None:
        assert any(res["n"] > 0 and res["picked"][0] == 1 for res in sc["ref"]), name
    sc["conditions"].update(rings=[list(s) for s in size_lists], stale_entry_fires_in_scan=expect_label0_after)
    return sc


def scenes_small_geometry():
    out = [
        _small("small_ring0_empty", [(0, 30, 71, 22), (0, 71, 23, 16)], 51, expect_label0_after=0),
        _small("small_ring0_17_then_30", [(17, 71, 23, 13), (30, 71, 22, 16)], 52, expect_label0_after=1),
        _small("small_ring0_21_then_22", [(21, 12, 11, 71), (22, 13, 30, 71)], 53, expect_label0_after=None),
        _small("small_short_previous_ring", [(71, 8, 71, 5), (30, 10, 71, 3)], 54, expect_label0_after=0),
        _small("small_mixture", [(11, 12, 13, 16), (17, 21, 22, 23), (23, 30, 71, 0)], 55, expect_label0_after=2),
        _small("small_whole_scans", [(0,), (1,), (10,), (11,), (12,), (16,), (17,), (71,)], 56, expect_label0_after=7),
    ]
    seen = {m for sc in out for s in sc["scans"] for m in s["ring_sizes"]}
    assert {0, 11, 12, 13, 16, 17, 21, 22, 23, 30, 71} <= seen
    widths = {ep - sp for sc in out for s in sc["scans"] for _, _, sp, ep in sectors_of(s)}
    assert 1 in widths                                                            # a sector with ep = sp + 1
    return out


def _ring_size_for_longest_sector(want):
    for m in range(6 * (want - 20), 6 * (want + 2)):
        if longest_sector(dict(start_ring_index=[4], end_ring_index=[m - 6])) == want:
            return m
    raise AssertionError(want)


def _boundary(want, seed):
    rs = np.random.RandomState(seed)
    m = _ring_size_for_longest_sector(want)
    mk = lambda: assemble([rough_ring(rs, m, base=20.0, noise=0.3, spike_every=0.02)])
    sc = finish(f"capacity_{want}", [mk(), mk()], tie_free=True, seed=seed)
    assert all(longest_sector(s) == want for s in sc["scans"]) and sc["big"] == (want > FEAT_SEG_CAP)
    sc["conditions"].update(ring=m, longest_sector=want, kernel="big" if sc["big"] else "LDS")
    return sc


def scenes_capacity():
    out = [_boundary(FEAT_SEG_CAP - 1, 61), _boundary(FEAT_SEG_CAP, 62), _boundary(FEAT_SEG_CAP + 1, 63)]
    # the big kernel proper: one ring of 50 000 quantised points, ties and breaks
    rs = np.random.RandomState(64)
    scans = []
    for rep in range(2):
        r, gaps = _quantised_ring(rs, 50000, gaps=(1, 1, 1, 10, 11), spike_p=0.05)
        r[100:400] = np.float32(8.0)
        scans.append(assemble([r], [_cols(gaps)]))
    sc = finish("big_ties_and_breaks", scans, edge=1.0, surf=1.0)
    assert sc["big"] and not sc["tie_free"] and all(len(r["corner_idx"]) > 100 for r in sc["ref"])
    sc["conditions"].update(ring=50000, longest_sector=longest_sector(scans[0]), tied_eligible_points=len(tied_points(scans[0], 1.0, 1.0)))
    out.append(sc)
    # an oversize ring next to ordinary ones
    rs = np.random.RandomState(65)
    m = _ring_size_for_longest_sector(FEAT_SEG_CAP + 40)
    mk = lambda: assemble([rough_ring(rs, 300), rough_ring(rs, m, base=20.0, noise=0.3, spike_every=0.02), rough_ring(rs, 500)])
    sc = finish("big_mixed", [mk(), mk()], tie_free=True, seed=65)
    assert sc["big"]
    sc["conditions"].update(rings=[300, m, 500], longest_sector=longest_sector(sc["scans"][0]))
    out.append(sc)
    return out


@functools.lru_cache(maxsize=None)
def all_scenes():
    scenes = [scene_tie_free(), scene_ties(), scene_column_breaks(), scene_cap(), scene_equalities()]
    scenes += scenes_small_geometry() + scenes_capacity()
    return {sc["name"]: sc for sc in scenes}


SCENE_NAMES = ("tie_free", "ties", "column_breaks", "cap", "equalities", "small_ring0_empty", "small_ring0_17_then_30",
               "small_ring0_21_then_22", "small_short_previous_ring", "small_mixture", "small_whole_scans",
               f"capacity_{FEAT_SEG_CAP - 1}", f"capacity_{FEAT_SEG_CAP}", f"capacity_{FEAT_SEG_CAP + 1}", "big_ties_and_breaks", "big_mixed")
TIED_SCENES = ("ties", "equalities", "big_ties_and_breaks")         # curvature ties among eligible points: only the reference can judge


# ----------------------------------------------------------------------------- running a scene through a library
OUTPUTS = ("curv", "occl", "label", "picked", "corner_idx")


def run_scene(pkg, lib, scene, n_scan, **handle_kw):
    """every scan of the scene through one handle of `lib`; per scan the five outputs in the reference's layout"""
    A = pkg._abi
    n_max = max(s["n"] for s in scene["scans"])
    P = dict(N_SCAN=n_scan, Horizon_SCAN=max(1024, n_max + 64), max_raw_points=n_max + 64, max_map_points=4096,
             edgeThreshold=scene["edge"], surfThreshold=scene["surf"])
    P.update(handle_kw)
    h = pkg.LidarHotpath(lib, **P)
    rows = []
    try:
        for s in scene["scans"]:
            h.extract_features(pad_rings(s, n_scan))
            n = s["n"]
            rows.append(dict(n=n, curv=h.debug_get(A.DBG_CURVATURE, np.float32)[:n], occl=h.debug_get(A.DBG_PICKED_OCCL, np.int32)[:n],
                             label=h.debug_get(A.DBG_LABEL, np.int32)[:n], picked=h.debug_get(A.DBG_PICKED_FINAL, np.int32)[:n],
                             corner_idx=h.debug_get(A.DBG_CORNER_INDEX, np.int32)))
    finally:
        h.close()
    return rows


def assert_same(got, want, what):
    """the five outputs, exact: the per-point arrays over [5, n-5) — the window a scan rewrites; outside it the reference keeps
    whatever earlier scans left, which no walk reads — and the corner indices whole"""
    n = want["n"]
    assert got["n"] == n
    w = slice(5, max(n - 5, 5))
    for key in OUTPUTS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if key == "corner_idx":
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: corner indices")
        elif key == "curv":
            np.testing.assert_array_equal(a[w].view(np.uint32), b[w].view(np.uint32), err_msg=f"{what}: curvature bits")
        else:
            np.testing.assert_array_equal(a[w], b[w], err_msg=f"{what}: {key}")
