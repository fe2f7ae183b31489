"""The bars of the tracker references, applied to any library behind the C-ABI: the CPU tier holds the oracle to them
(tests/test_tracker_ref.py), the GPU tier the HIP library (tests/test_gpu_tracker_ref.py).  Every function returns the measured
figures so that the caller can print them; every reference is computed once per process and shared."""
import numpy as np

import tracker_ref as R
import tracker_scenes as SC

STEP_MARGIN = 1e-5          # a status is compared where every decision is at least this far (relative) from its boundary
RUN_MARGIN = 1e-3
UNDECIDABLE_CAP = 0.05      # of a run / chain scene's points
UNSETTLED_CAP = 0.10        # of a run scene's points
SWEEP_UNDECIDED_CAP = 0.02

# The oracle's greatest distance (px) from lk_track_ref over the decidable settled points of each scene (chains: decidable points),
# measured with this reference on 2026-10-19 (x86-64, the oracle's integer-sum form).  test_tracker_ref.py checks that the oracle
# still stays within them; the device's bar is max(4 E_orc, 4 ulp32).
E_ORC = {
    "run-win21": 1.8310546875e-04, "run-win7": 2.2125244140625e-04, "run-win15-eps0": 3.814697265625e-06,
    "run-win5-l0": 4.76837158203125e-07, "run-win5-7lvl": 1.3885498046875e-03, "run-24x18-win7": 3.4332275390625e-05,
    "run-equalize": 0.0, "reload-blobs": 1.331329345703125e-03,
    "chain-win3-8lvl-it1": 3.0517578125e-05, "chain-win3-8lvl-it2": 2.777099609375e-03,
    "chain-win21-it1": 9.918212890625e-05, "chain-win21-it2": 7.62939453125e-05,
}
# the oracle's worst figures on the other bars, same date: the step (as a share of its bar; 0.376 of 2 ulp = 0.75 ulp), err at zero
# iterations (ulp), the min-eigenvalue map (units u; the worst pixel lies in the 320 x 240 noise image of 250..255)
ORC_STEP_RATIO, ORC_ERR_ULP, ORC_MINEIG_RATIO = 0.3761, 0.4978, 0.5948

_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def scenes(pkg, kind):
    S = pkg.synth
    return cached(("scenes", kind), lambda: {"step": SC.step_scenes, "run": SC.run_scenes, "chain": SC.chain_scenes}[kind](S))


def scene(pkg, kind, name):
    return {s["name"]: s for s in scenes(pkg, kind)}[name]


def reload_scene():
    return cached(("scenes", "reload"), SC.reload_scene)


def tracker(pkg, lib, w, h, **kw):
    return pkg.TrackerHotpath(lib, max_width=max(w, 64), max_height=max(h, 64), max_features=kw.pop("max_features", 1024), **kw)


# ----------------------------------------------------------------------------- item 1: the exact step
def step_refs(scene):
    return cached(("stepref", scene["name"]),
                  lambda: [R.lk_step_exact(scene["I"], scene["J"], q, scene["win"], scene["min_eig"]) for q in scene["pts64"]])


def check_step(pkg, lib, scene):
    win, thr = scene["win"], scene["min_eig"]
    h, w = scene["I"].shape
    refs = step_refs(scene)
    pts = (scene["pts64"].astype(np.float64) / 64.0).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) * 64.0, scene["pts64"])             # the starts are float32 numbers exactly
    kw = dict(lk_win=win, lk_max_level=0, lk_eps=0.0, lk_min_eig_threshold=thr)
    t0 = tracker(pkg, lib, w, h, lk_max_iters=0, **kw)
    x0, s0, e0 = t0.lk_track(scene["I"], scene["J"], pts)
    t0.close()
    t1 = tracker(pkg, lib, w, h, lk_max_iters=1, **kw)
    x1, s1, e1 = t1.lk_track(scene["I"], scene["J"], pts)
    t1.close()
    st0 = np.array([r["status"] for r in refs])
    st1 = np.array([r.get("status1", r["status"]) for r in refs])
    m0 = np.array([r["margin"] for r in refs])
    m1 = np.array([r.get("margin1", r["margin"]) for r in refs])
    rep = dict(name=scene["name"], n=len(pts), tracked=int(st1.sum()), undecided=int((m1 < STEP_MARGIN).sum()))
    # ---- zero iterations: the position is the input, err is the start's residual
    np.testing.assert_array_equal(x0.view(np.uint32), pts.view(np.uint32), err_msg=scene["name"])
    d0 = m0 >= STEP_MARGIN
    np.testing.assert_array_equal(s0[d0], st0[d0], err_msg=f"{scene['name']}: status at max_iters = 0")
    k0 = d0 & (st0 == 1)
    err_ref = np.array([r["err"] for r in refs])
    u = R.ulp32(err_ref)
    rep["err_ulp"] = float((np.abs(e0[k0].astype(np.float64) - err_ref[k0]) / u[k0]).max()) if k0.any() else 0.0
    assert rep["err_ulp"] <= 1.0, rep
    # ---- one iteration
    d1 = m1 >= STEP_MARGIN
    np.testing.assert_array_equal(s1[d1], st1[d1], err_msg=f"{scene['name']}: status at max_iters = 1")
    k1 = d1 & (st1 == 1)
    want = pts.astype(np.float64) + np.array([r["delta"] for r in refs])
    s = np.array([[r["sx"], r["sy"]] for r in refs])
    t_round = 2.0 * R.ulp32(np.abs(pts.astype(np.float64)) + win)
    t_cond = 16.0 * 2.0 ** -24 * s
    dev = np.abs(x1.astype(np.float64) - want)
    rep["ratio"] = float((dev[k1] / (t_round + t_cond)[k1]).max()) if k1.any() else 0.0
    rep["ratio_round_only"] = float((dev[k1] / t_round[k1]).max()) if k1.any() else 0.0          # > 1 where the conditioning term is needed
    rep["cond_max"] = float(max((r["sums"][0] * r["sums"][2]) / max(r["sums"][0] * r["sums"][2] - r["sums"][1] ** 2, 1)
                                for r, k in zip(refs, k1) if k)) if k1.any() else 0.0
    assert rep["ratio"] <= 1.0, rep
    if scene["sweep"]:
        assert rep["undecided"] <= SWEEP_UNDECIDED_CAP * len(pts), rep
        gate = np.array([r["gate"] for r in refs]) & ~np.array([r["exit_prev"] for r in refs])
        inside = ~np.array([r["exit_prev"] for r in refs])
        rep["above"], rep["below"] = int((d1 & gate).sum()), int((d1 & inside & ~gate).sum())
        assert rep["above"] >= 10 and rep["below"] >= 10, rep
    else:
        assert rep["undecided"] == 0, rep
    return rep


# ----------------------------------------------------------------------------- items 2 and 3: runs, chains, the reload scene
def lk_params(scene):
    return dict(lk_win=scene["win"], lk_max_level=scene["max_level"], lk_max_iters=scene["max_iters"], lk_eps=scene["eps"],
                lk_min_eig_threshold=scene["min_eig"])


def track(pkg, lib, scene):
    """(xy, status, err, frames the reference must use): an equalised scene goes through push_image / set_points / run_lk"""
    h, w = scene["I"].shape
    t = tracker(pkg, lib, w, h, **lk_params(scene))
    if scene["equalize"]:
        t.set_equalize(True, 3.0, (8, 8))
        t.push_image(scene["I"]); t.push_image(scene["J"])
        t.set_points(scene["pts"]); t.run_lk()
        out = t.get_lk()
        frames = (t.clahe(scene["I"], 3.0, (8, 8)), t.clahe(scene["J"], 3.0, (8, 8)))
    else:
        out = t.lk_track(scene["I"], scene["J"], scene["pts"])
        frames = (scene["I"], scene["J"])
    t.close()
    return out + (frames,)


def run_ref(scene, frames):
    def make():
        pI = R.build_pyramid(frames[0], scene["win"], scene["max_level"])
        pJ = R.build_pyramid(frames[1], scene["win"], scene["max_level"])
        return R.lk_track_ref(pI, pJ, scene["pts"], scene["win"], scene["max_level"], scene["max_iters"], scene["eps"], scene["min_eig"])
    return cached(("runref", scene["name"], frames[0].tobytes()[:64], int(frames[0].sum())), make)


def check_run(pkg, lib, scene, e_orc=None):
    """e_orc None: measure only (the oracle's own pass); otherwise assert the bar max(4 e_orc, 4 ulp32)"""
    xy, st, err, frames = track(pkg, lib, scene)
    ref = run_ref(scene, frames)
    n = len(scene["pts"])
    decid = ref["margin"] >= RUN_MARGIN
    settled = ref["settled"] if scene["kind"] == "run" else np.ones(n, bool)
    rep = dict(name=scene["name"], n=n, undecidable=int((~decid).sum()), unsettled=int((~settled).sum()), tracked=int(ref["status"].sum()),
               travel_gt8=int((ref["travel"] > 8).sum()))
    assert rep["undecidable"] <= UNDECIDABLE_CAP * n, rep
    if scene["kind"] == "run":
        assert rep["unsettled"] <= UNSETTLED_CAP * n, rep
    k = decid & settled
    np.testing.assert_array_equal(st[k], ref["status"][k], err_msg=scene["name"])
    k &= ref["status"] == 1
    assert k.sum() >= 0.5 * n, rep                                       # the asserted class is most of the scene
    d = np.abs(xy[k].astype(np.float64) - ref["xy"][k].astype(np.float64))
    rep["E"] = float(d.max())
    ulp = R.ulp32(np.abs(ref["xy"][k].astype(np.float64)))
    rep["E_ulp"] = float((d / ulp).max())
    u = ~decid | ~settled
    both = u & (st == 1) & (ref["status"] == 1)
    rep["E_unasserted"] = float(np.abs(xy[both].astype(np.float64) - ref["xy"][both]).max()) if both.any() else 0.0
    rep["flips_unasserted"] = int((st[u] != ref["status"][u]).sum())
    if e_orc is not None:
        bar = np.maximum(4.0 * e_orc, 4.0 * ulp)
        rep["ratio"] = float((d / bar).max())
        assert rep["ratio"] <= 1.0, rep
    return rep


# ----------------------------------------------------------------------------- items 5 and 6: the map and the selection
def mineig_refs(img):
    return cached(("mineig", img.shape, img.tobytes()), lambda: R.mineig_ref(img))


def check_mineig(t, pkg, img, name):
    """t: a TrackerHotpath with max_features = 4096.  Returns the device map (float32, h x w) and the worst |dev - ref| / u"""
    A = pkg._abi
    h, w = img.shape
    t.good_features(img, 1, 0.5, 1.0)
    eig = t.debug_get(A.TDBG_MINEIG, np.float32).reshape(h, w)
    ref, apc = mineig_refs(img)
    u = R.mineig_unit(apc)
    z = apc == 0
    assert (eig[z] == 0).all(), name
    ratio = float((np.abs(eig.astype(np.float64) - ref)[~z] / u[~z]).max()) if (~z).any() else 0.0
    assert ratio <= 2.0, (name, ratio)
    return eig, ratio


def check_selection(t, pkg, img, mask, quality, min_dist, quota, name):
    A = pkg._abi
    h, w = img.shape
    got = t.good_features(img, quota, quality, min_dist, mask)
    eig = t.debug_get(A.TDBG_MINEIG, np.float32).reshape(h, w)
    ncand = int(t.debug_get(A.TDBG_GFTT_NCAND, np.int32)[0])
    want, nref = R.gftt_select(eig, mask, quality, min_dist, quota)
    assert ncand == nref, (name, ncand, nref)
    np.testing.assert_array_equal(got, want, err_msg=str(name))
    return len(got), ncand
