"""rejectWithF's RANSAC for the 8 cameras of a rig (include/lvi_fmatb.h), two forms that alternate in one process
after warm-up, at n = 150 and outlier fractions 0, 0.3 and 0.5 of tests/fmat_ref.two_view scenes (0.3 px noise, F_THRESHOLD 1,
a scene of its own per slot):

  (a) 8 lvi_fmat handles called in turn (each call: its upload, two launches, download and wait) — what a rig with
      use_device_fundamental does;
  (b) one lvi_fmatb_find over an 8-slot handle (8 uploads and 9 launches on one stream, one download, one wait).

Both are timed by a host clock around library calls that end in a wait, through ctypes with the argument tables built
beforehand, so the binding costs the same handful of foreign calls in either form.  Reported per outlier fraction: wall median
and p99 over --calls calls, and the host's sample-stream time summed over the 8 slots (lvi_fmat_info.stream_us), which neither
form can hide behind the device for slot 0 and which (b) overlaps with the device from slot 1 on.

Then the rig: us per stream-frame of FeatureTrackerRig::readImages (1280 x 720, 150 points, 8 streams, every frame published)
without a hook, with the per-camera device hook and with the batched hook, alternating.  Prints one JSON line.

    timeout -k 10 300 python tools/diag/fmatb_time.py [--calls 200] [--reps 9] [--frames 20] [--no-rig]

Kernel times come from separate profiler runs of this script, one per outlier fraction:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d fmatb_prof -o o05 -- python tools/diag/fmatb_time.py --no-rig --calls 50 --outliers 0.5
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

SLOTS, N = 8, 150
W, H, NPTS, RADIUS = 1280, 720, 150, 20
CAM = dict(xi=1.9926618269451453, k1=-0.0399258932468764, k2=0.15160828121223818, p1=0.00017756967825777937, p2=-0.0011531239076798612,
           gamma1=669.8940458885896, gamma2=669.1450614220616, u0=0.5 * W, v0=0.5 * H)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 2), p99=round(float(np.percentile(v, 99)), 2), min=round(float(v.min()), 2))


def ransac_forms(pkg, hip, calls, outliers):
    import fmat_ref as R
    A = pkg._abi
    FmatInfo = pkg.fmat.FmatInfo
    singles = [pkg.FundamentalRansac(hip, max_points=N, max_iters=1000) for _ in range(SLOTS)]
    batch = pkg.FundamentalRansacBatch(hip, SLOTS, max_points=N, max_iters=1000)
    dll = hip.dll
    out = {}
    for o in outliers:
        pairs = [R.two_view(N, o, 0.3, seed=7 + N + 31 * s)[:2] for s in range(SLOTS)]
        st_a = [np.zeros(N, np.uint8) for _ in range(SLOTS)]
        st_b = [np.zeros(N, np.uint8) for _ in range(SLOTS)]
        info_a = (FmatInfo * SLOTS)()
        info_b = (FmatInfo * SLOTS)()
        tab = lambda arrs: (C.c_void_p * SLOTS)(*[A._ptr(x) for x in arrs])   # noqa: E731
        p1t, p2t, stt = tab([p[0] for p in pairs]), tab([p[1] for p in pairs]), tab(st_b)
        nt, tht = (C.c_int32 * SLOTS)(*[N] * SLOTS), (C.c_double * SLOTS)(*[1.0] * SLOTS)
        args_a = [(singles[s]._h, A._ptr(pairs[s][0]), A._ptr(pairs[s][1]), N, 1.0, 0.99, A._ptr(st_a[s]), C.byref(info_a[s])) for s in range(SLOTS)]

        def run_a():
            for a in args_a:
                if dll.lvi_fmat_find(*a) != 0:
                    raise RuntimeError("lvi_fmat_find failed")

        def run_b():
            if dll.lvi_fmatb_find(batch._h, p1t, p2t, nt, tht, 0.99, stt, info_b) != 0:
                raise RuntimeError("lvi_fmatb_find failed")
        for _ in range(10):
            run_a(); run_b()
        for s in range(SLOTS):                     # the two forms return the same bits, at the size that is timed
            assert (st_a[s] == st_b[s]).all() and info_a[s].iters == info_b[s].iters and bytes(info_a[s].F) == bytes(info_b[s].F)
        wall = dict(a=[], b=[])
        stream = dict(a=[], b=[])
        for _ in range(calls):
            for name, f, info in (("a", run_a, info_a), ("b", run_b, info_b)):
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1e6)
                stream[name].append(sum(info[s].stream_us for s in range(SLOTS)))
        out[f"n{N}_o{o}"] = dict(a_wall_us=_stats(wall["a"]), b_wall_us=_stats(wall["b"]), a_stream_us_sum=_stats(stream["a"]), b_stream_us_sum=_stats(stream["b"]),
                                 walk_iters=[int(info_b[s].iters) for s in range(SLOTS)], b_over_a=round(float(np.median(wall["b"]) / np.median(wall["a"])), 3),
                                 b_faster_beyond_spread=bool(np.percentile(wall["b"], 99) < np.min(wall["a"])))
    out["counters"] = batch.counters()
    for h in singles + [batch]:
        h.close()
    return out


def rig_forms(pkg, hip, reps, frames):
    S = pkg.synth
    hl = pkg.load_host()
    tp = pkg.default_tracker_params(hip, max_width=W, max_height=H, max_features=1024, max_cnt=NPTS, min_dist=float(RADIUS))
    seq = []
    for s in range(SLOTS):
        img0 = S.make_texture(W, H, 4242 + s)
        seq.append([img0] + [S.warp_homography(img0, S.small_motion_homography(W, H, 100 + 7 * s + i)) for i in range(3)])
    rigs = {}
    for form in ("no_hook", "per_camera", "batched"):
        rigs[form] = pkg.host_api.TrackerRig(hl, tp, SLOTS, H, W, equalize=True, cams=[CAM] * SLOTS, batched=True)
        if form == "per_camera":
            rigs[form].use_device_fundamental()
        elif form == "batched":
            rigs[form].use_batched_fundamental()
    clock = dict.fromkeys(rigs, 0)

    def run(form, n):
        for _ in range(n):
            k = clock[form]
            rigs[form].read_images([seq[s][k % 4] for s in range(SLOTS)], [100.0 + k / 30.0] * SLOTS, [True] * SLOTS)
            rigs[form].update_ids()
            clock[form] = k + 1
    for form in rigs:
        run(form, 8)
    us = {form: [] for form in rigs}
    for _ in range(reps):
        for form in rigs:
            t0 = time.perf_counter()
            run(form, frames)                      # (every frame ends in the frame end's wait)
            us[form].append(1e6 * (time.perf_counter() - t0) / (frames * SLOTS))
    out = dict(size=[W, H], points=NPTS, streams=SLOTS, reps=reps, frames_per_rep=frames)
    for form, v in us.items():
        v = np.array(v)
        out[form] = dict(us_per_stream_frame=[round(float(x), 1) for x in v], median=round(float(np.median(v)), 1), min=round(float(v.min()), 1),
                         max=round(float(v.max()), 1), features_last=[len(rigs[form].camera(s)["ids"]) for s in range(SLOTS)], stats=rigs[form].fundamental_stats())
    out["batched_faster_than_per_camera_beyond_spread"] = bool(out["batched"]["max"] < out["per_camera"]["min"])
    for r in rigs.values():
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--no-rig", action="store_true")
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.0, 0.3, 0.5], help="one fraction per profiler run gives per-fraction kernel times")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except Exception:
        pass
    pkg = graft.import_package()
    hip = pkg.load_hip()
    out = dict(tool="fmatb_time", slots=SLOTS, n=N, calls=a.calls, ransac=ransac_forms(pkg, hip, a.calls, a.outliers))
    if not a.no_rig:
        out["rig"] = rig_forms(pkg, hip, a.reps, a.frames)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
