"""The full tracker frame path (push with CLAHE, LK, circles, GFTT, frame end) for 8 image streams at 1280 x 720 and 150 points, in
three forms that alternate in one process after warm-up:

  (a) one lvi_tracker, the 8 streams one after another, a stretch of frames each (each frame: its launch chain and its two waits);
  (b) 8 lvi_tracker handles on 8 streams, the phases interleaved across the handles (every handle's LK is enqueued before the
      first result is read, every handle's GFTT before the first frame end), so that the device has all 8 in flight;
  (c) one 8-slot lvi_tbatch (include/lvi_tbatch.h): one launch chain and two waits for all 8.

Every figure is a host clock around work that ends in a synchronise (the frame end's read), through the Python binding, whose
per-call cost is part of every form.  Prints one JSON line: us per stream-frame of every repetition, median and spread, and the
kernel launches per frame of (a) and (c).

    python tools/diag/tbatch_time.py [--reps 9] [--frames 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import __graft_entry__ as graft  # noqa: E402

W, H, NPTS, STREAMS, RADIUS = 1280, 720, 150, 8, 20
CAM = dict(xi=1.9926618269451453, k1=-0.0399258932468764, k2=0.15160828121223818, p1=0.00017756967825777937, p2=-0.0011531239076798612,
           gamma1=669.8940458885896, gamma2=669.1450614220616, u0=0.5 * W, v0=0.5 * H)


def inside(xy, st):
    k = xy[st == 1]
    return k[(k[:, 0] >= 1) & (k[:, 0] < W - 1) & (k[:, 1] >= 1) & (k[:, 1] < H - 1)]


def frame_single(t, img, pts):
    t.push_image(img); t.set_points(pts); t.run_lk()
    xy, st, _ = t.get_lk()
    kept = inside(xy, st)
    t.set_mask_circles(kept, RADIUS)
    t.run_gftt_async(max(NPTS - len(kept), 1))
    t.finish_frame(kept, CAM)


def frame_interleaved(ts, imgs, pts):
    for t, img, p in zip(ts, imgs, pts):
        t.push_image(img); t.set_points(p); t.run_lk()
    kept = []
    for t in ts:
        xy, st, _ = t.get_lk()
        kept.append(inside(xy, st))
        t.set_mask_circles(kept[-1], RADIUS)
        t.run_gftt_async(max(NPTS - len(kept[-1]), 1))
    for t, k in zip(ts, kept):
        t.finish_frame(k, CAM)


def frame_batch(b, imgs, pts):
    b.push_images(imgs); b.set_points(pts); b.run_lk()
    kept = []
    for s in range(b.slots):
        xy, st, _ = b.get_lk(s)
        kept.append(inside(xy, st))
    b.set_mask_circles(kept, RADIUS)
    b.run_gftt_async([max(NPTS - len(k), 1) for k in kept])
    b.finish_frame(kept, [CAM] * b.slots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    pkg = graft.import_package(); hip = pkg.load_hip(); S = pkg.synth
    kw = dict(max_width=W, max_height=H, max_features=1024)
    # per stream: a texture of its own, four small-motion warps of it, and the 150 corners of its first frame
    seq, pts = [], []
    finder = pkg.TrackerHotpath(hip, **kw)
    finder.set_equalize(True)
    for s in range(STREAMS):
        img0 = S.make_texture(W, H, 4242 + s)
        seq.append([img0] + [S.warp_homography(img0, S.small_motion_homography(W, H, 100 + 7 * s + i)) for i in range(3)])
        pts.append(finder.good_features(finder.clahe(img0), NPTS, 0.01, float(RADIUS)))
    finder.close()
    one = pkg.TrackerHotpath(hip, **kw)
    many = [pkg.TrackerHotpath(hip, **kw) for _ in range(STREAMS)]
    batch = pkg.TrackerBatch(hip, STREAMS, **kw)
    for t in [one] + many:
        t.set_equalize(True)
    batch.set_equalize(True)

    def run_a(n):
        # one handle, stream after stream: it stays with a stream for n frames, so all but the first LK of a stretch track the
        # stream's own motion, as in (b) and (c)
        for s in range(STREAMS):
            for k in range(n):
                frame_single(one, seq[s][k % 4], pts[s])

    def run_b(n):
        for k in range(n):
            frame_interleaved(many, [seq[s][k % 4] for s in range(STREAMS)], pts)

    def run_c(n):
        for k in range(n):
            frame_batch(batch, [seq[s][k % 4] for s in range(STREAMS)], pts)

    forms = dict(a=run_a, b=run_b, c=run_c)
    for f in forms.values():                    # warm-up: every handle has its pair, every kernel is loaded
        f(4)
    us = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, f in forms.items():
            one.sync(); batch.sync()
            for t in many:
                t.sync()
            t0 = time.perf_counter()
            f(args.frames)                      # (every frame ends in the frame end's wait)
            us[name].append(1e6 * (time.perf_counter() - t0) / (args.frames * STREAMS))
    # launches per frame (a separate pass: the profiler's events are not part of the timed runs)
    launches = {}
    for name, h, f in (("a", one, run_a), ("c", batch, run_c)):
        f(1)
        h.prof_enable(True); h.prof_reset()
        f(1)
        launches[name] = {r["name"]: r["launches"] for r in h.prof_read()}
        h.prof_enable(False)
    out = dict(tool="tbatch_time", size=[W, H], points=NPTS, streams=STREAMS, reps=args.reps, frames_per_rep=args.frames)
    for name, v in us.items():
        v = np.array(v)
        out[name] = dict(us_per_stream_frame=[round(float(x), 1) for x in v], median=round(float(np.median(v)), 1), min=round(float(v.min()), 1),
                         max=round(float(v.max()), 1))
    out["launches_per_8_stream_frames"] = {k: dict(total=int(sum(v.values())), by_kernel=v) for k, v in launches.items()}
    out["c_faster_than_a_beyond_spread"] = bool(out["c"]["max"] < out["a"]["min"])
    out["c_vs_b"] = round(out["c"]["median"] / out["b"]["median"], 3)
    print(json.dumps(out))
    one.close(); batch.close()
    for t in many:
        t.close()


if __name__ == "__main__":
    main()
