"""Deterministic scenes for the tracker references (tests/tracker_ref.py): every image comes from the package's `synth`
module and numpy seeds.  `S` is `pkg.synth` throughout.  Shared by the CPU tier (oracle) and the GPU tier (HIP library), so both
are held to the same cases."""
import numpy as np


# ----------------------------------------------------------------------------- images
def texture_pair(S, w, h, seed, max_px):
    """(I, J): make_texture and its warp by a small homography; sizes too small for make_texture are cut out of a larger pair"""
    W, H = max(w, 64), max(h, 48)
    a = S.make_texture(W, H, seed)
    b = S.warp_homography(a, S.small_motion_homography(W, H, seed + 1, max_px=max_px))
    y0, x0 = (H - h) // 2, (W - w) // 2
    return np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(b[y0:y0 + h, x0:x0 + w])


def squeeze_half(img):
    """the left half squeezed to about 6 grey levels around 100: minEig falls to the neighbourhood of 1e-4 there"""
    out = img.copy()
    hw = img.shape[1] // 2
    out[:, :hw] = (97 + (img[:, :hw].astype(np.int32) * 6) // 256).astype(np.uint8)
    return out


def contrast_sweep_pair(S, w, h, seed):
    """a flat band (minEig = 0 exactly), then the texture at a contrast rising geometrically from 0.02 to 4 (saturating) across the
    width: minEig sweeps over five decades, so gates at 1e-6, 1e-4 and 1e-2 all have points on both sides"""
    a, b = texture_pair(S, w, h, seed, 1.0)
    x = np.arange(w)
    flat = w // 5
    c = np.where(x < flat, 0.0, 0.02 * (4.0 / 0.02) ** ((x - flat) / max(w - 1 - flat, 1)))
    f = lambda im: np.clip(np.rint(100.0 + (im.astype(np.float64) - 128.0) * c[None, :]), 0, 255).astype(np.uint8)
    return f(a), f(b)


def oblique_edge_pair(w, h, seed):
    """a steep 45-degree edge plus noise of one grey level on a quarter of the pixels: the gradient is one-directional, A12^2 is close to
    A11 A22 and D passes FLT_EPSILON with A11 A22 / D in the thousands (the conditioning term of the step tolerance)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    def render(shift):
        return 40.0 + 180.0 * np.clip((xx + yy - (w + h) / 2.0 - shift) / 3.0 + 0.5, 0.0, 1.0)
    noise = (rng.random((h, w)) < 0.25) * rng.choice([-1.0, 1.0], (h, w))
    noise2 = (rng.random((h, w)) < 0.25) * rng.choice([-1.0, 1.0], (h, w))
    return (np.clip(render(0.0) + noise, 0, 255) + 0.5).astype(np.uint8), (np.clip(render(0.7) + noise2, 0, 255) + 0.5).astype(np.uint8)


def blob_pair(w, h, seed, shift):
    """wide Gaussian blobs (sigma about 12 px), the second frame shifted by `shift` px along x"""
    rng = np.random.default_rng(seed)
    n = (w * h) // 900
    cx, cy = rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)
    amp, sig = rng.uniform(40, 110, n) * rng.choice([-1.0, 1.0], n), rng.uniform(10.5, 13.5, n)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    def render(dx):
        f = np.full((h, w), 128.0)
        for k in range(n):
            f += amp[k] * np.exp(-((xx - cx[k] - dx) ** 2 + (yy - cy[k]) ** 2) / (2 * sig[k] ** 2))
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return render(0.0), render(float(shift))


# ----------------------------------------------------------------------------- step scenes (starts on the 1/64 grid)
def step_points64(w, h, win, seed, n_inside=44):
    """integer starts in 1/64 px: the two corners, >= 40 interior points, and on every side the two starts either side of the exit
    (floor(x - halfWin) < -win, >= cols) plus random starts up to win + 2 outside"""
    rng = np.random.default_rng(seed)
    half = (win - 1) // 2
    pts = [(0, 0), (64 * (w - 1), 64 * (h - 1))]
    pts += [(int(rng.integers(0, 64 * (w - 1) + 1)), int(rng.integers(0, 64 * (h - 1) + 1))) for _ in range(n_inside)]
    lo = 64 * (half - win)                       # x - half == -win exactly: the last start that stays
    for k in range(2):                           # k = 0: x-sides, k = 1: y-sides
        size = (w, h)[k]
        other = (h, w)[k]
        hi = 64 * (size + half)                  # x - half == size: the first start that exits
        side = [lo, lo - 1, hi, hi - 1, -64 * (win + 2), 64 * (size - 1 + win + 2)]
        side += [-int(rng.integers(1, 64 * (win + 2))) for _ in range(3)]
        side += [64 * (size - 1) + int(rng.integers(1, 64 * (win + 2))) for _ in range(3)]
        for v in side:
            o = int(rng.integers(0, 64 * (other - 1) + 1))
            pts.append((v, o) if k == 0 else (o, v))
    return np.array(pts, np.int64)


STEP_SIZES = [(97, 61, (21, 7)), (64, 48, (3, 15)), (53, 47, (5,)), (24, 18, (21, 7))]


STEP_NAMES = [f"{tag}-{w}x{h}-win{win}" for (w, h, wins) in STEP_SIZES for win in wins for tag in ("tex", "squeezed")] + \
             ["sweep-160x96-win7-thr0.01", "sweep-160x96-win7-thr1e-06", "oblique-80x72-win15"]


def step_scenes(S):
    """list of dicts: name, I, J, win, min_eig, pts64, sweep (True for the minEig sweep scenes)"""
    out = []
    for (w, h, wins) in STEP_SIZES:
        a, b = texture_pair(S, w, h, 1000 + w, 1.5)
        pairs = (("tex", a, b), ("squeezed", squeeze_half(a), squeeze_half(b)))
        for win in wins:
            for tag, I, J in pairs:
                out.append(dict(name=f"{tag}-{w}x{h}-win{win}", I=I, J=J, win=win, min_eig=1e-4, pts64=step_points64(w, h, win, 7 * w + win),
                                sweep=False))
    I, J = contrast_sweep_pair(S, 160, 96, 321)
    for thr in (1e-2, 1e-6):
        out.append(dict(name=f"sweep-160x96-win7-thr{thr:g}", I=I, J=J, win=7, min_eig=thr, pts64=step_points64(160, 96, 7, 99, n_inside=150), sweep=True))
    I, J = oblique_edge_pair(80, 72, 5)
    out.append(dict(name="oblique-80x72-win15", I=I, J=J, win=15, min_eig=1e-7, pts64=step_points64(80, 72, 15, 17, n_inside=60), sweep=False))
    return out


# ----------------------------------------------------------------------------- run, chain and reload scenes
def _run_points(w, h, seed, n=80):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(2, w - 3, n), rng.uniform(2, h - 3, n)], axis=1).astype(np.float32)


#            name               w    h   win lvl iters eps  motion equalize
RUN_TABLE = [("run-win21",      160, 120, 21, 3, 30, 0.01, 3.0, False),
             ("run-win7",       160, 120, 7,  2, 30, 0.01, 2.0, False),
             ("run-win15-eps0", 160, 120, 15, 1, 100, 0.0, 2.0, False),
             ("run-win5-l0",    97,  61,  5,  0, 30, 0.01, 0.4, False),
             ("run-win5-7lvl",  643, 517, 5,  6, 30, 0.01, 3.0, False),
             ("run-24x18-win7", 24,  18,  7,  1, 30, 0.01, 1.0, False),
             ("run-equalize",   643, 517, 21, 3, 30, 0.01, 3.0, True)]
CHAIN_TABLE = [("chain-win3-8lvl-it1", 643, 517, 3, 7, 1), ("chain-win3-8lvl-it2", 643, 517, 3, 7, 2),
               ("chain-win21-it1", 160, 120, 21, 3, 1), ("chain-win21-it2", 160, 120, 21, 3, 2)]


RUN_NAMES = [r[0] for r in RUN_TABLE]
CHAIN_NAMES = [r[0] for r in CHAIN_TABLE]


def run_scenes(S):
    out = []
    for (name, w, h, win, lvl, iters, eps, motion, eq) in RUN_TABLE:
        I, J = texture_pair(S, w, h, 2000 + w + win, motion)
        out.append(dict(name=name, I=I, J=J, win=win, max_level=lvl, max_iters=iters, eps=eps, min_eig=1e-4, equalize=eq,
                        pts=_run_points(w, h, 31 * win + w), kind="run"))
    return out


def chain_scenes(S):
    out = []
    for (name, w, h, win, lvl, iters) in CHAIN_TABLE:
        I, J = texture_pair(S, w, h, 3000 + w + win, 3.0)
        out.append(dict(name=name, I=I, J=J, win=win, max_level=lvl, max_iters=iters, eps=0.0, min_eig=1e-4, equalize=False,
                        pts=_run_points(w, h, 17 * win + w), kind="chain"))
    return out


def reload_scene():
    w, h = 240, 160
    I, J = blob_pair(w, h, 77, 12)
    ys, xs = np.mgrid[24:h - 24:8j, 30:w - 40:8j]
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)
    return dict(name="reload-blobs", I=I, J=J, win=21, max_level=0, max_iters=30, eps=0.01, min_eig=1e-4, equalize=False, pts=pts, kind="run")


# ----------------------------------------------------------------------------- min-eigenvalue map and selection
MINEIG_SIZES = [(320, 240), (97, 61), (65, 17), (33, 9), (31, 7)]
TINY_SIZES = [(1, 5), (2, 2), (3, 3), (5, 2)]          # (w, h)

TINY_3X3 = ([[0, 0, 0], [0, 255, 0], [0, 0, 0]],            # reflection makes every derivative vanish: no corner
            [[0, 255, 0], [255, 0, 0], [0, 0, 0]],            # in exact arithmetic all nine values are equal (the centre would win the
            [[128, 128, 128], [255, 128, 128], [128, 255, 128]])   # tie); in float32 the sums' order decides: whatever the map says holds


def mineig_images(S, w, h):
    """name -> image: texture, uniform noise, noise in 250..255 (flat and nearly saturated), 6-pixel checkerboard, periodic tiling"""
    rng = np.random.default_rng(100 * w + h)
    big = S.make_texture(max(w, 64), max(h, 48), 500 + w)
    tex = np.ascontiguousarray(big[:h, :w])
    yy, xx = np.mgrid[0:h, 0:w]
    per = min(16, h, w)
    return {"texture": tex,
            "noise": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "noise250": rng.integers(250, 256, (h, w), dtype=np.uint8),
            "checker6": (((yy // 6) + (xx // 6)) % 2 * 200 + 20).astype(np.uint8),
            "tiled": np.ascontiguousarray(np.tile(big[:per, :per], (h // per + 1, w // per + 1))[:h, :w])}


def selection_cases(w, h, image="texture"):
    """(mask name, quality, min_dist, quota): the product of qualities, distances and quotas, the three masks taken in turn.
    The qualities are 0.01 and 0.3, except where an unlimited quota would return more than the 4096 corners a handle holds
    (320 x 240 noise and checkerboard): there the quality level is raised instead of leaving the image out"""
    # (the 320 x 240 checkerboard's corners all tie, far beyond 4096 at any quality: its selection runs under a box mask)
    masks = ("box", "box", "single", "box") if (w * h > 50000 and image == "checker6") else ("none", "half", "single", "half")
    cases = []
    i = 0
    dense = w * h > 50000 and image in ("noise", "noise250", "checker6")
    for q in ((0.3, 0.6) if dense else (0.01, 0.3)):
        for md in (0.5, 1.0, 7.0, 20.5):
            for quota in (0, 1, 25):
                cases.append((masks[i % 4], q, md, quota))
                i += 1
    return cases


def make_mask(name, w, h):
    if name == "none":
        return None
    m = np.zeros((h, w), np.uint8)
    if name == "half":
        m[:, w // 2:] = 255
    elif name == "box":
        m[h // 4:h - h // 4, w // 4:w - w // 4] = 1
    else:
        m[h // 2, w // 2] = 7
    return m
