"""GPU tier of the sliding-window marginalisation (include/lvi_marg.h) against tests/marg_ref.py.

What is compared, every figure printed before it is asserted: A and b (lvi_marg_debug_system); H = J'J and g = J'r0 of the
prior against the mpmath Schur complement (Hp, gp of tests/marg_ref.py: the Schur complement without what the threshold drops —
an exact eigenvalue below eps that is not zero, as the chain's third step has, takes (v'g) v out of J'r0 in the reference
too; without one the two are the same numbers); the prior's cost change ||r0 + J dx||^2 - ||r0||^2 for five seeded dx against
dx'H dx + 2 g'dx; the rank where the scene's conditions allow it (tests/test_marg_ref.py asserts them).  The tolerance of a
quantity is max(10 G, floor): G is the distance between the float64 and the mpmath reference for that scene and quantity
(the margin of 10 because the device sums and rotates in another order than numpy), floor = dim x 2.2e-16 x the 2-norm of
the matrix (or of b) the quantity is computed from — the backward-error scale of a symmetric eigen-solver.  Nothing is
measured against the code under test."""
import numpy as np
import pytest

import marg_ref as R

pytestmark = pytest.mark.gpu
U = 2.2e-16
LD = np.longdouble


class Device:
    """the scene script's interface over a Marginalizer; projection records go up in one call, in order"""

    def __init__(self, marg):
        self.m, self.recs = marg, []
        marg.begin()

    def set_block(self, bid, values):
        self.m.set_block(bid, values)

    def _flush(self):
        if self.recs:
            a = np.zeros(len(self.recs), self.m.record_dtype)
            for k, r in enumerate(self.recs):
                for key, v in r.items():
                    a[k][key] = v
            self.m.add_projection(a)
            self.recs = []

    def add_projection(self, rec):
        self.recs.append(rec)

    def add_dense(self, ids, residual, jacobians, drop):
        self._flush()
        self.m.add_dense(ids, residual, jacobians, drop)

    def marginalize(self):
        self._flush()
        return self.m.marginalize()


@pytest.fixture(scope="module")
def marg(pkg, hip):
    m = pkg.Marginalizer(hip, max_blocks=512, max_projections=512, max_dense_factors=2, max_dense_rows=128, max_drop_dim=160, max_keep_dim=96)
    yield m
    m.close()


def _params(m, sc):
    base = dict(loss_type=R.LOSS_CAUCHY, loss_a=1.0, sqrt_info=R.SQRT_INFO, tr_over_row=0.0, half_row=240.0, eps=R.EPS, max_sweeps=30)
    base.update(sc["params"])
    m.set_params(**base)


def _tol(G, floor):
    return max(10 * G, floor)


def _hg(J, r):
    J, r = J.astype(LD), r.astype(LD)
    return (J.T @ J).astype(np.float64), (J.T @ r).astype(np.float64)


def _cost_changes(J, r, n, seed=77, count=5):
    """||r + J dx||^2 - ||r||^2 for the seeded dx, in extended precision"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        dx = rs.normal(0, 1e-2, n)
        J_, r_ = np.asarray(J, object if J.dtype == object else LD), np.asarray(r, object if J.dtype == object else LD)
        d = dx.astype(LD) if J.dtype != object else R.MP.arr(dx)
        e = r_ + J_ @ d
        out.append((dx, float(e @ e - r_ @ r_)))
    return out


def _compare_prior(tag, Jd, rd, f, m, perm=None):
    """the device prior (J, r) against the references f (float64) and m (mpmath) of one marginalisation; perm: the
    device's column order in terms of the reference's.  Returns the figures."""
    n, pos = m["n"], m["m"] + m["n"]
    Hd, gd = _hg(Jd, rd)
    if perm is not None:
        Hd, gd, Jd = Hd[np.ix_(perm, perm)], gd[perm], Jd[:, perm]
    nA, nb = R.norm2(m["A"]), float(np.linalg.norm(R.to_f64(m["b"])))
    GH, Gg = R.gap(f["Hp"], m["Hp"]), R.gap(f["gp"], m["gp"])
    dH, dg = R.gap(Hd, m["Hp"]), R.gap(gd, m["gp"])
    tH, tg = _tol(GH, pos * U * nA), _tol(Gg, pos * U * nb)
    print(f"[marg] {tag}: H: G {GH:.3e} device {dH:.3e} tolerance {tH:.3e}; g: G {Gg:.3e} device {dg:.3e} tolerance {tg:.3e}")
    nH, ng = R.norm2(m["Hp"]), float(np.linalg.norm(R.to_f64(m["gp"])))
    worst = 0.0
    for (dx, cd), (_, cf) in zip(_cost_changes(Jd, rd, n), _cost_changes(f["J"], f["r"], n)):
        dm = R.MP.arr(dx)
        cm = float(dm @ (m["Hp"] @ dm) + 2 * (m["gp"] @ dm))
        nd = float(np.linalg.norm(dx))
        tc = _tol(abs(cf - cm), pos * U * (nH * nd * nd + 2 * ng * nd))
        print(f"[marg] {tag}: cost change {cm:.6e}: G {abs(cf - cm):.3e} device {abs(cd - cm):.3e} tolerance {tc:.3e}")
        worst = max(worst, abs(cd - cm) - tc)              # a prior of rank 0 has cost change, G and floor all exactly zero
    assert dH <= tH and dg <= tg and worst <= 0.0
    return dict(GH=GH, dH=dH, Gg=Gg, dg=dg)


def _compare_system(tag, Ad, bd, f, m):
    pos = m["m"] + m["n"]
    GA, Gb = R.gap(f["A"], m["A"]), R.gap(f["b"], m["b"])
    dA, db = R.gap(Ad, m["A"]), R.gap(bd, m["b"])
    tA, tb = _tol(GA, pos * U * R.norm2(m["A"])), _tol(Gb, pos * U * float(np.linalg.norm(R.to_f64(m["b"]))))
    print(f"[marg] {tag}: A: G {GA:.3e} device {dA:.3e} tolerance {tA:.3e}; b: G {Gb:.3e} device {db:.3e} tolerance {tb:.3e}")
    assert dA <= tA and db <= tb
    assert np.array_equal(Ad, Ad.T), "A is not bitwise symmetric"


def _run_scene(marg, name):
    sc = R.gpu_scene(name)
    _params(marg, sc)
    info = R.play(sc, Device(marg)).marginalize()
    A, b = marg.debug_system()
    return sc, info, A, b


# ---- 1, 2, 4, 6: one factor; three features with and without td; the eigen-solver's sizes; the IMU-like block --------
@pytest.mark.parametrize("name", [n for n in R.GPU_SCENES if n not in R.SYSTEM_ONLY])
def test_scene_against_the_reference(marg, name):
    f, m = R.scene_reference(name)
    sc, info, A, b = _run_scene(marg, name)
    print(f"[marg] {name}: status {info['status']} m {info['m']} n {info['n']} rank {info['rank']} (float64 {f['rank']}, mpmath {m['rank']}) rank_mm {info['rank_mm']} "
          f"sweeps ({info['sweeps_mm']}, {info['sweeps_rr']}) last off-diagonal ({info['off_mm']:.2e}, {info['off_rr']:.2e}) cost {info['cost']:.6e}")
    assert info["status"] == 0 and (info["m"], info["n"]) == (m["m"], m["n"])
    _compare_system(name, A, b, f, m)
    lay = marg.layout()
    assert list(lay["ids"]) == m["ids"] and list(lay["sizes"]) == m["sizes"] and list(lay["idx"] - info["m"]) == m["col"]
    assert all(np.array_equal(a, x0) for a, x0 in zip(lay["values"], m["x0"]))
    J, r = marg.prior()
    _compare_prior(name, J, r, f, m)
    if sc["rank"]:
        assert info["rank"] == m["rank"] and info["rank_mm"] == sum(1 for x in m["w_mm"] if x > R.EPS)
    else:
        print(f"[marg] {name}: the threshold decisions of this scene are rounding noise (tests/test_marg_ref.py): compared on H and g only")
    assert not J[:info["n"] - info["rank"]].any(), "the rows of the dropped eigenvalues are not zero"
    if name == "eig_3_6":                                  # a kept block that no factor touches: exactly zero row and column
        H, g = _hg(J, r)
        assert not A[5:9].any() and not A[:, 5:9].any() and not b[5:9].any() and not H[2:6].any() and not H[:, 2:6].any() and not g[2:6].any()


# ---- 3: an accumulation that crosses the reduction's boundaries ---------------------------------------------------
@pytest.mark.parametrize("name", R.SYSTEM_ONLY)
def test_accumulation_across_partials(marg, name):
    f, m = R.scene_reference(name)
    _, info, A, b = _run_scene(marg, name)
    assert info["status"] == 0 and (info["m"], info["n"]) == (m["m"], m["n"])
    _compare_system(name, A, b, f, m)
    J, r = marg.prior()
    _, info2, A2, b2 = _run_scene(marg, name)
    J2, r2 = marg.prior()
    print(f"[marg] {name}: sweeps ({info['sweeps_mm']}, {info['sweeps_rr']}); second run equal bits: A {np.array_equal(A, A2)} b {np.array_equal(b, b2)} "
          f"J {np.array_equal(J, J2)} r {np.array_equal(r, r2)}")
    assert np.array_equal(A, A2) and np.array_equal(b, b2) and np.array_equal(J, J2) and np.array_equal(r, r2)


# ---- 5: the chain MARGIN_OLD -> MARGIN_SECOND_NEW -> MARGIN_OLD ----------------------------------------------------
def _perm(lay, info, ref):
    """the device's columns in the reference's order"""
    at = {int(b): int(i) - info["m"] for b, i in zip(lay["ids"], lay["idx"])}
    return np.concatenate([np.arange(at[b], at[b] + R.local_size(s)) for b, s in zip(ref["ids"], ref["sizes"])])


def _dense_prior(prior, win_blocks):
    """MarginalizationFactor::Evaluate (:332-380) on the host from a downloaded prior: (ids, residual, jacobians)"""
    J, r, lay = prior
    n = J.shape[0]
    dx, Js = np.zeros(n), []
    for b, s, c, x0 in zip(lay["ids"], lay["sizes"], lay["idx"] - lay["info"]["m"], lay["values"]):
        ls = R.local_size(int(s))
        dx[c:c + ls] = R.prior_dx(int(s), win_blocks[int(b)], x0, R.F64)
        Jb = np.zeros((n, int(s)))
        Jb[:, :ls] = J[:, c:c + ls]
        Js.append(Jb)
    return [int(b) for b in lay["ids"]], r + J @ dx, Js


def test_chain_resident_and_downloaded_prior(pkg, hip, marg):
    ref, steps = R.chain_reference(), R.chain_steps()
    V = pkg.host_api.VinsMarginalizer(pkg.load_host(), hip, max_features=16, estimate_td=True)
    m2 = pkg.Marginalizer(hip, max_blocks=64, max_projections=256, max_dense_factors=2, max_dense_rows=128, max_drop_dim=64, max_keep_dim=96)
    fed = None
    try:
        for k, (flag, win, feats, imu) in enumerate(steps):
            V.set_window(win["pose"], win["speed_bias"], win["ex"], win["td"])
            V.set_features(feats)
            V.set_imu(0.5, *((imu["residual"], imu["jacobians"]) if imu else (None, None)))
            out = V.run(flag)
            f, m = ref[k]
            lay = V.marg.layout()
            print(f"[marg] chain step {k}: ran {out['ran']} status {out['status']} m {out['m']} n {out['n']} rank {out['rank']} (float64 {f['rank']}, mpmath {m['rank']}) "
                  f"sweeps ({out['sweeps_mm']}, {out['sweeps_rr']}); kept ids {list(lay['ids'])}")
            assert out["ran"] and out["status"] == 0 and (out["m"], out["n"]) == (m["m"], m["n"]) and sorted(lay["ids"]) == sorted(m["ids"])
            A, b = V.marg.debug_system()
            _compare_system(f"chain step {k}", A, b, f, m)
            J, r = V.marg.prior()
            fig = _compare_prior(f"chain step {k}, resident", J, r, f, m, _perm(lay, out, m))
            # the same step with the previous prior downloaded, evaluated here and handed in as a dense factor
            blocks = {R.ID_POSE + i: win["pose"][i] for i in range(11)}
            blocks.update({R.ID_SPEEDBIAS + i: win["speed_bias"][i] for i in range(11)})
            blocks.update({R.ID_EX: win["ex"], R.ID_TD: np.array([win["td"]])})
            m2.begin()
            d = Device(m2)
            for b_, v in blocks.items():
                d.set_block(b_, v)
            if fed is not None:
                ids, res, Js = _dense_prior(fed, blocks)
                dropped = (R.ID_POSE, R.ID_SPEEDBIAS) if flag == R.MARGIN_OLD else (R.ID_POSE + R.WINDOW_SIZE - 1,)
                d.add_dense(ids, res, Js, [int(b_ in dropped) for b_ in ids])
            if flag == R.MARGIN_OLD:
                d.add_dense([R.ID_POSE, R.ID_SPEEDBIAS, R.ID_POSE + 1, R.ID_SPEEDBIAS + 1], imu["residual"], imu["jacobians"], [1, 1, 0, 0])
                recs, fblocks = R.vins_projections(win, feats, True)
                for b_, v in fblocks.items():
                    d.set_block(b_, [v])
                for rec in recs:
                    d.add_projection(rec)
            i2 = d.marginalize()
            if flag == R.MARGIN_OLD:
                old = [R.ID_POSE + i for i in range(1, 11)] + [R.ID_SPEEDBIAS + i for i in range(1, 11)]
                m2.remap(old, [b_ - 1 for b_ in old])
            else:
                m2.remap([R.ID_POSE + 10, R.ID_SPEEDBIAS + 10], [R.ID_POSE + 9, R.ID_SPEEDBIAS + 9])
            lay2 = m2.layout()
            J2, r2 = m2.prior()
            assert i2["status"] == 0 and (i2["m"], i2["n"]) == (m["m"], m["n"])
            fig2 = _compare_prior(f"chain step {k}, downloaded", J2, r2, f, m, _perm(lay2, i2, m))
            (H1, g1), (H2, g2) = _hg(J[:, _perm(lay, out, m)], r), _hg(J2[:, _perm(lay2, i2, m)], r2)
            pos = m["m"] + m["n"]
            tH = 2 * _tol(fig["GH"], pos * U * R.norm2(m["A"]))
            tg = 2 * _tol(fig["Gg"], pos * U * float(np.linalg.norm(R.to_f64(m["b"]))))
            print(f"[marg] chain step {k}: resident vs downloaded: H {np.abs(H1 - H2).max():.3e} (tolerance {tH:.3e}), g {np.abs(g1 - g2).max():.3e} "
                  f"(tolerance {tg:.3e}); each twice one side's tolerance against the reference; downloaded vs reference H {fig2['dH']:.3e} g {fig2['dg']:.3e}")
            assert np.abs(H1 - H2).max() <= tH and np.abs(g1 - g2).max() <= tg
            fed = (J2, r2, lay2)
    finally:
        V.close()
        m2.close()
    with pytest.raises(pkg.LviError) as e:                               # the view went with the object it looked at
        V.marg.layout()
    assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG


# ---- 7: refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_prior_unchanged(pkg, hip, marg):
    E = pkg._abi
    _run_scene(marg, "three_td")
    J0, r0 = marg.prior()
    lay0 = marg.layout()

    def unchanged():
        J, r = marg.prior()
        lay = marg.layout()
        return np.array_equal(J, J0) and np.array_equal(r, r0) and list(lay["ids"]) == list(lay0["ids"]) and lay["info"] == lay0["info"]

    sc = R.gpu_scene("three_td")
    blocks = [o for o in sc["ops"] if o[0] == "block"]
    recs = [o[1] for o in sc["ops"] if o[0] == "proj"]

    def declared():
        d = Device(marg)
        for _, b, v in blocks:
            d.set_block(b, v)
        return d

    def refused(code, fn):
        with pytest.raises(pkg.LviError) as e:
            fn()
        assert e.value.code == code, (e.value.code, code)
        assert unchanged()

    d = declared()
    d.add_projection(dict(recs[0], feature=9999))                        # an unknown id
    refused(E.LVI_ERR_INVALID_ARG, d._flush)
    d = declared()
    refused(E.LVI_ERR_INVALID_ARG, lambda: marg.set_block(R.ID_POSE, np.zeros(9)))       # a size mismatch on a re-declared id
    d.add_projection(dict(recs[0], pose_j=R.ID_TD))                      # a block of the wrong size in a factor
    refused(E.LVI_ERR_INVALID_ARG, d._flush)
    d = declared()
    refused(E.LVI_ERR_INVALID_ARG, lambda: marg.add_last_prior([R.ID_FEATURE]))          # a drop id the prior does not keep
    marg.add_last_prior([R.ID_POSE + 1])
    refused(E.LVI_ERR_STATE, lambda: marg.remap([R.ID_POSE + 1], [R.ID_POSE + 7]))       # renaming the prior while the description names it
    refused(E.LVI_ERR_STATE, lambda: marg.add_last_prior([]))                            # the prior twice
    marg.begin()
    fresh = pkg.Marginalizer(hip, max_blocks=8, max_projections=2, max_dense_factors=1, max_dense_rows=4, max_drop_dim=6, max_keep_dim=32)
    try:
        for _, b, v in blocks[:7]:
            fresh.set_block(b, v)
        with pytest.raises(pkg.LviError) as e:                           # add_last_prior without a previous result
            fresh.add_last_prior([])
        assert e.value.code == E.LVI_ERR_STATE
        with pytest.raises(pkg.LviError) as e:                           # more blocks than max_blocks
            fresh.set_block(500, [1.0]), fresh.set_block(501, [1.0])
        assert e.value.code == E.LVI_ERR_CAPACITY
        a = np.zeros(3, pkg.marg.PROJECTION_DTYPE)
        for k in range(3):
            for key, v in recs[k].items():
                a[k][key] = v
        with pytest.raises(pkg.LviError) as e:                           # more projections than max_projections
            fresh.add_projection(a)
        assert e.value.code == E.LVI_ERR_CAPACITY
        fresh.add_projection(a[:2])                                      # pose 0 and a feature: m = 7 > max_drop_dim
        with pytest.raises(pkg.LviError) as e:
            fresh.marginalize()
        assert e.value.code == E.LVI_ERR_CAPACITY
        with pytest.raises(pkg.LviError) as e:                           # more dense rows than max_dense_rows
            fresh.add_dense([R.ID_POSE], np.zeros(5), [np.zeros((5, 7))], [1])
        assert e.value.code == E.LVI_ERR_CAPACITY
    finally:
        fresh.close()
    assert unchanged()
    # inv_dep = 0: a soft status, the previous prior stays
    d = declared()
    d.set_block(R.ID_FEATURE, [0.0])
    for rec in recs:
        d.add_projection(rec)
    info = d.marginalize()
    print(f"[marg] inv_dep = 0: status {info['status']} flags {info['flags']}")
    assert info["status"] == pkg.marg.NOT_FINITE == 2 and unchanged()
    # and the handle still works: the same scene again gives the same prior, bit for bit
    _run_scene(marg, "three_td")
    assert unchanged()
    # the bound on the sweeps is a soft status
    sc2 = R.gpu_scene("eig_7_12")
    _params(marg, sc2)
    marg.set_params(max_sweeps=1)
    info = R.play(sc2, Device(marg)).marginalize()
    print(f"[marg] max_sweeps 1: status {info['status']} sweeps ({info['sweeps_mm']}, {info['sweeps_rr']}) off ({info['off_mm']:.2e}, {info['off_rr']:.2e})")
    assert info["status"] == pkg.marg.EIG_NOT_CONVERGED == 1 and info["sweeps_mm"] == 1
    for bad in (dict(max_sweeps=0), dict(max_sweeps=pkg.marg.MAX_SWEEPS + 1), dict(loss_type=3), dict(loss_a=0.0), dict(eps=-1.0)):
        with pytest.raises(pkg.LviError) as e:
            marg.set_params(**bad)
        assert e.value.code == E.LVI_ERR_INVALID_ARG
    for bad in (dict(max_blocks=0), dict(max_drop_dim=pkg.marg.MAX_DROP_DIM + 1), dict(max_keep_dim=0), dict(max_projections=pkg.marg.MAX_PROJECTIONS + 1)):
        with pytest.raises(pkg.LviError) as e:
            pkg.Marginalizer(hip, **bad)
        assert e.value.code == E.LVI_ERR_INVALID_ARG
