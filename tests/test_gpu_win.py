"""GPU tier of the sliding-window solve (include/lvi_win.h) against tests/win_ref.py.

Every figure is printed before it is asserted and nothing is measured against the code under test.  The tolerance of a
quantity is max(10 G, floor): G is the distance between the float64 and the mpmath reference for that scene and quantity
(the margin of 10 because the device sums in another order than numpy); the floor is dim x 2.2e-16 x the 2-norm of what the
quantity is computed from, dim being the dimension of the system: its reduced columns plus its eliminated blocks.  For a step the floor is multiplied by the condition number of the scaled H + mu D of the mpmath reference.
The scenes of S.F64_ONLY are too slow in mpmath and are compared with float64 at the floor alone."""
import numpy as np
import pytest

import marg_ref as M
import win_ref as R
import win_scenes as S

pytestmark = pytest.mark.gpu
U = 2.2e-16


class Device:
    """a scene script's interface over a WindowSolver"""

    def __init__(self, w, **params):
        self.w, self.recs, self.ids = w, [], []
        P = dict(R.DEFAULTS)
        P.update(params)
        w.set_params(**P)
        w.begin()

    def set_block(self, bid, values, flags=0):
        if bid not in self.ids:
            self.ids.append(bid)
        self.w.set_block(bid, values, flags)

    def add_projection(self, rec):
        self.recs.append(rec)

    def add_imu(self, rec):
        a = np.zeros(1, self.w.imu_dtype)
        for k, v in rec.items():
            a[0][k] = v
        self.w.add_imu(a)

    def set_prior(self, p):
        self.w.set_prior(M.to_f64(p["J"]), M.to_f64(p["r"]), p["ids"], p["sizes"], p["col"], p["x0"])

    def flush(self):
        if self.recs:
            a = np.zeros(len(self.recs), self.w.record_dtype)
            for k, r in enumerate(self.recs):
                for key, v in r.items():
                    a[k][key] = v
            self.w.add_projection(a)
            self.recs = []
        return self

    def state(self):
        return {b: self.w.block(b) for b in self.ids}


@pytest.fixture(scope="module")
def win(pkg, hip):
    w = pkg.WindowSolver(hip, max_blocks=256, max_projections=512, max_eliminated=160, max_imu=12, max_prior_rows=128, max_dim=192)
    yield w
    w.close()


def _device(win, name, x=None, **params):
    sc = S.scene(name)
    P = dict(sc["params"])
    P.update(params)
    d = S.play(sc, Device(win, **P)).flush()
    if x is not None:
        for op in sc["ops"]:
            if op[0] == "block":
                d.set_block(op[1], M.to_f64(x[op[1]]), op[3])
    return d


def _tol(G, floor):
    return max(10 * G, floor)


def _check(tag, got, f, m, floor):
    """one quantity against the float64 reference f and the mpmath one m (None: float64 at the floor alone) -> the figures"""
    f = np.atleast_1d(np.asarray(f, object))
    m = None if m is None else np.atleast_1d(np.asarray(m, object))
    G = M.gap(f, m) if m is not None else 0.0
    ref = M.to_f64(m) if m is not None else M.to_f64(f)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - ref))) if np.size(ref) else 0.0
    tol = _tol(G, floor)
    print(f"[win gpu] {tag}: device distance {err:.3e}, G {G:.3e}, floor {floor:.3e}, bound {tol:.3e}")
    assert err <= tol, tag
    return err, G


def _full(sys):
    H, W, h = M.to_f64(sys["H"]), M.to_f64(sys["W"]), M.to_f64(sys["h"])
    return np.block([[H, W.T], [W, np.diag(h)]]) if len(h) else H


def _compare_system(tag, dev, f, m):
    D, E = f["D"], f["E"]
    assert dev["H"].shape == (D, D) and dev["W"].shape == (E, D)
    n = D + E                                                # dim: the system's dimension, reduced columns plus eliminated blocks
    Hn = np.linalg.norm(_full(m or f), 2)
    rn = float(np.sqrt(float((m or f)["rr"])))
    mm = m or {}
    _check(f"{tag} H", dev["H"], f["H"], mm.get("H"), n * U * Hn)
    _check(f"{tag} g", dev["g"], f["g"], mm.get("g"), n * U * np.sqrt(Hn) * rn)
    if E:
        _check(f"{tag} W", dev["W"], f["W"], mm.get("W"), n * U * Hn)
        _check(f"{tag} hdiag", dev["hdiag"], f["h"], mm.get("h"), n * U * Hn)
        _check(f"{tag} gf", dev["gf"], f["gf"], mm.get("gf"), n * U * np.sqrt(Hn) * rn)
    _check(f"{tag} cost", dev["cost"], f["cost"], mm.get("cost"), n * U * float(f["cost"]))
    assert np.array_equal(dev["H"], dev["H"].T), "H is not bitwise symmetric"


# ---- factors and system -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SYSTEM_SCENES)
def test_system_at_the_declared_state(win, name):
    dev = _device(win, name).w.debug_system()
    assert dev["status"] == 0
    f, m = S.system_reference(name)
    _compare_system(name, dev, f, m)


@pytest.mark.parametrize("name", ["two_frames", "three_td", "half_constant"])
def test_system_at_a_perturbed_state(win, name):
    """the state after the reference's first accepted step"""
    sf, sm = S.solve_reference(name)
    x = sf["iterates"][1]["x"]
    dev = _device(win, name, x=x).w.debug_system()
    pf, pm = S.problem(name, R.F64), S.problem(name, R.MP)
    _compare_system(f"{name} x1", dev, pf.system(x), pm.system({b: R.MP.arr(M.to_f64(v)) for b, v in x.items()}))


def test_factor_rows(win):
    """per factor: the loss-corrected projection rows and the IMU and prior rows of `three_td`"""
    d = _device(win, "three_td")
    dev = d.w.debug_system()
    pf, pm = S.problem("three_td", R.F64), S.problem("three_td", R.MP)
    ff, fm = pf.factors(pf.x0()), pm.factors(pm.x0())
    col = pf.layout()[0]
    P, worst = len(pf.proj), 0.0
    for k in range(P):
        ids, r, Js, _ = ff[k]
        got = dev["proj_rows"][k]
        want = np.concatenate([np.concatenate([M.to_f64(J) for J in Js], axis=1), M.to_f64(r)[:, None]], axis=1)
        wm = np.concatenate([np.concatenate([M.to_f64(J) for J in fm[k][2]], axis=1), M.to_f64(fm[k][1])[:, None]], axis=1)
        tol = _tol(float(np.abs(want - wm).max()), 30 * U * M.SQRT_INFO * 10)       # the bound of tests/test_marg_ref.py's header comparison
        worst = max(worst, float(np.abs(got - want).max()) / tol)
    print(f"[win gpu] three_td projection rows: worst distance / bound {worst:.3e}")
    assert worst <= 1.0
    row = 0
    for (ids, r, Js, _), (_, rm, Jm, _) in zip(ff[P:], fm[P:]):
        want, wantm = np.zeros((len(r), dev["dense"].shape[1])), np.zeros((len(r), dev["dense"].shape[1]))
        for b, J, J2 in zip(ids, Js, Jm):
            if b in col:
                want[:, col[b]:col[b] + J.shape[1]], wantm[:, col[b]:col[b] + J.shape[1]] = M.to_f64(J), M.to_f64(J2)
        want[:, -1], wantm[:, -1] = M.to_f64(r), M.to_f64(rm)
        got = dev["dense"][row:row + len(r)]
        _check(f"three_td dense rows {row}..{row + len(r) - 1}", got, want, R.MP.arr(wantm), 15 * U * float(np.abs(want).max()))
        row += len(r)
    assert row == dev["dense"].shape[0]


# ---- single steps ---------------------------------------------------------------------------------------------
def _dim(sys):
    """the issue's dim: the dimension of the system the quantity belongs to, reduced columns plus eliminated blocks"""
    return sys["D"] + sys["E"]


def _cond(prob, sys, mu):
    """condition number of the scaled H + mu D after the elimination, from the reference; a free block no factor names is a
    1 x 1 block of its own (mu dg^2, step exactly 0) and is left out"""
    Sm, _, _ = R.Strategy(prob, sys).reduced(mu)
    keep = np.diag(M.to_f64(sys["H"])) != 0
    return float(np.linalg.cond(M.to_f64(Sm)[np.ix_(keep, keep)]))


def _single_step(win, name, x, radius, mu, tag, retry=False, **params):
    """restart device and references from (x, radius, mu) for one iteration and compare the step.  retry: the scene forces
    float64 retries that exact arithmetic does not take (tests/test_win_ref.py); the count and the final mu are compared with
    float64, and the mpmath reference starts at that final mu"""
    pf, pm = S.problem(name, R.F64, max_iterations=1, **params), S.problem(name, R.MP, max_iterations=1, **params)
    xm = {b: R.MP.arr(M.to_f64(v)) for b, v in x.items()}
    f = R.solve(pf, x=x, radius=radius, mu=mu)
    m = R.solve(pm, x=xm, radius=radius, mu=float(f["log"][1]["mu"]) if retry else mu)
    dev_params = dict(params, max_iterations=1, initial_radius=float(radius), initial_mu=float(mu))
    d = _device(win, name, x=x, **dev_params)
    info = d.w.solve()
    log = d.w.log()
    assert info["status"] == 0 and len(log) == 2
    ef, em, ed = f["log"][1], m["log"][1], log[1]
    sys_m = pm.system(xm)
    cond = _cond(pm, sys_m, em["mu"])
    n, cost0 = _dim(sys_m), float(sys_m["cost"])
    print(f"[win gpu] {tag}: kind {ed['step_kind']} accepted {ed['accepted']} retries {ed['mu_retries']} mu {ed['mu']:.3e}; reference {ef['step_kind']} {ef['accepted']} "
          f"{ef['mu_retries']} mu {float(ef['mu']):.3e}; cond {cond:.3e}")
    if retry:
        assert ef["mu_retries"] > 0 and (em["step_kind"], em["accepted"]) == (ef["step_kind"], ef["accepted"])
        assert ed["mu"] == float(ef["mu"]) and info["mu"] == float(f["mu"])
    else:
        assert R.decisions(f) == R.decisions(m), "the references disagree: not a scene for a step comparison"
    assert (ed["step_kind"], ed["accepted"], ed["mu_retries"]) == (ef["step_kind"], ef["accepted"], ef["mu_retries"])
    assert info["termination"] == f["termination"] and info["iterations"] == f["iterations"]
    for key in ("gauss_newton_norm", "cauchy_norm", "step_norm", "model_cost_change"):
        _check(f"{tag} {key}", ed[key], ef[key], em[key], n * U * cond * abs(float(em[key])))
    fl_cost = n * U * cost0
    _check(f"{tag} cost change", ed["cost_change"], ef["cost_change"], em["cost_change"], 2 * fl_cost)
    mcc = abs(float(em["model_cost_change"]))
    _check(f"{tag} rho", ed["rho"], ef["rho"], em["rho"], (2 * fl_cost + n * U * cond * mcc * abs(float(em["rho"]))) / mcc)
    got = d.state()
    worst = 0.0
    for b in got:
        step = float(np.abs(M.to_f64(m["x"][b]) - M.to_f64(xm[b])).max())
        tol = _tol(M.gap(f["x"][b], m["x"][b]), n * U * cond * max(step, float(np.abs(M.to_f64(xm[b])).max()) * U))
        worst = max(worst, float(np.abs(got[b] - M.to_f64(m["x"][b])).max()) / tol) if tol > 0 else worst
    print(f"[win gpu] {tag}: state after the iteration, worst distance / bound {worst:.3e}")
    assert worst <= 1.0
    return ed, d


@pytest.mark.parametrize("radius, kind", list(zip(S.STEP_RADII, (R.STEP_GAUSS_NEWTON, R.STEP_INTERPOLATED, R.STEP_CAUCHY))))
def test_single_step_kinds(win, radius, kind):
    p = S.problem("two_frames", R.F64)
    ed, _ = _single_step(win, "two_frames", p.x0(), radius, R.DEFAULTS["initial_mu"], f"two_frames radius {radius:g}")
    assert ed["step_kind"] == kind


@pytest.mark.parametrize("name", ["two_frames", "three_td"])
def test_single_steps_along_the_reference_trajectory(win, name):
    """one restart per iteration of the reference's trajectory, all eight"""
    f, _ = S.solve_reference(name)
    assert len(f["iterates"]) == 8
    for k, it in enumerate(f["iterates"]):
        assert not it["reuse"]
        _single_step(win, name, it["x"], it["radius"], it["mu"], f"{name} iteration {k + 1}")


@pytest.mark.parametrize("name", ["chol_32", "chol_33", "chol_64", "chol_65"])
def test_single_step_at_the_cholesky_panel_widths(win, name):
    """D = width, width + 1, 2 x width, 2 x width + 1: the factorisation and the solves, through the step they give"""
    p = S.problem(name, R.F64)
    assert p.layout()[2] == int(name.split("_")[1])
    _single_step(win, name, p.x0(), R.DEFAULTS["initial_radius"], R.DEFAULTS["initial_mu"], name)


def test_single_step_with_mu_retries(win):
    """`chol_33` under S.RETRY_PARAMS: the free block's pivot underflows to zero seven times; the ladder's count, the mu it
    ends at and the step are the reference's, and the free block comes back unchanged"""
    p = S.problem("chol_33", R.F64)
    ed, d = _single_step(win, "chol_33", p.x0(), R.DEFAULTS["initial_radius"], S.RETRY_PARAMS["initial_mu"], "chol_33 mu retries", retry=True, **S.RETRY_PARAMS)
    assert ed["mu_retries"] == 7 and ed["accepted"] == 1
    after = d.state()
    assert np.array_equal(after[S.ID_PAD], M.to_f64(p.x0()[S.ID_PAD])) and not np.array_equal(after[M.ID_POSE], M.to_f64(p.x0()[M.ID_POSE]))


def test_single_step_rejected(win):
    """`no_prior`'s first rejected iteration: the state comes back unchanged"""
    f, _ = S.solve_reference("no_prior", max_iterations=10)
    k = next(i for i, e in enumerate(f["log"][1:]) if not e["accepted"])
    it = f["iterates"][k]
    ed, d = _single_step(win, "no_prior", it["x"], it["radius"], it["mu"], f"no_prior iteration {k + 1} (rejected)")
    assert ed["accepted"] == 0
    assert all(np.array_equal(v, M.to_f64(it["x"][b])) for b, v in d.state().items())


# ---- whole solves ---------------------------------------------------------------------------------------------
WHOLE = [(name, {}) for name in S.SOLVE_SCENES] + [("no_prior", dict(max_iterations=10))]          # the last one holds rejected steps


@pytest.mark.parametrize("name, params", WHOLE, ids=[w[0] for w in WHOLE])
def test_whole_solve(win, name, params):
    f, m = S.solve_reference(name, **params)
    d = _device(win, name, **params)
    info, log = d.w.solve(), d.w.log()
    seq = [(e["step_kind"], e["accepted"], e["mu_retries"]) for e in log]
    print(f"[win gpu] {name}: device {seq} termination {info['termination']} iterations {info['iterations']}; reference {R.decisions(f)}")
    n = _dim(S.system_reference(name)[1])
    _check(f"{name} initial cost", info["initial_cost"], f["initial_cost"], m["initial_cost"], n * U * float(f["initial_cost"]))
    ok = name in S.admitted() if not params else (R.decisions(f) == R.decisions(m) and R.min_margin(f, m)[0] >= 1000.0)
    if not ok:
        print(f"[win gpu] {name}: not admitted for a decision-sequence comparison (tests/test_win_ref.py names it)")
        return
    assert (seq, info["termination"], info["iterations"]) == R.decisions(f)
    # a cost after an iteration is a function of the steps taken, so its floor carries the step's factor: the condition number
    # of the scaled H + mu D (of the mpmath reference, at the state the solve starts from); the cost before any step does not
    cond = _cond(S.problem(name, R.MP, **params), S.system_reference(name)[1], R.DEFAULTS["initial_mu"])
    print(f"[win gpu] {name}: dim {n}, cond {cond:.3e}")
    _check(f"{name} final cost", info["final_cost"], f["cost"], m["cost"], n * U * cond * float(f["cost"]))
    for ed, ef, em in zip(log, f["log"], m["log"]):
        _check(f"{name} cost after iteration {ed['iteration']}", ed["cost"], ef["cost"], em["cost"], n * U * (cond if ed["iteration"] else 1.0) * float(em["cost"]))


def test_solve_from_the_converged_point_and_zero_iterations(win):
    """`two_frames` to its function tolerance: 25 iterations in mpmath are too slow, so the count and the termination are
    the float64 reference's alone"""
    f, _ = S.solve_reference_f64("two_frames", max_iterations=60)
    assert f["termination"] == R.TERM_FUNCTION
    d = _device(win, "two_frames", max_iterations=60)
    info = d.w.solve()
    print(f"[win gpu] two_frames to convergence: device {info['iterations']} iterations, termination {info['termination']}, cost {info['final_cost']:.12g}; "
          f"reference {f['iterations']}, {f['termination']}, {float(f['cost']):.12g}")
    assert (info["iterations"], info["termination"]) == (f["iterations"], f["termination"])
    assert [e["accepted"] for e in d.w.log()] == [e["accepted"] for e in f["log"]]
    again = d.w.solve()                                     # the description stays: the second solve starts where the first ended
    print(f"[win gpu] restarted at the converged point: {again['iterations']} iteration(s), termination {again['termination']}")
    assert again["iterations"] <= 1 and again["termination"] in (R.TERM_FUNCTION, R.TERM_GRADIENT, R.TERM_PARAMETER)
    d = _device(win, "two_frames", max_iterations=0)
    before = d.state()
    info = d.w.solve()
    ref = S.system_reference("two_frames")[0]
    assert info["iterations"] == 0 and info["termination"] == R.TERM_ITERATIONS and info["initial_cost"] == info["final_cost"]
    assert abs(info["initial_cost"] - float(ref["cost"])) <= _dim(ref) * U * float(ref["cost"])
    assert all(np.array_equal(before[b], v) for b, v in d.state().items()) and len(d.w.log()) == 1


def test_gauge_free_solve(win):
    """without a prior or an IMU factor the gauge is free: the cost, the gradient's max-norm, and what does not depend on the
    gauge (the relative poses q_0^-1 (p_k - p_0), q_0^-1 q_k and the inverse depths) are compared after three iterations.
    Floor: dim x u x cond(scaled H + mu D) x the quantity's size, as for a step"""
    f, m = S.solve_reference("no_prior", max_iterations=3)
    d = _device(win, "no_prior", max_iterations=3)
    info, log = d.w.solve(), d.w.log()
    pm = S.problem("no_prior", R.MP)
    sys_m = S.system_reference("no_prior")[1]
    n, cond = _dim(sys_m), _cond(pm, sys_m, R.DEFAULTS["initial_mu"])
    print(f"[win gpu] no_prior: dim {n}, cond {cond:.3e}")
    _check("no_prior final cost", info["final_cost"], f["cost"], m["cost"], n * U * cond * float(f["cost"]))
    _check("no_prior gradient max-norm", log[-1]["gradient_max_norm"], f["log"][-1]["gradient_max_norm"], m["log"][-1]["gradient_max_norm"],
           n * U * cond * float(m["log"][-1]["gradient_max_norm"]))
    got = d.state()

    def inv(x, X):
        x = {b: X.arr(M.to_f64(v)) if X is R.F64 else v for b, v in x.items()}
        out = [x[b][0] for b in sorted(x) if b >= M.ID_FEATURE]
        q0i = R.qinv(x[M.ID_POSE][3:7], X)
        R0 = M.quat_to_rot(x[M.ID_POSE][3:7], X)
        for k in (1, 2):
            out += list(R0.T @ (x[M.ID_POSE + k][:3] - x[M.ID_POSE][:3]))
            q = R.qmul(q0i, x[M.ID_POSE + k][3:7], X)
            out += list(q if q[3] >= 0 else -q)
        return np.array(out, dtype=object)
    gd, gf, gm = inv(got, R.F64), inv(f["x"], R.F64), inv(m["x"], R.MP)
    _check("no_prior relative poses and inverse depths", M.to_f64(gd), gf, gm, n * U * cond * float(np.abs(M.to_f64(gm)).max()))


# ---- the prior's two routes ---------------------------------------------------------------------------------
def test_prior_routes_give_the_same_bits(pkg, hip, win):
    """a marginalisation on the device (tests/marg_ref.py's `three_td`), then the window over its kept blocks: the prior
    read where it lies and the prior through lvi_marg_get_prior + lvi_win_set_prior give the same bits, and both agree
    with the reference solve over that same prior (the marginalisation's own distance from its reference is DESIGN §21's)"""
    from test_gpu_marg import Device as MargDevice
    sc = M.gpu_scene("three_td")
    marg = pkg.Marginalizer(hip, max_blocks=64, max_projections=64, max_dense_factors=2, max_dense_rows=32, max_drop_dim=64, max_keep_dim=64)
    win2 = pkg.WindowSolver(hip, max_blocks=64, max_projections=64, max_eliminated=16, max_imu=2, max_prior_rows=64, max_dim=64)
    try:
        marg.set_params(**dict(dict(loss_type=M.LOSS_CAUCHY, loss_a=1.0, sqrt_info=M.SQRT_INFO, tr_over_row=0.0, half_row=240.0, eps=M.EPS, max_sweeps=30), **sc["params"]))
        md = M.play(sc, MargDevice(marg))
        assert md.marginalize()["status"] == 0
        lay = marg.layout()
        Jd, rd = marg.prior()
        lo = int(min(lay["idx"]))
        prior = dict(J=Jd, r=rd, ids=[int(b) for b in lay["ids"]], sizes=[int(z) for z in lay["sizes"]], col=[int(c) - lo for c in lay["idx"]], x0=lay["values"])
        rs = np.random.RandomState(3)
        values = {}
        for b, v in zip(lay["ids"], lay["values"]):
            v = np.array(v)
            if len(v) == 7:
                v = np.r_[v[:3] + rs.normal(0, 1e-2, 3), M.quat_mul(v[3:], M.rand_quat(rs, 1e-2))]
            else:
                v = v + rs.normal(0, 1e-3, len(v))
            values[int(b)] = v
        params = dict(sc["params"], max_iterations=4)

        def declare(target):
            for b, v in values.items():
                target.set_block(b, v, 0)
            return target
        states, logs = [], []
        for route, w in (("resident", win), ("host", win2)):
            d = declare(Device(w, **params))
            if route == "resident":
                w.set_prior_from_marg(marg)
            else:
                J, r = marg.prior()
                w.set_prior(J, r, lay["ids"], lay["sizes"], lay["idx"], lay["values"])
            info = w.solve()
            assert info["status"] == 0
            states.append(d.state())
            logs.append([(e["cost"], e["rho"], e["step_norm"], e["accepted"]) for e in w.log()])
        assert logs[0] == logs[1] and all(np.array_equal(states[0][b], states[1][b]) for b in states[0]), "the two routes differ"
        ref = []
        for X in (R.F64, R.MP):
            prob = declare(R.Problem(X, **params))
            prob.set_prior(prior)
            ref.append(R.solve(prob))
        f, m = ref
        n = len(rd)
        print(f"[win gpu] prior routes: same bits; device log costs {[l[0] for l in logs[0]]}; reference {[float(e['cost']) for e in f['log']]}")
        _check("prior routes initial cost", logs[0][0][0], f["initial_cost"], m["initial_cost"], n * U * float(f["initial_cost"]))
        assert [l[3] for l in logs[0]] == [e["accepted"] for e in f["log"]]
        _check("prior routes final cost", logs[0][-1][0], f["cost"], m["cost"], n * U * float(f["initial_cost"]))
        # an undeclared or resized prior block is refused before anything is touched
        w = win2
        w.begin()
        for b, v in list(values.items())[1:]:
            w.set_block(b, v, 0)
        with pytest.raises(pkg.LviError) as e:
            w.set_prior_from_marg(marg)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    finally:
        marg.close()
        win2.close()


# ---- the front end the two handles share --------------------------------------------------------------------
def test_marginaliser_and_window_solve_build_the_same_matrix(pkg, hip, win):
    """One factor set (S.shared_front_scene: 129 projection factors with td and CauchyLoss, one chunk boundary) given to a
    Marginalizer that drops pose 0 and the features, and to a WindowSolver with every block free: A, b and H, g are the same
    sums over the same rows in the same chunk order, so they are the same bits up to the column permutation
    between the two layouts.  The costs are other quantities (sum r'r of the corrected residuals, sum rho / 2)."""
    from test_gpu_marg import Device as MargDevice
    blocks, recs = S.shared_front_scene()
    perm = S.shared_front_permutation(blocks, recs)
    marg = pkg.Marginalizer(hip, max_blocks=160, max_projections=160, max_dense_factors=1, max_dense_rows=1, max_drop_dim=144, max_keep_dim=32)
    try:
        marg.set_params(loss_type=M.LOSS_CAUCHY, loss_a=1.0, sqrt_info=M.SQRT_INFO, tr_over_row=0.0, half_row=240.0, eps=M.EPS, max_sweeps=30)
        md, wd = MargDevice(marg), Device(win)
        for b, v in blocks:
            md.set_block(b, v)
            wd.set_block(b, v, 0)
        for rec in recs:
            md.add_projection(rec)
            wd.add_projection(rec)
        info = md.marginalize()
        A, b = marg.debug_system()
    finally:
        marg.close()
    dev = wd.flush().w.debug_system()
    assert info["status"] != pkg.marg.NOT_FINITE and (info["m"], info["n"]) == (135, 19) and dev["status"] == 0 and dev["H"].shape == (154, 154)
    Ap, bp = A[np.ix_(perm, perm)], b[perm]
    print(f"[win gpu] shared front end: {len(recs)} factors, m {info['m']} n {info['n']} D {len(bp)}; entries of A that differ from H {int((Ap != dev['H']).sum())}, "
          f"of b from g {int((bp != dev['g']).sum())}; ||A|| {np.linalg.norm(A, 2):.3e}")
    assert np.array_equal(Ap, dev["H"]) and np.array_equal(bp, dev["g"])


# ---- other cases -----------------------------------------------------------------------------------------------
def test_second_run_gives_the_same_bits(win):
    runs = []
    for _ in range(2):
        d = _device(win, "eleven_frames", max_iterations=3)
        info = d.w.solve()
        runs.append((info["final_cost"], [tuple(sorted(e.items())) for e in d.w.log()], d.state()))
    print(f"[win gpu] eleven_frames twice: final cost {runs[0][0]!r} and {runs[1][0]!r}, {len(runs[0][1]) - 1} iterations")
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(np.array_equal(runs[0][2][b], runs[1][2][b]) for b in runs[0][2])


def test_eleven_frames_first_step_against_float64(win):
    """D = 172: mpmath is too slow, so float64 at the floor alone (n u cond x the value)"""
    p = S.problem("eleven_frames", R.F64, max_iterations=1)
    f = R.solve(p)
    d = _device(win, "eleven_frames", max_iterations=1)
    info, log = d.w.solve(), d.w.log()
    sys = S.system_reference("eleven_frames")[0]
    Sf, _, _ = R.Strategy(p, sys).reduced(f["log"][1]["mu"])
    cond, n = float(np.linalg.cond(Sf)), sys["D"] + sys["E"]
    ed, ef = log[1], f["log"][1]
    print(f"[win gpu] eleven_frames first step: device kind {ed['step_kind']} accepted {ed['accepted']}, reference {ef['step_kind']} {ef['accepted']}; cond {cond:.3e}")
    assert (ed["step_kind"], ed["accepted"]) == (ef["step_kind"], ef["accepted"]) and info["dim"] == 172
    for key in ("gauss_newton_norm", "cauchy_norm", "step_norm", "model_cost_change"):
        _check(f"eleven_frames {key}", ed[key], ef[key], None, n * U * cond * abs(float(ef[key])))
    _check("eleven_frames cost", ed["cost"], ef["cost"], None, n * U * (float(f["initial_cost"]) + cond * abs(float(ef["model_cost_change"]))))


def test_zero_inverse_depth_is_not_finite_and_leaves_the_blocks(pkg, win):
    d = _device(win, "zero_depth")
    before = d.state()
    info = d.w.solve()
    assert info["status"] == pkg.win.NOT_FINITE and info["flags"] & 1
    assert all(np.array_equal(before[b], v) for b, v in d.state().items())
    # a covariance that is not positive definite has a status of its own
    sc = S.scene("two_frames")
    d = Device(win, **sc["params"])
    for op in sc["ops"]:
        if op[0] == "imu":
            op = ("imu", dict(op[1], covariance=-op[1]["covariance"]))
        S.play(dict(ops=[op]), d)
    d.flush()
    before = d.state()
    info = d.w.solve()
    assert info["status"] == pkg.win.BAD_COVARIANCE and info["flags"] & 2
    assert all(np.array_equal(before[b], v) for b, v in d.state().items())
    d = _device(win, "two_frames", max_iterations=2)            # the handle is usable afterwards
    info = d.w.solve()
    f, _ = S.solve_reference("two_frames")
    assert info["status"] == 0 and [e["accepted"] for e in d.w.log()] == [e["accepted"] for e in f["log"][:3]]


def test_errors_leave_the_description_as_it_was(pkg, hip, win):
    E = pkg._abi
    d = _device(win, "two_frames", max_iterations=2)
    want = d.w.debug_system()

    def refused(code, fn, *a, **k):
        with pytest.raises(pkg.LviError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, code)
    w = d.w
    refused(E.LVI_ERR_INVALID_ARG, w.set_block, M.ID_POSE, np.zeros(9))                       # another size
    refused(E.LVI_ERR_INVALID_ARG, w.set_block, M.ID_POSE, np.r_[np.zeros(6), 1.0], pkg.win.CONSTANT)   # other flags
    refused(E.LVI_ERR_INVALID_ARG, w.set_block, 900, np.zeros(2), pkg.win.ELIMINATED)         # only a scalar is eliminated
    refused(E.LVI_ERR_INVALID_ARG, w.set_block, 901, [np.nan])
    rec = np.zeros(1, w.record_dtype)
    rec[0]["pose_i"], rec[0]["pose_j"], rec[0]["ex"], rec[0]["feature"], rec[0]["td"] = M.ID_POSE, M.ID_POSE + 1, M.ID_EX, 12345, -1
    refused(E.LVI_ERR_INVALID_ARG, w.add_projection, rec)                                     # an undeclared feature
    rec[0]["feature"], rec[0]["ex"] = M.ID_FEATURE, M.ID_FEATURE + 1
    refused(E.LVI_ERR_INVALID_ARG, w.add_projection, rec)                                     # an eliminated block outside the feature slot
    imu = np.zeros(1, w.imu_dtype)
    imu[0]["pose_i"], imu[0]["speed_bias_i"], imu[0]["pose_j"], imu[0]["speed_bias_j"] = M.ID_POSE, M.ID_SPEEDBIAS, M.ID_POSE, M.ID_SPEEDBIAS + 1
    refused(E.LVI_ERR_INVALID_ARG, w.add_imu, imu)                                            # one block twice
    refused(E.LVI_ERR_CAPACITY, w.add_projection, np.zeros(600, w.record_dtype))
    refused(E.LVI_ERR_INVALID_ARG, w.set_params, max_iterations=65)
    refused(E.LVI_ERR_INVALID_ARG, w.set_prior, np.eye(6), np.zeros(6), [777], [7], [0], [np.r_[np.zeros(6), 1.0]])   # an undeclared prior block
    pose, sb = w.block(M.ID_POSE), w.block(M.ID_SPEEDBIAS)
    refused(E.LVI_ERR_INVALID_ARG, w.set_prior, np.eye(15), np.zeros(15), [M.ID_POSE, M.ID_SPEEDBIAS], [7, 9], [0, 3], [pose, sb])   # overlapping columns
    got = w.debug_system()
    assert all(np.array_equal(got[k], want[k]) for k in ("H", "g", "W", "hdiag", "gf", "dense", "proj_rows")) and got["cost"] == want["cost"]
    small = pkg.WindowSolver(hip, max_blocks=64, max_projections=64, max_eliminated=2, max_imu=2, max_prior_rows=64, max_dim=20)
    try:
        ds = Device(small)
        sc = S.scene("two_frames")
        with pytest.raises(pkg.LviError) as e:
            S.play(sc, ds)
        assert e.value.code == E.LVI_ERR_CAPACITY                                             # the third eliminated block
        small.begin()
        for op in sc["ops"]:
            if op[0] == "block" and op[1] < M.ID_FEATURE:
                small.set_block(op[1], op[2], op[3])
            elif op[0] == "prior":
                ds.set_prior(op[1])
        refused(E.LVI_ERR_CAPACITY, small.solve)                                              # D = 37 beyond max_dim = 20
    finally:
        small.close()


# ---- the host mirror -------------------------------------------------------------------------------------------
def _vins_problem(d, win, feats, estimate_td, estimate_extrinsic, lidar=()):
    """estimator.cpp:698-789 restated over a Device: the blocks, the feature filter and feature_index, the records"""
    W = M.WINDOW_SIZE
    for k in range(W + 1):
        d.set_block(M.ID_POSE + k, win["pose"][k], 0)
        d.set_block(M.ID_SPEEDBIAS + k, win["speed_bias"][k], 0)
    d.set_block(M.ID_EX, win["ex"], 0 if estimate_extrinsic else R.CONSTANT)
    if estimate_td:
        d.set_block(M.ID_TD, [win["td"]], 0)
    index, where = -1, {}
    for n, f in enumerate(feats):
        if not (len(f["obs"]) >= 2 and f["start_frame"] < W - 2):
            continue
        index += 1
        where[n] = M.ID_FEATURE + index
        d.set_block(M.ID_FEATURE + index, [f["inv_dep"]], R.CONSTANT if n in lidar else R.ELIMINATED)
        for j, o in enumerate(f["obs"][1:], f["start_frame"] + 1):
            d.add_projection(M._rec(M.ID_POSE + f["start_frame"], M.ID_POSE + j, M.ID_FEATURE + index, f["obs"][0], o, M.ID_TD if estimate_td else -1))
    return where


def test_host_mirror_optimize_marginalize_optimize(pkg, hip, win):
    """VinsWindowOptimizer over a VinsMarginalizer's arrays: optimize, marginalize (MARGIN_OLD), optimize with the resident
    prior.  Each optimize gives the bits of the same problem declared through the Python binding, the second one with the
    prior taken from the same marginaliser's handle; a lidar feature and the constant extrinsic keep their values."""
    H = pkg.host_api
    hl = pkg.load_host()
    steps = M.chain_steps()
    V = H.VinsMarginalizer(hl, hip, max_features=16, estimate_td=True)
    O = H.VinsWindowOptimizer(hl, hip, V, max_features=16, estimate_extrinsic=0, num_iterations=6, solver_time=0.0)
    try:
        lidar = (1,)
        # pre_integrations[2] is a real record (its ids are the mirror's to fill in); pre_integrations[1] has sum_dt > 10 and is
        # skipped (estimator.cpp:740); the other intervals have none
        pre = dict([op[1] for op in S.scene("three_td")["ops"] if op[0] == "imu"][0])
        rec = np.zeros(1, win.imu_dtype)
        for key, v in pre.items():
            rec[0][key] = v
        rec[0]["pose_i"] = rec[0]["speed_bias_i"] = rec[0]["pose_j"] = rec[0]["speed_bias_j"] = -7
        O.set_imu(2, rec)
        late = rec.copy()
        late[0]["sum_dt"] = 10.5
        O.set_imu(1, late)
        for k, (flag, w0, feats, imu) in enumerate((steps[0], steps[2])):
            V.set_window(w0["pose"], w0["speed_bias"], w0["ex"], w0["td"])
            V.set_features(feats)
            flags = np.zeros(len(feats), np.int32)
            flags[list(lidar)] = 1
            O.set_lidar_flags(flags)
            d = Device(win, max_iterations=6)
            where = _vins_problem(d, w0, feats, True, 0, lidar)
            d.flush()
            d.add_imu(dict(pre, pose_i=M.ID_POSE + 1, speed_bias_i=M.ID_SPEEDBIAS + 1, pose_j=M.ID_POSE + 2, speed_bias_j=M.ID_SPEEDBIAS + 2))
            if k == 1:
                win.set_prior_from_marg(V.marg)
            want = win.solve()
            got = O.optimize(flag)
            out = O.window()
            print(f"[win gpu] host mirror step {k}: steps {[(e['step_kind'], e['accepted']) for e in win.log()]}")
            print(f"[win gpu] host mirror step {k}: cost {got['initial_cost']:.6g} -> {got['final_cost']:.6g} in {got['iterations']} iterations; "
                  f"binding {want['initial_cost']:.6g} -> {want['final_cost']:.6g}")
            assert got["status"] == 0 and (got["initial_cost"], got["final_cost"], got["iterations"], got["termination"], got["dim"], got["eliminated"]) == \
                (want["initial_cost"], want["final_cost"], want["iterations"], want["termination"], want["dim"], want["eliminated"])
            # step 0 has no prior: the gauge is free and nothing is asserted about its progress
            assert got["final_cost"] <= got["initial_cost"] and got["dim"] == 11 * 15 + 1 and (k == 0 or got["final_cost"] < got["initial_cost"])
            for j in range(M.WINDOW_SIZE + 1):
                assert np.array_equal(out["pose"][j], win.block(M.ID_POSE + j)) and np.array_equal(out["speed_bias"][j], win.block(M.ID_SPEEDBIAS + j))
            assert np.array_equal(out["ex_pose"], w0["ex"]) and out["td"] == win.block(M.ID_TD)[0]
            for n, bid in where.items():
                assert out["inv_dep"][n] == win.block(bid)[0]
            assert out["inv_dep"][1] == feats[1]["inv_dep"]
            if k == 0:
                # the marginalisation that follows works on the optimised window, as the reference's does
                V.set_imu(0.5, imu["residual"], imu["jacobians"])
                assert V.run(flag)["ran"]
    finally:
        O.close()
        V.close()


# ---- the chain -------------------------------------------------------------------------------------------------
def _window_of(x, where, feats):
    W = M.WINDOW_SIZE
    win = dict(pose=np.array([M.to_f64(x[M.ID_POSE + j]) for j in range(W + 1)]), speed_bias=np.array([M.to_f64(x[M.ID_SPEEDBIAS + j]) for j in range(W + 1)]),
               ex=M.to_f64(x[M.ID_EX]), td=float(x[M.ID_TD][0]))
    return win, [dict(f, inv_dep=float(x[where[n]][0])) if n in where else f for n, f in enumerate(feats)]


def test_three_step_chain_of_optimize_and_marginalize(pkg, hip, win):
    """M.chain_steps(): optimize + marginalize three times (MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_OLD), every marginalisation
    on the window the solve before it left.  At every step the prior read where it lies (lvi_win_set_prior_from_marg, after
    the remaps and the buffer swaps of the marginalisations before) and the prior through lvi_marg_get_prior + lvi_win_set_prior
    give the same bits, and the chain agrees with the float64 chain of tests/win_ref.py + tests/marg_ref.py: the decisions, and
    the costs at dim x u x cond x the step's initial cost (D = 172: mpmath is too slow, so float64 at the floor alone; the
    initial cost of steps 1 and 2 is the chained prior evaluated at the new window)."""
    H = pkg.host_api
    V = H.VinsMarginalizer(pkg.load_host(), hip, max_features=16, estimate_td=True)
    win2 = pkg.WindowSolver(hip, max_blocks=256, max_projections=512, max_eliminated=32, max_imu=2, max_prior_rows=128, max_dim=192)
    prior_ref, flags = None, []
    try:
        for k, (flag, w0, feats, imu) in enumerate(M.chain_steps()):
            flags.append(flag)
            runs = []
            for route, w in (("resident", win), ("host", win2)):
                d = Device(w, max_iterations=3)
                where = _vins_problem(d, w0, feats, True, 1)
                d.flush()
                if k > 0 and route == "resident":
                    w.set_prior_from_marg(V.marg)
                elif k > 0:
                    J, r = V.marg.prior()
                    lay = V.marg.layout()
                    w.set_prior(J, r, lay["ids"], lay["sizes"], lay["idx"], lay["values"])
                info = w.solve()
                assert info["status"] == 0
                runs.append((info, [tuple(sorted(e.items())) for e in w.log()], d.state()))
            (ia, la, xa), (ib, lb, xb) = runs
            assert la == lb and (ia["initial_cost"], ia["final_cost"], ia["iterations"], ia["termination"]) == (ib["initial_cost"], ib["final_cost"], ib["iterations"], ib["termination"])
            assert all(np.array_equal(xa[b], xb[b]) for b in xa), f"step {k}: the two prior routes differ"
            prob = R.Problem(R.F64, max_iterations=3)
            _vins_problem(prob, w0, feats, True, 1)
            if prior_ref is not None:
                prob.set_prior(prior_ref)
            f = R.solve(prob)
            sys = prob.system(prob.x0())
            n, cond = _dim(sys), _cond(prob, sys, R.DEFAULTS["initial_mu"])
            seq = [(e["step_kind"], e["accepted"], e["mu_retries"]) for e in win.log()]
            print(f"[win gpu] chain step {k} (flag {flag}): device {seq} termination {ia['termination']}; reference {R.decisions(f)}; dim {n} cond {cond:.3e}")
            floor = n * U * cond * float(f["initial_cost"])
            _check(f"chain step {k} initial cost", ia["initial_cost"], f["initial_cost"], None, floor)
            assert (seq, ia["termination"], ia["iterations"]) == R.decisions(f)
            _check(f"chain step {k} final cost", ia["final_cost"], f["cost"], None, floor)
            wd, fd = _window_of(xa, where, feats)
            V.set_window(wd["pose"], wd["speed_bias"], wd["ex"], wd["td"])
            V.set_features(fd)
            V.set_imu(0.5, *((imu["residual"], imu["jacobians"]) if imu else (None, None)))
            assert V.run(flag)["ran"]
            wr, fr = _window_of(f["x"], where, feats)
            prior_ref = M.vins_marginalize(M.F64, prior_ref, flag, wr, fr, imu)
            assert sorted(int(b) for b in V.marg.layout()["ids"]) == sorted(prior_ref["ids"])
        assert flags == [M.MARGIN_OLD, M.MARGIN_SECOND_NEW, M.MARGIN_OLD]
    finally:
        win2.close()
        V.close()
