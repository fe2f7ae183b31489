"""CPU tier: the float64 reference of the end of a Gauss-Newton iteration (tests/step_ref.py) against known answers, then
the ORACLE alone against it on every scene of tests/step_scenes.py: the scenes' preconditions (a degenerate frame really is
one, the threshold family really straddles 100), the step of every recorded iteration, the flags, the zero step of the
shadowed matP.  What the oracle deviates by here is the yardstick of tests/test_gpu_step.py.

Bar for the oracle's step (float32 Householder QR, float32 Jacobi, float32 pose) against float64: a backward-stable solve
errs along eigenvector i by about eps * lambda_max / lambda_i * |X|; after the projection only the kept eigenvectors
(lambda_i >= 100; all of them on a non-degenerate frame) remain, and a Jacobi eigenvector is off by about
eps * lambda_max / (spectral gap) times the removed component, the gap being at least lambda_kept_min - lambda_removed_max.
With eps = 2^-24 and a constant of 8 for the 6 x 6 sums of both:
    bar = 8 eps (lambda_max / lambda_kept_min) |X|_inf  +  8 eps (lambda_max / gap) proj_gap  +  2 U
U = the float32 spacing at the pose component the step is added to (the trace holds rounded poses).  Measured on the
corridor family: <= 2e-8, some 100 times inside the bar; a skipped or garbled projection misses by proj_gap >= 1e-3."""
import numpy as np
import pytest

import step_ref
import step_scenes as S

EPS = 2.0 ** -24


# ----------------------------------------------------------------------------- step_ref against known answers
def test_tri_index_is_row_major_upper_triangle():
    want = [(r, c) for r in range(6) for c in range(r, 6)]
    assert [step_ref.tri_index(r, c) for r, c in want] == list(range(21))
    A = np.arange(36, dtype=np.float64).reshape(6, 6); A = A + A.T
    b = np.arange(6) + 0.5
    A2, b2 = step_ref.unpack(step_ref.pack(A, b))
    np.testing.assert_array_equal(A2, A); np.testing.assert_array_equal(b2, b)


def test_diagonal_threshold_is_strict():
    """eigenvalue 99.999 is dropped, 100.001 is kept (matE < eignThre, :1277)"""
    d = np.array([500.0, 99.999, 100.001, 300.0, 1000.0, 2000.0])
    b = np.array([5.0, 7.0, -3.0, 30.0, 10.0, -20.0])
    s = step_ref.gn_step(step_ref.pack(np.diag(d), b), 0)
    want = b / d
    want[1] = 0.0
    np.testing.assert_allclose(s.step, want, rtol=0, atol=1e-15)
    assert s.degenerate and not s.converged
    assert s.proj_gap == pytest.approx(7.0 / 99.999, rel=1e-12)
    np.testing.assert_allclose(s.eigenvalues, np.sort(d), rtol=1e-14)
    d[1] = 100.0                                                   # exactly 100 is NOT below the threshold
    s = step_ref.gn_step(step_ref.pack(np.diag(d), b), 0)
    assert not s.degenerate and s.proj_gap == 0.0
    np.testing.assert_allclose(s.step, b / d, rtol=1e-15)


def test_rotated_deficient_matrix_drops_its_null_vector():
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]); w /= np.linalg.norm(w)
    Q = np.eye(6) - 2.0 * np.outer(w, w)                           # Householder reflection: orthogonal, columns = eigenvectors
    d = np.array([0.5, 150.0, 400.0, 1000.0, 5000.0, 9000.0])
    A = Q @ np.diag(d) @ Q.T
    u = Q[:, 0]                                                    # the direction the data do not constrain
    y = Q[:, 1:] @ np.array([0.01, -0.02, 0.03, 0.004, -0.005])    # a step orthogonal to u
    s = step_ref.gn_step(step_ref.pack(A, A @ (y + 7.0 * u)), 0)
    assert s.degenerate
    np.testing.assert_allclose(s.X, y + 7.0 * u, atol=1e-10)
    np.testing.assert_allclose(s.step, y, atol=1e-10)
    assert abs(u @ s.step) < 1e-10
    assert s.proj_gap == pytest.approx(7.0 * np.abs(u).max(), rel=1e-9)
    # two directions below the threshold: rank-4 projector
    d[1] = 60.0
    A = Q @ np.diag(d) @ Q.T
    s = step_ref.gn_step(step_ref.pack(A, A @ (y + 7.0 * u)), 0)
    np.testing.assert_allclose(s.step, y - Q[:, 1] * 0.01, atol=1e-10)
    assert int((s.eigenvalues < 100).sum()) == 2


def test_iterations_after_the_first_of_a_degenerate_frame_do_not_move():
    d = np.array([500.0, 200.0, 300.0, 300.0, 1000.0, 2000.0])
    b = np.array([5.0, 7.0, -3.0, 30.0, 10.0, -20.0])
    rec = step_ref.pack(np.diag(d), b)
    s = step_ref.gn_step(rec, 1, degenerate_in=True)
    np.testing.assert_array_equal(s.step, np.zeros(6))
    assert s.degenerate and s.converged and s.delta_r == 0.0 and s.delta_t == 0.0
    s = step_ref.gn_step(rec, 1, degenerate_in=False)
    np.testing.assert_allclose(s.step, b / d, rtol=1e-15)
    assert not s.degenerate and not s.converged
    # the eigenvalues of a later iteration decide nothing (:1262 `if (iterCount == 0)`)
    d[0] = 1.0
    assert not step_ref.gn_step(step_ref.pack(np.diag(d), b), 3, degenerate_in=False).degenerate


def test_convergence_thresholds():
    """deltaR = |X[0:3] * 57.29578| [deg], deltaT = |X[3:6] * 100| [cm], both < 0.05 (:1303-1311)"""
    d = np.full(6, 1000.0)
    for x, conv in ((0.049 / 57.29578, True), (0.051 / 57.29578, False)):
        s = step_ref.gn_step(step_ref.pack(np.diag(d), d * np.array([x, 0, 0, 0, 0, 0])), 0)
        assert s.converged == conv
    for x, conv in ((0.049 / 100, True), (0.051 / 100, False)):
        s = step_ref.gn_step(step_ref.pack(np.diag(d), d * np.array([0, 0, 0, 0, x, 0])), 0)
        assert s.converged == conv
    steps, deg, conv, iters = step_ref.replay(np.concatenate([step_ref.pack(np.diag(d), d * 0.01), step_ref.pack(np.diag(d), d * 1e-6),
                                                              step_ref.pack(np.diag(d), d * 1e-7)]))
    assert (deg, conv, iters) == (False, True, 2)


# ----------------------------------------------------------------------------- the oracle on every scene
def step_bar(s, pose_before):
    """the docstring's bar for one recorded iteration: (rotation, translation)"""
    w = s.eigenvalues
    kept = w[w >= step_ref.EIG_THRESHOLD] if s.degenerate else w
    if len(kept) == 0 or not np.abs(s.step).any():                # the zero step is exact
        return 0.0, 0.0
    solve = 8 * EPS * (w[-1] / kept[0]) * np.abs(s.X).max()
    removed = w[w < step_ref.EIG_THRESHOLD]
    proj = 8 * EPS * (w[-1] / (kept[0] - removed[-1])) * s.proj_gap if s.degenerate and len(removed) else 0.0
    u = [2 * max(step_ref.f32_spacing(v) for v in part) for part in (pose_before[:3], pose_before[3:])]
    return solve + proj + u[0], solve + proj + u[1]


@pytest.fixture(scope="module", params=S.SCENE_NAMES)
def scene(request, pkg, oracle):
    return S.get(request.param, pkg, oracle)


@pytest.fixture(scope="module")
def runs(scene, pkg, oracle):
    """the oracle's two matches of the scene (break enabled / six iterations without the break), computed once"""
    return {k: S.run(pkg, oracle, scene, **kw) for k, kw in S.BREAK_SETTINGS.items()}


@pytest.mark.parametrize("mode", list(S.BREAK_SETTINGS))
def test_oracle_meets_the_scene_preconditions(scene, runs, mode):
    r = runs[mode]
    S.check_preconditions(scene, r)
    if scene["name"] == "slab":
        assert r["n_corner_ds"] > 10 and r["n_sel"][0] == r["n_surf_ds"]          # the gate passes, no corner row is selected
    # the convergence verdict of every iteration is decidable: no delta within 2 % of 0.05
    for s in S.step_errors(r)[2]:
        assert abs(s.delta_r - 0.05) > 1e-3 and abs(s.delta_t - 0.05) > 1e-3, (s.delta_r, s.delta_t)


@pytest.mark.parametrize("mode", list(S.BREAK_SETTINGS))
def test_oracle_step_against_float64(scene, runs, mode):
    r = runs[mode]
    er, et, steps, _ = S.step_errors(r)
    worst = [0.0, 0.0]
    for i, s in enumerate(steps):
        bar = step_bar(s, np.maximum(np.abs(r["trace"][i]), np.abs(r["trace"][i + 1])))
        print(f"{scene['name']} {mode} iter {i}: E_rot {er[i].max():.3e} (bar {bar[0]:.3e})  E_trans {et[i].max():.3e} (bar {bar[1]:.3e})")
        assert er[i].max() <= bar[0] and et[i].max() <= bar[1], (scene["name"], i, er[i], et[i], bar)
        worst = [max(worst[0], er[i].max()), max(worst[1], et[i].max())]
    print(f"{scene['name']} {mode}: E_orc rot {worst[0]:.3e} trans {worst[1]:.3e}  lambda_min {steps[0].eigenvalues[0]:.3f}")


@pytest.mark.parametrize("mode", list(S.BREAK_SETTINGS))
def test_oracle_flags_and_the_zero_step(scene, runs, mode):
    r = runs[mode]
    steps, degenerate, converged, iters = step_ref.replay(r["jtj"], break_enabled=(mode == "break"))
    assert (r["degenerate"], r["converged"], r["iters"]) == (degenerate, converged, iters)
    assert r["degenerate"] == scene["expect"]["degenerate"]
    if mode == "nobreak":
        assert r["iters"] == 6
    if degenerate:
        t = r["trace"].view(np.uint32)
        assert (t[1:] == t[1]).all(), "iterations >= 1 of a degenerate frame must not move the pose by a bit"
        assert (t[1] != t[0]).any()
        np.testing.assert_array_equal(r["pose"].view(np.uint32), t[1])          # the tolerances of transformUpdate are far away
        if mode == "break":
            assert r["iters"] == 2
    else:
        assert r["iters"] >= 3 and np.abs(r["trace"][2] - r["trace"][1]).max() > 0
