"""CPU tests of tests/step_ref.py, the reference of tests/test_gpu_step_stages.py: that its
block-sparse reduction and back-substitution are the dense step, that its float64 restatement's
floors stay under the caps the GPU test holds them to on every input it uses, and that its
measures see the errors the stage checks exist for."""
import numpy as np
import pytest

import step_ref as sr


def _sets(P, lm=None, g=None):
    """e-sets to reduce by: every free capture; every free tag; with lm, Ceres' mixed set."""
    free = P.free[3:].reshape(-1, 6)[:, 0]
    caps = free & (np.arange(P.nc + P.nt) < P.nc)
    out = {"captures": caps, "tags": free & ~(np.arange(P.nc + P.nt) < P.nc)}
    if lm is not None:
        m = lm.debug_mixed_groups(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag)
        out["mixed"] = free & np.concatenate([m["e_cap"], m["e_tag"]]).astype(bool)
    return out


def _state(oracle, name):
    P = sr.spec_problem(oracle, name)
    R = sr.Rows(P)
    g, cn, rr = sr.sums(R)
    g64, cn64, _ = sr.sums(R, np.float64)
    return P, R, (g, cn, rr), sr.scale_diag(P, cn), sr.scale_diag(P, cn64, dtype=np.float64)


def test_rows_are_the_dense_reference_rows(oracle):
    """Rows is tag_size_ref._Problem.linearize by observation, bit for bit, and its sums in
    float64 are J'r and the column norms of that dense Jacobian to rounding."""
    P = sr.spec_problem(oracle, "small_cauchy")
    R = sr.Rows(P)
    _, J, r, _ = P.linearize(P.x0)
    for i in range(len(R.obs)):
        assert np.array_equal(J[8 * i:8 * i + 8][:, R.cols[i]], R.J[i]) and np.array_equal(r[8 * i:8 * i + 8], R.r[i])
    g, cn, rr = sr.sums(R)
    np.testing.assert_allclose(np.asarray(g, np.float64), J.T @ r, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(np.asarray(cn, np.float64), np.sum(J * J, axis=0), rtol=1e-12)
    assert R.wrel.max() > 0 and sr.Rows(sr.spec_problem(oracle, "small")).wrel.max() == 0


@pytest.mark.parametrize("radius", [1e-2, 1e4])
@pytest.mark.parametrize("name", ["k1to11_const", "small", "g20_radial_est", "pair70"])
def test_reduction_and_back_substitution_are_the_dense_step(oracle, name, radius):
    """Reduce, solve S y = rhs, back-substitute, all in long double: z = -d / s solves the whole
    H z = b (H = Js'Js + D^2 over every free slot) to the backward error of a Cholesky solve.

    Bound.  The elimination is a block Cholesky of H, so (Higham, Accuracy and Stability, Thm 10.4
    with || |L||L'| || <= n ||H||) the computed z satisfies (H + dH) z = b with
    ||dH|| <= n gamma_{3n+1} ||H||, gamma_k ~ k u, u = 2^-64: the normwise backward error
    eta = ||H z - b|| / (||H|| ||z|| + ||b||) (infinity norms) is at most n (3 n + 1) 2^-64.
    The dense long-double solve of the same H (tag_size_ref._chol_solve's algorithm) is held to
    the same bound; both measure a few 1e-19.  A wrong sign of W y gives 1e-2 (below)."""
    P, R, _, (s, d), _ = _state(oracle, name)
    for label, elim in _sets(P).items():
        red = sr.reduce(R, elim, s, d, radius, True)
        y = sr._chol_solve(sr._chol(red.S), red.rhs)
        st = sr.back_substitute(R, red, y, s, True)
        fi, H, b, y_dense = sr.dense_step(R, s, d, radius)
        z = -st.delta[fi] / s[fi]
        n = len(fi)
        bound = n * (3 * n + 1) * sr.ULD

        def eta(v):
            return float(np.max(np.abs(H @ v - b)) / (np.max(np.sum(np.abs(H), axis=1)) * np.max(np.abs(v)) +
                                                       np.max(np.abs(b))))
        print(f"step_ref: {name} {label} r={radius:g} n={n} eta {eta(z):.1e} dense {eta(y_dense):.1e} bound {bound:.1e}")
        assert eta(z) <= bound and eta(y_dense) <= bound
        # ... and the two steps agree as far as H's condition lets two backward-stable solves
        assert float(np.max(np.abs(z - y_dense)) / np.max(np.abs(y_dense))) <= 1e-6
        # the model change is the dense one: -Js d . (r + Js d / 2) = z'b - z'(H - D^2) z / 2
        D2 = np.asarray(d, sr.LD)[fi] / sr.LD(radius)
        dense_model = z @ b - (z @ (H @ z) - z @ (D2 * z)) / 2
        assert abs(float(st.model - dense_model)) <= 1e-15 * abs(float(dense_model))


@pytest.mark.parametrize("name", sorted(sr.INPUT_RADII))
def test_restatement_floors_stay_under_the_caps(oracle, name):
    """The float64 restatement's own error against the long-double reduction, by the H-normalised
    measure, on every input of the GPU test at every radius it runs there, by captures and, where
    the GPU test eliminates them (`small`), by tags: at most step_ref.CAPS (5e-15, 1e-12, 1e-9 at
    radius 1e-2, 1e4, 1e16)."""
    P, R, _, (s, d), (s64, d64) = _state(oracle, name)
    for label, elim in _sets(P).items():
        if label == "tags" and name != "small":
            continue
        for radius in sr.INPUT_RADII[name]:
            ref = sr.reduce(R, elim, s, d, radius, True)
            r64 = sr.reduce(R, elim, s64, d64, radius, False)
            eS, er = sr.errors(r64.S, r64.rhs, ref)
            print(f"step_ref: {name} {label} r={radius:g} nf={len(ref.slots)} floor S {eS:.1e} rhs {er:.1e}")
            assert eS <= sr.CAPS[radius]


def test_mixed_set_floors(oracle):
    """The same on `small` by Ceres' mixed e-set (direct residuals: plain normal blocks)."""
    from ar_slam_amd import lm
    P, R, _, (s, d), (s64, d64) = _state(oracle, "small")
    elim = _sets(P, lm, sr.spec("small")["g"])["mixed"]
    assert elim[:P.nc].any() and elim[P.nc:].any()
    groups, _ = sr._groups(R, elim, s, sr.LD)
    assert any(g.e is None for g in groups), "no direct residuals"
    for radius in sr.ALL_RADII:
        ref = sr.reduce(R, elim, s, d, radius, True)
        r64 = sr.reduce(R, elim, s64, d64, radius, False)
        assert sr.errors(r64.S, r64.rhs, ref)[0] <= sr.CAPS[radius]


def test_the_measures_see_a_wrong_restatement(oracle):
    """What the stage checks exist for, done to the restatement on purpose (numpy only): one
    contribution of a split destination dropped -- capture 69 of pair70's 70, the last piece of
    the first tag's diagonal block -- and the sign of W y flipped in the back-substitution.
    Either is many orders over the rule's bound, 16 max(floor, 2.3e-16)."""
    P, R, _, (s, d), (s64, d64) = _state(oracle, "pair70")
    elim = _sets(P)["captures"]
    for radius in (1e-2, 1e4):
        ref = sr.reduce(R, elim, s, d, radius, True)
        good = sr.reduce(R, elim, s64, d64, radius, False)
        bad = sr.reduce(R, elim, s64, d64, radius, False, drop=(69, 3, 9))
        bound = 16 * max(sr.errors(good.S, good.rhs, ref)[0], sr.FLOOR)
        e_bad = sr.errors(bad.S, bad.rhs, ref)[0]
        print(f"step_ref: dropped contribution r={radius:g} e_S {e_bad:.1e} bound {bound:.1e}")
        assert e_bad > 1e6 * bound
        y = sr._chol_solve(sr._chol(ref.S), ref.rhs)
        st = sr.back_substitute(R, ref, y, s, True)
        st64 = sr.back_substitute(R, good, np.asarray(y, np.float64), s64, False)
        flip = sr.back_substitute(R, good, np.asarray(y, np.float64), s64, False, flip_wy=True)
        e = [float(np.sqrt(np.sum((v.delta - st.delta) ** 2) / np.sum(st.delta ** 2))) for v in (st64, flip)]
        print(f"step_ref: flipped W y r={radius:g} step error {e[1]:.1e} against {e[0]:.1e}")
        assert e[1] > 1e6 * 16 * max(e[0], sr.FLOOR)
        assert abs(float(flip.model - st.model)) > 1e6 * 16 * max(abs(float(st64.model - st.model)), sr.FLOOR * abs(float(st.model)))
