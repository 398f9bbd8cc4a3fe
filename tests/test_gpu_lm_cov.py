"""GPU tests of the LM solver's marginal covariances (arslam_lm_covariance, include/arslam_lm.h)
and of the selected inverse behind them (arslam_debug_selinv), against the numpy restatement of
their definition in tests/lm_cov_ref.py.

The parity reference is evaluated at the parameters the device returned, with the Jacobi scale of
the initial ones (the scale the handle keeps), so the two differ by rounding alone.
  * |C_dev - C_ref|_ij <= tol sqrt(C_ref,ii C_ref,jj), tol = 16 e_ref of that input, not below
    1e-10.  The device factors the reduced system's normal equations (Cholesky), as the
    reference's route 1 does the whole system's, in another summation order; e_ref is route 1's
    disagreement with the QR route, so it measures that error class on the input, and the factor
    16 is room for the order.  A wrong term is O(1).  Every input is
    asserted to have e_ref <= 1e-9 and min_pivot >= 1e-5 (tests/test_lm_cov.py's caps; min_pivot
    in the reference's own elimination order).
  * min_pivot within 1e-10 of the reference's scaled Cholesky in the device's elimination order.
  * statuses equal; every block exactly symmetric.

Measured on an MI355X (each case prints its figures; profiles/lm_cov/device_errors.txt):
  * the selected inverse alone: <= 1.6e-15 of sqrt(Z_ii Z_jj);
  * min_pivot: equal to the reference in every printed digit;
  * capture elimination: 1e-13 .. 3.3e-11, 10 to 100 times below e_ref (the device eliminates by
    an orthogonal factorization, which does not square the e-blocks' condition number);
  * tag elimination: 2e-12 .. 5.0e-10, at e_ref's level (at most 1.3 e_ref; e_ref 4e-12 .. 6e-10).
"""
import dataclasses

import numpy as np
import pytest

import lm_cov_ref as cov_ref
from ar_slam_amd import synth
from test_lm_cov import E_REF_CAP, GRAPHS, MIN_PIVOT_CAP, CovInput, _spd, arrow_pattern, reference

pytestmark = pytest.mark.gpu


# ---- the selected inverse alone ----

@pytest.mark.parametrize("n, pattern", [(5, None), (64, None), (130, None), (200, None), (340, "arrow")])
def test_selinv_matches_numpy(lm, n, pattern):
    """n = 5: one tile, the rhs row inside it; 64: the rhs row alone in the last tile row; 130,
    200: several tiles; the arrow pattern: a two-level tree, Z_ij read transposed, |I_k| > 1, fill."""
    mask = arrow_pattern() if pattern else None
    A = _spd(n, 3 + n, mask)
    Z, P, info = lm.debug_selinv(A, mask)
    assert info == 0
    _, P_ref = cov_ref.tile_selinv(A, mask)
    assert np.array_equal(P.astype(bool), P_ref)
    full = np.kron(P_ref | P_ref.T, np.ones((64, 64)))[:n, :n] != 0
    ref = np.linalg.inv(A)
    d = np.sqrt(np.diag(ref))
    err = np.max(np.abs(Z - ref)[full] / np.outer(d, d)[full])
    print(f"selinv n={n}: max error {err:.2e} of sqrt(Z_ii Z_jj)")
    assert err <= 1e-10
    assert np.all(Z[~full] == 0.0)
    for k in range((n + 63) // 64):   # the diagonal tiles: the same bits both ways
        t = Z[64 * k:64 * (k + 1), 64 * k:64 * (k + 1)]
        assert np.array_equal(t, t.T)


def test_selinv_reports_a_failed_pivot(lm):
    A = _spd(70, 1)
    A[40, 40] = -1.0
    _, _, info = lm.debug_selinv(A)
    assert info == 41


# ---- arslam_lm_covariance ----

def _problem(lm, inp, loss=None, **opts):
    g = inp.g
    cc, tc = inp.consts()
    return lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, inp.camera_const, cc, tc,
                              obs_loss=loss, **opts)


def _check_parity(lm, oracle, inp, loss, elimination, executor):
    rp = _problem(lm, inp, loss, elimination=elimination, factor_executor=executor)
    s = rp.solve()
    assert s["elimination_used"] == elimination
    out = rp.covariance()
    ref = reference(oracle, inp, rp.camera, rp.cap, rp.tag, loss, rows=rp.debug_reduced_rows())
    assert ref.e_ref <= E_REF_CAP and ref.min_pivot >= MIN_PIVOT_CAP
    tol = max(16.0 * ref.e_ref, 1e-10)
    info = out["info"]
    assert info["status"] == lm.COV_OK
    assert np.array_equal(out["cap_status"], ref.cap_status)
    assert np.array_equal(out["tag_status"], ref.tag_status)
    worst = 0.0
    for dev, want, st in ((out["cap"], ref.cap, ref.cap_status), (out["tag"], ref.tag, ref.tag_status)):
        assert np.all(dev[st != cov_ref.OK] == -1.0)
        ok = st == cov_ref.OK
        assert np.array_equal(dev[ok], np.transpose(dev[ok], (0, 2, 1)))   # the same bits both ways
        d = np.sqrt(np.einsum("bii->bi", want[ok]))
        worst = max(worst, float(np.max(np.abs(dev[ok] - want[ok]) / (d[:, :, None] * d[:, None, :]))))
    if inp.camera_const:
        assert out["var_f"] == -1.0
    else:
        worst = max(worst, abs(out["var_f"] - ref.var_f) / ref.var_f)
    print(f"error {worst:.2e} (tol {tol:.2e}, e_ref {ref.e_ref:.2e}); min_pivot {info['min_pivot']:.6e} "
          f"(reference {ref.min_pivot_rows:.6e}); {info['n_reduced']} reduced rows, {info['n_factor_tiles']} tiles")
    assert abs(info["min_pivot"] - ref.min_pivot_rows) <= 1e-10
    assert worst <= tol
    return out


@pytest.mark.parametrize("executor", [0, 1])
@pytest.mark.parametrize("side", ["captures", "tags"])
@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", ["g20", "g60", "g6", "gk"])
def test_parity(lm, oracle, name, loss, side, executor):
    inp, l = GRAPHS[name], None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    _check_parity(lm, oracle, inp, l, lm.ELIM_CAPTURES if side == "captures" else lm.ELIM_TAGS, executor)


@pytest.mark.parametrize("side", ["captures", "tags"])
@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", ["g20_cap_const", "g20_camera_const", "g20_two_tags_const"])
def test_parity_constant_blocks(lm, oracle, name, loss, side):
    """A constant capture in place of the tag; a constant camera; a second constant tag."""
    inp, l = GRAPHS[name], None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    out = _check_parity(lm, oracle, inp, l, lm.ELIM_CAPTURES if side == "captures" else lm.ELIM_TAGS, 1)
    cc, tc = inp.consts()
    assert np.all(out["cap_status"][cc == 1] == lm.COV_UNAVAILABLE) and np.all(out["cap"][cc == 1] == -1.0)
    assert np.all(out["tag_status"][tc == 1] == lm.COV_UNAVAILABLE) and np.all(out["tag"][tc == 1] == -1.0)


def test_no_reduced_system(lm, oracle):
    """Every tag and the camera constant: C_e = U_e^-1 alone."""
    g = GRAPHS["g20"].g
    inp = CovInput(g, camera_const=True, tag_const=tuple(range(g.n_tag)))
    rp = _problem(lm, inp, elimination=lm.ELIM_CAPTURES)
    rp.solve()
    out = rp.covariance()
    ref = reference(oracle, inp, rp.camera, rp.cap, rp.tag)
    assert out["info"]["status"] == lm.COV_OK and out["info"]["n_reduced"] == 0 and out["info"]["min_pivot"] == 1.0
    d = np.sqrt(np.einsum("bii->bi", ref.cap))
    assert np.max(np.abs(out["cap"] - ref.cap) / (d[:, :, None] * d[:, None, :])) <= max(16 * ref.e_ref, 1e-10)
    assert np.all(out["tag"] == -1.0) and np.all(out["tag_status"] == lm.COV_UNAVAILABLE) and out["var_f"] == -1.0


def _bits(rp, s):
    return (rp.camera.copy(), rp.cap.copy(), rp.tag.copy(), s["final_cost"], s["initial_cost"],
            [it["cost"] for it in s["iterations"]])


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("executor", [0, 1])
def test_repeated_calls_and_later_solves_keep_their_bits(lm, executor):
    inp = GRAPHS["g60"]
    plain = _problem(lm, inp, factor_executor=executor)
    want = _bits(plain, plain.solve())
    rp = _problem(lm, inp, factor_executor=executor)
    first = _bits(rp, rp.solve())
    assert _same(first, want)
    a = rp.covariance()
    b = rp.covariance()
    for k in ("cap", "tag", "cap_status", "tag_status"):
        assert np.array_equal(a[k], b[k])
    assert a["var_f"] == b["var_f"] and a["info"]["min_pivot"] == b["info"]["min_pivot"]
    assert _same(_bits(rp, rp.solve()), want)     # a solve after it: the bits of a solve without one
    c = rp.covariance()
    assert np.array_equal(a["cap"], c["cap"]) and np.array_equal(a["tag"], c["tag"])


def _all_minus_one(lm, out):
    assert out["info"]["status"] == lm.COV_RANK_DEFICIENT
    assert np.all(out["cap"] == -1.0) and np.all(out["tag"] == -1.0) and out["var_f"] == -1.0
    assert not np.any(out["cap_status"] == lm.COV_OK) and not np.any(out["tag_status"] == lm.COV_OK)


def test_gauge_free_problem_is_rank_deficient(lm):
    rp = _problem(lm, CovInput(GRAPHS["g20"].g, tag_const=()))
    rp.solve()
    out = rp.covariance()
    _all_minus_one(lm, out)
    assert np.all(out["cap_status"] == lm.COV_RANK_DEFICIENT)


def test_unanchored_component_is_rank_deficient(lm):
    """Two copies of one graph side by side, sharing only the camera; the anchor is in the first."""
    g = GRAPHS["g6"].g
    two = synth.Graph(g.camera, np.vstack([g.cap, g.cap]), np.vstack([g.tag, g.tag]),
                      np.concatenate([g.obs_cap, g.obs_cap + g.n_cap]).astype(np.int32),
                      np.concatenate([g.obs_tag, g.obs_tag + g.n_tag]).astype(np.int32),
                      np.vstack([g.corners, g.corners]), g.camera_true, np.vstack([g.cap_true, g.cap_true]),
                      np.vstack([g.tag_true, g.tag_true]))
    rp = _problem(lm, CovInput(two, tag_const=(0,)))
    rp.solve()
    out = rp.covariance()
    _all_minus_one(lm, out)
    assert out["tag_status"][0] == lm.COV_UNAVAILABLE
    # anchored in both: a covariance
    rp = _problem(lm, CovInput(two, tag_const=(0, g.n_tag)))
    rp.solve()
    assert rp.covariance()["info"]["status"] == lm.COV_OK


def test_state_and_unsupported(lm):
    inp = GRAPHS["g6"]
    rp = _problem(lm, inp)
    with pytest.raises(lm.LMError) as e:
        rp.covariance()
    assert e.value.code == -7            # ARSLAM_E_STATE: no solve yet
    rp.solve()
    assert rp.covariance()["info"]["status"] == lm.COV_OK
    rp.set_options(max_num_iterations=0)   # NO_CONVERGENCE: the linearization at the returned point
    assert rp.solve()["termination"] == "NO_CONVERGENCE"
    assert rp.covariance()["info"]["status"] == lm.COV_OK
    # (the forced multi-rank path on one rank, through the host callback: the identity all-reduce)
    multi = _problem(lm, inp, force_multirank=True, comm=(0, 1, lambda a, op: None))
    multi.solve()
    with pytest.raises(lm.LMError) as e:
        multi.covariance()
    assert e.value.code == -2            # ARSLAM_E_UNSUPPORTED
    small = synth.config_graph("small")
    mixed = _problem(lm, CovInput(small), elimination=lm.ELIM_MIXED)
    assert mixed.solve()["elimination_used"] == lm.ELIM_MIXED
    with pytest.raises(lm.LMError) as e:
        mixed.covariance()
    assert e.value.code == -2
    # MIXED resolving to one whole side is supported (cfg1's set is all tags)
    cfg1 = synth.config_graph("cfg1")
    whole = _problem(lm, CovInput(cfg1), elimination=lm.ELIM_MIXED)
    assert whole.solve()["elimination_used"] == lm.ELIM_TAGS
    assert whole.covariance()["info"]["status"] == lm.COV_OK


def test_pointer_keyed_blocks(lm, oracle):
    """Problem.covariance_block against the SoA call on the same graph (the two number the tags
    differently, so the reduced system is ordered differently: parity tolerance, not bits)."""
    inp = GRAPHS["g20"]
    g = inp.g
    rp = _problem(lm, inp)
    rp.solve()
    soa = rp.covariance()
    ref = reference(oracle, inp, rp.camera, rp.cap, rp.tag)
    tol = max(16.0 * ref.e_ref, 1e-10)
    cam = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(g.n_cap)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem()
    for o in range(g.n_obs):
        prob.add_residual_block(g.corners[o], cam, caps[g.obs_cap[o]], tags[g.obs_tag[o]])
    prob.set_parameter_block_constant(tags[0])
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block(caps[0])
    assert e.value.code == -7
    prob.solve()
    for blocks, want, st in ((caps, soa["cap"], soa["cap_status"]), (tags, soa["tag"], soa["tag_status"])):
        for i, b in enumerate(blocks):
            c, s = prob.covariance_block(b)
            assert s == st[i]
            if s != lm.COV_OK:
                assert np.all(c == -1.0)
                continue
            assert np.array_equal(c, c.T)
            d = np.sqrt(np.diag(want[i]))
            assert np.max(np.abs(c - want[i]) / np.outer(d, d)) <= 2 * tol
    c, s = prob.covariance_block(cam)
    assert s == lm.COV_OK and c.shape == (3, 3)
    assert abs(c[0, 0] - soa["var_f"]) <= 2 * tol * soa["var_f"] and np.all(c.ravel()[1:] == 0.0)
    c2, _ = prob.covariance_block(cam)
    assert np.array_equal(c, c2)
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block(np.zeros(6))
    assert e.value.code == -1            # ARSLAM_E_INVALID_ARG


def test_printed_figures(lm):
    """The README's figures: the 60-tag graph at 0.5 px corner noise, tag 0 the anchor."""
    rp = _problem(lm, GRAPHS["g60"])
    rp.solve()
    out = rp.covariance()
    ok = out["tag_status"] == lm.COV_OK
    pos = 0.5 * np.sqrt(np.einsum("bii->b", out["tag"][ok][:, :3, :3]))
    info = out["info"]
    print(f"60 tags, 60 captures, 0.5 px: 1-sigma tag position median {1e3 * np.median(pos):.2f} mm, "
          f"largest {1e3 * pos.max():.2f} mm; sigma_f {0.5 * np.sqrt(out['var_f']):.3f} px; "
          f"device ms linearize {info['t_linearize_ms']:.3f} factor {info['t_factor_ms']:.3f} "
          f"selinv {info['t_selinv_ms']:.3f} blocks {info['t_blocks_ms']:.3f}")
    assert np.all(pos > 0) and out["var_f"] > 0
