"""GPU tests of the LM solver's cross-covariance blocks (arslam_lm_covariance_pairs,
arslam_lm_covariance_block_pair, include/arslam_lm.h) and of the multi-right-hand-side tile solve
behind them (arslam_debug_tile_solve), against tests/lm_cov_pairs_ref.py.

The parity reference is set up as in tests/test_gpu_lm_cov.py: at the parameters the device
returned, with the Jacobi scale of the initial ones.
  * the solve alone: |X - A^-1 B|_ij <= 1e-10 sqrt(Z_ii Z_jj) for identity columns (the selected
    inverse's bound), 1e-10 max|X_ref| per column for a random B.
  * |C_dev - C_ref|_ij <= tol sqrt(C_ref,ii C_ref,jj) over every requested block, tol = 16
    max(e_ref, e_ref_pairs) of that input, not below 1e-10: the rule of tests/test_gpu_lm_cov.py
    extended to the requested blocks.  Every input and pair list is asserted to have e_ref_pairs <=
    1e-9 (tests/test_lm_cov_pairs.py).
  * statuses equal the reference's; (a, b) and (b, a) transposes with equal bits; (a, a) exactly
    symmetric.

Measured on an MI355X (each case prints its figures; profiles/lm_cov_pairs/device_errors.txt):
  * the solve alone: <= 1.5e-15 of sqrt(Z_ii Z_jj), off the factor's tile pattern too;
  * capture elimination: 2e-13 .. 2.4e-11; tag elimination: 5e-12 .. 3.2e-10 (the closest case at
    1/14 of its tol), as the marginals of tests/test_gpu_lm_cov.py;
  * (a, a) against covariance()'s marginal: 4e-15 .. 7e-12.
"""
import numpy as np
import pytest

import lm_cov_pairs_ref as pairs_ref
from ar_slam_amd import synth
from lm_cov_pairs_ref import CAMERA, CAPTURE, TAG
from test_gpu_lm_cov import _bits, _problem, _same
from test_lm_cov import E_REF_CAP, GRAPHS, MIN_PIVOT_CAP, CovInput, _spd, arrow_pattern, reference
from test_lm_cov_pairs import BATCH_BLOCKS, SOLVE_SHAPES, batch_input, pairs_reference

pytestmark = pytest.mark.gpu


# ---- the solve alone ----

@pytest.mark.parametrize("nrhs", [6, 60, 66])
@pytest.mark.parametrize("n, pattern", SOLVE_SHAPES)
def test_tile_solve_matches_numpy(lm, n, pattern, nrhs):
    """n = 5: one tile, the rhs row inside it; 64: the rhs row alone in the last tile row; 130, 200:
    several tiles; the arrow pattern: a two-level tree with fill, and rows of X in tiles that are
    structurally zero in the factor (tile (1, 0) for a column of tile 0's leaf sibling: columns
    128.. against rows 0..127), which the selected inverse does not hold.  nrhs = 66: a second panel."""
    mask = arrow_pattern() if pattern else None
    A = _spd(n, 3 + n, mask)
    cols = pairs_ref.solve_columns(n, nrhs)
    X, info = lm.debug_tile_solve(A, np.eye(n)[:, cols], mask)
    assert info == 0
    Z = np.linalg.inv(A)
    d = np.sqrt(np.diag(Z))
    err = np.abs(X - Z[:, cols]) / np.outer(d, d[cols])
    print(f"tile solve n={n} nrhs={nrhs}: max error {err.max():.2e} of sqrt(Z_ii Z_jj)")
    assert err.max() <= 1e-10
    if mask is not None:
        # a column of tile column 2 against the rows of tile rows 0 and 1: tiles (2, 0), (2, 1) are not in the factor
        c = [k for k, col in enumerate(cols) if 128 <= col < 192]
        assert c and not mask[2, 0] and not mask[2, 1]
        print(f"  off the factor's pattern: max error {err[:128, c].max():.2e}, largest |X| there "
              f"{np.abs(X[:128, c]).max():.2e}")
        assert np.abs(X[:128, c]).max() > 0.0


@pytest.mark.parametrize("n, pattern", [(200, None), (340, "arrow")])
def test_tile_solve_random_rhs(lm, n, pattern):
    mask = arrow_pattern() if pattern else None
    A = _spd(n, 3 + n, mask)
    B = np.random.default_rng(n).standard_normal((n, 66))
    X, info = lm.debug_tile_solve(A, B, mask)
    assert info == 0
    ref = np.linalg.solve(A, B)
    err = np.max(np.abs(X - ref) / np.max(np.abs(ref), axis=0))
    print(f"tile solve n={n} random B: max error {err:.2e} of max|X_ref| per column")
    assert err <= 1e-10
    X2, _ = lm.debug_tile_solve(A, B, mask)
    assert np.array_equal(X, X2)


def test_tile_solve_reports_a_failed_pivot(lm):
    A = _spd(70, 1)
    A[40, 40] = -1.0
    _, info = lm.debug_tile_solve(A, np.eye(70)[:, :6])
    assert info == 41


# ---- arslam_lm_covariance_pairs ----

def _elim(lm, side):
    return lm.ELIM_CAPTURES if side == "captures" else lm.ELIM_TAGS


def _solved(lm, inp, loss=None, **opts):
    rp = _problem(lm, inp, loss, **opts)
    s = rp.solve()
    return rp, s


def _reference(oracle, rp, inp, pairs, loss=None):
    ref = pairs_reference(oracle, inp, pairs, rp.camera, rp.cap, rp.tag, loss, rows=rp.debug_reduced_rows())
    assert ref.e_ref_pairs <= E_REF_CAP and ref.ref.e_ref <= E_REF_CAP and ref.ref.min_pivot >= MIN_PIVOT_CAP
    return ref, max(16.0 * max(ref.ref.e_ref, ref.e_ref_pairs), 1e-10)


def _worst(cov, ref):
    ok = ref.status == pairs_ref.OK
    return max(float(np.max(np.abs(cov[p] - ref.cov[p]) / ref.scale[p])) for p in np.nonzero(ok)[0])


@pytest.mark.parametrize("executor", [0, 1])
@pytest.mark.parametrize("side", ["captures", "tags"])
@pytest.mark.parametrize("name, loss", [("g6", False), ("g20", False), ("g20", True), ("g60", False), ("gk", False)])
def test_parity(lm, oracle, name, loss, side, executor):
    inp, l = GRAPHS[name], None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    rp, s = _solved(lm, inp, l, elimination=_elim(lm, side), factor_executor=executor)
    assert s["elimination_used"] == _elim(lm, side)
    pairs, cat = pairs_ref.pair_list(inp)
    cov, st, info = rp.covariance_pairs(pairs)
    ref, tol = _reference(oracle, rp, inp, pairs, l)
    assert info["status"] == lm.COV_OK
    assert np.array_equal(st, ref.status)
    worst = _worst(cov, ref)
    n_solved = len(pairs_ref.solved_blocks(pairs, side == "tags"))
    print(f"{name} loss={loss} {side} executor {executor}: error {worst:.2e} (tol {tol:.2e}, e_ref {ref.ref.e_ref:.2e}, "
          f"e_ref_pairs {ref.e_ref_pairs:.2e}); {len(pairs)} pairs, {n_solved} solved blocks, "
          f"{info['n_selinv_products']} tile products, solve {info['t_selinv_ms']:.3f} ms")
    assert abs(info["min_pivot"] - ref.ref.min_pivot_rows) <= 1e-10
    assert worst <= tol
    assert n_solved > pairs_ref.PANEL_BLOCKS and info["n_selinv_products"] > 0
    # both orders of one pair, the duplicate, the layout with the camera
    i, j = pairs.index(cat["cap_tag_seen"]), pairs.index(cat["reversed"])
    assert np.array_equal(cov[i], cov[j].T)
    dup = [p for p, pr in enumerate(pairs) if pr == cat["duplicate"]]
    assert len(dup) >= 2 and all(np.array_equal(cov[dup[0]], cov[p]) for p in dup[1:])
    for k in ("camera_tag", "camera_capture"):
        assert np.all(cov[pairs.index(cat[k])].ravel()[6:] == 0.0)
    assert np.all(cov[pairs.index(cat["camera_camera"])].ravel()[1:] == 0.0)


@pytest.mark.parametrize("side", ["captures", "tags"])
def test_more_solved_blocks_than_one_batch(lm, oracle, side):
    """More solved blocks than a batch holds: a second batch of panels through the same buffers."""
    inp, pairs = batch_input()
    rp, _ = _solved(lm, inp, elimination=_elim(lm, side))
    cov, st, info = rp.covariance_pairs(pairs)
    ref, tol = _reference(oracle, rp, inp, pairs)
    assert len(pairs_ref.solved_blocks(pairs, side == "tags")) > BATCH_BLOCKS
    assert info["status"] == lm.COV_OK and np.all(st == lm.COV_OK)
    worst = _worst(cov, ref)
    print(f"batch input {side}: error {worst:.2e} (tol {tol:.2e}); {len(pairs)} pairs, {info['n_selinv_products']} tile "
          f"products, solve {info['t_selinv_ms']:.3f} ms")
    assert worst <= tol
    again, _, _ = rp.covariance_pairs(pairs[150:] + pairs[:150])    # the list in another order: the same bits
    assert np.array_equal(cov, np.concatenate([again[-150:], again[:-150]]))


@pytest.mark.parametrize("side", ["captures", "tags"])
@pytest.mark.parametrize("name", ["g20", "g60"])
def test_consistency(lm, oracle, name, side):
    """(a, b) against (b, a), (a, a) against itself and against covariance()'s marginal, and the
    joint matrix of every pair from device blocks alone."""
    inp = GRAPHS[name]
    rp, _ = _solved(lm, inp, elimination=_elim(lm, side))
    base, _ = pairs_ref.pair_list(inp)
    base = [pr for pr in dict.fromkeys(base) if pr[0] != pr[1]]
    pairs = [q for a, b in base for q in ((a, b), (b, a), (a, a), (b, b))]
    cov, st, _ = rp.covariance_pairs(pairs)
    ref, tol = _reference(oracle, rp, inp, pairs)
    assert np.all(st == lm.COV_OK)
    marg = rp.covariance()
    worst_m = 0.0
    for q, (a, b) in enumerate(base):
        ab, ba, aa, bb = cov[4 * q:4 * q + 4]
        fa, fb = a[0] == CAMERA, b[0] == CAMERA
        if fa or fb:
            assert np.array_equal(ab, ba)            # the focal's six values first, in either order
        else:
            assert np.array_equal(ab, ba.T)
        assert np.array_equal(aa, aa.T) and np.array_equal(bb, bb.T)
        for blk, c in ((a, aa), (b, bb)):
            want = marg["var_f"] * np.eye(6)[:1].T @ np.eye(6)[:1] if blk[0] == CAMERA else \
                marg["cap" if blk[0] == CAPTURE else "tag"][blk[1]]
            d = np.sqrt(np.where(np.diag(want) > 0, np.diag(want), 1.0))
            worst_m = max(worst_m, float(np.max(np.abs(c - want) / np.outer(d, d))))
        J = pairs_ref.joint_from_blocks(aa, ab, ba, bb, fa, fb)
        assert np.array_equal(J, J.T) and np.all(np.linalg.eigvalsh(J) > 0), (a, b)
    print(f"{name} {side}: (a, a) against covariance()'s marginal {worst_m:.2e} (tol {tol:.2e}); "
          f"pairs against the reference {_worst(cov, ref):.2e}")
    assert worst_m <= tol and _worst(cov, ref) <= tol


@pytest.mark.parametrize("side", ["captures", "tags"])
@pytest.mark.parametrize("name", ["g20_cap_const", "g20_camera_const", "g20_two_tags_const"])
def test_constant_blocks_are_unavailable(lm, oracle, name, side):
    inp = GRAPHS[name]
    g = inp.g
    rp, _ = _solved(lm, inp, elimination=_elim(lm, side))
    pairs = [((CAMERA, 0), (TAG, 3)), ((CAPTURE, 0), (TAG, 3)), ((TAG, 0), (TAG, 3)), ((TAG, 3), (TAG, 7)),
             ((CAPTURE, 0), (CAPTURE, 0)), ((TAG, 3), (CAPTURE, 2)), ((TAG, 0), (TAG, 0)), ((CAMERA, 0), (CAMERA, 0))]
    cov, st, info = rp.covariance_pairs(pairs)
    ref, tol = _reference(oracle, rp, inp, pairs)
    assert info["status"] == lm.COV_OK
    assert np.array_equal(st, ref.status)
    cc, tc = inp.consts()
    const = lambda b: inp.camera_const if b[0] == CAMERA else bool((cc if b[0] == CAPTURE else tc)[b[1]])
    for p, (a, b) in enumerate(pairs):
        assert (st[p] == lm.COV_UNAVAILABLE) == (const(a) or const(b))
        if st[p] != lm.COV_OK:
            assert np.all(cov[p] == -1.0)
    assert np.any(st == lm.COV_UNAVAILABLE) and np.any(st == lm.COV_OK)
    assert _worst(cov, ref) <= tol


def test_rank_deficient_problems(lm):
    pairs = [((TAG, 1), (TAG, 2)), ((CAPTURE, 0), (TAG, 1)), ((CAMERA, 0), (CAPTURE, 1)), ((TAG, 0), (TAG, 1))]
    rp, _ = _solved(lm, CovInput(GRAPHS["g20"].g, tag_const=()))     # gauge-free
    cov, st, info = rp.covariance_pairs(pairs)
    assert info["status"] == lm.COV_RANK_DEFICIENT
    assert np.all(st == lm.COV_RANK_DEFICIENT) and np.all(cov == -1.0)
    # two copies of one graph sharing only the camera; the anchor is in the first
    g = GRAPHS["g6"].g
    two = synth.Graph(g.camera, np.vstack([g.cap, g.cap]), np.vstack([g.tag, g.tag]),
                      np.concatenate([g.obs_cap, g.obs_cap + g.n_cap]).astype(np.int32),
                      np.concatenate([g.obs_tag, g.obs_tag + g.n_tag]).astype(np.int32),
                      np.vstack([g.corners, g.corners]), g.camera_true, np.vstack([g.cap_true, g.cap_true]),
                      np.vstack([g.tag_true, g.tag_true]))
    rp, _ = _solved(lm, CovInput(two, tag_const=(0,)))
    cov, st, info = rp.covariance_pairs(pairs)
    assert info["status"] == lm.COV_RANK_DEFICIENT and np.all(cov == -1.0)
    assert list(st) == [lm.COV_RANK_DEFICIENT] * 3 + [lm.COV_UNAVAILABLE]
    rp, _ = _solved(lm, CovInput(two, tag_const=(0, g.n_tag)))
    cov, st, info = rp.covariance_pairs(pairs[:3] + [((TAG, 1), (TAG, g.n_tag + 1))])
    assert info["status"] == lm.COV_OK and np.all(st == lm.COV_OK) and np.all(cov[:, 0, 0] != -1.0)


def test_state_unsupported_and_arguments(lm):
    inp = GRAPHS["g6"]
    pairs = [((TAG, 1), (TAG, 2))]
    rp = _problem(lm, inp)
    with pytest.raises(lm.LMError) as e:
        rp.covariance_pairs(pairs)
    assert e.value.code == -7            # ARSLAM_E_STATE: no solve yet
    rp.solve()
    cov, st, info = rp.covariance_pairs(pairs)   # without an earlier covariance() call
    assert info["status"] == lm.COV_OK and st[0] == lm.COV_OK
    cov0, st0, info0 = rp.covariance_pairs([])
    assert cov0.shape == (0, 6, 6) and len(st0) == 0 and info0["status"] == lm.COV_OK
    for bad in (((3, 0), (TAG, 1)), ((TAG, 1), (-1, 0)), ((TAG, inp.g.n_tag), (TAG, 1)), ((TAG, 1), (CAPTURE, -1)),
                ((CAPTURE, inp.g.n_cap), (TAG, 1)), ((CAMERA, 1), (TAG, 1))):
        with pytest.raises(lm.LMError) as e:
            rp.covariance_pairs([pairs[0], bad])
        assert e.value.code == -1, bad   # ARSLAM_E_INVALID_ARG
    cov2, _, _ = rp.covariance_pairs(pairs)
    assert np.array_equal(cov, cov2)
    multi = _problem(lm, inp, force_multirank=True, comm=(0, 1, lambda a, op: None))
    multi.solve()
    with pytest.raises(lm.LMError) as e:
        multi.covariance_pairs(pairs)
    assert e.value.code == -2            # ARSLAM_E_UNSUPPORTED
    small = synth.config_graph("small")
    mixed = _problem(lm, CovInput(small), elimination=lm.ELIM_MIXED)
    assert mixed.solve()["elimination_used"] == lm.ELIM_MIXED
    with pytest.raises(lm.LMError) as e:
        mixed.covariance_pairs(pairs)
    assert e.value.code == -2
    cfg1 = synth.config_graph("cfg1")    # MIXED resolving to one whole side
    whole = _problem(lm, CovInput(cfg1), elimination=lm.ELIM_MIXED)
    assert whole.solve()["elimination_used"] == lm.ELIM_TAGS
    cov, st, info = whole.covariance_pairs([((TAG, 1), (TAG, cfg1.n_tag - 1)), ((CAPTURE, 0), (TAG, 1))])
    assert info["status"] == lm.COV_OK and np.all(st == lm.COV_OK)


def test_no_reduced_system(lm, oracle):
    """Every tag and the camera constant: the e-e diagonal pair is U_e^-1, the cross pairs of free
    captures exactly 0."""
    g = GRAPHS["g20"].g
    inp = CovInput(g, camera_const=True, tag_const=tuple(range(g.n_tag)))
    rp, _ = _solved(lm, inp, elimination=lm.ELIM_CAPTURES)
    pairs = [((CAPTURE, 2), (CAPTURE, 2)), ((CAPTURE, 2), (CAPTURE, 5)), ((CAPTURE, 5), (CAPTURE, 2)),
             ((CAPTURE, 1), (TAG, 3)), ((CAMERA, 0), (CAPTURE, 1))]
    cov, st, info = rp.covariance_pairs(pairs)
    ref = reference(oracle, inp, rp.camera, rp.cap, rp.tag)
    assert info["status"] == lm.COV_OK and info["n_reduced"] == 0 and info["n_selinv_products"] == 0
    assert list(st) == [lm.COV_OK] * 3 + [lm.COV_UNAVAILABLE] * 2
    d = np.sqrt(np.diag(ref.cap[2]))
    assert np.max(np.abs(cov[0] - ref.cap[2]) / np.outer(d, d)) <= max(16 * ref.e_ref, 1e-10)
    assert np.array_equal(cov[0], cov[0].T)
    assert np.all(cov[1] == 0.0) and np.all(cov[2] == 0.0) and np.all(cov[3:] == -1.0)


@pytest.mark.parametrize("executor", [0, 1])
def test_repeated_calls_and_later_solves_keep_their_bits(lm, executor):
    inp = GRAPHS["g60"]
    pairs, _ = pairs_ref.pair_list(inp)
    plain = _problem(lm, inp, factor_executor=executor)
    want = _bits(plain, plain.solve())
    rp = _problem(lm, inp, factor_executor=executor)
    assert _same(_bits(rp, rp.solve()), want)
    m0 = rp.covariance()
    a, sa, _ = rp.covariance_pairs(pairs)
    b, sb, _ = rp.covariance_pairs(pairs)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    m1 = rp.covariance()                 # covariance() before and after a pairs call
    for k in ("cap", "tag", "cap_status", "tag_status"):
        assert np.array_equal(m0[k], m1[k])
    assert m0["var_f"] == m1["var_f"] and m0["info"]["min_pivot"] == m1["info"]["min_pivot"]
    c, _, _ = rp.covariance_pairs(pairs[::-1])   # after covariance() overwrote the factor's tiles; another order
    assert np.array_equal(a, c[::-1])
    assert _same(_bits(rp, rp.solve()), want)     # a solve after it: the bits of a solve without one
    d, _, _ = rp.covariance_pairs(pairs[:3])     # a shorter list: a pair's bits do not depend on the list
    assert np.array_equal(a[:3], d)


def test_pointer_keyed_block_pairs(lm, oracle):
    """Problem.covariance_block_pair against the SoA call on the same graph (the two order the
    reduced system differently: parity tolerance, not bits), the camera's shapes, an unknown pointer."""
    inp = GRAPHS["g20"]
    g = inp.g
    rp, _ = _solved(lm, inp)
    pairs, cat = pairs_ref.pair_list(inp)
    soa, st, _ = rp.covariance_pairs(pairs)
    ref, tol = _reference(oracle, rp, inp, pairs)
    cam = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(g.n_cap)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem()
    for o in range(g.n_obs):
        prob.add_residual_block(g.corners[o], cam, caps[g.obs_cap[o]], tags[g.obs_tag[o]])
    prob.set_parameter_block_constant(tags[0])
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block_pair(caps[0], tags[1])
    assert e.value.code == -7
    prob.solve()
    blk = lambda b: cam if b[0] == CAMERA else (caps if b[0] == CAPTURE else tags)[b[1]]
    for p, (a, b) in enumerate(pairs[:len(cat)]):
        c, s = prob.covariance_block_pair(blk(a), blk(b))
        assert s == st[p] == lm.COV_OK
        assert c.shape == (3 if a[0] == CAMERA else 6, 3 if b[0] == CAMERA else 6)
        fa, fb = a[0] == CAMERA, b[0] == CAMERA
        if fa and fb:
            got, rest = c[:1, :1].ravel(), np.delete(c.ravel(), 0)
        elif fa:
            got, rest = c[0], c[1:].ravel()
        elif fb:
            got, rest = c[:, 0], c[:, 1:].ravel()
        else:
            got, rest = c.ravel(), np.zeros(0)
        assert np.all(rest == 0.0)
        want, sc = soa[p].ravel()[:got.size], ref.scale[p].ravel()[:got.size]
        assert np.max(np.abs(got - want) / sc) <= 2 * tol, (a, b)
    c, s = prob.covariance_block_pair(tags[0], tags[1])      # the constant tag
    assert s == lm.COV_UNAVAILABLE and np.all(c == -1.0)
    c, s = prob.covariance_block_pair(cam, tags[0])
    assert s == lm.COV_UNAVAILABLE and c.shape == (3, 6) and np.all(c == -1.0)
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block_pair(tags[1], np.zeros(6))
    assert e.value.code == -1            # ARSLAM_E_INVALID_ARG


def test_printed_figures_relative(lm, oracle):
    """The README's setting: the 60-tag graph at 0.5 px corner noise, tag 0 the anchor.  1-sigma of
    a tag's position relative to its nearest neighbour, from C_ii + C_jj - C_ij - C_ji over the
    translations, beside the absolute figure."""
    inp = GRAPHS["g60"]
    g = inp.g
    rp, _ = _solved(lm, inp)
    tags = list(range(1, g.n_tag))
    pos = g.tag_true[:, :3]
    dist = np.linalg.norm(pos[tags][:, None] - pos[tags][None], axis=2)
    np.fill_diagonal(dist, np.inf)
    near = [tags[j] for j in np.argmin(dist, axis=1)]
    pairs = [q for i, j in zip(tags, near) for q in (((TAG, i), (TAG, i)), ((TAG, j), (TAG, j)), ((TAG, i), (TAG, j)))]
    cov, st, info = rp.covariance_pairs(pairs)
    assert np.all(st == lm.COV_OK)
    ref, tol = _reference(oracle, rp, inp, pairs)

    def relative(c):
        ii, jj, ij = c[0::3, :3, :3], c[1::3, :3, :3], c[2::3, :3, :3]
        return ii + jj - ij - np.transpose(ij, (0, 2, 1))
    rel, rel_ref = relative(cov), relative(ref.cov)
    var, var_ref = np.einsum("bii->b", rel), np.einsum("bii->b", rel_ref)
    sig_rel = 0.5 * np.sqrt(var)
    sig_abs = 0.5 * np.sqrt(np.einsum("bii->b", cov[0::3, :3, :3]))
    print(f"60 tags, 60 captures, 0.5 px: 1-sigma tag position relative to the nearest neighbour median "
          f"{1e3 * np.median(sig_rel):.2f} mm, largest {1e3 * sig_rel.max():.2f} mm (absolute: median "
          f"{1e3 * np.median(sig_abs):.2f} mm, largest {1e3 * sig_abs.max():.2f} mm); {len(pairs)} pairs, "
          f"{info['n_selinv_products']} tile products, device ms solve {info['t_selinv_ms']:.3f} "
          f"blocks {info['t_blocks_ms']:.3f}")
    assert np.all(var > 0)
    # each of the four terms is within tol sqrt(C_ii C_jj) of the reference's
    d2 = np.einsum("bii->bi", ref.cov[0::3])[:, :3], np.einsum("bii->bi", ref.cov[1::3])[:, :3]
    bound = tol * (d2[0] + d2[1] + 2 * np.sqrt(d2[0] * d2[1])).sum(axis=1)
    assert np.all(np.abs(var - var_ref) <= bound)
