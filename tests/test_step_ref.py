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


# ---- the sharded reduction (tests/test_gpu_step_stages_sharded.py) ----

# name: (top cols, top tiles, [(own cols, owned captures) per rank]); every case has two active ranks
SPLIT_FACTS = {"medium": (3, 6, [(3, 108), (3, 92)]), "medium_cauchy": (3, 6, [(3, 108), (3, 92)]),
               "medium_const": (2, 3, [(3, 108), (3, 92)]), "sh400": (4, 10, [(6, 204), (6, 194), (0, 2)]),
               "shmix200": (4, 10, [(9, 99), (7, 101)])}


def _slot_rank(P, owners):
    """A stand-in for the device's row classes (which need the loaded plan): an f-side slot is
    rank k's when every capture that sees its tag is k's, the top's (-1) otherwise.  Any such
    partition serves the arithmetic checked here."""
    slot_rank = np.full(P.n, -1, np.int64)
    for t in range(P.nt):
        ks = np.unique(owners[P.obs_cap[P.active & (P.obs_tag == t)]])
        if len(ks) == 1:
            slot_rank[sr.block_slots(P, P.nc + t)] = ks[0]
    return slot_rank


def _sharded_state(oracle, name):
    P, R, _, (s, d), (s64, d64) = _state(oracle, name)
    infos, owners = sr.rank_split(name)
    owners = owners.astype(np.int64)
    return P, R, (s, d), (s64, d64), owners, _slot_rank(P, owners), len(infos), _sets(P)["captures"]


@pytest.mark.parametrize("name", sorted(sr.SHARDED))
def test_split_facts_of_the_sharded_inputs(name):
    """What the GPU test relies on, by the host-only arslam_debug_rank_split: a replicated top,
    two ranks owning subtrees, the captures partitioned among the ranks; sh400's third rank owns
    two top-only captures and no subtree; both ranks of shmix200 own captures of more than 10 tags
    (k_schur<true>) and of more than 8 observations (the chunked instances)."""
    infos, owners = sr.rank_split(name)
    top_cols, top_tiles, per_rank = SPLIT_FACTS[name]
    assert len(infos) == sr.SHARDED[name] == len(per_rank)
    g = sr.spec(name)["g"]
    assert owners.min() >= 0 and owners.max() < len(infos) and len(owners) == g.n_cap   # a partition
    for k, info in enumerate(infos):
        assert (info["n_top_cols"], info["n_top_tiles"], info["n_active"], info["dag_valid"]) == (top_cols, top_tiles, 2, 1)
        assert (info["n_own_cols"], info["n_owned_captures"]) == per_rank[k]
        assert np.count_nonzero(owners == k) == info["n_owned_captures"]
    if name == "shmix200":
        tags = np.array([len(set(g.obs_tag[g.obs_cap == c].tolist())) for c in range(g.n_cap)])
        obs = np.bincount(g.obs_cap, minlength=g.n_cap)
        assert [int(np.sum((owners == k) & (tags > 10))) for k in (0, 1)] == [39, 36]
        assert all(np.any((owners == k) & (obs > 8)) for k in (0, 1))


@pytest.mark.parametrize("name", ["medium", "medium_const", "sh400", "shmix200"])
def test_shares_sum_to_the_whole_system(oracle, name):
    """The long-double shares, summed in rank order with the top's D^2, are reduce()'s S and rhs of
    the whole problem to the rounding of the sum.

    Bound.  An entry of S is a sum of at most nc captures' contributions c_k, taken in one order by
    reduce() and share-first here: each sum is within (nc - 1) u sum |c_k| of the exact one,
    u = 2^-64.  A capture's F'F and W'U^-1 W are positive semi-definite with W'U^-1 W <= F'F, so
    |c_k|_ij <= 2 sqrt((F'F)_ii (F'F)_jj) and sum_k |c_k|_ij <= 2 sqrt(H_ii H_jj) (Cauchy-Schwarz):
    in the H-normalised measure the two differ by at most 4 nc u; the rhs likewise with
    sum_k sqrt((F'F)_ii) |r_k| <= sqrt(H_ii) |r|."""
    P, R, (s, d), _, owners, slot_rank, world, elim = _sharded_state(oracle, name)
    radius = 1e4
    ref = sr.reduce(R, elim, s, d, radius, True)
    shares = sr.reduce_shares(R, elim, s, d, radius, owners, slot_rank, world, True)
    top = slot_rank[ref.slots] < 0
    assert top.any() and not top.all()
    S, rhs = sr.sum_shares(shares, np.where(top, ref.D2[ref.slots], 0))
    eS, er = sr.errors(S, rhs, ref)
    print(f"step_ref: {name} x{world} shares' sum against the whole: S {eS:.1e} rhs {er:.1e} bound {4 * P.nc * sr.ULD:.1e}")
    assert eS <= 4 * P.nc * sr.ULD and er <= 4 * P.nc * sr.ULD
    # a share is zero outside its own captures' blocks and in the rows of another rank's slots
    for k, sh in enumerate(shares):
        other = (slot_rank[ref.slots] >= 0) & (slot_rank[ref.slots] != k)
        assert np.all(sh.S[~sh.struct] == 0) and np.all(sh.S[other] == 0) and np.all(sh.rhs[other] == 0)


@pytest.mark.parametrize("name", sorted(sr.SHARDED))
def test_share_first_restatement_stays_under_the_caps(oracle, name):
    """The float64 restatement of the shares and of their sum in rank order (the device's two-level
    sum): each share's and the sum's own S error, by the whole problem's H, stays under
    step_ref.CAPS at every radius the GPU test runs the input at."""
    P, R, (s, d), (s64, d64), owners, slot_rank, world, elim = _sharded_state(oracle, name)
    for radius in sr.INPUT_RADII[name]:
        ref = sr.reduce(R, elim, s, d, radius, True)
        ld = sr.reduce_shares(R, elim, s, d, radius, owners, slot_rank, world, True)
        f64 = sr.reduce_shares(R, elim, s64, d64, radius, owners, slot_rank, world, False)
        top = slot_rank[ref.slots] < 0
        S, rhs = sr.sum_shares(f64, np.where(top, f64[0].D2[ref.slots], 0.0))
        e_sum = sr.errors(S, rhs, ref)[0]
        e_share = [sr.errors(a.S, a.rhs, _by_whole(b, ref))[0] for a, b in zip(f64, ld)]
        print(f"step_ref: {name} x{world} r={radius:g} share-first floor S {e_sum:.1e}, shares {max(e_share):.1e}")
        assert max([e_sum] + e_share) <= sr.CAPS[radius]


def _by_whole(share, ref):
    """A share as errors()' reference: its S and rhs, normalised by the whole problem's H and r'r."""
    import types
    return types.SimpleNamespace(S=share.S, rhs=share.rhs, H=ref.H, rr=ref.rr)


def test_the_sharded_measures_see_a_misplaced_capture_and_a_doubled_top_diagonal(oracle):
    """What the per-rank and the summed checks exist for, done to the restatement (numpy only) on
    medium x 2.  One capture's contribution assembled on the other rank: the sum of the shares is
    unchanged to rounding, each of the two shares is wrong by many orders over the rule's bound.
    The top rows' D^2 added on both ranks: seen in the sum."""
    P, R, (s, d), (s64, d64), owners, slot_rank, world, elim = _sharded_state(oracle, "medium")
    moved = owners.copy()
    c = int(np.nonzero(owners == 0)[0][3])
    moved[c] = 1
    for radius in (1e-2, 1e4):
        ref = sr.reduce(R, elim, s, d, radius, True)
        ld = sr.reduce_shares(R, elim, s, d, radius, owners, slot_rank, world, True)
        good = sr.reduce_shares(R, elim, s64, d64, radius, owners, slot_rank, world, False)
        bad = sr.reduce_shares(R, elim, s64, d64, radius, moved, slot_rank, world, False)
        top_d2 = np.where(slot_rank[ref.slots] < 0, good[0].D2[ref.slots], 0.0)
        e_good = sr.errors(*sr.sum_shares(good, top_d2), ref)[0]
        bound = 16 * max(e_good, sr.FLOOR)
        e_sum = sr.errors(*sr.sum_shares(bad, top_d2), ref)[0]
        e_rank = [sr.errors(b.S, b.rhs, _by_whole(a, ref))[0] for a, b in zip(ld, bad)]
        e_twice = sr.errors(*sr.sum_shares(good, world * top_d2), ref)[0]
        print(f"step_ref: r={radius:g} moved capture {c}: sum {e_sum:.1e}, ranks {e_rank[0]:.1e} {e_rank[1]:.1e}; "
              f"top D^2 on both ranks: {e_twice:.1e}; bound {bound:.1e}")
        assert e_sum <= bound and min(e_rank) > 1e6 * bound
        assert e_twice > 1e6 * bound


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
