"""CPU tests of the yardstick the sparse-plan Cholesky and solve are held to (tests/llt_ref.py):
the numpy restatement of the device's tile algorithm against LAPACK, its symbolic fill and the
properties of the named patterns against the planner (arslam_debug_tile_plan, host only), and the
restatement's own backward errors on every input of tests/test_gpu_tile_llt.py."""
import numpy as np
import pytest

import llt_ref as R


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    lm.lib()
    return lm


PATTERNS, TWO_PHASE = R.PATTERNS, R.TWO_PHASE


@pytest.mark.parametrize("name", ["dense_n1", "dense_n63", "dense_n64", "dense_n65", "dense_n191", "nd12_n740_c2",
                                  "nd12_n704_c2", "nd12_n767_c2"])
def test_restatement_equals_lapack_when_well_conditioned(name):
    inp = R.make_input(name)
    ref = R.reference_figures(name).ref
    Lc = np.linalg.cholesky(inp.A)
    yc = np.linalg.solve(inp.A, inp.b)
    assert ref.info == 0
    assert np.max(np.abs(ref.L - Lc)) <= 1e-13 * np.max(np.abs(Lc))
    assert np.max(np.abs(ref.y - yc)) <= 1e-11 * np.max(np.abs(yc))   # (condition number ~1e3 at most)
    full = np.kron(ref.pattern, np.ones((64, 64)))[:inp.n, :inp.n] != 0
    assert np.all(ref.L[~full] == 0.0)


@pytest.mark.parametrize("name", ["nd12_top2", "wide23_top7"])
def test_two_phase_restatement_equals_lapack(name):
    pat, cls = TWO_PHASE[name]
    inp = R.make_input({"nd12": "nd12_n740_c2", "wide23": "wide23_n1440"}[pat])
    ref = R.tile_llt(inp.A, inp.b, inp.pattern, cls)
    Lc = np.linalg.cholesky(inp.A)
    tol = 1e-13 if pat == "nd12" else 1e-8   # (wide23's input is the 1e8 class)
    assert np.max(np.abs(ref.L - Lc)) <= tol * np.max(np.abs(Lc))


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_symbolic_fill_equals_the_planner(L, name):
    P = PATTERNS[name]()
    T = P.shape[0]
    out, facts = L.debug_tile_plan(T, P)
    ours = R.tile_fill(R.taken(P))
    assert np.array_equal(np.tril(out != 0), ours)
    assert facts["n_assembled"] == int(R.taken(P).sum())
    assert facts["n_tiles"] == int(ours.sum())
    _, height = R.elimination_levels(ours)
    assert facts["n_levels"] == int(height.max()) + 1
    assert facts["dag_valid"] == 1


def test_restatement_plan_facts_equal_the_planner(L):
    """The restatement's fill tiles, split targets and level count on the inputs that have them."""
    for name in ["arrow_n340", "nd12_n740_c2", "forest_n450", "wide23_n1440"]:
        inp = R.make_input(name)
        ref = R.reference_figures(name).ref
        out, facts = L.debug_tile_plan(inp.T, inp.pattern)
        assert np.array_equal(np.tril(out != 0), ref.pattern)
        assert facts["n_assembled"] == ref.n_assembled
        assert facts["n_tiles"] - facts["n_assembled"] == len(ref.fill)
        assert facts["n_split"] == len(ref.split_targets)
        assert facts["n_levels"] == ref.n_levels


def test_patterns_have_what_they_were_chosen_for(L):
    facts = {k: L.debug_tile_plan(P().shape[0], P())[1] for k, P in PATTERNS.items()}
    for k, f in facts.items():
        print(k, f)
        assert f["dag_valid"] == 1, k
        assert f["n_cont_tasks"] > 0, k           # continuation targets in every plan with a parent
    # dense: a chain -- as many levels as tiles a side, no fill
    assert facts["dense4"]["n_levels"] == 4 and facts["dense4"]["n_tiles"] == facts["dense4"]["n_assembled"] == 10
    # arrow, nd12, wide23: fill tiles, an elimination tree (fewer levels than tile rows), and the
    # fill-first store is allowed on each
    for k, n_fill in (("arrow", 2), ("nd12", 4), ("wide23", 7)):
        f = facts[k]
        assert f["n_tiles"] - f["n_assembled"] == n_fill, k
        assert f["n_levels"] < f["tiles_per_side"], k
        assert f["fill_first_ok"] == 1, k
    assert facts["nd12"]["n_assembled"] == 41 and facts["nd12"]["n_levels"] == 5
    assert facts["nd12"]["n_split"] == 0          # (k-lists are split per level: see nd12's docstring)
    # forest: independent columns, two levels; seven of them update (7, 7) at once: one split target
    assert facts["forest8"]["n_levels"] == 2 and facts["forest8"]["n_tiles"] == facts["forest8"]["n_assembled"]
    assert facts["forest8"]["n_split"] == 1
    # wide23: 16 leaves in one level, six split targets, one of them a fill tile
    assert facts["wide23"]["n_split"] == 6 and facts["wide23"]["n_levels"] == 5
    ref = R.reference_figures("wide23_n1440").ref
    assert (21, 20) in ref.fill and (21, 20, 0) in ref.split_targets


@pytest.mark.parametrize("name", sorted(TWO_PHASE))
def test_two_phase_plans_are_valid(L, name):
    pat, cls = TWO_PHASE[name]
    P = PATTERNS[pat]()
    out, f = L.debug_tile_plan(P.shape[0], P, cls)
    print(name, f)
    assert f["dag_valid"] == 1
    assert 0 < f["phase_split"] < f["n_dag_tasks"]
    assert f["grid"][0] > 0 and f["grid"][1] > 0
    assert f["fill_first_ok"] == 0                 # (the fill-first store is a one-phase matter)
    assert np.array_equal(np.tril(out != 0), R.tile_fill(R.taken(P)))


def test_class_one_columns_must_be_closed_under_the_parent(L):
    P = R.nd12()
    with pytest.raises(L.LMError):
        L.debug_tile_plan(12, P, [0] * 8 + [1, 0, 0, 0])     # column 8's parent 10 is class 0
    with pytest.raises(L.LMError):
        L.debug_tile_plan(12, P, [0] * 10 + [1, 0])          # the last column is every column's ancestor


@pytest.mark.parametrize("name", sorted(R.INPUTS))
def test_reference_error_caps(name):
    """eta_ref and omega_ref of every input under the caps of its class, LAPACK at rounding level,
    and the smallest pivot of the longdouble factor."""
    inp = R.make_input(name)
    f = R.reference_figures(name)
    cls = R.input_class(name)
    piv, failed = R.cholesky_ld(inp.A, inp.pattern)
    d_min = float(np.sqrt(piv.min()))
    print(f"{name}: cond {np.linalg.cond(inp.A):.1e} eta_ref {f.eta_ref:.2e} (componentwise {f.comp_ref:.2e}) "
          f"omega_ref {f.omega_ref:.2e} | lapack eta {f.eta_lapack:.2e} ({f.comp_lapack:.2e}) omega "
          f"{f.omega_lapack:.2e} | smallest pivot {d_min:.2e} (squared {piv.min():.2e})")
    assert failed == -1
    assert f.eta_ref <= R.ETA_REF_CAP[cls]
    assert f.omega_ref <= R.OMEGA_REF_CAP[cls]
    assert f.eta_lapack <= 1e-15 and f.omega_lapack <= 2e-15
    # the pivot is the factor's diagonal entry L_kk; the Schur complement it is the root of is
    # its square, and a unit-diagonal matrix of condition 1e12 has one near 1e-11 at best
    assert d_min >= R.MIN_PIVOT


def test_conditioning_classes():
    """The three classes are about 1e2, 1e8 and 1e12 on nd12; the fourth spreads its diagonal."""
    for cls, lo, hi in (("c2", 1e1, 1e4), ("c8", 1e7, 1e9), ("c12", 1e11, 1e13)):
        c = np.linalg.cond(R.make_input(f"nd12_n740_{cls}").A)
        assert lo <= c <= hi, (cls, c)
    d = np.diag(R.make_input("nd12_n740_lm").A)
    assert d.min() < 1.0 + 1e-5 and d.max() > 1e5


def test_first_failed_pivot_of_the_reference():
    """cholesky_ld and the restatement agree on a lowered diagonal entry."""
    inp = R.make_input("nd12_n740_c2")
    piv, _ = R.cholesky_ld(inp.A, inp.pattern)
    for r in (0, 63, 64, 300, 739):
        A = inp.A.copy()
        A[r, r] -= 1.5 * piv[r]
        _, failed = R.cholesky_ld(A, inp.pattern)
        assert failed == r
        assert R.tile_llt(A, inp.b, inp.pattern).info == r + 1
