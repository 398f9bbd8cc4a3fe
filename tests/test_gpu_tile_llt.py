"""GPU tests of the tile Cholesky and solve, one stage alone (arslam_debug_tile_llt), against
extended precision: k_factor_dag / k_bsolve_dag (executor 1) and the level launches (executor 0) on
sparse tile plans -- elimination trees, fill tiles, split targets, the fill-first store, two-phase
plans -- and on ill-conditioned input, where an LM solve would correct a wrong step and hide it.

Tolerance (the rule of test_gpu_lm_cov.py): with eta the largest per-tile backward error of the
factor and omega the componentwise backward error of the solve (tests/llt_ref.py, evaluated in
np.longdouble),
    eta_dev   <= 16 max(eta_ref, eta_lapack),     omega_dev <= 16 max(omega_ref, omega_lapack),
eta_ref / omega_ref the float64 numpy restatement's of the device's tile algorithm on the same
input, eta_lapack / omega_lapack np.linalg.cholesky's with a longdouble substitution.  16 is the
room for another summation order and for MFMA against BLAS.  A dropped update is O(1); a lost
Newton step of a reciprocal pivot is about 1e-12 and shows on the well-conditioned class.

Every case prints its figures on a line starting "tile_llt:"; profiles/tile_llt/device_errors.txt
is that record from an MI355X.
"""
import numpy as np
import pytest

import llt_ref as R
from llt_ref import TWO_PHASE

pytestmark = pytest.mark.gpu

EXECUTORS = [0, 1]
FILL_FIRST_INPUTS = ["arrow_n340", "nd12_n704_c8", "nd12_n740_c12", "nd12_n767_lm", "wide23_n1440"]
TWO_PHASE_INPUT = {"nd12": "nd12_n740_c8", "wide23": "wide23_n1440"}


def _run(lm, name, executor, **kw):
    inp = R.make_input(name)
    return lm.debug_tile_llt(inp.A, inp.b, inp.pattern, executor=executor, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(lm, name, executor, label, col_class=None):
    """One device run held to the tolerance rule; returns (L, y, facts)."""
    inp = R.make_input(name)
    f = R.reference_figures(name, None if col_class is None else tuple(col_class))
    L, y, info, pat, facts = _run(lm, name, executor, col_class=col_class)
    assert info == 0, info
    assert np.array_equal(np.tril(pat != 0), f.ref.pattern)           # the reference's symbolic fill
    assert facts["n_tiles"] == int(f.ref.pattern.sum())
    if col_class is None:
        assert facts["n_assembled"] == f.ref.n_assembled
    on = np.kron(f.ref.pattern, np.ones((64, 64)))[:inp.n, :inp.n] != 0
    assert np.all(L[~on] == 0.0)                                      # exactly 0 off the pattern
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(y))
    eta, comp = R.factor_error(inp.A, L, f.ref.pattern)
    omega = R.solve_error(inp.A, inp.b, L, y)
    tol_eta, tol_omega = R.tolerances(f)
    print(f"tile_llt: {label:<12} {name:<15} executor {executor} | eta {eta:.2e} (componentwise {comp:.2e}) ref "
          f"{f.eta_ref:.2e} lapack {f.eta_lapack:.2e} bound {tol_eta:.2e} | omega {omega:.2e} ref {f.omega_ref:.2e} "
          f"lapack {f.omega_lapack:.2e} bound {tol_omega:.2e} | grid {facts['grid']}")
    assert eta <= tol_eta, (eta, tol_eta)
    assert omega <= tol_omega, (omega, tol_omega)
    return L, y, facts


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 191])
def test_tile_edges_dense(lm, n, executor):
    """n = 63: the rhs row is the last row of the only tile; n = 64, 128: it is alone in a tile row
    that has no real rows; 65, 127, 191: one real row, or one row short, in the last tile."""
    _check(lm, f"dense_n{n}", executor, "edge")


SPARSE = ["arrow_n340", "forest_n450", "wide23_n1440"] + [k for k in sorted(R.INPUTS) if k.startswith("nd12_")]


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("name", SPARSE)
def test_sparse_plans(lm, name, executor):
    _, _, facts = _check(lm, name, executor, "sparse")
    ref = R.reference_figures(name).ref
    assert facts["n_split"] == len(ref.split_targets)
    assert facts["n_levels"] == ref.n_levels


@pytest.mark.parametrize("name", FILL_FIRST_INPUTS)
def test_fill_first_store(lm, name):
    """The fill tiles hold quiet NaNs and the factorization stores their first update instead of
    reading them (first_store = n_assembled, as the solver runs): any read of a fill tile before its
    first store would poison the factor.  Bit-identical to the run over zeroed fill tiles."""
    L0, y0, info0, _, facts = _run(lm, name, 1)
    L1, y1, info1, _, _ = _run(lm, name, 1, fill_first=True)
    assert facts["fill_first_ok"] == 1 and facts["n_tiles"] > facts["n_assembled"]
    assert info0 == 0 and info1 == 0
    assert np.all(np.isfinite(L1)) and np.all(np.isfinite(y1))
    assert _same_bits(L0, L1) and _same_bits(y0, y1)


def test_fill_first_store_needs_its_plan_and_executor(lm):
    inp = R.make_input("nd12_n740_c2")
    with pytest.raises(lm.LMError):
        lm.debug_tile_llt(inp.A, inp.b, inp.pattern, executor=0, fill_first=True)
    with pytest.raises(lm.LMError):   # a two-phase plan never has fill_first_ok
        lm.debug_tile_llt(inp.A, inp.b, inp.pattern, executor=1, fill_first=True, col_class=TWO_PHASE["nd12_top2"][1])


@pytest.mark.parametrize("case", sorted(TWO_PHASE))
def test_two_phase_plans(lm, case):
    """Phase 0 (the class-0 columns and their updates of the top tiles), then phase 1, as a
    multi-rank solve launches them -- on one rank, so with no exchange between."""
    pat, cls = TWO_PHASE[case]
    name = TWO_PHASE_INPUT[pat]
    L, y, facts = _check(lm, name, 1, case, col_class=cls)
    assert 0 < facts["phase_split"] < facts["n_dag_tasks"] and min(facts["grid"]) > 0
    L1, y1, _, _, _ = _run(lm, name, 1)
    print(f"tile_llt: {case:<12} {name:<15} bits equal the one-phase run: L {_same_bits(L, L1)} y {_same_bits(y, y1)}")


@pytest.mark.parametrize("name", ["nd12_n740_c8", "wide23_n1440"])
def test_schedule_independence(lm, name, monkeypatch):
    """Every tile sums its updates in a fixed order, so the grid and the number of workgroups that
    ever start change nothing: L and y are bit-identical to the default grid's."""
    L0, y0, info0, _, facts = _run(lm, name, 1)
    assert info0 == 0
    for grid in ("1", "3"):
        monkeypatch.setenv("ARSLAM_DAG_GRID", grid)
        L, y, info, _, f = _run(lm, name, 1)
        assert f["grid"][0] == int(grid) < facts["grid"][0]
        assert info == 0 and _same_bits(L, L0) and _same_bits(y, y0), grid
    monkeypatch.delenv("ARSLAM_DAG_GRID")
    try:
        for k in (1, 2):
            lm.debug_dag_workgroup_limit(k)
            L, y, info, _, _ = _run(lm, name, 1)
            assert info == 0 and _same_bits(L, L0) and _same_bits(y, y0), k
    finally:
        lm.debug_dag_workgroup_limit(0)


# rows of nd12 at n = 740: the first tile's first and last row, the second tile's first, the
# last real row (in the rhs row's tile), a leaf (column 5), separator 8, column 10
PIVOT_INPUT = "nd12_n740_c2"
PIVOT_ROWS = {"row0": 0, "row63": 63, "row64": 64, "last": 739, "leaf5": 350, "sep8": 8 * 64 + 10, "col10": 10 * 64 + 40}
_pivots = {}


def _reference_pivots():
    if not _pivots:
        inp = R.make_input(PIVOT_INPUT)
        _pivots["p"], failed = R.cholesky_ld(inp.A, inp.pattern)
        assert failed == -1
    return _pivots["p"]


@pytest.mark.parametrize("executor", EXECUTORS)
@pytest.mark.parametrize("where", sorted(PIVOT_ROWS))
def test_failed_pivot(lm, where, executor):
    """One diagonal entry lowered by 1.5 times its exact pivot: the pivot becomes -1/2 of its value,
    a margin no rounding crosses.  info = k + 1, k the longdouble Cholesky's first failure."""
    inp = R.make_input(PIVOT_INPUT)
    r = PIVOT_ROWS[where]
    A = inp.A.copy()
    A[r, r] -= 1.5 * _reference_pivots()[r]
    piv, k = R.cholesky_ld(A, inp.pattern)
    assert k == r and piv[k] < -0.4 * _reference_pivots()[r]
    _, _, info, _, _ = lm.debug_tile_llt(A, inp.b, inp.pattern, executor=executor)
    print(f"tile_llt: pivot        {where:<15} executor {executor} | reference fails at {k}, info {info}")
    assert info == k + 1


@pytest.mark.parametrize("executor", EXECUTORS)
def test_failed_pivot_under_a_positive_diagonal(lm, executor):
    """The diagonal stays 1 everywhere; a coupling of 1.2 between rows 299 and 300 makes the
    Schur complement fail."""
    inp = R.make_input(PIVOT_INPUT)
    A = inp.A.copy()
    A[300, 299] = A[299, 300] = 1.2
    assert np.all(np.diag(A) > 0.99)
    piv, k = R.cholesky_ld(A, inp.pattern)
    assert k >= 0 and piv[k] < -0.1
    _, _, info, _, _ = lm.debug_tile_llt(A, inp.b, inp.pattern, executor=executor)
    print(f"tile_llt: pivot        schur           executor {executor} | reference fails at {k}, info {info}")
    assert info == k + 1


@pytest.mark.parametrize("executor", EXECUTORS)
def test_zero_rhs_gives_zero(lm, executor):
    inp = R.make_input("nd12_n740_c8")
    _, y, info, _, _ = lm.debug_tile_llt(inp.A, np.zeros(inp.n), inp.pattern, executor=executor)
    assert info == 0 and np.all(y == 0.0)
