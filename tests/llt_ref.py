"""numpy reference of the tile Cholesky and solve of the reduced system (test helper, no GPU).

What arslam_debug_tile_llt (include/arslam_lm_debug.h) is held to by tests/test_gpu_tile_llt.py:

  patterns   named lower tile patterns, each chosen for something a dense pattern's plan lacks;
  inputs     SPD matrices restricted to a pattern, equilibrated, in four conditioning classes;
  tile_llt   the device's tile algorithm (llt_tile.h, llt_levels.hip, llt_dag.hip, llt_plan.cpp) restated in float64;
  metrics    backward errors of a factor (eta) and of a solve (omega), evaluated in np.longdouble;
  pivots     a longdouble Cholesky, for the first failed pivot and the smallest pivot.

The device multiplies by explicit inverses where LAPACK substitutes, so its backward error grows
with the conditioning of the diagonal tiles; the restatement has the same operations and is the
yardstick for that growth.  What the device code does, and tile_llt restates:

  POTRF 64    right-looking over 16-column panels.  A 16 x 16 diagonal block is factored by one
              pass of Gaussian elimination (diag16): the multipliers, -a_ij times a Newton-refined
              reciprocal of the pivot, build U = Dg Lu^T and Lu^-1 together, then L = U^T Dg^-1/2
              and the EXPLICIT inverse L16^-1 = Dg^-1/2 Lu^-1.  The 16-row blocks below are
              MULTIPLIED by L16^-T; the trailing blocks get the panel's product subtracted.
  TRSM 64     X L_kk^T = A_ik by SUBSTITUTION over the four 16-column blocks, each block's own
              16 x 16 solve a MULTIPLICATION by the explicit L16^-T.
  update      tile (i, j) -= sum over the level's columns k of L_ik L_jk^T, the levels applied in
              order; a k-list longer than kSplitMin is cut into chunks whose partial products are
              summed in chunk order.
  forward     the right-hand side rides along as row n (pivot 1e300): it is solved by the TRSMs.
  INV 64      the EXPLICIT 64 x 64 inverse X_kk of L_kk, assembled from the four L16^-1.
  backward    root first: y_k = X_kk^T (z_k - sum_i L_ik^T y_i), a MULTIPLICATION by X_kk; the
              ancestors i are summed farthest first; rows >= n are masked to zero.

Summation order inside a product (MFMA against BLAS) is not restated; the tolerance rule's factor
16 is the room for it.
"""
import functools

import numpy as np

from lm_cov_ref import tile_fill

TILE = 64
BLK = 16
K_SPLIT_MIN = 6   # llt_plan.cpp kSplitMin: k-lists longer than this are split

LD = np.longdouble


# ---- patterns ----

def tiles_of(n):
    """Tiles a side for n real rows: the right-hand side is row n."""
    return (n + 1 + TILE - 1) // TILE


def dense(T):
    """Every lower tile: the plan is a chain, T levels, no fill."""
    return np.tril(np.ones((T, T), bool))


def arrow():
    """test_lm_cov.arrow_pattern: 6 tile rows, two leaves {0, 1} and {2, 3} under separator 4 and
    the last row; tiles (4, 1) and (4, 3) are fill.  Run at n = 340, the rhs row cuts the last tile."""
    from test_lm_cov import arrow_pattern
    return arrow_pattern()


def nd12():
    """A two-level nested dissection on 12 tile rows: leaves {0, 1}, {2, 3}, {4, 5}, {6, 7} (the
    couplings (1, 0), (3, 2), (5, 4), (7, 6)), separator 8 over columns 0-3, separator 9 over
    columns 4-7, row 10 over {0, 2, 3, 4, 6, 7} and row 11 over {0, 1, 3, 4, 5, 7, 10}.

    37 tiles as written.  Row 11 is the last tile row at every n it is run at (704 .. 767), and the
    entries take the whole last tile row (it holds the right-hand side), so the plan has 41
    assembled tiles and 4 fill tiles, (10, 1), (10, 5), (10, 8), (10, 9): 45 in all, 5 levels, and
    fill_first_ok.  The k-lists of (10, 10), (11, 10) and (11, 11) have 10, 10 and 11 columns, but
    the planner splits a k-list per LEVEL, and no level gives one of them more than 4 columns:
    nothing is split here (n_split = 0).  The split targets are wide23's."""
    P = np.eye(12, dtype=bool)
    for i, j in [(1, 0), (3, 2), (5, 4), (7, 6)]:
        P[i, j] = True
    P[8, 0:4] = True
    P[9, 4:8] = True
    P[10, [0, 2, 3, 4, 6, 7]] = True
    P[11, [0, 1, 3, 4, 5, 7, 10]] = True
    return P


def forest(T):
    """Block diagonal, coupled only through the last row: T - 1 independent columns, 2 levels."""
    P = np.eye(T, dtype=bool)
    P[T - 1, :] = True
    return P


def wide23():
    """16 independent single-column leaves under two separator levels, 23 tile rows: separators
    16 .. 19 each over four leaves (4 g .. 4 g + 3), separator 20 over leaves 0 .. 7, separator 21
    over all 16 leaves, and the last row 22.  All 16 leaves are one level, so many workgroups and
    claims are in flight at once, and the level gives (20, 20), (21, 21), (22, 20), (22, 21),
    (22, 22) and (21, 20) k-lists of 8 or 16 columns: six split targets.  Seven fill tiles,
    (20, 16), (20, 17), (21, 16 .. 19) and (21, 20) -- the last one a fill tile AND a split target,
    so the fill-first store runs in a chunk reducer too.  fill_first_ok."""
    T = 23
    P = np.eye(T, dtype=bool)
    for g in range(4):
        P[16 + g, 4 * g:4 * g + 4] = True
    P[20, 0:8] = True
    P[21, 0:16] = True
    P[22, :] = True
    return P


PATTERNS = {"dense4": lambda: dense(4), "arrow": arrow, "nd12": nd12, "forest8": lambda: forest(8), "wide23": wide23}
# two-phase column classes (0 own subtree, 1 the replicated top): the top separators and the last
# row are class 1 -- pattern name, classes
TWO_PHASE = {"nd12_top2": ("nd12", [0] * 10 + [1] * 2), "nd12_top4": ("nd12", [0] * 8 + [1] * 4),
             "wide23_top3": ("wide23", [0] * 20 + [1] * 3), "wide23_top7": ("wide23", [0] * 16 + [1] * 7)}


def taken(pattern, T=None):
    """The lower pattern the entries factor: the given one (None: dense), the diagonal tiles and
    the whole last tile row."""
    P = dense(T) if pattern is None else np.tril(np.asarray(pattern) != 0)
    T = P.shape[0]
    P[np.arange(T), np.arange(T)] = True
    P[T - 1, :] = True
    return P


def elimination_levels(P):
    """(parent, height) of the tile elimination tree of a filled lower pattern."""
    T = P.shape[0]
    parent = -np.ones(T, np.int64)
    height = np.zeros(T, np.int64)
    for k in range(T):
        below = np.nonzero(P[k + 1:, k])[0]
        if len(below):
            parent[k] = k + 1 + below[0]
    for k in range(T):
        if parent[k] >= 0:
            height[parent[k]] = max(height[parent[k]], height[k] + 1)
    return parent, height


# ---- inputs ----

CLASSES = {          # (eps, delta, LM diagonal on top)
    "c2": (1.0, 1e-3, False),      # condition number about 1e2
    "c8": (1e-3, 1e-8, False),     # about 1e8
    "c12": (1e-5, 1e-12, False),   # about 1e12
    "lm": (1e-3, 1e-8, True),      # c8 with an LM diagonal spread over 1e-6 .. 1e6 added on top:
}                                  # the system after a run of rejected steps


class Input:
    """A (n, n) SPD, zero off the pattern's tiles; b (n,); pattern: the lower (T, T) pattern given."""

    def __init__(self, name, A, b, pattern):
        self.name, self.A, self.b, self.pattern = name, A, b, pattern
        self.n = A.shape[0]
        self.T = tiles_of(self.n)


def spd_on_pattern(pattern, n, cls, seed):
    """A sum over the pattern's tile pairs (i, j), i >= j, of J'J on the real rows of tiles i and
    j, the columns of J a common vector plus eps x noise; plus delta I; equilibrated to a unit
    diagonal; the class "lm" then adds diag(10^u), u uniform in [-6, 6]."""
    eps, delta, lm_diag = CLASSES[cls]
    rng = np.random.default_rng(seed)
    P = np.tril(np.asarray(pattern) != 0)
    T = P.shape[0]
    assert T == tiles_of(n)
    A = np.zeros((n, n))
    for i in range(T):
        for j in range(i + 1):
            if not (P[i, j] or i == j):
                continue
            rows = np.unique(np.concatenate([np.arange(TILE * i, min(TILE * (i + 1), n)),
                                             np.arange(TILE * j, min(TILE * (j + 1), n))]))
            if len(rows) == 0:
                continue
            m = len(rows) + 8
            J = rng.standard_normal(m)[:, None] + eps * rng.standard_normal((m, len(rows)))
            A[np.ix_(rows, rows)] += J.T @ J
    A += delta * np.mean(np.diag(A)) * np.eye(n)
    d = 1.0 / np.sqrt(np.diag(A))
    A = A * np.outer(d, d)
    A = 0.5 * (A + A.T)
    A[np.arange(n), np.arange(n)] = 1.0
    if lm_diag:
        A[np.arange(n), np.arange(n)] += 10.0 ** rng.uniform(-6.0, 6.0, n)
    b = A @ rng.standard_normal(n)
    return A, b


# name -> (pattern builder, n, class): every input of the GPU tests
def _dense_for(n):
    return lambda: dense(tiles_of(n))


INPUTS = {}
for _n in (1, 63, 64, 65, 127, 128, 191):
    INPUTS[f"dense_n{_n}"] = (_dense_for(_n), _n, "c2")
INPUTS["arrow_n340"] = (arrow, 340, "c8")
for _n in (704, 740, 767):
    for _c in CLASSES:
        INPUTS[f"nd12_n{_n}_{_c}"] = (nd12, _n, _c)
INPUTS["forest_n450"] = (lambda: forest(8), 450, "c8")
INPUTS["wide23_n1440"] = (wide23, 1440, "c8")

# the restatement's own backward errors stay under these, per class: about 4 x the largest
# measured on tile_llt over the inputs above (eta / omega: c2 1.7e-16 / 1.0e-16, c8 7.2e-15 /
# 1.4e-16, c12 7.9e-13 / 8.2e-17, lm 9.6e-16 / 8.2e-16).  eta grows with the condition number
# as the explicit inverses predict; omega does not, and LAPACK's are 4e-16 at most on all of them.
ETA_REF_CAP = {"c2": 7e-16, "c8": 3e-14, "c12": 3e-12, "lm": 4e-15}
OMEGA_REF_CAP = {"c2": 5e-16, "c8": 6e-16, "c12": 5e-16, "lm": 4e-15}
# the smallest diagonal entry L_kk of the longdouble factor of every input: none sits on the
# border between a positive and a failed pivot (rounding moves a pivot by about 1e-16)
MIN_PIVOT = 1e-7


@functools.lru_cache(maxsize=None)
def make_input(name):
    build, n, cls = INPUTS[name]
    P = build()
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    A, b = spd_on_pattern(P, n, cls, seed)
    A.setflags(write=False)
    b.setflags(write=False)
    return Input(name, A, b, P)


def input_class(name):
    return INPUTS[name][2]


# ---- the restatement ----

def _blk(X, p, q):
    return X[BLK * p:BLK * (p + 1), BLK * q:BLK * (q + 1)]


def diag16(Ablk):
    """One Gaussian elimination pass over the 16 x 16 block (lower triangle valid): returns
    (L16, L16^-1, pivots).  Rows below pivot j: row_i += nf row_j over all 16 columns, nf =
    -a_ij (1 / a_jj); then entry (i, j) becomes nf -- so row i ends as U (columns >= i) and
    Lu^-1 (columns < i)."""
    x = np.tril(Ablk) + np.tril(Ablk, -1).T
    for j in range(BLK):
        r = 1.0 / x[j, j]          # (the device refines v_rcp_f64 to 1 - e^3: a rounded reciprocal)
        nf = -x[j + 1:, j] * r
        x[j + 1:, :] += nf[:, None] * x[j, :][None, :]
        x[j + 1:, j] = nf
    piv = np.diag(x).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.sqrt(piv)
        rd = 1.0 / d
    L = np.triu(x, 1).T * rd[None, :] + np.diag(d)
    Li = np.tril(x, -1) * rd[:, None] + np.diag(rd)
    return L, Li, piv


def potrf64(D):
    """In place on the 64 x 64 tile (lower triangle valid): L in the lower triangle, 0 above.
    Returns (the four L16^-1, the 64 pivots)."""
    Li, piv = [], np.zeros(TILE)
    for p in range(4):
        L16, Li16, pv = diag16(_blk(D, p, p))
        _blk(D, p, p)[:] = L16
        Li.append(Li16)
        piv[BLK * p:BLK * (p + 1)] = pv
        for q in range(p + 1, 4):
            _blk(D, q, p)[:] = _blk(D, q, p) @ Li16.T          # explicit inverse
        for i in range(p + 1, 4):
            for c in range(p + 1, i + 1):
                _blk(D, i, c)[:] -= _blk(D, i, p) @ _blk(D, c, p).T
    D[:] = np.tril(D)
    return Li, piv


def trsm64(X, Lkk, Li):
    """X <- X L_kk^-T in place: substitution over the 16-column blocks, explicit 16 x 16 inverses."""
    for p in range(4):
        if p:
            X[:, BLK * p:BLK * (p + 1)] -= X[:, :BLK * p] @ Lkk[BLK * p:BLK * (p + 1), :BLK * p].T
        X[:, BLK * p:BLK * (p + 1)] = X[:, BLK * p:BLK * (p + 1)] @ Li[p].T


def trinv64(Lkk, Li):
    """L_kk^-1 from the four 16 x 16 inverses: X_qq = Li_q, X_pq = -Li_p sum_{r=q}^{p-1} L_pr X_rq."""
    X = np.zeros((TILE, TILE))
    for q in range(4):
        _blk(X, q, q)[:] = Li[q]
        for p in range(q + 1, 4):
            acc = np.zeros((BLK, BLK))
            for r in range(q, p):
                acc += _blk(Lkk, p, r) @ _blk(X, r, q)
            _blk(X, p, q)[:] = -(Li[p] @ acc)
    return X


class TileLLT:
    """L (n, n) lower, 0 off the factor's tiles; y (n,); pattern: the filled lower (T, T) pattern;
    info: 0, or k + 1 for the first pivot k that is not positive (y is then meaningless);
    n_assembled, fill: the plan's tile counts and fill tiles; split_targets: the (i, j, level) cut
    into chunks; n_levels."""


def tile_llt(A, b, pattern=None, col_class=None):
    """The device's factorization and solve of A y = b on a tile pattern, in float64 numpy.
    col_class: None, or T values 0 / 1 -- the two-phase plan: every level of the class-0 columns,
    then every level of the class-1 columns."""
    n = A.shape[0]
    T = tiles_of(n)
    N = T * TILE
    P0 = taken(pattern, T)
    P = tile_fill(P0)
    _, height = elimination_levels(P)
    nlev = int(height.max()) + 1
    cls = np.zeros(T, np.int64) if col_class is None else np.asarray(col_class, np.int64)
    M = np.zeros((N, N))
    M[:n, :n] = np.tril(A) * np.kron(P0, np.ones((TILE, TILE)))[:n, :n]
    M[n, :n] = b
    M[n, n] = 1e300
    M[np.arange(n + 1, N), np.arange(n + 1, N)] = 1.0

    def t(i, j):
        return M[TILE * i:TILE * (i + 1), TILE * j:TILE * (j + 1)]

    out = TileLLT()
    out.pattern = P
    out.n_assembled = int(P0.sum())
    out.fill = [(i, j) for i in range(T) for j in range(i + 1) if P[i, j] and not P0[i, j]]
    out.n_levels = nlev * (1 if col_class is None else 2)
    out.split_targets = []
    out.info = 0
    out.pivots = np.ones(N)
    X = [None] * T
    for lp in range(nlev * (1 if col_class is None else 2)):
        lev, phase = lp % nlev, lp // nlev
        cols = [k for k in range(T) if height[k] == lev and cls[k] == phase]
        klists = {}
        for k in cols:
            Li, piv = potrf64(t(k, k))
            out.pivots[TILE * k:TILE * (k + 1)] = piv
            bad = np.nonzero(~(piv > 0.0))[0]
            if len(bad) and TILE * k + bad[0] < n:
                first = TILE * k + int(bad[0]) + 1
                out.info = first if out.info == 0 else min(out.info, first)
            X[k] = trinv64(t(k, k), Li)
            rows = [i for i in range(k + 1, T) if P[i, k]]
            for i in rows:
                trsm64(t(i, k), t(k, k), Li)
            for a, i in enumerate(rows):
                for j in rows[:a + 1]:
                    klists.setdefault((i, j), []).append(k)
        for (i, j), ks in klists.items():
            m = len(ks)
            chunks = [ks]
            if m > K_SPLIT_MIN:
                nch = min(255, int(np.ceil(np.sqrt(m))))
                ch = (m + nch - 1) // nch
                chunks = [ks[c:c + ch] for c in range(0, m, ch)]
                out.split_targets.append((i, j, lp))
            acc = np.zeros((TILE, TILE))
            for chunk in chunks:        # the partial products, summed in chunk order
                part = np.zeros((TILE, TILE))
                for k in chunk:
                    part += t(i, k) @ t(j, k).T
                acc = acc + part if len(chunks) > 1 else part
            t(i, j)[:] -= acc
            if i == j:
                t(i, j)[:] = np.tril(t(i, j))
    # backward solve, root level first; z = row n of the factor
    kr, r0 = n // TILE, n % TILE
    y = np.zeros(N)
    for lev in range(nlev - 1, -1, -1):
        for k in [k for k in range(T) if height[k] == lev]:
            acc = np.zeros(TILE)
            for i in [i for i in range(T - 1, k, -1) if P[i, k]]:   # farthest ancestor first
                acc += t(i, k).T @ y[TILE * i:TILE * (i + 1)]
            rhs = M[n, TILE * k:TILE * (k + 1)] - acc
            live = TILE * k + np.arange(TILE) < n
            rhs = np.where(live, rhs, 0.0)
            y[TILE * k:TILE * (k + 1)] = np.where(live, X[k].T @ rhs, 0.0)
    out.L = (np.tril(M) * np.kron(P, np.ones((TILE, TILE))))[:n, :n]
    out.y = y[:n]
    assert kr == T - 1 and r0 < TILE
    return out


# ---- metrics, in extended precision ----

def _tile_rows(i, n):
    return slice(TILE * i, min(TILE * (i + 1), n))


def factor_error(A, L, P):
    """(eta, componentwise): eta = max over the factor's tiles of |(A - L L')_tile|_F /
    |(|L| |L|')_tile|_F; componentwise = max over their entries of |A - L L'| / (|L| |L|').
    The products run over the tiles of P only and in np.longdouble."""
    n = A.shape[0]
    T = P.shape[0]
    if not np.all(np.isfinite(L)):
        return np.inf, np.inf
    Ll = L.astype(LD)
    La = np.abs(Ll)
    eta = comp = LD(0)
    for i in range(T):
        ri = _tile_rows(i, n)
        if ri.start >= n:
            continue
        for j in range(i + 1):
            if not P[i, j]:
                continue
            rj = _tile_rows(j, n)
            R = A[ri, rj].astype(LD)
            G = np.zeros(R.shape, LD)
            for k in range(j + 1):
                if P[i, k] and P[j, k]:
                    rk = _tile_rows(k, n)
                    R = R - Ll[ri, rk] @ Ll[rj, rk].T
                    G = G + La[ri, rk] @ La[rj, rk].T
            if i == j:
                R, G = np.tril(R), np.tril(G)
            nr, ng = np.sqrt((R * R).sum()), np.sqrt((G * G).sum())
            # (a tile the last row takes where A and the factor are both zero: 0 / 0 counts 0)
            eta = max(eta, nr / ng if ng > 0 else (LD(0) if nr == 0 else LD(np.inf)))
            if np.any((G == 0) & (R != 0)):
                comp = LD(np.inf)
            nz = G > 0
            if nz.any():
                comp = max(comp, np.max(np.abs(R[nz]) / G[nz]))
    return float(eta), float(comp)


def solve_error(A, b, L, y):
    """omega = max_i |b - A y|_i / (|L| |L'| |y|)_i, in np.longdouble."""
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(y))):
        return np.inf
    yl = y.astype(LD)
    r = np.abs(b.astype(LD) - _matvec_ld(A, yl))
    La = np.abs(L).astype(LD)
    den = La @ (La.T @ np.abs(yl))
    nz = den > 0
    if not nz.any():
        return 0.0
    return float(np.max(r[nz] / den[nz]))


def _matvec_ld(A, x):
    # (a float64 matrix times a longdouble vector, without converting the whole matrix at once)
    out = np.zeros(A.shape[0], LD)
    for r in range(0, A.shape[0], 256):
        out[r:r + 256] = A[r:r + 256].astype(LD) @ x
    return out


def solve_ld(L, b):
    """y of L L' y = b by substitution in np.longdouble (L: a float64 factor)."""
    n = L.shape[0]
    Ll = L.astype(LD)
    z = np.zeros(n, LD)
    for i in range(n):
        z[i] = (LD(b[i]) - Ll[i, :i] @ z[:i]) / Ll[i, i]
    y = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        y[i] = (z[i] - Ll[i + 1:, i] @ y[i + 1:]) / Ll[i, i]
    return y.astype(np.float64)


def cholesky_ld(A, pattern=None, stop_at_failure=True):
    """Left-looking Cholesky of A in np.longdouble, skipping the tile columns the filled pattern
    rules out.  Returns (pivots (n,) -- the squared diagonal of the factor, up to and including
    the first non-positive one; first_failed: its row, or -1)."""
    n = A.shape[0]
    T = tiles_of(n)
    P = tile_fill(taken(pattern, T))
    Ll = np.zeros((n, n), LD)
    piv = np.zeros(n, LD)
    for j in range(n):
        tj = j // TILE
        cols = np.concatenate([np.arange(TILE * k, TILE * (k + 1)) for k in range(tj) if P[tj, k]] +
                              [np.arange(TILE * tj, j)]).astype(np.int64)
        c = A[j:, j].astype(LD)
        if len(cols):
            c = c - Ll[j:, cols] @ Ll[j, cols]
        piv[j] = c[0]
        if not c[0] > 0:
            if stop_at_failure:
                return piv[:j + 1].astype(np.float64), j
            raise ValueError("cholesky_ld: pivot %d is not positive" % j)
        Ll[j:, j] = c / np.sqrt(c[0])
    return piv.astype(np.float64), -1


class Figures:
    """eta_ref, omega_ref (the restatement's), eta_lapack, omega_lapack, their componentwise
    companions comp_ref, comp_lapack, and ref: the TileLLT."""


@functools.lru_cache(maxsize=None)
def reference_figures(name, col_class=None):
    """The yardsticks of one input, computed once: the restatement's and LAPACK's backward errors."""
    inp = make_input(name)
    ref = tile_llt(inp.A, inp.b, inp.pattern, None if col_class is None else list(col_class))
    assert ref.info == 0
    f = Figures()
    f.ref = ref
    f.eta_ref, f.comp_ref = factor_error(inp.A, ref.L, ref.pattern)
    f.omega_ref = solve_error(inp.A, inp.b, ref.L, ref.y)
    Ll = np.linalg.cholesky(inp.A)
    # (LAPACK's factor is exactly zero off the filled pattern: zeros in, zeros out)
    f.eta_lapack, f.comp_lapack = factor_error(inp.A, Ll, ref.pattern)
    f.omega_lapack = solve_error(inp.A, inp.b, Ll, solve_ld(Ll, inp.b))
    return f


TOL_FACTOR = 16.0   # room for another summation order and for MFMA against BLAS


def tolerances(f):
    """(eta bound, omega bound) of a device result on the input whose figures are f."""
    return TOL_FACTOR * max(f.eta_ref, f.eta_lapack), TOL_FACTOR * max(f.omega_ref, f.omega_lapack)
