"""numpy reference for the stages of one LM step between the rows and the factorization (test
helper, no GPU): the gradient, column norms, Jacobi scale and LM diagonal; the reduced system of a
Schur elimination, block-sparse; and the back-substitution from a given reduced solution.

Everything is by the caller's parameter slots (camera 3, captures 6 each, tags 6 each) and built
on tag_size_ref._Problem, so the rows are the oracle's with the loss, the tag side, the radial
model and the l columns (distortion_ref / distortion_free_ref oracles) already in them.

With Js = J diag(s) the scaled Jacobian of the free slots, D^2 = clamp(s^2 colnorm) / radius and
an eliminated set of blocks no two of which share a residual (e-blocks; every other free slot is on
the f-side), each e-block with its rows E (its own 6 columns) and F (the f-side columns) gives

    U = E'E + D_e^2,  W = E'F,  S += F'F - W' U^-1 W,  rhs += F'r - W' U^-1 E'r,

a residual with no e-block (a direct residual) adds its plain F'F and F'r, and D_f^2 goes on the
diagonal.  S y = rhs, and the step is  d_f = -s y,  d_e = -s_e U^-1 (E'r - W y).

Two evaluations of the same sums:
  * `reduce(..., longdouble=True)`: numpy.longdouble throughout (64-bit mantissa), U^-1 applied
    by a Cholesky solve.  No dense J'J is formed (numpy has no BLAS for the type): the products
    are per e-block.
  * `reduce(..., longdouble=False)`: float64, the e-blocks in order, U^-1 as the explicit inverse
    from an LLT and two triangular solves against I (inv6, Ceres' InvertPSDMatrix) -- what the
    device does, so its error against the long-double one is the floor a device error is held to.

Error measures (errors(); DESIGN "Stage checks of one step"): S by max |D_ij| / sqrt(H_ii H_jj)
and rhs by max |D_i| / (sqrt(H_ii) |r|), H_ii = (F'F + D^2)_ii the un-eliminated diagonal.  Not
by S_ii: S = F'F - W'U^-1 W cancels, and normalised by S the float64 restatement's own error is
7e-12 .. 2e-9; by H it is 2e-16 .. 9e-16 at radius 1e-2.
"""
import functools
import os
import sys

import numpy as np

import distortion_ref
import loss_ref
import tag_size_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import make_schur_golden  # noqa: E402
from ar_slam_amd import synth  # noqa: E402

LD = np.longdouble
U64 = 2.0 ** -53       # float64 unit roundoff
ULD = 2.0 ** -64       # numpy.longdouble (x87 extended) unit roundoff
FLOOR = 2.3e-16        # the rounding floor of the tolerance rule (test_gpu_tile_llt.py)


def make_problem(oracle, arrays, tag_size=None, camera_const=False, cap_const=None, tag_const=None, kinds=0, a=0.0):
    return tag_size_ref._Problem(oracle, arrays, tag_size, camera_const, cap_const, tag_const, kinds, a)


class Rows:
    """The corrected rows of P's active observations at x, zero outside the free slots:
    obs [m], cols [m, 15] (slots), J [m, 8, 15], r [m, 8]; by_block[b] the indices (into obs) of
    the rows of caller block b (captures first, then tags).

    rerr [m, 8], wrel [m]: what no float64 evaluation of the rows avoids.  A residual is
    r = p - o with the projection p rounded to 2^-53 |p| (hundreds of pixels) before the observed
    corner o is taken off: rerr, about 1e-13 absolute, which is 2e-13 of a residual of half a
    pixel at a converged point.  Under a loss |r|^2 then carries ds = 2 sum |r_i| 2^-53 |p_i| and
    the weight rho' carries wrel = |d log rho' / ds| ds into every entry of the corrected rows
    (0 without a loss; rerr includes the weight's share).  The long-double reference and the
    float64 restatement share these rows, so the restatement's error against the reference does
    not contain that rounding; the device evaluates its own rows, so its error does.
    sum_floors() and Step.model_floor restate it: they are added to the restatement's error
    wherever r or the weights enter (g, colnorm and what is made of it, rhs, the model change)."""

    def __init__(self, P, x=None):
        x = P.x0 if x is None else x
        cam, cap, tag = P.unpack(x)
        self.P = P
        self.obs = np.nonzero(P.active)[0]
        m = len(self.obs)
        self.cols = np.zeros((m, 15), np.int64)
        self.J = np.zeros((m, 8, 15))
        self.r = np.zeros((m, 8))
        self.by_block = [[] for _ in range(P.nc + P.nt)]
        self.wrel = np.zeros(m)
        self.rerr = np.zeros((m, 8))
        for i, o in enumerate(self.obs):
            r, Jo = tag_size_ref.residual_jacobian(P.oracle, cam, cap[P.obs_cap[o]], tag[P.obs_tag[o]], P.corners[o],
                                                   P.size[o])
            ss = float(r @ r)
            _, p1 = loss_ref.rho(int(P.kinds[o]), float(P.a[o]), ss)
            w = np.sqrt(float(p1))
            perr = U64 * np.abs(r + P.corners[o].reshape(8))   # one rounding of each projection
            if int(P.kinds[o]) != loss_ref.NONE and ss > 0:
                # d log rho' / ds by a difference, times the ds of those roundings
                _, p1h = loss_ref.rho(int(P.kinds[o]), float(P.a[o]), ss * (1 + 1e-6))
                ds = 2.0 * float(np.sum(np.abs(r) * perr))
                self.wrel[i] = abs(float(p1h) - float(p1)) / (float(p1) * 1e-6 * ss) * ds
            self.rerr[i] = w * (perr + np.abs(r) * self.wrel[i])
            c = P.cols(o)
            self.cols[i] = c
            self.J[i] = w * Jo * P.free[c]
            self.r[i] = w * r
            self.by_block[P.obs_cap[o]].append(i)
            self.by_block[P.nc + P.obs_tag[o]].append(i)


def block_slots(P, b):
    return 3 + 6 * b + np.arange(6)


def sums(R, dtype=LD):
    """(g, colnorm, r'r) of the rows: J'r and the squared column norms by slot."""
    P = R.P
    g = np.zeros(P.n, dtype)
    cn = np.zeros(P.n, dtype)
    J, r = R.J.astype(dtype), R.r.astype(dtype)
    for i in range(len(R.obs)):
        np.add.at(g, R.cols[i], J[i].T @ r[i])
        np.add.at(cn, R.cols[i], np.sum(J[i] * J[i], axis=0))
    return g, cn, np.sum(r * r)


def sum_floors(R, g, cn, rr):
    """(g floor, colnorm floor) by slot from Rows.rerr and wrel, in the measures of g (|D_i| /
    (sqrt(cn_i) |r|)) and colnorm (relative): |J|' rerr, and since both J and r carry sqrt(rho'),
    J'r and J^2 carry rho'.  The same floor bounds rhs in its own measure, twice: F'r is g's
    scaled entry (H_ii >= s_i^2 colnorm_i), and W'U^-1 E'r passes E'r through a contraction."""
    P = R.P
    fg = np.zeros(P.n)
    fc = np.zeros(P.n)
    for i in range(len(R.obs)):
        np.add.at(fg, R.cols[i], np.abs(R.J[i]).T @ (R.rerr[i] + np.abs(R.r[i]) * R.wrel[i]))
        if R.wrel[i]:
            np.add.at(fc, R.cols[i], np.sum(R.J[i] * R.J[i], axis=0) * R.wrel[i])
    cn = np.asarray(cn, np.float64)
    ok = cn > 0
    fg[ok] /= np.sqrt(cn[ok]) * float(np.sqrt(rr))
    fc[ok] /= cn[ok]
    return fg, fc


def scale_diag(P, colnorm, dmin=1e-6, dmax=1e32, jacobi=True, dtype=LD):
    """(scale, diag): 1 / (1 + sqrt(colnorm)) on the free slots, 0 elsewhere; clamp(s^2 colnorm)."""
    cn = np.asarray(colnorm, dtype)
    one = dtype(1.0)
    s = np.where(P.free, one / (one + np.sqrt(cn)) if jacobi else one, dtype(0.0))
    return s, np.clip(s * s * cn, dtype(dmin), dtype(dmax))


def e_set(P, cap_row, tag_row):
    """The eliminated blocks (bool [nc + nt]) from the device's reduced rows: free and row -1."""
    free = P.free[3:].reshape(-1, 6)[:, 0]
    return free & (np.concatenate([np.asarray(cap_row), np.asarray(tag_row)]) < 0)


def _chol(A):
    """Lower Cholesky factor of a small SPD matrix in its own dtype (column by column)."""
    n = len(A)
    L = np.array(A)
    for j in range(n):
        d = L[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, "e-block not positive definite"
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        L[j, j + 1:] = 0
    return L


def _chol_solve(L, B):
    """U^-1 B from U = L L' by two triangular solves."""
    n = len(L)
    Z = np.array(B)
    for i in range(n):
        Z[i] = (Z[i] - L[i, :i] @ Z[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        Z[i] = (Z[i] - L[i + 1:, i] @ Z[i + 1:]) / L[i, i]
    return Z


def inv6(U):
    """The explicit inverse as the device forms it: LLT, then the two solves against I."""
    L = _chol(U)
    return _chol_solve(L, np.eye(len(U), dtype=U.dtype))


class _Group:
    """One e-block's rows, scaled: slots e [6], f [m]; E [k, 6], F [k, m], r [k]."""


def _groups(R, elim, scale, dtype):
    """The e-blocks in caller order, then one group of the direct residuals per capture (e = None)."""
    P = R.P
    s = np.asarray(scale, dtype)
    J, r = R.J.astype(dtype), R.r.astype(dtype)
    f_side = P.free.copy()
    for b in np.nonzero(elim)[0]:
        f_side[block_slots(P, b)] = False
    out = []
    seen = np.zeros(len(R.obs), bool)

    def group(e_slots, idx):
        g = _Group()
        fs = np.unique(R.cols[idx].reshape(-1))
        fs = fs[f_side[fs]]
        pos = {int(sl): k for k, sl in enumerate(fs)}
        g.e, g.f = e_slots, fs
        g.cap = int(R.P.obs_cap[R.obs[idx[0]]]) if e_slots is None or e_slots[0] < 3 + 6 * R.P.nc else -1
        g.E = np.zeros((8 * len(idx), 6), dtype)
        g.F = np.zeros((8 * len(idx), len(fs)), dtype)
        g.r = np.zeros(8 * len(idx), dtype)
        g.rerr = np.zeros(8 * len(idx))
        for k, i in enumerate(idx):
            Js = J[i] * s[R.cols[i]]
            for j, sl in enumerate(R.cols[i]):
                if e_slots is not None and e_slots[0] <= sl < e_slots[0] + 6:
                    g.E[8 * k:8 * k + 8, sl - e_slots[0]] = Js[:, j]
                elif int(sl) in pos:
                    g.F[8 * k:8 * k + 8, pos[int(sl)]] = Js[:, j]
            g.r[8 * k:8 * k + 8] = r[i]
            g.rerr[8 * k:8 * k + 8] = R.rerr[i]
        return g

    for b in np.nonzero(elim)[0]:
        idx = R.by_block[b]
        assert not seen[idx].any(), "two eliminated blocks share a residual"
        seen[idx] = True
        out.append(group(block_slots(P, b), idx))
    for c in range(P.nc):
        idx = [i for i in R.by_block[c] if not seen[i]]
        if idx:
            out.append(group(None, idx))
    return out, f_side


class Reduced:
    """S [nf, nf] (both triangles), rhs [nf], H [nf] = (F'F + D^2)_ii, rr = r'r, slots [nf] the
    f-side slots in caller order, struct [nf, nf] True where some contribution or D^2 landed,
    groups (for back_substitute), D2 [n]."""


def reduce(R, elim, scale, diag, radius, longdouble=True, drop=None, only_caps=None, d2_slots=None):
    """The reduced system.  drop = (group index, a, b) is for the self-test of the measures only:
    that group's contribution to the diagonal block of its local f-slots [a, b) is left out.
    only_caps (bool [nc]) and d2_slots (bool [n]) make it a rank's share (reduce_shares): the
    groups of those captures alone, D_f^2 on those slots alone; H and rr are then the share's."""
    dtype = LD if longdouble else np.float64
    P = R.P
    groups, f_side = _groups(R, elim, scale, dtype)
    D2 = np.asarray(diag, dtype) / dtype(radius)
    slots = np.nonzero(f_side)[0]
    pos = np.full(P.n, -1)
    pos[slots] = np.arange(len(slots))
    nf = len(slots)
    out = Reduced()
    out.S = np.zeros((nf, nf), dtype)
    out.rhs = np.zeros(nf, dtype)
    out.H = np.zeros(nf, dtype)
    out.struct = np.zeros((nf, nf), bool)
    out.rr = dtype(0.0)
    for gi, g in enumerate(groups):
        if only_caps is not None and not only_caps[g.cap]:
            continue
        p = pos[g.f]
        FF, Fr = g.F.T @ g.F, g.F.T @ g.r
        out.H[p] += np.diag(FF)
        out.rr += g.r @ g.r
        if g.e is not None:
            g.U = g.E.T @ g.E + np.diag(D2[g.e])
            g.W = g.E.T @ g.F
            g.Er = g.E.T @ g.r
            if longdouble:
                g.L = _chol(g.U)
                UiW, UiEr = _chol_solve(g.L, g.W), _chol_solve(g.L, g.Er)
            else:
                g.Ui = inv6(g.U)
                UiW, UiEr = g.Ui @ g.W, g.Ui @ g.Er
            FF = FF - g.W.T @ UiW
            Fr = Fr - g.W.T @ UiEr
        if drop is not None and drop[0] == gi:
            FF[drop[1]:drop[2], drop[1]:drop[2]] = 0
        out.S[np.ix_(p, p)] += FF
        out.rhs[p] += Fr
        # (structure by block: the camera's 3 slots, a pose's 6)
        blk = np.where(g.f < 3, 0, 1 + (g.f - 3) // 6)
        fb = np.where(slots < 3, 0, 1 + (slots - 3) // 6)
        touched = np.isin(fb, blk)
        out.struct |= np.outer(touched, touched)
    on = np.ones(nf, bool) if d2_slots is None else np.asarray(d2_slots, bool)[slots]
    out.S[np.arange(nf)[on], np.arange(nf)[on]] += D2[slots][on]
    out.H[on] += D2[slots][on]
    out.struct[np.arange(nf)[on], np.arange(nf)[on]] = True
    out.slots, out.groups, out.D2, out.f_side = slots, groups, D2, f_side
    return out


def reduce_shares(R, elim, scale, diag, radius, owners, slot_rank, n_ranks, longdouble=True):
    """The sharded reduction: rank k's share is the sum over the captures it owns (owners [nc]) of
    F'F - W'U^-1 W and of the rhs terms, plus D_f^2 on the f-side slots of its own subtrees
    (slot_rank [n] == k; -1: the replicated top, whose D^2 no share carries).  The e-set is the
    captures (the ranks own captures).  One Reduced per rank, by the same slots as reduce()."""
    P = R.P
    assert not np.any(np.asarray(elim)[P.nc:]), "the sharded path eliminates captures"
    owners, slot_rank = np.asarray(owners), np.asarray(slot_rank)
    return [reduce(R, elim, scale, diag, radius, longdouble, only_caps=owners == k, d2_slots=slot_rank == k)
            for k in range(n_ranks)]


def sum_shares(shares, top_d2):
    """The shares summed in rank order, then top_d2 [nf] (D_f^2 of the top slots, 0 elsewhere) on
    the diagonal, in the shares' dtype: the device's two-level sum (captures within a rank, then
    the ranks), and in long double the whole problem's system to the rounding of the sum."""
    S, rhs = shares[0].S.copy(), shares[0].rhs.copy()
    for sh in shares[1:]:
        S += sh.S
        rhs += sh.rhs
    S[np.arange(len(rhs)), np.arange(len(rhs))] += np.asarray(top_d2, S.dtype)
    return S, rhs


def errors(test_S, test_rhs, ref):
    """(e_S, e_rhs) of a reduced system against the long-double one, by the H-normalised measures."""
    H = np.sqrt(ref.H)
    eS = np.max(np.abs(np.asarray(test_S, LD) - ref.S) / np.outer(H, H)) if len(H) else LD(0)
    er = np.max(np.abs(np.asarray(test_rhs, LD) - ref.rhs) / (H * np.sqrt(ref.rr))) if len(H) else LD(0)
    return float(eS), float(er)


class Step:
    """delta [n] (0 outside the free slots), model (the model cost change), model_floor (what
    Rows.rerr leaves uncertain in it, absolute), e_step2, f_step2."""


def back_substitute(R, red, y, scale, longdouble=True, flip_wy=False):
    """The step from the reduced solution y [nf] (by red.slots) and the scale, on red's own
    groups (so in red's dtype; float64: the explicit inverse).  flip_wy: the self-test's wrong
    sign of W y."""
    dtype = LD if longdouble else np.float64
    P = R.P
    s = np.asarray(scale, dtype)
    yf = np.zeros(P.n, dtype)
    yf[red.slots] = np.asarray(y, dtype)
    out = Step()
    out.delta = np.zeros(P.n, dtype)
    out.delta[red.slots] = -s[red.slots] * yf[red.slots]
    model, floor = dtype(0.0), 0.0
    for g in red.groups:
        m = -(g.F @ yf[g.f])
        if g.e is not None:
            v = g.Er - (-1 if flip_wy else 1) * (g.W @ yf[g.f])
            z = _chol_solve(g.L, v) if longdouble else g.Ui @ v
            out.delta[g.e] = -s[g.e] * z
            m = m - g.E @ z
        model -= np.sum(m * (g.r + m / 2))
        floor += float(np.sum(np.abs(m) * g.rerr))
    out.model, out.model_floor = model, floor
    free_f = np.zeros(P.n, bool)
    free_f[red.slots] = True
    out.f_step2 = np.sum(out.delta[free_f] ** 2)
    out.e_step2 = np.sum(out.delta[~free_f] ** 2)
    return out


def dense_step(R, scale, diag, radius):
    """The dense long-double step of the whole H (tag_size_ref._chol_solve): (H, b, y) over the
    free slots fi, Js'Js + D^2, Js'r and H^-1 b in long double."""
    P = R.P
    fi = np.nonzero(P.free)[0]
    pos = np.full(P.n, -1)
    pos[fi] = np.arange(len(fi))
    s = np.asarray(scale, LD)
    H = np.zeros((len(fi), len(fi)), LD)
    b = np.zeros(len(fi), LD)
    for i in range(len(R.obs)):
        c = R.cols[i]
        keep = P.free[c]
        Js = (R.J[i].astype(LD) * s[c])[:, keep]
        p = pos[c[keep]]
        H[np.ix_(p, p)] += Js.T @ Js
        b[p] += Js.T @ R.r[i].astype(LD)
    H[np.arange(len(fi)), np.arange(len(fi))] += np.asarray(diag, LD)[fi] / LD(radius)
    L = _chol(H)
    return fi, H, b, _chol_solve(L, b)


# ---- the inputs the CPU and GPU tests share ----

CAPS = {1e-2: 5e-15, 1e4: 1e-12, 1e16: 1e-9}   # the restatement's own S error is at most this, by radius

def pair_graph(n_cap, both, seed):
    """n_cap captures over two tags: each sees both tags (both) or one of them in turn -- the
    reduced system stays at 15 rows while a gather destination takes n_cap contributions."""
    rng = np.random.default_rng(seed)
    tag_true = np.zeros((2, 6))
    tag_true[1, 0] = synth.TAG_SPACING
    tag_true[:, 5] = rng.uniform(-1.0, 1.0, 2)
    R_cw, pos = synth._sample_cameras(rng, n_cap, 0.0, synth.TAG_SPACING, -0.1, 0.1, np.deg2rad(15.0), depth=(0.8, 1.4))
    cap_true = np.zeros((n_cap, 6))
    cap_true[:, :3] = -pos
    cap_true[:, 3:] = synth.log_so3(R_cw)
    if both:
        obs_cap = np.repeat(np.arange(n_cap), 2).astype(np.int32)
        obs_tag = np.tile([0, 1], n_cap).astype(np.int32)
    else:
        obs_cap = np.arange(n_cap, dtype=np.int32)
        obs_tag = (np.arange(n_cap) % 2).astype(np.int32)
    camera_true = np.array([synth.F_TRUE, 0.0, 0.0])
    corners = synth.project_corners(camera_true, cap_true[obs_cap], tag_true[obs_tag])
    corners += rng.normal(0.0, 0.5, corners.shape)
    cap0 = cap_true + rng.normal(0.0, 0.02, cap_true.shape)
    tag0 = tag_true + rng.normal(0.0, 0.02, tag_true.shape)
    return synth.Graph(np.array([1.1 * synth.F_TRUE, 0.0, 0.0]), cap0, tag0, obs_cap, obs_tag,
                       np.ascontiguousarray(corners), camera_true, cap_true, tag_true, "pair")


# The sharded step's inputs: name -> world size.  The smallest with a real split (a replicated top
# and two ranks owning subtrees): `medium`; the same with outliers under a Cauchy loss, and with a
# constant tag and camera; sh400 x 3, whose third rank owns two top-only captures and no subtree
# (the shape of the split at 4 and 8 ranks); shmix200, captures of 8 .. 30 tags on both ranks
# (k_schur<true> and the chunked instances).  tests/test_step_ref.py holds the split facts.
SHARDED = {"medium": 2, "medium_cauchy": 2, "medium_const": 2, "sh400": 3, "shmix200": 2}


def sharded_graph(name):
    if name == "sh400":
        return synth.make_graph(400, 14, 10, 31)
    if name == "shmix200":
        return synth.make_graph(200, 16, 12, 31, k=(8, 11, 16, 8, 8, 30, 8, 8), depth=(1.5, 3.5))
    g = synth.config_graph("medium")
    return loss_ref.outliers(g)[0] if name == "medium_cauchy" else g


@functools.lru_cache(maxsize=None)
def rank_split(name, world=None):
    """(infos [world] of arslam_split_info as dicts, cap_owner [nc]) of a sharded input, by the
    host-only arslam_debug_rank_split on the problem as the ranks load it (constants included)."""
    import ctypes as C
    from ar_slam_amd import build
    from ar_slam_amd.lm import _abi, mapper
    build.build()
    s = spec(name)
    A = mapper._Soa(*tag_size_ref.arrays(s["g"]), s["camera_const"], s["cap_const"], s["tag_const"])
    world = SHARDED[name] if world is None else world
    infos, owner = [], np.zeros(A.cap.shape[0], np.int32)
    for r in range(world):
        info = _abi.SplitInfo()
        _abi._check(_abi.lib().arslam_debug_rank_split(C.byref(A.s), world, r, C.byref(info), _abi._ptr(owner)))
        infos.append(info.to_dict())
    return infos, owner


LATE_SPECS = {}   # specs a GPU test builds from what the device told it (the appended problem)


@functools.lru_cache(maxsize=None)
def spec(name):
    """name -> dict(g, camera_const, cap_const, tag_const, sizes, loss, model): the problem as the
    device loads it and as the reference evaluates it."""
    if name in LATE_SPECS:
        return LATE_SPECS[name]
    s = dict(camera_const=False, cap_const=None, tag_const=None, sizes=None, loss=None, model="pinhole")
    if name in ("k1to11", "k1to11_const"):
        s["g"] = make_schur_golden.graph()
        if name == "k1to11_const":
            s["camera_const"], s["tag_const"] = make_schur_golden.const_blocks(s["g"])
    elif name == "k30":      # one capture of 30 distinct tags: k_schur<true> over several block rows
        s["g"] = synth.make_graph(5, 7, 6, 3, k=(30, 5, 5, 5, 5), depth=(2.5, 3.5))
    elif name == "pair70":   # the tag diagonal block: 70 > 64 contributions, two pieces, the last of 6
        s["g"] = pair_graph(70, True, 1)
    elif name == "pair170":  # the 6-element tag x camera and tag x rhs blocks: 170 > 160
        s["g"] = pair_graph(170, True, 2)
    elif name == "single1030":   # the camera diagonal and camera x rhs: 1030 > 1024
        s["g"] = pair_graph(1030, False, 3)
    elif name in SHARDED:   # the sharded step's inputs (tests/test_gpu_step_stages_sharded.py)
        s["g"] = sharded_graph(name)
        if name == "medium_cauchy":
            s["loss"] = (loss_ref.CAUCHY, 3.0)
        if name == "medium_const":   # a constant tag (one a rank's subtree holds) and a constant camera
            s["camera_const"] = True
            s["tag_const"] = np.zeros(s["g"].n_tag, np.uint8)
            s["tag_const"][5] = 1
    elif name == "small":
        s["g"] = synth.config_graph("small")
    elif name == "small_cauchy":
        s["g"] = loss_ref.outliers(synth.config_graph("small"))[0]
        s["loss"] = (loss_ref.CAUCHY, 3.0)
    elif name == "small_sized":
        s["g"], _, _, _, s["sizes"] = tag_size_ref.trace_graphs(True)["small"]
    elif name in ("g20_cap_const", "g20_tag_const", "g20_camera_const"):
        s["g"], s["camera_const"], s["cap_const"], s["tag_const"], _ = tag_size_ref.trace_graphs()[name]
    elif name == "g20_f_const":   # the camera and every tag constant: no reduced system
        s["g"] = tag_size_ref.trace_graphs()["g20"][0]
        s["camera_const"], s["tag_const"] = True, np.ones(s["g"].n_tag, np.uint8)
    elif name in ("g20_radial", "g20_radial_est"):
        s["g"] = distortion_ref.trace_graphs()["g20"][0]
        s["model"] = "radial_est" if name.endswith("est") else "radial"
    else:
        raise KeyError(name)
    return s


def oracle_for(oracle, model):
    """The oracle of a spec's camera model: the pinhole, the radial model held, or with l1, l2 free."""
    import distortion_free_ref
    return {"pinhole": oracle, "radial": distortion_ref.RadialOracle(oracle),
            "radial_est": distortion_free_ref.FreeRadialOracle(oracle)}[model]


def spec_problem(oracle, name):
    s = spec(name)
    kinds, a = s["loss"] if s["loss"] else (0, 0.0)
    return make_problem(oracle_for(oracle, s["model"]), tag_size_ref.arrays(s["g"]), s["sizes"], s["camera_const"],
                        s["cap_const"], s["tag_const"], kinds, a)


# every named input of tests/test_gpu_step_stages.py, and the radii it runs each at
ALL_RADII = (1e-2, 1e4, 1e16)
INPUT_RADII = {"k1to11": ALL_RADII, "small": ALL_RADII, "k1to11_const": ALL_RADII[:2], "k30": ALL_RADII[:2],
               "pair70": ALL_RADII[:2], "pair170": ALL_RADII[:2], "single1030": ALL_RADII[:2],
               "small_cauchy": ALL_RADII[:2], "small_sized": ALL_RADII[:2], "g20_radial": ALL_RADII[:2],
               "g20_radial_est": ALL_RADII[:2], "g20_cap_const": ALL_RADII[:2], "g20_tag_const": ALL_RADII[:2],
               "g20_camera_const": ALL_RADII[:2], "g20_f_const": ALL_RADII[:2],
               # ... and of tests/test_gpu_step_stages_sharded.py
               "medium": ALL_RADII, "medium_cauchy": ALL_RADII[:2], "medium_const": ALL_RADII[:2],
               "sh400": ALL_RADII[:2], "shmix200": ALL_RADII[:2]}
