"""CPU tests of the definition the LM solver's marginal covariances are held to
(tests/lm_cov_ref.py): the tile recursion of the selected inverse against the dense inverse, the
statistical meaning of the covariance, and the reference's own error on every parity input of
tests/test_gpu_lm_cov.py."""
import dataclasses

import numpy as np
import pytest

import lm_cov_ref as cov_ref
from ar_slam_amd import synth

E_REF_CAP = 1e-9      # every parity input: the two routes of the reference agree this well
MIN_PIVOT_CAP = 1e-5  # ... and its reduced system is this far from singular
N_SHIFTED = 3         # detections of a loss input shifted 40 px (the losses then reject them)


@dataclasses.dataclass
class CovInput:
    """One parity input: a graph, what is held constant, and whether its observations carry
    losses (kinds cycle o % 4, scales 2 + o % 3, as in test_gpu_localize_loss, and N_SHIFTED of
    the detections are shifted 40 px in a random direction, all four corners alike)."""
    g: object
    camera_const: bool = False
    cap_const: tuple = ()
    tag_const: tuple = (0,)

    def consts(self):
        cc = np.zeros(self.g.n_cap, np.uint8)
        tc = np.zeros(self.g.n_tag, np.uint8)
        cc[list(self.cap_const)] = 1
        tc[list(self.tag_const)] = 1
        return cc, tc

    def with_loss(self):
        g = self.g
        nb = g.n_obs
        rng = np.random.default_rng(5)
        bad = rng.choice(nb, N_SHIFTED, replace=False)
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        corners = np.array(g.corners, np.float64).reshape(nb, 8).copy()
        corners[bad] += np.tile(np.stack([np.cos(ang), np.sin(ang)], 1) * 40.0, (1, 4))
        o = np.arange(nb)
        return dataclasses.replace(self, g=dataclasses.replace(g, corners=corners)), (o % 4).astype(np.uint8), 2.0 + (o % 3)


def _graphs():
    g20 = synth.make_graph(20, 5, 4, seed=5, k=6)
    return {
        "g20": CovInput(g20),
        # 361 reduced rows under capture elimination: several tiles, blocks straddling tile
        # boundaries, a real elimination tree
        "g60": CovInput(synth.make_graph(60, 10, 6, seed=7, k=8)),
        "g6": CovInput(synth.make_graph(6, 3, 2, seed=5, k=4)),
        # captures of 12 and 6 tags: more than kSchurMfmaBlocks (10) distinct tags, and more than
        # kObsChunk (8) observations (the chunked launches)
        "gk": CovInput(synth.make_graph(12, 5, 4, seed=9, k=(12, 6), depth=(1.2, 1.8))),
        "g20_cap_const": CovInput(g20, cap_const=(0,), tag_const=()),
        "g20_camera_const": CovInput(g20, camera_const=True),
        "g20_two_tags_const": CovInput(g20, tag_const=(0, 7)),
    }


GRAPHS = _graphs()


def reference(oracle, inp, camera, cap, tag, loss=None, rows=None):
    """The reference at (camera, cap, tag), with the Jacobi scale of the input's initial parameters."""
    cc, tc = inp.consts()
    kinds, a = (0, 0.0) if loss is None else loss
    return cov_ref.covariance(oracle, cov_ref.graph_arrays(inp.g, camera, cap, tag), inp.camera_const, cc, tc, kinds, a,
                              scale_arrays=cov_ref.graph_arrays(inp.g), rows=rows)


def _spd(n, seed, mask=None):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    A = B @ B.T + n * np.eye(n)
    if mask is not None:
        # restricted to a tile pattern: keep it diagonally dominant
        A = (B + B.T) * 0.5 * np.kron(mask | mask.T, np.ones((64, 64)))[:n, :n] + 2.0 * n * np.eye(n)
    return A


def arrow_pattern():
    """6 tile rows (n = 340: the rhs row cuts the last tile): two leaves {0, 1} and {2, 3} under
    the separator 4 and the dense last row 5 -- a two-level tree below the border; column 0 has
    I_0 = {1, 4, 5}, and Z_14 (i < j) is read transposed.  Tiles (4, 1) and (4, 3) are fill."""
    P = np.eye(6, dtype=bool)
    for i, j in [(1, 0), (3, 2), (4, 0), (4, 2), (5, 0), (5, 1), (5, 2), (5, 3), (5, 4)]:
        P[i, j] = True
    return P


@pytest.mark.parametrize("n, pattern", [(5, None), (64, None), (130, None), (200, None), (340, "arrow")])
def test_tile_recursion_equals_dense_inverse(n, pattern):
    mask = arrow_pattern() if pattern else None
    A = _spd(n, 3 + n, mask)
    Z, P = cov_ref.tile_selinv(A, mask)
    if mask is not None:
        assert P[4, 1] and P[4, 3] and not mask[4, 1] and not mask[4, 3]   # the pattern fills
        assert n % 64 not in (0, 63)                           # the rhs row cuts the last tile
    full = np.kron(P | P.T, np.ones((64, 64)))[:n, :n] != 0
    ref = np.linalg.inv(A)
    d = np.sqrt(np.diag(ref))
    err = np.max(np.abs(Z - ref)[full] / np.outer(d, d)[full])
    assert err <= 1e-12, err
    assert np.all(Z[~full] == 0.0)
    assert np.array_equal(Z, Z.T)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
def test_reference_error_caps(oracle, name, loss):
    """e_ref and min_pivot of every parity input, at its true parameters."""
    inp = GRAPHS[name]
    l = None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    g = inp.g
    ref = reference(oracle, inp, g.camera_true, g.cap_true, g.tag_true, l)
    print(f"{name} loss={loss}: e_ref {ref.e_ref:.2e} min_pivot {ref.min_pivot:.2e} "
          f"free parameters {len(ref.cols)}")
    assert ref.e_ref <= E_REF_CAP
    assert ref.min_pivot >= MIN_PIVOT_CAP
    assert (ref.var_f > 0) == (not inp.camera_const)
    cc, tc = inp.consts()
    assert np.array_equal(ref.cap_status == cov_ref.UNAVAILABLE, cc.astype(bool))
    assert np.array_equal(ref.tag_status == cov_ref.UNAVAILABLE, tc.astype(bool))
    for blocks, st in ((ref.cap, ref.cap_status), (ref.tag, ref.tag_status)):
        assert np.all(blocks[st != cov_ref.OK] == -1.0)
        assert np.all(np.linalg.eigvalsh(blocks[st == cov_ref.OK]) > 0)


def test_gk_graph_has_the_large_captures():
    g = GRAPHS["gk"].g
    k = np.bincount(g.obs_cap)
    assert set(k) == {12, 6}
    # (distinct tags per capture = observations: make_graph gives a capture each tag once)
    assert all(len(set(g.obs_tag[g.obs_cap == c])) == k[c] for c in range(g.n_cap))


STAT_N = 512
STAT_SIGMA = 0.1


def test_covariance_is_the_spread_of_the_estimates(oracle):
    """N noisy copies of one graph, each solved from the truth: with d = estimate - truth, the mean
    of d_b' (sigma^2 C_b)^-1 d_b over the copies is 6 for every free block b, to first order, with
    standard error sqrt(12 / N) = 0.153 (a chi-square of 6 degrees of freedom has variance 12).
    The bound is 6 +- 4 standard errors.  A factor of two in C gives 3 or 12; swapped t / w halves
    far worse."""
    g = synth.make_graph(20, 5, 4, seed=5, k=6, noise_px=0)
    inp = CovInput(g)
    cc, tc = inp.consts()
    arr = cov_ref.graph_arrays(g, g.camera_true, g.cap_true, g.tag_true)
    ref = cov_ref.covariance(oracle, arr, False, cc, tc)
    rng = np.random.default_rng(17)
    acc_c = np.zeros(g.n_cap)
    acc_t = np.zeros(g.n_tag)
    acc_f = 0.0
    inv_c = np.array([np.linalg.inv(STAT_SIGMA ** 2 * ref.cap[c]) for c in range(g.n_cap)])
    inv_t = np.array([np.linalg.inv(STAT_SIGMA ** 2 * ref.tag[t]) if not tc[t] else np.zeros((6, 6))
                      for t in range(g.n_tag)])
    for _ in range(STAT_N):
        corners = g.corners + rng.normal(0.0, STAT_SIGMA, g.corners.shape)
        cam, cap, tag, s = oracle.solve(g.camera_true, g.cap_true, g.tag_true, g.obs_cap, g.obs_tag, corners,
                                        tag_const=tc, function_tolerance=1e-14, parameter_tolerance=1e-12,
                                        max_num_iterations=200)
        assert s["termination"] == "CONVERGENCE"
        dc, dt = cap - g.cap_true, tag - g.tag_true
        acc_c += np.einsum("ci,cij,cj->c", dc, inv_c, dc)
        acc_t += np.einsum("ci,cij,cj->c", dt, inv_t, dt)
        acc_f += (cam[0] - g.camera_true[0]) ** 2 / (STAT_SIGMA ** 2 * ref.var_f)
    means = np.concatenate([acc_c, acc_t[~tc.astype(bool)]]) / STAT_N
    se = np.sqrt(12.0 / STAT_N)
    print(f"block means {means.min():.3f} .. {means.max():.3f} over {len(means)} blocks; "
          f"focal {acc_f / STAT_N:.3f} (1 +- {np.sqrt(2.0 / STAT_N):.3f})")
    assert len(means) == 39
    assert np.all(np.abs(means - 6.0) <= 4.0 * se), means
    assert abs(acc_f / STAT_N - 1.0) <= 4.0 * np.sqrt(2.0 / STAT_N)
