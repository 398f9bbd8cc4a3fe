"""CPU tests of the definition the LM solver's cross-covariance blocks are held to
(tests/lm_cov_pairs_ref.py): the tile forward / backward solve against numpy.linalg.solve, the
reference's own error over the requested blocks on every parity input and pair list of
tests/test_gpu_lm_cov_pairs.py, and the helper's cutting."""
import numpy as np
import pytest

import lm_cov_pairs_ref as pairs_ref
import lm_cov_ref as cov_ref
from ar_slam_amd import synth
from test_lm_cov import E_REF_CAP, GRAPHS, MIN_PIVOT_CAP, CovInput, _spd, arrow_pattern, reference

# the parity inputs of the GPU tests: (graph, with per-observation losses)
PARITY = [("g6", False), ("g20", False), ("g20", True), ("g60", False), ("gk", False)]
SOLVE_SHAPES = [(5, None), (64, None), (130, None), (200, None), (340, "arrow")]
ALL_CATEGORIES = {"tag_tag_far", "tag_tag_adjacent", "cap_cap_sharing", "cap_cap_disjoint", "cap_tag_seen",
                  "cap_tag_unseen", "camera_tag", "camera_capture", "camera_camera", "tag_self", "cap_self",
                  "reversed", "duplicate"}


BATCH_BLOCKS = 160    # solved blocks of one batch (lm_handle.h: kCovBatchPanels panels of ten)


def batch_input():
    """100 captures, 100 tags, and chains of neighbours over every free tag in use and every
    capture: more solved blocks under either elimination than one batch holds."""
    g = synth.make_graph(100, 10, 10, seed=12, k=8)
    tags = [t for t in range(1, g.n_tag) if np.any(g.obs_tag == t)]
    pairs = [((pairs_ref.TAG, x), (pairs_ref.TAG, y)) for x, y in zip(tags, tags[1:])] + \
        [((pairs_ref.CAPTURE, c), (pairs_ref.CAPTURE, c + 1)) for c in range(g.n_cap - 1)]
    return CovInput(g), pairs


def pairs_reference(oracle, inp, pairs, camera, cap, tag, loss=None, rows=None):
    """test_lm_cov.reference for a pair list: at (camera, cap, tag), the Jacobi scale of the initial parameters."""
    cc, tc = inp.consts()
    kinds, a = (0, 0.0) if loss is None else loss
    return pairs_ref.covariance_pairs(oracle, cov_ref.graph_arrays(inp.g, camera, cap, tag), pairs, inp.camera_const,
                                      cc, tc, kinds, a, scale_arrays=cov_ref.graph_arrays(inp.g), rows=rows)


@pytest.mark.parametrize("nrhs", [6, 60, 66])
@pytest.mark.parametrize("n, pattern", SOLVE_SHAPES)
def test_tile_solve_equals_numpy_solve(n, pattern, nrhs):
    mask = arrow_pattern() if pattern else None
    A = _spd(n, 3 + n, mask)
    B = np.eye(n)[:, pairs_ref.solve_columns(n, nrhs)]
    X = pairs_ref.tile_solve(A, B, mask)
    ref = np.linalg.solve(A, B)
    Z = np.linalg.inv(A)
    d = np.sqrt(np.diag(Z))
    err = np.max(np.abs(X - ref) / np.outer(d, d[pairs_ref.solve_columns(n, nrhs)]))
    assert err <= 1e-12, err
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, nrhs))
    X = pairs_ref.tile_solve(A, B, mask)
    ref = np.linalg.solve(A, B)
    assert np.max(np.abs(X - ref) / np.max(np.abs(ref), axis=0)) <= 1e-12


def test_solve_columns_cover_the_edges():
    cols = pairs_ref.solve_columns(340, 60)
    for c in (0, 339, 63, 64, 127, 128, 319, 320):
        assert c in cols
    assert len(pairs_ref.solve_columns(5, 66)) == 66 and len(set(pairs_ref.solve_columns(200, 66))) == 66


@pytest.mark.parametrize("name", sorted({n for n, _ in PARITY}))
def test_pair_lists_hold_every_category(name):
    pairs, cat = pairs_ref.pair_list(GRAPHS[name])
    missing = ALL_CATEGORIES - set(cat)
    # g6: six captures of four of its six tags, any two share one; the larger graphs supply everything
    assert missing == ({"cap_cap_disjoint"} if name == "g6" else set()), missing
    assert cat["tag_tag_far"] != cat["tag_tag_adjacent"]
    for tags_eliminated in (False, True):   # two panels under either elimination
        assert len(pairs_ref.solved_blocks(pairs, tags_eliminated)) > pairs_ref.PANEL_BLOCKS


@pytest.mark.parametrize("name, loss", PARITY)
def test_reference_error_caps_of_the_pair_lists(oracle, name, loss):
    """e_ref_pairs and min_pivot of every parity input and pair list, at its true parameters, and
    the joint matrix of every requested pair positive definite."""
    inp, l = GRAPHS[name], None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    g = inp.g
    pairs, cat = pairs_ref.pair_list(inp)
    ref = pairs_reference(oracle, inp, pairs, g.camera_true, g.cap_true, g.tag_true, l)
    print(f"{name} loss={loss}: e_ref_pairs {ref.e_ref_pairs:.2e} e_ref {ref.ref.e_ref:.2e} "
          f"min_pivot {ref.ref.min_pivot:.2e}; {len(pairs)} pairs")
    assert ref.e_ref_pairs <= E_REF_CAP
    assert ref.ref.e_ref <= E_REF_CAP
    assert ref.ref.min_pivot >= MIN_PIVOT_CAP
    assert np.all(ref.status == pairs_ref.OK)
    for p, (a, b) in enumerate(pairs):
        assert np.all(np.linalg.eigvalsh(ref.joint[p]) > 0), (a, b)
    # the cut: (b, a) is the transpose of (a, b)
    assert np.array_equal(ref.cov[pairs.index(cat["reversed"])], ref.cov[pairs.index(cat["cap_tag_seen"])].T)
    # the camera's layout: six values, the rest zero
    for p, (a, b) in enumerate(pairs):
        if (a[0] == pairs_ref.CAMERA) != (b[0] == pairs_ref.CAMERA):
            assert np.all(ref.cov[p].ravel()[6:] == 0.0) and np.all(ref.cov[p].ravel()[:6] != 0.0)
        if a[0] == b[0] == pairs_ref.CAMERA:
            assert ref.cov[p][0, 0] == ref.ref.var_f and np.all(ref.cov[p].ravel()[1:] == 0.0)


def test_reference_error_caps_of_the_batch_input(oracle):
    inp, pairs = batch_input()
    g = inp.g
    for tags_eliminated in (False, True):
        assert len(pairs_ref.solved_blocks(pairs, tags_eliminated)) > BATCH_BLOCKS
    ref = pairs_reference(oracle, inp, pairs, g.camera_true, g.cap_true, g.tag_true)
    print(f"batch input: e_ref_pairs {ref.e_ref_pairs:.2e} e_ref {ref.ref.e_ref:.2e} min_pivot {ref.ref.min_pivot:.2e}; "
          f"{len(pairs)} pairs")
    assert ref.e_ref_pairs <= E_REF_CAP and ref.ref.e_ref <= E_REF_CAP and ref.ref.min_pivot >= MIN_PIVOT_CAP
    assert np.all(ref.status == pairs_ref.OK)


def test_constant_and_unused_blocks_are_unavailable(oracle):
    inp = GRAPHS["g20_two_tags_const"]
    g = inp.g
    pairs = [((pairs_ref.TAG, 0), (pairs_ref.TAG, 1)), ((pairs_ref.TAG, 1), (pairs_ref.TAG, 7)),
             ((pairs_ref.TAG, 1), (pairs_ref.TAG, 2))]
    ref = pairs_reference(oracle, inp, pairs, g.camera_true, g.cap_true, g.tag_true)
    assert list(ref.status) == [pairs_ref.UNAVAILABLE, pairs_ref.UNAVAILABLE, pairs_ref.OK]
    assert np.all(ref.cov[:2] == -1.0)
    ia = pairs_ref._block_cols(ref.ref, g.n_cap, pairs_ref.TAG, 1)
    assert np.array_equal(ref.ref.C[np.ix_(ia, ia)], ref.ref.tag[1])
