"""CPU tests of arslam_lm_evaluate: the exported symbols, the argument and state checks that run
before any device call, the loud failure without a device, and the reference
(tests/evaluate_ref.py) checked against itself."""
import ctypes as C
import functools

import numpy as np
import pytest

import evaluate_ref
import loss_ref
import tag_size_ref as tref
from ar_slam_amd import synth

NEW = ["arslam_lm_evaluate_options_init", "arslam_lm_evaluate", "arslam_lm_evaluate_blocks",
       "arslam_lm_gradient_block", "arslam_slam_evaluate"]
E_INVALID_ARG, E_UNSUPPORTED, E_STATE = -1, -2, -7
KINDS = {"none": (loss_ref.NONE, 0.0), "huber": (loss_ref.HUBER, 3.0), "soft_l_one": (loss_ref.SOFT_L_ONE, 3.0),
         "cauchy": (loss_ref.CAUCHY, 3.0)}


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


def _two_blocks(L, **kw):
    prob = L.Problem(**kw)
    cam = np.array([900.0, 0.0, 0.0])
    caps = [np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0]) for _ in range(2)]
    tags = [np.zeros(6) for _ in range(2)]
    return prob, cam, caps, tags


def test_exports_and_python_surface(L):
    lib = C.CDLL(L.library_path())
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS
    o = L.EvaluateOptions(0)
    assert lib.arslam_lm_evaluate_options_init(C.byref(o)) == 0 and o.apply_loss_function == 1
    assert lib.arslam_lm_evaluate_options_init(None) == E_INVALID_ARG
    for cls, name in ((L.ResidentProblem, "evaluate"), (L.Problem, "evaluate"), (L.Problem, "gradient_block"),
                      (L.SlamSolver, "evaluate")):
        assert callable(getattr(cls, name))


def test_null_arguments(L):
    lib = L.lib()
    assert lib.arslam_lm_evaluate(None, None, None, None, None, None, None) == E_INVALID_ARG
    assert lib.arslam_lm_evaluate_blocks(None, None, None, None, None, None) == E_INVALID_ARG
    assert lib.arslam_lm_gradient_block(None, None, None) == E_INVALID_ARG
    assert lib.arslam_slam_evaluate(None, None, None, None) == E_INVALID_ARG
    prob, cam, caps, tags = _two_blocks(L)
    out = np.zeros(6)
    assert lib.arslam_lm_gradient_block(prob._h, None, out.ctypes.data_as(L._dp)) == E_INVALID_ARG
    assert lib.arslam_lm_gradient_block(prob._h, cam.ctypes.data_as(L._dp), None) == E_INVALID_ARG


def test_state_errors(L):
    lib = L.lib()
    h = L._Handle()
    assert lib.arslam_lm_evaluate(h._h, None, None, None, None, None, None) == E_STATE      # nothing loaded
    assert lib.arslam_lm_evaluate_blocks(h._h, None, None, None, None, None) == E_STATE     # no blocks
    prob, cam, caps, tags = _two_blocks(L)
    with pytest.raises(L.LMError) as e:
        prob.evaluate()
    assert e.value.code == E_STATE
    prob.add_residual_block(np.zeros(8), cam, caps[0], tags[0])
    with pytest.raises(L.LMError) as e:      # no evaluate yet
        prob.gradient_block(caps[0])
    assert e.value.code == E_STATE
    with pytest.raises(L.LMError) as e:      # not a block of the problem
        prob.gradient_block(caps[1])
    assert e.value.code == E_INVALID_ARG
    # blocks alone are no problem of arslam_lm_load_soa's
    assert lib.arslam_lm_evaluate(prob._h, None, None, None, None, None, None) == E_STATE
    s = L.SlamSolver()
    with pytest.raises(L.LMError) as e:      # the mirror: no block added yet
        s.evaluate()
    assert e.value.code == E_STATE


def test_apply_loss_function_is_validated(L):
    prob, cam, caps, tags = _two_blocks(L)
    prob.add_residual_block(np.zeros(8), cam, caps[0], tags[0])
    o = L.EvaluateOptions(2)
    assert L.lib().arslam_lm_evaluate_blocks(prob._h, C.byref(o), None, None, None, None) == E_INVALID_ARG


def test_several_ranks_are_unsupported(L):
    prob, cam, caps, tags = _two_blocks(L)
    prob.add_residual_block(np.zeros(8), cam, caps[0], tags[0])
    prob.debug_force_multirank(True)
    with pytest.raises(L.LMError) as e:
        prob.evaluate()
    assert e.value.code == E_UNSUPPORTED


def test_evaluate_without_gpu_fails_loudly(L):
    if L.device_count() > 0:
        pytest.skip("a GPU is present")
    prob, cam, caps, tags = _two_blocks(L)
    prob.add_residual_block(np.zeros(8), cam, caps[0], tags[0])
    with pytest.raises(L.LMError) as e:
        prob.evaluate()
    assert e.value.code not in (E_STATE, E_UNSUPPORTED, E_INVALID_ARG)
    g = synth.config_graph("tiny")
    with pytest.raises(L.LMError):           # (the load itself fails: the same failure)
        L.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners).evaluate()


# ---- the reference against itself ----

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_gradient_matches_central_differences(oracle, kind):
    g = tref.trace_graphs()["g6"][0]
    arrays = tref.arrays(g)
    k, a = KINDS[kind]
    ref = evaluate_ref.evaluate(oracle, arrays, k, a)
    x0 = loss_ref.pack(g.camera, g.cap, g.tag)
    nc = g.n_cap

    def cost(x):
        arr = (x[:3], x[3:3 + 6 * nc].reshape(-1, 6), x[3 + 6 * nc:].reshape(-1, 6)) + arrays[3:]
        return loss_ref.RobustTerms(oracle, arr, k, a).cost

    h = 1e-6
    fd = np.zeros(len(x0))
    for i in range(len(x0)):
        e = np.zeros(len(x0))
        e[i] = h
        fd[i] = (cost(x0 + e) - cost(x0 - e)) / (2.0 * h)
    fd[1:3] = 0.0   # (the pinhole: l1, l2 are no parameters)
    err = np.max(np.abs(fd - ref.gradient))
    print(f"{kind}: max |fd - grad| {err:.3e}, largest entry {np.max(np.abs(ref.gradient)):.3e}")
    assert err <= 1e-6 * np.max(np.abs(ref.gradient))
    if kind != "none":
        assert np.min(ref.weight) < 1.0   # (the loss bites on this graph)


def test_reference_zeroes_constant_unseen_and_lens_entries(oracle):
    g = tref.trace_graphs()["g20"][0]
    arrays = tuple(np.asarray(v)[:9] if i >= 3 else v for i, v in enumerate(tref.arrays(g)))   # first 9 observations
    cc = np.zeros(g.n_cap, np.uint8)
    cc[0] = 1
    ref = evaluate_ref.evaluate(oracle, arrays, loss_ref.CAUCHY, 3.0, cap_const=cc)
    seen_c = np.isin(np.arange(g.n_cap), arrays[3])
    seen_t = np.isin(np.arange(g.n_tag), arrays[4])
    assert not seen_c.all() and not seen_t.all()
    gc = ref.gradient[3:3 + 6 * g.n_cap].reshape(-1, 6)
    gt = ref.gradient[3 + 6 * g.n_cap:].reshape(-1, 6)
    assert np.all(gc[~seen_c] == 0.0) and np.all(gt[~seen_t] == 0.0) and np.all(gc[0] == 0.0)
    assert np.all(gc[seen_c & (np.arange(g.n_cap) != 0)] != 0.0)
    assert ref.gradient[0] != 0.0 and np.all(ref.gradient[1:3] == 0.0)
    assert np.all(ref.tol_gradient[ref.zero] == 0.0) and np.all(ref.tol_gradient[~ref.zero] > 0.0)


@functools.lru_cache(maxsize=None)
def solved_outliers(oracle):
    """loss_ref.outliers(g50) solved under Cauchy(3 px) by the dense reference LM."""
    g, bad = loss_ref.outliers(synth.config_graph("small"))
    cam, cap, tag, s = tref.solve(oracle, tref.arrays(g), kinds=loss_ref.CAUCHY, a=3.0)
    return g, bad, (cam, cap, tag, g.obs_cap, g.obs_tag, g.corners), s


def test_reference_weights_separate_the_shifted_observations(oracle):
    g, bad, arrays, s = solved_outliers(oracle)
    assert s["termination"] == "CONVERGENCE" and len(bad) == 20
    ref = evaluate_ref.evaluate(oracle, arrays, loss_ref.CAUCHY, 3.0)
    hi_bad, lo_good = evaluate_ref.weights_separate(ref.weight, bad)
    print(f"largest weight of a shifted observation {hi_bad:.4g}, smallest of the others {lo_good:.4g}")
    assert hi_bad < lo_good
