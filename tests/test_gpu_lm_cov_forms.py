"""GPU test of the kept-result rule of the pointer-keyed covariance block forms
(arslam_lm_covariance_block, _block_lens, _block_anchored; include/arslam_lm.h): a handle keeps
the last computed result with the form it was computed for -- plain, _lens, or _anchored with its
anchor -- and serves a block from it to that form alone.  So on one handle, calls of the forms
interleaved in any order return what a fresh handle returns when it is asked only for that form.

The comparison is np.array_equal: two handles built the same way number the blocks the same way,
and the solve and the covariance are bit-reproducible across handles (tests/test_gpu_lm_cov.py,
test_gpu_lm_cov_anchored.py: test_repeated_calls_and_later_solves_keep_their_bits), so no
tolerance applies to any output here.
"""
import numpy as np
import pytest

from ar_slam_amd import synth

pytestmark = pytest.mark.gpu

TAG_CONST, TAG_K, TAG_J, CAPTURE = 0, 3, 5, 2   # the constant tag, the two anchors, the capture asked for


def _solved(lm):
    """A pointer-keyed problem on the tiny graph with tag TAG_CONST constant, solved; and its blocks."""
    g = synth.config_graph("tiny")
    assert g.n_cap == 6
    camera = g.camera.copy()
    caps, tags = [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    for b in range(g.n_obs):
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    prob.set_parameter_block_constant(tags[TAG_CONST])
    prob.solve()
    # the blocks asked for: the camera, one capture, one tag (TAG_K: under its own anchor, the anchor itself)
    return prob, tags, {"camera": camera, "capture": caps[CAPTURE], "tag": tags[TAG_K]}


FORMS = {
    "block": lambda prob, tags, b: prob.covariance_block(b),
    "block_lens": lambda prob, tags, b: prob.covariance_block_lens(b),
    "block_anchored(None)": lambda prob, tags, b: prob.covariance_block_anchored(None, b),
    "block_anchored(tag_k)": lambda prob, tags, b: prob.covariance_block_anchored(tags[TAG_K], b),
    "block_anchored(tag_j)": lambda prob, tags, b: prob.covariance_block_anchored(tags[TAG_J], b),
}
ORDER = list(FORMS) + ["block"]   # ... and the first again


def test_interleaved_forms_return_what_a_fresh_handle_returns(lm):
    want = {}
    for form, call in FORMS.items():
        prob, tags, blocks = _solved(lm)
        want[form] = {name: call(prob, tags, b) for name, b in blocks.items()}
    # what the forms must tell apart
    assert want["block"]["camera"][1] == lm.COV_OK and want["block_lens"]["capture"][1] == lm.COV_OK
    assert want["block_anchored(tag_k)"]["tag"][1] == lm.COV_UNAVAILABLE and want["block_anchored(tag_j)"]["tag"][1] == lm.COV_OK
    assert not np.array_equal(want["block_anchored(tag_k)"]["capture"][0], want["block_anchored(tag_j)"]["capture"][0])
    assert not np.array_equal(want["block_anchored(None)"]["capture"][0], want["block_anchored(tag_j)"]["capture"][0])

    prob, tags, blocks = _solved(lm)
    # every call after a call of another form (a kept result of another form is never served), then
    # each form's three blocks in a row (the second and third are served from the kept result)
    calls = [(form, name) for name in blocks for form in ORDER] + [(form, name) for form in ORDER for name in blocks]
    for form, name in calls:
        cov, status = FORMS[form](prob, tags, blocks[name])
        ref_cov, ref_status = want[form][name]
        assert status == ref_status, (form, name)
        assert cov.shape == ref_cov.shape and np.array_equal(cov, ref_cov), (form, name)
    print(f"{len(calls)} interleaved calls of {len(FORMS)} forms: np.array_equal to a fresh handle's, statuses equal")
