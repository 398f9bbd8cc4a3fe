"""CPU tests for the anchored covariance forms (arslam_lm_covariance_anchored, include/arslam_lm.h):
the new exports, the reference's own error on every parity input of
tests/test_gpu_lm_cov_anchored.py with the call-time anchor added to the constant flags, and the
e-block set of each input (oracle/schur_ordering.py), so the GPU cases hit every group kind of a
mixed set: eliminated captures, eliminated tags and direct groups."""
import dataclasses
import os
import re

import numpy as np
import pytest

from ar_slam_amd import synth
from oracle.schur_ordering import ceres_e_blocks
from test_lm_cov import E_REF_CAP, GRAPHS, MIN_PIVOT_CAP, CovInput, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURE, TAG = 1, 2   # ARSLAM_BLOCK_CAPTURE, _TAG

NEW_EXPORTS = ["arslam_lm_covariance_anchored", "arslam_lm_covariance_pairs_anchored",
               "arslam_lm_covariance_block_anchored", "arslam_lm_covariance_block_pair_anchored"]


def free(inp):
    """The input with no constant pose block (the anchor comes at the call)."""
    return dataclasses.replace(inp, cap_const=(), tag_const=())


def anchored(inp, anchor):
    """What the anchored call is held to: the input with the anchor added to the constant flags."""
    if anchor is None:
        return inp
    kind, i = anchor
    if kind == CAPTURE:
        return dataclasses.replace(inp, cap_const=tuple(sorted(set(inp.cap_const) | {i})))
    return dataclasses.replace(inp, tag_const=tuple(sorted(set(inp.tag_const) | {i})))


def _inputs():
    return {
        "g6": GRAPHS["g6"], "g20": GRAPHS["g20"], "g60": GRAPHS["g60"],
        "small": CovInput(synth.config_graph("small"), tag_const=()),
        # one direct group of 11 observations (more than kObsChunk) and 12 local blocks (more than
        # kSchurMfmaBlocks); an eliminated capture of 12 observations
        "g30k": CovInput(synth.make_graph(30, 5, 4, seed=3, k=(12, 6))),
        # a constant capture in place of the tag under a set that stays mixed (g20's becomes every tag)
        "g60_cap_const": CovInput(GRAPHS["g60"].g, cap_const=(0,), tag_const=()),
    }


INPUTS = _inputs()

# (graph, anchor on the graph with no constant block)
ANCHORED = [("g6", (TAG, 0)), ("g6", (CAPTURE, 2)), ("g20", (TAG, 3)), ("g20", (CAPTURE, 4)), ("small", (TAG, 0)),
            ("small", (CAPTURE, 7)), ("g30k", (TAG, 0))]


def e_set(inp):
    g = inp.g
    cc, tc = inp.consts()
    m = ceres_e_blocks(g.obs_cap, g.obs_tag, g.n_cap, g.n_tag, camera_const=inp.camera_const, cap_const=cc, tag_const=tc,
                       members=True)
    e_cap, e_tag = np.asarray(m["e_cap"], bool), np.asarray(m["e_tag"], bool)
    direct = ~e_cap[g.obs_cap] & ~e_tag[g.obs_tag]    # residuals with no e-block, grouped by capture
    return e_cap, e_tag, direct


def test_new_exports_are_declared_and_in_the_signature_table():
    from ar_slam_amd.lm import _abi
    header = open(os.path.join(ROOT, "include", "arslam_lm.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _abi.SIGNATURES, name
    assert re.search(r"^#define ARSLAM_BLOCK_NONE \(-1\)", header, flags=re.M) and _abi.BLOCK_NONE == -1
    assert _abi.SIGNATURES["arslam_lm_covariance_anchored"][1:3] == [_abi._i, _abi._i]
    assert len(_abi.SIGNATURES["arslam_lm_covariance_block_pair_anchored"]) == 6


@pytest.mark.parametrize("name, anchor", ANCHORED, ids=[f"{n}-{'cap' if a[0] == CAPTURE else 'tag'}{a[1]}" for n, a in ANCHORED])
def test_reference_error_caps(oracle, name, anchor):
    inp = anchored(free(INPUTS[name]), anchor)
    g = inp.g
    ref = reference(oracle, inp, g.camera_true, g.cap_true, g.tag_true)
    print(f"{name} anchor {anchor}: e_ref {ref.e_ref:.2e} min_pivot {ref.min_pivot:.2e}")
    assert ref.e_ref <= E_REF_CAP
    assert ref.min_pivot >= MIN_PIVOT_CAP
    kind, i = anchor
    assert (ref.cap_status if kind == CAPTURE else ref.tag_status)[i] == 1   # UNAVAILABLE


@pytest.mark.parametrize("name", ["g30k", "g60_cap_const"])
@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
def test_reference_error_caps_of_the_new_graphs(oracle, name, loss):
    """The inputs that are new here and used with their constant blocks alone (the others are
    tests/test_lm_cov.py's)."""
    inp, l = INPUTS[name], None
    if loss:
        inp, kinds, a = inp.with_loss()
        l = (kinds, a)
    g = inp.g
    ref = reference(oracle, inp, g.camera_true, g.cap_true, g.tag_true, l)
    print(f"{name} loss={loss}: e_ref {ref.e_ref:.2e} min_pivot {ref.min_pivot:.2e}")
    assert ref.e_ref <= E_REF_CAP and ref.min_pivot >= MIN_PIVOT_CAP


@pytest.mark.parametrize("name, const, n_cap, n_tag, n_direct", [
    ("g20", True, 3, 13, 13), ("g60", True, 9, 33, 51), ("g6", True, 1, 2, 5), ("small", False, 32, 7, 18),
    ("g60", False, 9, 34, 51), ("g20", False, 0, 20, 0), ("g30k", True, 22, 2, 8)])
def test_e_block_sets(name, const, n_cap, n_tag, n_direct):
    """The e-block set of each GPU input: eliminated captures, eliminated tags, direct groups."""
    inp = INPUTS[name] if const else free(INPUTS[name])
    assert inp.tag_const == ((0,) if const else ())
    e_cap, e_tag, direct = e_set(inp)
    g = inp.g
    assert (int(e_cap.sum()), int(e_tag.sum()), len(set(g.obs_cap[direct]))) == (n_cap, n_tag, n_direct)


def test_a_constant_capture_in_place_of_the_tag():
    """g20 with any one capture constant and no tag: every tag is eliminated, one whole side.  g60
    with capture 0 constant stays mixed: 7 + 36, 53 direct groups."""
    g = GRAPHS["g20"].g
    for c in range(g.n_cap):
        e_cap, e_tag, direct = e_set(CovInput(g, cap_const=(c,), tag_const=()))
        assert (int(e_cap.sum()), int(e_tag.sum()), int(direct.sum())) == (0, g.n_tag, 0)
    inp = INPUTS["g60_cap_const"]
    e_cap, e_tag, direct = e_set(inp)
    assert (int(e_cap.sum()), int(e_tag.sum()), len(set(inp.g.obs_cap[direct]))) == (7, 36, 53)


def test_g30k_has_the_large_groups():
    inp = INPUTS["g30k"]
    g = inp.g
    e_cap, e_tag, direct = e_set(inp)
    per_cap = np.bincount(g.obs_cap[direct], minlength=g.n_cap)
    assert per_cap.max() == 11                                   # > kObsChunk; 11 tags + its own pose = 12 local blocks
    assert np.bincount(g.obs_cap, minlength=g.n_cap)[e_cap].max() == 12
