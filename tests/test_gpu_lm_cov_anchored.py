"""GPU tests of the anchored covariance forms (arslam_lm_covariance_anchored, _pairs_anchored,
_block_anchored, _block_pair_anchored; include/arslam_lm.h): the covariance in the gauge of a pose
block named at the call, under every e-block set, the mixed one (ELIM_MIXED) included.

The definition: what the same handle would return had the anchor been constant, at the same point.
So the reference is tests/lm_cov_ref.py (lm_cov_pairs_ref.py, lm_cov_lens_ref.py) as it stands with
the anchor added to the constant flags, evaluated at the parameters the device returned, with
rows = debug_reduced_rows().  The bounds are tests/test_gpu_lm_cov.py's:
  * |C_dev - C_ref|_ij <= tol sqrt(C_ii C_jj), tol = max(16 e_ref of that input, 1e-10);
  * min_pivot within 1e-10 of the reference's in the device's row order (the anchor's rows left out);
  * statuses equal (the anchor: UNAVAILABLE, -1 in its values); every diagonal block exactly symmetric;
  * pairs: tests/test_gpu_lm_cov_pairs.py's bound, 16 max(e_ref, e_ref_pairs).
Every case prints its measured error (profiles/lm_cov_anchored/device_errors.txt).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lm_cov_pairs_ref as pairs_ref
from ar_slam_amd import synth
from lm_cov_pairs_ref import CAMERA
from test_gpu_lm_cov import _bits, _problem, _same
from test_lm_cov import E_REF_CAP, GRAPHS, MIN_PIVOT_CAP, CovInput, reference
from test_lm_cov_anchored import CAPTURE, INPUTS, NEW_EXPORTS, TAG, anchored, e_set, free
from test_lm_cov_pairs import pairs_reference

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID_ARG = -2, -1


def _loss(inp, with_loss):
    if not with_loss:
        return inp, None
    inp, kinds, a = inp.with_loss()
    return inp, (kinds, a)


def _solved(lm, inp, loss=None, **opts):
    rp = _problem(lm, inp, loss, **opts)
    return rp, rp.solve()


def _check(lm, oracle, rp, inp, anchor, loss, label):
    """covariance_anchored(anchor) against the reference with the anchor constant."""
    out = rp.covariance_anchored(anchor)
    ref = reference(oracle, anchored(inp, anchor), rp.camera, rp.cap, rp.tag, loss, rows=rp.debug_reduced_rows())
    assert ref.e_ref <= E_REF_CAP and ref.min_pivot >= MIN_PIVOT_CAP
    tol = max(16.0 * ref.e_ref, 1e-10)
    info = out["info"]
    assert info["status"] == lm.COV_OK
    assert np.array_equal(out["cap_status"], ref.cap_status)
    assert np.array_equal(out["tag_status"], ref.tag_status)
    if anchor is not None:
        kind, i = anchor
        assert (out["cap_status"] if kind == CAPTURE else out["tag_status"])[i] == lm.COV_UNAVAILABLE
    worst = 0.0
    for dev, want, st in ((out["cap"], ref.cap, ref.cap_status), (out["tag"], ref.tag, ref.tag_status)):
        assert np.all(dev[st != lm.COV_OK] == -1.0)
        ok = st == lm.COV_OK
        assert np.array_equal(dev[ok], np.transpose(dev[ok], (0, 2, 1)))   # the same bits both ways
        d = np.sqrt(np.einsum("bii->bi", want[ok]))
        worst = max(worst, float(np.max(np.abs(dev[ok] - want[ok]) / (d[:, :, None] * d[:, None, :]))))
    cam = out["cam"]
    if inp.camera_const:
        assert out["cam_status"] == lm.COV_UNAVAILABLE and np.all(cam == -1.0)
    else:
        assert out["cam_status"] == lm.COV_OK and np.all(cam.ravel()[1:] == 0.0) and out["var_f"] == cam[0, 0]
        worst = max(worst, abs(cam[0, 0] - ref.var_f) / ref.var_f)
    print(f"{label}: error {worst:.2e} (tol {tol:.2e}, e_ref {ref.e_ref:.2e}); min_pivot {info['min_pivot']:.6e} "
          f"(reference {ref.min_pivot_rows:.6e}); {info['n_reduced']} reduced rows, {info['n_factor_tiles']} tiles")
    assert abs(info["min_pivot"] - ref.min_pivot_rows) <= 1e-10
    assert worst <= tol
    return out, ref, tol


def _device_set_is(rp, inp):
    """The loaded e-block set is the one tests/test_lm_cov_anchored.py pins (the reduced blocks have rows)."""
    e_cap, e_tag, _ = e_set(inp)
    cap_row, tag_row, _ = rp.debug_reduced_rows()
    cc, tc = inp.consts()
    assert np.array_equal(cap_row >= 0, ~e_cap & (cc == 0)) and np.array_equal(tag_row >= 0, ~e_tag & (tc == 0))


# ---- 0. what fails without the feature ----

def test_anchored_forms_exist_and_work_where_the_other_forms_are_refused(lm):
    for n in NEW_EXPORTS:
        assert n in lm.EXPORTS and hasattr(lm.lib(), n)
    rp, s = _solved(lm, INPUTS["g6"], elimination=lm.ELIM_MIXED)
    assert s["elimination_used"] == lm.ELIM_MIXED
    for call in (rp.covariance, rp.covariance_lens, lambda: rp.covariance_pairs([((TAG, 1), (TAG, 2))]),
                 lambda: rp.covariance_pairs_lens([((TAG, 1), (TAG, 2))])):
        with pytest.raises(lm.LMError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    assert rp.covariance_anchored(None)["info"]["status"] == lm.COV_OK


# ---- 1. the mixed set, constants only ----

@pytest.mark.parametrize("executor", [0, 1])
@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("name", ["g6", "g20", "g60", "g30k"])
def test_mixed_set_constants_only(lm, oracle, name, with_loss, executor):
    inp, loss = _loss(INPUTS[name], with_loss)
    rp, s = _solved(lm, inp, loss, elimination=lm.ELIM_MIXED, factor_executor=executor)
    assert s["elimination_used"] == lm.ELIM_MIXED
    _device_set_is(rp, inp)
    _check(lm, oracle, rp, inp, None, loss, f"mixed {name} {'loss' if with_loss else 'plain'} ex{executor}")


@pytest.mark.parametrize("name, used", [("g20_cap_const", "ELIM_TAGS"), ("g60_cap_const", "ELIM_MIXED"),
                                        ("g20_camera_const", "ELIM_MIXED")])
def test_mixed_set_other_constants(lm, oracle, name, used):
    """A constant capture in place of the tag; a constant camera.  With any one capture of g20
    constant and no tag, Ceres' set is every tag, so ELIM_MIXED resolves to ELIM_TAGS there
    (tests/test_lm_cov_anchored.py pins it); g60 with capture 0 constant is the mixed case."""
    inp = INPUTS[name] if name in INPUTS else GRAPHS[name]
    rp, s = _solved(lm, inp, elimination=lm.ELIM_MIXED)
    assert s["elimination_used"] == getattr(lm, used)
    out, _, _ = _check(lm, oracle, rp, inp, None, None, f"mixed {name}")
    cc, tc = inp.consts()
    assert np.all(out["cap_status"][cc == 1] == lm.COV_UNAVAILABLE) and np.all(out["tag_status"][tc == 1] == lm.COV_UNAVAILABLE)


# ---- 2. a call-time anchor on problems with no constant block ----

def _role_anchors(inp):
    """One anchor of each device role under the input's mixed set."""
    g = inp.g
    e_cap, e_tag, direct = e_set(inp)
    with_direct = np.zeros(g.n_cap, bool)
    with_direct[g.obs_cap[direct]] = True
    out = {"eliminated capture": (CAPTURE, int(np.nonzero(e_cap)[0][0])),
           "eliminated tag": (TAG, int(np.nonzero(e_tag)[0][0])),
           "reduced tag": (TAG, int(np.nonzero(~e_tag)[0][0])),
           "reduced capture with a direct group": (CAPTURE, int(np.nonzero(~e_cap & with_direct)[0][0]))}
    plain = np.nonzero(~e_cap & ~with_direct)[0]
    if len(plain):
        out["reduced capture without a direct group"] = (CAPTURE, int(plain[0]))
    return out


def test_call_time_anchor_of_each_role(lm, oracle):
    inp = free(INPUTS["small"])
    rp, s = _solved(lm, inp, elimination=lm.ELIM_MIXED)
    assert s["elimination_used"] == lm.ELIM_MIXED
    _device_set_is(rp, inp)
    roles = _role_anchors(inp)
    assert len(roles) >= 4
    for role, anchor in roles.items():
        _check(lm, oracle, rp, inp, anchor, None, f"small, anchor {anchor} ({role})")


@pytest.mark.parametrize("name, elimination, used, anchor", [
    ("g60", "ELIM_MIXED", "ELIM_MIXED", (TAG, 0)), ("g60", "ELIM_MIXED", "ELIM_MIXED", (CAPTURE, 5)),
    ("g20", "ELIM_MIXED", "ELIM_TAGS", (TAG, 3)), ("g20", "ELIM_MIXED", "ELIM_TAGS", (CAPTURE, 4)),
    ("g20", "ELIM_CAPTURES", "ELIM_CAPTURES", (TAG, 3)), ("g20", "ELIM_CAPTURES", "ELIM_CAPTURES", (CAPTURE, 4))])
def test_call_time_anchor(lm, oracle, name, elimination, used, anchor):
    inp = free(INPUTS[name])
    rp, s = _solved(lm, inp, elimination=getattr(lm, elimination))
    assert s["elimination_used"] == getattr(lm, used)
    _check(lm, oracle, rp, inp, anchor, None, f"{name} {elimination} -> {used}, anchor {anchor}")


# ---- 3. anchor equals constant ----

def test_an_anchor_that_is_constant_changes_nothing(lm):
    rp, _ = _solved(lm, INPUTS["g20"], elimination=lm.ELIM_CAPTURES)
    want = rp.covariance_lens()
    for anchor in (None, (TAG, 0)):
        got = rp.covariance_anchored(anchor)
        for k in ("cap", "tag", "cam", "cap_status", "tag_status"):
            assert np.array_equal(got[k], want[k]), (anchor, k)
        assert got["cam_status"] == want["cam_status"] and got["info"]["min_pivot"] == want["info"]["min_pivot"]


# ---- 4. the focal does not depend on the gauge ----

def test_the_focal_does_not_depend_on_the_gauge(lm, oracle):
    """var(f) under two anchors: each within tol of one reference value (anchor tag 3's), and within
    2 tol of each other.  The two numpy references themselves are two QR factorizations over
    different column sets: at the device's point they differ by 4.9e-15 relative (printed)."""
    inp = free(INPUTS["g20"])
    rp, _ = _solved(lm, inp, elimination=lm.ELIM_CAPTURES)
    (a, ra, ta), (b, rb, tb) = (_check(lm, oracle, rp, inp, an, None, f"g20 focal, anchor {an}") for an in ((TAG, 3), (CAPTURE, 4)))
    tol = max(ta, tb)
    print(f"var(f): anchor tag 3 {a['var_f']:.17g}, anchor capture 4 {b['var_f']:.17g}; references differ by "
          f"{abs(ra.var_f - rb.var_f) / ra.var_f:.2e}")
    for out in (a, b):
        assert abs(out["var_f"] - ra.var_f) <= tol * ra.var_f
    assert abs(a["var_f"] - b["var_f"]) <= 2 * tol * ra.var_f


# ---- 5. pairs ----

def _lens_to_soa(c, a, b):
    """A block in the _lens forms' layout (held lens) in lm_cov_pairs_ref's: the focal's values first."""
    if b[0] == CAMERA and a[0] != CAMERA:
        assert np.all(c[:, 1:] == 0.0)
        out = np.zeros(36)
        out[:6] = c[:, 0]
        return out.reshape(6, 6)
    return c


def test_pairs_across_every_role(lm, oracle):
    inp = free(INPUTS["g60"])
    anchor = (TAG, 0)
    rp, s = _solved(lm, inp, elimination=lm.ELIM_MIXED)
    assert s["elimination_used"] == lm.ELIM_MIXED
    _device_set_is(rp, inp)
    g = inp.g
    e_cap, e_tag, _ = e_set(inp)
    blocks = [(CAMERA, 0), (TAG, int(np.nonzero(~e_tag)[0][1])), (CAPTURE, int(np.nonzero(~e_cap)[0][0])),
              (CAPTURE, int(np.nonzero(e_cap)[0][0])), (TAG, int(np.nonzero(e_tag)[0][1])),
              (CAPTURE, int(np.nonzero(e_cap)[0][1])), (TAG, int(np.nonzero(e_tag)[0][2]))]
    assert anchor not in blocks
    pairs = [(a, b) for a in blocks for b in blocks]
    cov, st, info = rp.covariance_pairs_anchored(anchor, pairs)
    ref = pairs_reference(oracle, anchored(inp, anchor), pairs, rp.camera, rp.cap, rp.tag, rows=rp.debug_reduced_rows())
    assert ref.e_ref_pairs <= E_REF_CAP and ref.ref.e_ref <= E_REF_CAP and ref.ref.min_pivot >= MIN_PIVOT_CAP
    tol = max(16.0 * max(ref.ref.e_ref, ref.e_ref_pairs), 1e-10)
    assert info["status"] == lm.COV_OK and np.all(st == lm.COV_OK) and np.array_equal(st, ref.status)
    worst = max(float(np.max(np.abs(_lens_to_soa(cov[p], *pairs[p]) - ref.cov[p]) / ref.scale[p])) for p in range(len(pairs)))
    print(f"g60 mixed, anchor {anchor}: {len(pairs)} pairs over {len(blocks)} blocks, error {worst:.2e} (tol {tol:.2e}, "
          f"e_ref {ref.ref.e_ref:.2e}, e_ref_pairs {ref.e_ref_pairs:.2e}); solve {info['t_selinv_ms']:.3f} ms")
    assert abs(info["min_pivot"] - ref.ref.min_pivot_rows) <= 1e-10
    assert worst <= tol
    # (a, b) and (b, a): transposes of the same bits; (a, a): exactly symmetric, the marginal to rounding
    n = len(blocks)
    for i in range(n):
        for j in range(n):
            assert np.array_equal(cov[i * n + j], cov[j * n + i].T)
    marg = rp.covariance_anchored(anchor)
    worst_m = 0.0
    for i, (kind, idx) in enumerate(blocks):
        if kind == CAMERA:
            continue
        m = (marg["cap"] if kind == CAPTURE else marg["tag"])[idx]
        d = np.sqrt(np.diag(m))
        worst_m = max(worst_m, float(np.max(np.abs(cov[i * n + i] - m) / np.outer(d, d))))
    print(f"  (a, a) against the marginal: {worst_m:.2e}")
    assert worst_m <= 2 * tol
    # a pair with the anchor
    cov2, st2, _ = rp.covariance_pairs_anchored(anchor, [(anchor, blocks[1]), (blocks[3], anchor), (anchor, anchor)])
    assert np.all(st2 == lm.COV_UNAVAILABLE) and np.all(cov2 == -1.0)
    # repeated: the same bits
    again, _, _ = rp.covariance_pairs_anchored(anchor, pairs)
    assert np.array_equal(again, cov)


# ---- 6. rules ----

@pytest.mark.parametrize("executor", [0, 1])
def test_repeated_calls_and_later_solves_keep_their_bits(lm, executor):
    inp = free(INPUTS["g60"])
    plain = _problem(lm, inp, elimination=lm.ELIM_MIXED, factor_executor=executor)
    want = _bits(plain, plain.solve())
    rp = _problem(lm, inp, elimination=lm.ELIM_MIXED, factor_executor=executor)
    assert _same(_bits(rp, rp.solve()), want)
    a = rp.covariance_anchored((TAG, 0))
    b = rp.covariance_anchored((TAG, 0))
    for k in ("cap", "tag", "cam", "cap_status", "tag_status"):
        assert np.array_equal(a[k], b[k])
    assert a["info"]["min_pivot"] == b["info"]["min_pivot"]
    rp.covariance_pairs_anchored((CAPTURE, 1), [((TAG, 1), (CAPTURE, 2))])
    assert _same(_bits(rp, rp.solve()), want)     # a solve after it: the bits of a solve without one
    c = rp.covariance_anchored((TAG, 0))
    assert np.array_equal(a["cap"], c["cap"]) and np.array_equal(a["tag"], c["tag"])


def test_refusals(lm):
    inp = INPUTS["g6"]    # (tag 0 constant: a truly mixed set)
    rp = _problem(lm, inp, elimination=lm.ELIM_MIXED)
    with pytest.raises(lm.LMError) as e:
        rp.covariance_anchored((TAG, 0))
    assert e.value.code == -7            # ARSLAM_E_STATE: no solve yet
    assert rp.solve()["elimination_used"] == lm.ELIM_MIXED
    g = inp.g
    for anchor in ((CAMERA, 0), (TAG, g.n_tag), (TAG, -2), (CAPTURE, g.n_cap), (7, 0)):
        for call in (lambda: rp.covariance_anchored(anchor), lambda: rp.covariance_pairs_anchored(anchor, [((TAG, 1), (TAG, 1))])):
            with pytest.raises(lm.LMError) as e:
                call()
            assert e.value.code == INVALID_ARG, anchor
    for call in (rp.covariance, rp.covariance_lens, lambda: rp.covariance_pairs([((TAG, 1), (TAG, 2))])):
        with pytest.raises(lm.LMError) as e:      # the old forms: still refused under a mixed set
            call()
        assert e.value.code == UNSUPPORTED
    assert rp.covariance_anchored((TAG, 0))["info"]["status"] == lm.COV_OK
    multi = _problem(lm, inp, force_multirank=True, comm=(0, 1, lambda a, op: None))
    multi.solve()
    for call in (lambda: multi.covariance_anchored((TAG, 0)), lambda: multi.covariance_pairs_anchored((TAG, 0), [((TAG, 1), (TAG, 1))])):
        with pytest.raises(lm.LMError) as e:
            call()
        assert e.value.code == UNSUPPORTED


def _all_minus_one(lm, out):
    assert out["info"]["status"] == lm.COV_RANK_DEFICIENT and out["info"]["min_pivot"] == -1.0
    assert np.all(out["cap"] == -1.0) and np.all(out["tag"] == -1.0) and np.all(out["cam"] == -1.0)
    assert not np.any(out["cap_status"] == lm.COV_OK) and not np.any(out["tag_status"] == lm.COV_OK)


@pytest.mark.parametrize("elimination", ["ELIM_MIXED", "ELIM_CAPTURES"])
def test_rank_deficiency(lm, elimination):
    """No anchor and no constant; two components sharing only the camera, the anchor in the first."""
    g = INPUTS["g6"].g
    two = synth.Graph(g.camera, np.vstack([g.cap, g.cap]), np.vstack([g.tag, g.tag]),
                      np.concatenate([g.obs_cap, g.obs_cap + g.n_cap]).astype(np.int32),
                      np.concatenate([g.obs_tag, g.obs_tag + g.n_tag]).astype(np.int32),
                      np.vstack([g.corners, g.corners]), g.camera_true, np.vstack([g.cap_true, g.cap_true]),
                      np.vstack([g.tag_true, g.tag_true]))
    rp, s = _solved(lm, CovInput(two, tag_const=()), elimination=getattr(lm, elimination))   # (MIXED: resolves to all tags)
    out = rp.covariance_anchored(None)
    _all_minus_one(lm, out)
    assert np.all(out["cap_status"] == lm.COV_RANK_DEFICIENT) and np.all(out["tag_status"] == lm.COV_RANK_DEFICIENT)
    for anchor in ((TAG, 0), (CAPTURE, g.n_cap + 1)):
        out = rp.covariance_anchored(anchor)
        _all_minus_one(lm, out)
        st = out["tag_status"] if anchor[0] == TAG else out["cap_status"]
        assert st[anchor[1]] == lm.COV_UNAVAILABLE and np.sum(st == lm.COV_UNAVAILABLE) == 1
    # anchored in one, constant in the other: a covariance (MIXED: 1 capture + 8 tags eliminated, 5 direct groups)
    rp, s = _solved(lm, CovInput(two, tag_const=(g.n_tag,)), elimination=getattr(lm, elimination))
    assert s["elimination_used"] == getattr(lm, elimination)
    assert rp.covariance_anchored(None)["info"]["status"] == lm.COV_RANK_DEFICIENT
    assert rp.covariance_anchored((TAG, 0))["info"]["status"] == lm.COV_OK


# ---- 7. pointer-keyed, after an append ----

def _pk_rows(lm, prob, n_cap, n_tag):
    cr, tr, cam = np.zeros(n_cap, np.int32), np.zeros(n_tag, np.int32), C.c_int(-1)
    rc = lm.lib().arslam_lm_debug_reduced_rows(prob._h, cr.ctypes.data_as(C.POINTER(C.c_int)),
                                               tr.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cam))
    assert rc == 0
    return cr, tr, cam.value


def test_pointer_keyed_after_an_append(lm, oracle):
    g = INPUTS["small"].g
    assert np.all(np.diff(g.obs_cap) >= 0)     # captures are first seen in index order: the handle numbers them as the graph does
    cam = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(g.n_cap)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem(elimination=lm.ELIM_MIXED)
    for o in range(g.n_obs):
        prob.add_residual_block(g.corners[o], cam, caps[g.obs_cap[o]], tags[g.obs_tag[o]])
    s = prob.solve()
    assert s["elimination_used"] == lm.ELIM_MIXED
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block_lens(tags[1])
    assert e.value.code == UNSUPPORTED
    # a new capture: a copy of an eliminated one (every tag it sees is on the reduced side), moved a little
    cap_row, _, _ = _pk_rows(lm, prob, g.n_cap, g.n_tag)
    src = int(np.nonzero(cap_row < 0)[0][0])
    new = caps[src] + np.array([0.01, -0.01, 0.01, 0.0, 0.0, 0.0])
    caps.append(new)
    obs = np.nonzero(g.obs_cap == src)[0]
    for b in obs:
        prob.add_residual_block(g.corners[b], cam, new, tags[g.obs_tag[b]])
    before = (cam.copy(), np.stack(caps).copy(), np.stack(tags).copy())
    s = prob.solve()
    assert s["setup_kind"] == lm.SETUP_APPEND and s["elimination_used"] == lm.ELIM_MIXED
    grown = dataclasses.replace(g, cap=before[1], tag=before[2], camera=before[0],
                                obs_cap=np.concatenate([g.obs_cap, np.full(len(obs), g.n_cap)]).astype(np.int32),
                                obs_tag=np.concatenate([g.obs_tag, g.obs_tag[obs]]).astype(np.int32),
                                corners=np.vstack([np.asarray(g.corners).reshape(-1, 8), np.asarray(g.corners).reshape(-1, 8)[obs]]))
    inp = CovInput(grown, tag_const=())
    now = (cam.copy(), np.stack(caps), np.stack(tags))
    cap_row, tag_row, _ = _pk_rows(lm, prob, len(caps), len(tags))
    reduced_cap = int(np.nonzero(cap_row >= 0)[0][0])
    for anchor, block in (((TAG, 0), tags[0]), ((CAPTURE, reduced_cap), caps[reduced_cap])):
        ref = reference(oracle, anchored(inp, anchor), *now)
        assert ref.e_ref <= E_REF_CAP and ref.min_pivot >= MIN_PIVOT_CAP
        tol = max(16.0 * ref.e_ref, 1e-10)
        worst = 0.0
        for blocks, want, st in ((caps, ref.cap, ref.cap_status), (tags, ref.tag, ref.tag_status)):
            for i, b in enumerate(blocks):
                c, sb = prob.covariance_block_anchored(block, b)
                assert sb == st[i]
                if sb != lm.COV_OK:
                    assert np.all(c == -1.0)
                    continue
                assert np.array_equal(c, c.T)
                d = np.sqrt(np.diag(want[i]))
                worst = max(worst, float(np.max(np.abs(c - want[i]) / np.outer(d, d))))
        c, sb = prob.covariance_block_anchored(block, cam)
        assert sb == lm.COV_OK and c.shape == (3, 3) and np.all(c.ravel()[1:] == 0.0)
        worst = max(worst, abs(c[0, 0] - ref.var_f) / ref.var_f)
        c, sb = prob.covariance_block_anchored(block, block)
        assert sb == lm.COV_UNAVAILABLE and np.all(c == -1.0)
        # a cross block: the new capture against a tag it sees
        t = int(g.obs_tag[obs[-1]])
        pref = pairs_ref.covariance_pairs(oracle, now + (grown.obs_cap, grown.obs_tag, grown.corners),
                                          [((CAPTURE, g.n_cap), (TAG, t))], False, *anchored(inp, anchor).consts(),
                                          scale_arrays=before + (grown.obs_cap, grown.obs_tag, grown.corners))
        c, sb = prob.covariance_block_pair_anchored(block, new, tags[t])
        assert sb == pref.status[0]
        e_pair = float(np.max(np.abs(c - pref.cov[0]) / pref.scale[0])) if sb == lm.COV_OK else 0.0
        print(f"pointer-keyed small + 1 capture, anchor {anchor}: blocks {worst:.2e}, pair {e_pair:.2e} (tol {tol:.2e}, "
              f"e_ref {ref.e_ref:.2e}, e_ref_pairs {pref.e_ref_pairs:.2e})")
        assert worst <= tol and e_pair <= max(tol, 16.0 * pref.e_ref_pairs)
    # the same anchor: the kept result; None and a bad pointer
    a1, _ = prob.covariance_block_anchored(caps[reduced_cap], tags[2])
    a2, _ = prob.covariance_block_anchored(caps[reduced_cap], tags[2])
    assert np.array_equal(a1, a2)
    c, sb = prob.covariance_block_anchored(None, tags[2])
    assert sb == lm.COV_RANK_DEFICIENT and np.all(c == -1.0)
    with pytest.raises(lm.LMError) as e:
        prob.covariance_block_anchored(np.zeros(6), tags[2])
    assert e.value.code == INVALID_ARG
    # the camera block as the anchor, at the C-ABI (the wrapper would refuse a 3-vector itself)
    dp = C.POINTER(C.c_double)
    out, st = np.zeros((6, 6)), C.c_int(0)
    args = (cam.ctypes.data_as(dp), tags[2].ctypes.data_as(dp))
    assert lm.lib().arslam_lm_covariance_block_anchored(prob._h, *args, out.ctypes.data_as(dp), C.byref(st)) == INVALID_ARG
    assert lm.lib().arslam_lm_covariance_block_pair_anchored(prob._h, *args, tags[3].ctypes.data_as(dp),
                                                             out.ctypes.data_as(dp), C.byref(st)) == INVALID_ARG


# ---- 8. an estimated lens ----

def test_estimated_lens_anchored(lm, oracle):
    from test_gpu_lm_cov_lens import _check_marginals, _consts, _est_problem, _reference
    from test_lm_cov_lens import graph
    g = graph("g20")
    rp, A, cc, tc = _est_problem(lm, g, tag_const=(), elimination=lm.ELIM_CAPTURES)
    s = rp.solve()
    assert s["elimination_used"] == lm.ELIM_CAPTURES and abs(rp.camera[1]) > 1e-3
    for anchor in ((TAG, 3), (CAPTURE, 4)):
        ca, ta = _consts(g, cap_const=(4,) if anchor[0] == CAPTURE else (), tag_const=(3,) if anchor[0] == TAG else ())
        out = rp.covariance_anchored(anchor)
        _check_marginals(lm, out, _reference(oracle, rp, g, A, ca, ta), f"estimated lens g20, anchor {anchor}")
        assert (out["tag_status"][3] if anchor[0] == TAG else out["cap_status"][4]) == lm.COV_UNAVAILABLE
