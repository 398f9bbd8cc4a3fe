"""GPU tests of arslam_lm_evaluate (ceres::Problem::Evaluate for the mapper) against the numpy
reference over the oracle (tests/evaluate_ref.py).

Tolerances (evaluate_ref's header): the residuals at the project's row bound, rtol 1e-12 and
atol 1e-9 (tests/test_gpu_parity.py); every other quantity at that bound carried to first order
through it, computed from the reference's values.  Every reference case prints its worst measured
error over its tolerance ("evaluate-error ..."); the MI355X's figures are kept in
profiles/evaluate/device_errors.txt.  The exact conditions are array_equal.
"""
import dataclasses
import functools

import numpy as np
import pytest

import evaluate_ref as eref
import loss_ref
import tag_size_ref as tref
from ar_slam_amd import synth
from evaluate_ref import PINHOLE, RADIAL, RADIAL_FREE
from loss_ref import CAUCHY, HUBER, NONE, SOFT_L_ONE

pytestmark = pytest.mark.gpu

E_UNSUPPORTED, E_STATE = -2, -7
MILD = (-0.12, 0.03)
PREFIXES = (1, 7, 8, 9, 64, 65)


# ---- inputs, built once ----

@functools.lru_cache(maxsize=None)
def _base(oracle):
    """name -> (camera, cap, tag, obs_cap, obs_tag, corners): corners = the oracle's projection at the
    arrays' values + 0.5 px noise."""
    G = tref.trace_graphs()
    out = {}
    g20 = eref.project(oracle, tref.arrays(G["g20"][0]), seed=1)
    out["g20"] = g20
    for k in PREFIXES:   # all of g20's blocks, its first k observations: a partial wavefront, unseen blocks
        out[f"g20[:{k}]"] = g20[:3] + tuple(v[:k] for v in g20[3:])
    out["g6"] = eref.project(oracle, tref.arrays(G["g6"][0]), seed=2)
    out["gk11"] = eref.project(oracle, tref.arrays(G["gk11"][0]), seed=3)
    out["star"] = eref.star(oracle)
    g6 = tref.arrays(G["g6"][0])
    cap = np.array(g6[1], np.float64).copy()
    cap[0, 3:] = 0.0   # one capture at omega = 0 exactly: the angle-axis small branch
    out["omega0"] = eref.project(oracle, (g6[0], cap) + g6[2:], seed=4)
    return out


@functools.lru_cache(maxsize=None)
def _g20_outliers(oracle):
    """g20 with noisy corners and loss_ref.outliers' 5 % of 40 px shifts (the losses' outer branches)."""
    g = tref.trace_graphs()["g20"][0]
    gn = dataclasses.replace(g, corners=_base(oracle)["g20"][5])
    go, bad = loss_ref.outliers(gn)
    assert len(bad) >= 5
    return tref.arrays(go)


def _const(n, i):
    c = np.zeros(n, np.uint8)
    c[i] = 1
    return c


def _variants(oracle):
    """name -> (arrays, kwargs of eref.evaluate) on g20."""
    base = _base(oracle)["g20"]
    out_arr = _g20_outliers(oracle)
    nb, nc, nt = len(base[3]), len(base[1]), len(base[2])
    sizes = tref.tag_sizes(nt)
    mild_cam = np.array([base[0][0], *MILD])
    radial = eref.project(oracle, (mild_cam,) + base[1:], model=RADIAL, seed=5)
    return {
        "huber": (out_arr, dict(kinds=HUBER, a=3.0)),
        "soft_l_one": (out_arr, dict(kinds=SOFT_L_ONE, a=3.0)),
        "cauchy_outliers": (out_arr, dict(kinds=CAUCHY, a=3.0)),
        "mixed": (out_arr, dict(kinds=(np.arange(nb) % 4).astype(np.uint8), a=1.5 + 0.5 * (np.arange(nb) % 5))),
        "sized": (eref.project(oracle, base, tag_size=sizes, seed=6), dict(tag_size=sizes, kinds=CAUCHY, a=3.0)),
        "radial_held": (radial, dict(model=RADIAL)),
        "radial_free_from_0": ((np.array([base[0][0], 0.0, 0.0]),) + radial[1:], dict(model=RADIAL_FREE, kinds=CAUCHY, a=3.0)),
        "radial_free_from_mild": (radial, dict(model=RADIAL_FREE)),
        "radial_free_camera_const": (radial, dict(model=RADIAL_FREE, camera_const=True)),
        "tag_const": (base, dict(tag_const=_const(nt, 0), kinds=CAUCHY, a=3.0)),
        "cap_const": (base, dict(cap_const=_const(nc, 3))),
        "camera_const": (base, dict(camera_const=True)),
        "no_apply": (out_arr, dict(kinds=CAUCHY, a=3.0, apply_loss=False)),
    }


def _resident(lm, arrays, kinds=0, a=0.0, tag_size=None, model=PINHOLE, camera_const=False, cap_const=None,
              tag_const=None, apply_loss=True, **opts):
    nb = len(arrays[3])
    kw = {}
    if np.ndim(kinds):
        kw["obs_loss"] = (kinds, np.broadcast_to(np.asarray(a, np.float64), (nb,)))
    elif kinds != NONE:
        kw["loss"] = (int(kinds), float(a))
    if model != PINHOLE:
        kw["camera_model"] = lm.CAMERA_RADIAL
    if model == RADIAL_FREE:
        kw["estimate_distortion"] = True
    return lm.ResidentProblem(*arrays, camera_const, cap_const, tag_const, tag_size=tag_size, **kw, **opts)


def _check(lm, oracle, name, arrays, **kw):
    ref = eref.evaluate(oracle, arrays, **kw)
    R = _resident(lm, arrays, **kw)
    got = R.evaluate(apply_loss=kw.get("apply_loss", True))
    R.close()
    w = eref.worst(got, ref)
    print(f"evaluate-error {name}: n_obs {len(arrays[3])} " + " ".join(f"{k} {v:.3g}" for k, v in sorted(w.items())))
    assert got["residuals"].shape == (len(arrays[3]), 8)
    for k, v in w.items():
        assert v <= 1.0, (name, k, v)
    # the entries that must be exactly zero are
    assert np.all(eref.flat_gradient(got["gradient"])[ref.zero] == 0.0)
    return got, ref


SHAPES = ["g20"] + [f"g20[:{k}]" for k in PREFIXES] + ["g6", "gk11", "star", "omega0"]


# ---- 1. against the reference ----

@pytest.mark.parametrize("loss", ["none", "cauchy"])
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_reference_on_every_shape(lm, oracle, shape, loss):
    kw = dict(kinds=CAUCHY, a=3.0) if loss == "cauchy" else {}
    got, ref = _check(lm, oracle, f"{shape}/{loss}", _base(oracle)[shape], **kw)
    if loss == "none":
        assert np.all(got["weight"] == 1.0)


@pytest.mark.parametrize("variant", ["huber", "soft_l_one", "cauchy_outliers", "mixed", "sized", "radial_held",
                                     "radial_free_from_0", "radial_free_from_mild", "radial_free_camera_const",
                                     "tag_const", "cap_const", "camera_const", "no_apply"])
def test_matches_reference_on_every_variant(lm, oracle, variant):
    arrays, kw = _variants(oracle)[variant]
    got, ref = _check(lm, oracle, f"g20/{variant}", arrays, **kw)
    g = got["gradient"]
    if variant in ("huber", "soft_l_one", "cauchy_outliers", "mixed"):
        assert np.min(got["weight"]) < 0.5    # (the shifted observations are on the losses' outer branches)
    if variant == "huber":
        assert np.any(got["weight"] == 1.0)
    if variant.startswith("radial_free_from"):
        assert np.all(g["camera"][1:] != 0.0)
    if variant == "no_apply":
        assert np.all(got["weight"] == 1.0) and got["cost"] == pytest.approx(0.5 * np.sum(got["sq_norm"]), rel=1e-13)


# ---- 2. exact conditions ----

def _same(a, b, keys=("cost", "residuals", "sq_norm", "weight")):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    if a.get("gradient") is not None and b.get("gradient") is not None:
        assert np.array_equal(eref.flat_gradient(a["gradient"]), eref.flat_gradient(b["gradient"]))


def test_two_calls_give_the_same_bits(lm, oracle):
    R = _resident(lm, _g20_outliers(oracle), kinds=CAUCHY, a=3.0)
    _same(R.evaluate(), R.evaluate())


def test_independent_of_elimination_and_executor(lm):
    g, _ = loss_ref.outliers(synth.config_graph("small"))
    arrays = tref.arrays(g)
    first = None
    for elim in (lm.ELIM_CAPTURES, lm.ELIM_TAGS, lm.ELIM_MIXED):
        for executor in (0, 1):
            R = _resident(lm, arrays, kinds=CAUCHY, a=3.0, elimination=elim, factor_executor=executor)
            e = R.evaluate()
            R.close()
            if first is None:
                first = e
            _same(first, e)
    assert first["cost"] > 0.0 and np.min(first["weight"]) < 0.1


def test_all_none_kinds_equal_no_loss(lm, oracle):
    arrays = _g20_outliers(oracle)
    nb = len(arrays[3])
    a = _resident(lm, arrays, kinds=np.zeros(nb, np.uint8), a=3.0).evaluate()
    _same(a, _resident(lm, arrays).evaluate())


def test_default_sides_equal_unsized(lm, oracle):
    arrays = _g20_outliers(oracle)
    a = _resident(lm, arrays, kinds=CAUCHY, a=3.0, tag_size=np.full(len(arrays[2]), lm.DEFAULT_TAG_SIZE)).evaluate()
    _same(a, _resident(lm, arrays, kinds=CAUCHY, a=3.0).evaluate())


def test_apply_loss_off_equals_lossless_handle(lm, oracle):
    arrays = _g20_outliers(oracle)
    a = _resident(lm, arrays, kinds=CAUCHY, a=3.0).evaluate(apply_loss=False)
    _same(a, _resident(lm, arrays).evaluate())


def test_terms_do_not_depend_on_the_requested_outputs(lm, oracle):
    R = _resident(lm, _g20_outliers(oracle), kinds=CAUCHY, a=3.0)
    full = R.evaluate()
    for res, grad in ((False, True), (True, False), (False, False)):
        e = R.evaluate(residuals=res, gradient=grad)
        _same(full, e, keys=("cost", "sq_norm", "weight"))
        assert (e["residuals"] is None) == (not res) and (e["gradient"] is None) == (not grad)
        if res:
            assert np.array_equal(e["residuals"], full["residuals"])
        if grad:
            assert np.array_equal(eref.flat_gradient(e["gradient"]), eref.flat_gradient(full["gradient"]))


def test_constant_and_unseen_blocks_are_exactly_zero(lm, oracle):
    arrays = _base(oracle)["g20[:9]"]
    nc, nt = len(arrays[1]), len(arrays[2])
    c0, t0 = int(arrays[3][0]), int(arrays[4][0])
    g = _resident(lm, arrays, kinds=CAUCHY, a=3.0, cap_const=_const(nc, c0), tag_const=_const(nt, t0)).evaluate()["gradient"]
    seen_c, seen_t = np.isin(np.arange(nc), arrays[3]), np.isin(np.arange(nt), arrays[4])
    assert not seen_c.all() and not seen_t.all()
    assert np.all(g["cap"][~seen_c] == 0.0) and np.all(g["tag"][~seen_t] == 0.0)
    assert np.all(g["cap"][c0] == 0.0) and np.all(g["tag"][t0] == 0.0)
    free_c = seen_c & (np.arange(nc) != c0)
    assert np.all(g["cap"][free_c] != 0.0)
    assert g["camera"][0] != 0.0 and np.all(g["camera"][1:] == 0.0)
    gc = _resident(lm, arrays, camera_const=True).evaluate()["gradient"]
    assert np.all(gc["camera"] == 0.0) and np.all(gc["cap"][seen_c] != 0.0)


def test_pinhole_ignores_the_lens_entries(lm, oracle):
    arrays = _base(oracle)["g20"]
    lens = (np.array([arrays[0][0], *MILD]),) + arrays[1:]
    _same(_resident(lm, arrays, kinds=CAUCHY, a=3.0).evaluate(), _resident(lm, lens, kinds=CAUCHY, a=3.0).evaluate())


def test_reads_the_values_as_they_are_now(lm, oracle):
    """The SoA arrays given at load time are read at every call: a value written there shows."""
    arrays = _base(oracle)["g6"]
    R = _resident(lm, arrays)
    e0 = R.evaluate()
    R.cap[1, 0] += 0.01
    moved = (arrays[0], R.cap.copy()) + arrays[2:]
    e1 = R.evaluate()
    assert e1["cost"] != e0["cost"]
    _same(e1, _resident(lm, moved).evaluate())


# ---- 3. against the solver ----

def test_agrees_with_the_solver_and_leaves_it_alone(lm, oracle):
    g = tref.trace_graphs()["g20"][0]
    arrays = tref.arrays(g)
    tc = _const(g.n_tag, 0)
    R = _resident(lm, arrays, tag_const=tc)
    e0 = R.evaluate()
    s = R.solve()
    e1 = R.evaluate()
    rel = 4 * g.n_obs * 2.2e-16
    print(f"cost before {e0['cost']:.17g} initial_cost {s['initial_cost']:.17g}; after {e1['cost']:.17g} "
          f"final_cost {s['final_cost']:.17g}")
    assert abs(e0["cost"] - s["initial_cost"]) <= rel * s["initial_cost"]
    assert abs(e1["cost"] - s["final_cost"]) <= rel * s["final_cost"]
    # max |gradient| at the loaded point: the tolerance of the entry that attains it
    ref = eref.evaluate(oracle, arrays, tag_const=tc)
    gf = eref.flat_gradient(e0["gradient"])
    i = int(np.argmax(np.abs(ref.gradient)))
    gmax = s["iterations"][0]["gradient_max_norm"]
    print(f"max |gradient| {np.max(np.abs(gf)):.17g} solver {gmax:.17g} tolerance {ref.tol_gradient[i]:.3g}")
    assert abs(np.max(np.abs(gf)) - gmax) <= ref.tol_gradient[i]
    # a handle that never evaluated: the same trace, bit for bit
    R2 = _resident(lm, arrays, tag_const=tc)
    s2 = R2.solve()
    keys = ("cost", "cost_change", "gradient_max_norm", "gradient_norm", "step_norm", "relative_decrease",
            "trust_region_radius", "step_is_valid", "step_is_successful")
    assert len(s["iterations"]) == len(s2["iterations"])
    for a, b in zip(s["iterations"], s2["iterations"]):
        assert all(a[k] == b[k] for k in keys), (a, b)
    assert s["final_cost"] == s2["final_cost"] and s["termination"] == s2["termination"]
    assert np.array_equal(R.cap, R2.cap) and np.array_equal(R.tag, R2.tag) and np.array_equal(R.camera, R2.camera)


# ---- 4. pointer-keyed ----

def test_pointer_keyed_blocks_agree_with_the_soa_form(lm, oracle):
    arrays = _g20_outliers(oracle)
    camera, cap, tag, obs_cap, obs_tag, corners = arrays
    nb = len(obs_cap)
    kinds = (np.arange(nb) % 4).astype(np.uint8)
    a = 1.5 + 0.5 * (np.arange(nb) % 5)
    sizes = tref.tag_sizes(len(tag))
    cam = np.array(camera, np.float64).copy()
    caps = [np.array(c, np.float64).copy() for c in cap]
    tags = [np.array(t, np.float64).copy() for t in tag]
    P = lm.Problem()
    for o in range(nb - 1):
        P.add_residual_block(corners[o], cam, caps[obs_cap[o]], tags[obs_tag[o]], loss=(int(kinds[o]), float(a[o])),
                             size=float(sizes[obs_tag[o]]))
    P.set_parameter_block_constant(tags[0])

    def soa(n):
        # (the blocks number captures and tags in first-seen order; g20's observations are capture-major
        # and the SoA form keeps every block, so compare per block through the pointers' indices)
        return _resident(lm, (camera, cap, tag, obs_cap[:n], obs_tag[:n], corners[:n]), kinds=kinds[:n], a=a[:n],
                         tag_size=sizes, tag_const=_const(len(tag), 0)).evaluate()

    def compare(n):
        e, ref = P.evaluate(), soa(n)
        _same(e, ref, keys=("cost", "residuals", "sq_norm", "weight"))
        assert np.array_equal(P.gradient_block(cam), ref["gradient"]["camera"])
        for c in sorted(set(obs_cap[:n])):
            assert np.array_equal(P.gradient_block(caps[c]), ref["gradient"]["cap"][c])
        for t in sorted(set(obs_tag[:n])):
            assert np.array_equal(P.gradient_block(tags[t]), ref["gradient"]["tag"][t])
        assert np.all(P.gradient_block(tags[0]) == 0.0)

    compare(nb - 1)
    # one more block: the kept gradient is stale until the next evaluate
    o = nb - 1
    P.add_residual_block(corners[o], cam, caps[obs_cap[o]], tags[obs_tag[o]], loss=(int(kinds[o]), float(a[o])),
                         size=float(sizes[obs_tag[o]]))
    with pytest.raises(lm.LMError) as err:
        P.gradient_block(cam)
    assert err.value.code == E_STATE
    compare(nb)
    # after the blocks' solve: the cost at the values written back to the caller's blocks
    s = P.solve()
    assert abs(P.evaluate()["cost"] - s["final_cost"]) <= 4 * nb * 2.2e-16 * s["final_cost"]


# ---- 5. what it is for ----

def test_weights_show_the_rejected_detections(lm, oracle):
    g, bad = loss_ref.outliers(synth.config_graph("small"))
    R = _resident(lm, tref.arrays(g), kinds=CAUCHY, a=3.0)
    s = R.solve()
    assert s["termination"] == "CONVERGENCE"
    e = R.evaluate(residuals=False, gradient=False)
    hi_bad, lo_good = eref.weights_separate(e["weight"], bad)
    print(f"largest weight of a shifted observation {hi_bad:.4g}, smallest of the others {lo_good:.4g}")
    assert hi_bad < lo_good
    assert abs(e["cost"] - s["final_cost"]) <= 4 * g.n_obs * 2.2e-16 * s["final_cost"]


# ---- 6. the SLAM mirror ----

def test_mirror_evaluate(lm, oracle):
    g = synth.config_graph("tiny")
    S = lm.SlamSolver()
    S.set_camera(g.camera)
    S.set_loss(CAUCHY, 3.0)
    n_map = g.n_cap - 1          # the last capture's detections arrive after the solve
    misread = None
    for c in range(g.n_cap):
        sel = np.flatnonzero(g.obs_cap == c)
        corners = np.array(g.corners[sel], np.float64).reshape(-1, 8).copy()
        if c == 2:
            corners[1] += np.tile([30.0, -25.0], 4)   # one misread tag
            misread = int(sel[1])
        if c == n_map:
            S.solve()
        S.add_detections(f"cap{c}", [f"tag{t}" for t in g.obs_tag[sel]], corners, 1020, 768)
    e = S.evaluate()
    n_blocks = S.num_blocks
    assert len(e["weight"]) == n_blocks == g.n_obs
    added = np.array([S.block(b)[3] for b in range(n_blocks)], bool)
    assert added.sum() == np.sum(g.obs_cap < n_map) and not added.all()
    assert np.all(e["weight"][~added] == -1.0) and np.all(e["sq_norm"][~added] == -1.0)
    assert np.all(e["weight"][added] > 0.0)
    print(f"misread block {misread}: weight {e['weight'][misread]:.4g}; smallest other "
          f"{np.min(np.delete(e['weight'][added], misread)):.4g}")
    assert int(np.argmin(np.where(added, e["weight"], np.inf))) == misread
    # against the reference at the mirror's poses
    blocks = [S.block(b) for b in range(n_blocks) if added[b]]
    cap = np.array([S.capture(c)[1] for c in range(S.num_captures)])
    tag = np.array([S.aruco(a)[1] for a in range(S.num_arucos)])
    arrays = (S.camera()[0], cap, tag, np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks]),
              np.array([b[2] for b in blocks]).reshape(-1, 8))
    ref = eref.evaluate(oracle, arrays, CAUCHY, 3.0)
    got = {"cost": e["cost"], "sq_norm": e["sq_norm"][added], "weight": e["weight"][added]}
    w = eref.worst(got, ref)
    print("evaluate-error mirror: " + " ".join(f"{k} {v:.3g}" for k, v in sorted(w.items())))
    assert all(v <= 1.0 for v in w.values()), w


def test_several_ranks_are_refused(lm, oracle):
    arrays = _base(oracle)["g6"]
    R = lm.ResidentProblem(*arrays, comm=(0, 1, lambda a, op: None), force_multirank=True)
    with pytest.raises(lm.LMError) as err:
        R.evaluate()
    assert err.value.code == E_UNSUPPORTED
