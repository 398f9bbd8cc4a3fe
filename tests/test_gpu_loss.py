"""GPU tests of the robust losses (Huber, SoftLOne, Cauchy; include/arslam_lm.h
ARSLAM_LOSS_*) against numpy over the oracle's residuals and Jacobians
(tests/loss_ref.py; the oracle itself has no loss).

Tolerances: the corrected rows and rho per observation 1e-12 relative (the
residual / Jacobian test's); costs against numpy 1e-12 relative (sums of a few
hundred to a few thousand positive terms in another order); gradient norms
1e-9; the model cost change 1e-7 (the step is recovered by subtraction);
comparisons between elimination sides, APIs and rank counts at the tolerances
the existing tests use for them (test_gpu_elimination.py, test_gpu_multirank.py).
"""
import os
import socket

import numpy as np
import pytest

import loss_ref
from ar_slam_amd import synth
from gauge import assert_poses_match
from loss_ref import CAUCHY, HUBER, NONE, SOFT_L_ONE, outliers, pack, robust_terms

pytestmark = pytest.mark.gpu

LOSSES = {"huber": (HUBER, 3.0), "soft_l_one": (SOFT_L_ONE, 3.0), "cauchy": (CAUCHY, 3.0)}


def _random_obs(rng, n):
    """(as test_gpu_parity.test_residual_jacobian_matches_oracle draws them)"""
    cam = np.stack([rng.uniform(500, 3000, n), np.zeros(n), np.zeros(n)], 1)
    tag = np.concatenate([rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))], 1)
    w = rng.normal(0, 1, (n, 3)) * rng.choice([1.0, 1e-2, 0.0, 3.0], (n, 1))
    cap = np.concatenate([-tag[:, :3] + rng.normal(0, 0.2, (n, 3)) + [0, 0, 1.0], w], 1)
    tag[::5, 3:] = 0.0
    corners = rng.normal(0, 100, (n, 8))
    return cam, cap, tag, corners


def test_corrected_rows_match_numpy(lm, oracle):
    """Stage parity: every kind, each on both sides of its branch (a = sqrt(s) / 2 and 2 sqrt(s))."""
    rng = np.random.default_rng(7)
    n = 512
    cam, cap, tag, corners = _random_obs(rng, n)
    kinds = (np.arange(n) % 4).astype(np.uint8)
    ro = np.zeros((n, 8))
    Jo = np.zeros((n, 8, 15))
    for i in range(n):
        ro[i], Jo[i] = oracle.residual_jacobian(cam[i], cap[i], tag[i], corners[i])
    s = np.sum(ro * ro, 1)
    a = np.sqrt(s) * np.where((np.arange(n) // 4) % 2 == 0, 0.5, 2.0)
    r, J, rho = lm.debug_residual_jacobian_loss(cam, cap, tag, corners, kinds, a)
    bit = 0
    for i in range(n):
        p, p1 = loss_ref.rho(int(kinds[i]), a[i], s[i])
        w = np.sqrt(p1)
        bit += int(w < 1.0)
        print(f"obs {i} kind {kinds[i]} s/b {s[i] / a[i] ** 2:.3g} rho {rho[i]:.17g} ref {float(p):.17g}")
        assert abs(rho[i] - p) <= 1e-12 * abs(p)
        assert np.max(np.abs(r[i] - w * ro[i])) <= 1e-12 * np.max(np.abs(w * ro[i]))
        scale = np.abs(w * Jo[i]).max(axis=1, keepdims=True) + 1e-300
        assert np.max(np.abs(J[i] - w * Jo[i]) / scale) < 1e-12
    assert bit >= n // 4   # (the losses did bite: Huber's upper branch, SoftLOne and Cauchy everywhere)
    # kind NONE leaves the rows of the plain entry, bit for bit
    r0, J0 = lm.debug_residual_jacobian(cam, cap, tag, corners)
    none = kinds == NONE
    assert np.array_equal(r[none], r0[none]) and np.array_equal(J[none], J0[none])
    assert np.array_equal(J[..., 3:6], J[..., 9:12])


# ---- solves, shared between the tests below (each graph and loss solved once) ----
_GRAPHS = {}
_RUNS = {}


def _graph(name):
    if name not in _GRAPHS:
        clean = synth.config_graph(name.split("+")[0])
        _GRAPHS[name] = outliers(clean) if name.endswith("+outliers") else (clean, np.zeros(0, int))
    return _GRAPHS[name]


def _mixed_losses(g):
    o = np.arange(g.n_obs)
    return (o % 4).astype(np.uint8), 2.0 + (o % 3)


def _run(lm, name, loss_key, record=True, **opts):
    """One solve of graph `name` under LOSSES[loss_key] (None: no loss; "mixed": per-observation
    kinds o % 4, scales 2 + o % 3), with the state copied at every iteration callback."""
    key = (name, loss_key, record, tuple(sorted(opts.items())))
    if key in _RUNS:
        return _RUNS[key]
    g, _ = _graph(name)
    kw = {}
    if loss_key == "mixed":
        kw["obs_loss"] = _mixed_losses(g)
    elif loss_key is not None:
        kw["loss"] = LOSSES[loss_key]
    if record:
        opts = dict(opts, update_state_every_iteration=1)
    rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, **kw, **opts)
    states = []
    if record:
        rp.set_iteration_callback(lambda it: states.append(pack(rp.camera, rp.cap, rp.tag)))
    s = rp.solve()
    out = dict(camera=rp.camera.copy(), cap=rp.cap.copy(), tag=rp.tag.copy(), s=s, states=states)
    rp.close()
    _RUNS[key] = out
    return out


def _losses_of(g, loss_key):
    if loss_key == "mixed":
        return _mixed_losses(g)
    return (NONE, 1.0) if loss_key is None else LOSSES[loss_key]


def _terms_at(oracle, g, loss_key, x):
    nc, nt = g.n_cap, g.n_tag
    kinds, a = _losses_of(g, loss_key)
    return robust_terms(oracle, (x[:3], x[3:3 + 6 * nc].reshape(nc, 6), x[3 + 6 * nc:].reshape(nt, 6),
                                 g.obs_cap, g.obs_tag, g.corners), kinds, a)


def _bitwise_same(a, b):
    ia, ib = a["s"]["iterations"], b["s"]["iterations"]
    assert len(ia) == len(ib)
    for f in ("cost", "trust_region_radius", "step_norm"):
        assert [i[f] for i in ia] == [i[f] for i in ib], f
    for f in ("camera", "cap", "tag"):
        assert np.array_equal(a[f], b[f]), f


def test_loss_off_is_bit_identical(lm):
    g = synth.config_graph("small")
    args = (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)

    def solve(**kw):
        rp = lm.ResidentProblem(*args, **kw)
        s = rp.solve()
        return dict(camera=rp.camera.copy(), cap=rp.cap.copy(), tag=rp.tag.copy(), s=s)

    plain = solve()
    assert plain["s"]["termination"] == "CONVERGENCE" and len(plain["s"]["iterations"]) > 3
    _bitwise_same(solve(loss=(lm.LOSS_NONE, 0.0)), plain)
    _bitwise_same(solve(obs_loss=(np.zeros(g.n_obs, np.uint8), np.zeros(g.n_obs))), plain)
    # (the one-shot entry and solve_graph's loss arguments reach the same code)
    cam, cap, tag, s = lm.solve_graph(g, loss=(lm.LOSS_NONE, 0.0))
    _bitwise_same(dict(camera=cam, cap=cap, tag=tag, s=s), plain)


def test_loss_that_never_bites_agrees_with_no_loss(lm):
    """Huber(1e6) runs the kLoss kernels with rho' = 1: the same solve, the cost sums rounded otherwise."""
    g = synth.config_graph("small")
    args = (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    out = []
    for kw in ({}, dict(loss=(lm.LOSS_HUBER, 1e6))):
        rp = lm.ResidentProblem(*args, **kw)
        out.append((rp.solve(), rp.camera.copy(), rp.cap.copy(), rp.tag.copy()))
    (s0, cam0, cap0, tag0), (s1, cam1, cap1, tag1) = out
    assert len(s0["iterations"]) == len(s1["iterations"])
    assert (s0["termination"], s0["rule"]) == (s1["termination"], s1["rule"])
    for a, b in zip(s1["iterations"], s0["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-12 * b["cost"]
    assert_poses_match(cap1, tag1, cap0, tag0, tags=np.unique(g.obs_tag), caps=np.unique(g.obs_cap))


def _check_iteration0(oracle, g, run, loss_key):
    s = run["s"]
    ref = _terms_at(oracle, g, loss_key, pack(g.camera, g.cap, g.tag))
    it0 = s["iterations"][0]
    gmax, gnorm = np.abs(ref.grad).max(), np.linalg.norm(ref.grad)
    print(f"{loss_key}: iteration 0 cost {it0['cost']:.17g} numpy {ref.cost:.17g}; |g|max {it0['gradient_max_norm']:.17g} "
          f"numpy {gmax:.17g}; |g| {it0['gradient_norm']:.17g} numpy {gnorm:.17g}")
    assert abs(it0["cost"] - ref.cost) <= 1e-12 * ref.cost
    assert abs(s["initial_cost"] - ref.cost) <= 1e-12 * ref.cost
    assert abs(it0["gradient_max_norm"] - gmax) <= 1e-9 * gmax
    assert abs(it0["gradient_norm"] - gnorm) <= 1e-9 * gnorm
    assert s["fixed_cost"] == 0.0
    return ref


def _check_accepted_steps(oracle, g, run, loss_key, ref0):
    s, states = run["s"], run["states"]
    its = s["iterations"]
    assert len(states) == len(its)
    n_ok = 0
    for i, it in enumerate(its):
        if i and not it["step_is_successful"]:
            continue
        c = _terms_at(oracle, g, loss_key, states[i]).cost
        print(f"{loss_key}: iteration {i} cost {it['cost']:.17g} numpy {c:.17g}")
        assert abs(it["cost"] - c) <= 1e-12 * c, (i, it["cost"], c)
        n_ok += i > 0
    assert n_ok >= 3
    final = _terms_at(oracle, g, loss_key, pack(run["camera"], run["cap"], run["tag"])).cost
    assert abs(s["final_cost"] - final) <= 1e-12 * final
    # the model cost change is the corrected rows': the first accepted step, linearized at x0
    k = next(i for i in range(1, len(its)) if its[i]["step_is_successful"])
    delta = states[k] - states[0]
    m = ref0.model_cost_change(delta)
    it = its[k]
    print(f"{loss_key}: first accepted step {k}: relative_decrease * m {it['relative_decrease'] * m:.17g} "
          f"cost_change {it['cost_change']:.17g}")
    assert m > 0 and it["cost_change"] > 0
    assert abs(it["relative_decrease"] * m - it["cost_change"]) <= 1e-7 * it["cost_change"]


@pytest.mark.parametrize("loss_key", list(LOSSES))
def test_iteration0_matches_numpy(lm, oracle, loss_key):
    g, _ = _graph("small+outliers")
    _check_iteration0(oracle, g, _run(lm, "small+outliers", loss_key), loss_key)


@pytest.mark.parametrize("loss_key", list(LOSSES))
def test_accepted_steps_match_numpy(lm, oracle, loss_key):
    g, _ = _graph("small+outliers")
    run = _run(lm, "small+outliers", loss_key)
    ref0 = _terms_at(oracle, g, loss_key, pack(g.camera, g.cap, g.tag))
    _check_accepted_steps(oracle, g, run, loss_key, ref0)


def _inlier_rms(oracle, g, bad, run):
    """RMS per corner (px) of the plain residuals over the observations that were not shifted."""
    keep = np.setdiff1d(np.arange(g.n_obs), bad)
    ss = 0.0
    for o in keep:
        r = oracle.residual(run["camera"], run["cap"][g.obs_cap[o]], run["tag"][g.obs_tag[o]], g.corners[o])
        ss += float(r @ r)
    return np.sqrt(ss / (4.0 * len(keep)))


def test_loss_rejects_the_outliers(lm, oracle):
    g, bad = _graph("small+outliers")
    clean, _ = _graph("small")
    assert len(bad) == 20
    runs = {k: _run(lm, "small+outliers", k) for k in (None, "huber", "cauchy")}
    runs["clean"] = _run(lm, "small", None)
    for k, r in runs.items():
        s = r["s"]
        print(f"{k}: {s['termination']} after {len(s['iterations'])} iterations, f = {r['camera'][0]:.4f}")
        assert s["termination"] == "CONVERGENCE" and len(s["iterations"]) <= 51
    R = {k: _inlier_rms(oracle, clean if k == "clean" else g, np.zeros(0, int) if k == "clean" else bad, r)
         for k, r in runs.items()}
    print("inlier RMS per corner (px):", R)
    assert R["cauchy"] <= 1.25 * R["clean"]
    assert R["huber"] <= 0.5 * R[None]
    assert abs(runs["cauchy"]["camera"][0] - 900.0) <= 5.0


def test_chunked_captures_with_mixed_losses(lm, oracle):
    """kvar's captures see 8 to 80 tags (the kChunked instances, k_schur's big-capture launch), every
    observation with its own kind and scale: an observation order permuted on the host would show
    as a wrong iteration-0 cost."""
    g, _ = _graph("kvar+outliers")
    k = np.bincount(g.obs_cap)
    assert k.min() <= 8 and k.max() >= 80
    run = _run(lm, "kvar+outliers", "mixed")
    ref0 = _check_iteration0(oracle, g, run, "mixed")
    _check_accepted_steps(oracle, g, run, "mixed", ref0)


def _compare_sides(g, ours, ref):
    """(test_gpu_elimination._compare's tolerances)"""
    s_o, s_r = ours["s"], ref["s"]
    assert (s_o["termination"], s_o["rule"]) == (s_r["termination"], s_r["rule"])
    assert abs(len(s_o["iterations"]) - len(s_r["iterations"])) <= 1
    for a, b in list(zip([i["cost"] for i in s_o["iterations"]], [i["cost"] for i in s_r["iterations"]]))[:5]:
        assert abs(a - b) <= 1e-9 * abs(b)
    assert abs(s_o["final_cost"] - s_r["final_cost"]) <= 1e-8 * s_r["final_cost"]
    assert abs(ours["camera"][0] - ref["camera"][0]) <= 1e-8 * ref["camera"][0]
    assert_poses_match(ours["cap"], ours["tag"], ref["cap"], ref["tag"], tags=np.unique(g.obs_tag),
                       caps=np.unique(g.obs_cap))


@pytest.mark.parametrize("side", ["tags", "mixed"])
def test_elimination_sides_agree_under_a_loss(lm, side):
    """small's Ceres set mixes captures and tags (test_mixed_set_matches_oracle)."""
    g, _ = _graph("small+outliers")
    elim = {"tags": lm.ELIM_TAGS, "mixed": lm.ELIM_MIXED}[side]
    ref = _run(lm, "small+outliers", "huber", record=False, elimination=lm.ELIM_CAPTURES)
    ours = _run(lm, "small+outliers", "huber", record=False, elimination=elim)
    assert ref["s"]["elimination_used"] == lm.ELIM_CAPTURES
    assert ours["s"]["elimination_used"] == elim
    _compare_sides(g, ours, ref)


def test_pointer_keyed_losses(lm, oracle):
    g, _ = _graph("small+outliers")
    nb = g.n_obs
    kinds = np.where(np.arange(nb) % 2 == 0, HUBER, CAUCHY).astype(np.uint8)
    scales = np.where(np.arange(nb) % 2 == 0, 3.0, 2.0)
    camera = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(g.n_cap)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    for b in range(nb):
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]],
                                loss=(int(kinds[b]), float(scales[b])))
    s = prob.solve()
    rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, obs_loss=(kinds, scales),
                            elimination=lm.ELIM_CAPTURES)
    s2 = rp.solve()
    assert s["termination"] == s2["termination"]
    assert abs(s["final_cost"] - s2["final_cost"]) <= 1e-9 * s2["final_cost"]
    assert abs(camera[0] - rp.camera[0]) <= 1e-8 * rp.camera[0]
    # two more captures (copies of captures 0 and 1, moved a little: known tags) with Huber(3)
    obs_cap, obs_tag, corners = list(g.obs_cap), list(g.obs_tag), [c for c in g.corners]
    kinds, scales = list(kinds), list(scales)
    for src in (0, 1):
        new = np.array(caps[src]) + np.array([0.01, -0.01, 0.01, 0.0, 0.0, 0.0])
        caps.append(new)
        for b in np.nonzero(g.obs_cap == src)[0]:
            prob.add_residual_block(g.corners[b], camera, new, tags[g.obs_tag[b]], loss=(HUBER, 3.0))
            obs_cap.append(len(caps) - 1)
            obs_tag.append(int(g.obs_tag[b]))
            corners.append(g.corners[b])
            kinds.append(HUBER)
            scales.append(3.0)
    arrays = (camera.copy(), np.stack(caps).copy(), np.stack(tags).copy(), np.array(obs_cap), np.array(obs_tag),
              np.stack(corners))
    ref = robust_terms(oracle, arrays, np.array(kinds), np.array(scales)).cost
    s3 = prob.solve()
    print(f"grown problem: setup_kind {s3['setup_kind']} initial_cost {s3['initial_cost']:.17g} numpy {ref:.17g}")
    assert s3["n_obs"] == len(obs_cap)
    assert abs(s3["initial_cost"] - ref) <= 1e-12 * ref
    # (copies of captures 0 and 1 couple only tags already coupled: the appended-problem path ran)
    assert s3["setup_kind"] == lm.SETUP_APPEND, s3["setup_kind"]
    # the same blocks from moved values: the values-only path, the resident losses
    camera[0] *= 1.01
    for c in caps:
        c[:3] += 0.005
    arrays = (camera.copy(), np.stack(caps).copy(), np.stack(tags).copy()) + arrays[3:]
    ref = robust_terms(oracle, arrays, np.array(kinds), np.array(scales)).cost
    s3b = prob.solve()
    assert s3b["setup_kind"] == lm.SETUP_VALUES, s3b["setup_kind"]
    assert abs(s3b["initial_cost"] - ref) <= 1e-12 * ref
    # the same blocks again, all Cauchy(3): no loss array of the earlier problem survives
    start = (camera.copy(), np.stack(caps).copy(), np.stack(tags).copy())
    prob.reset()
    for b in range(len(obs_cap)):
        prob.add_residual_block(corners[b], camera, caps[obs_cap[b]], tags[obs_tag[b]], loss=(CAUCHY, 3.0))
    ref = robust_terms(oracle, start + (np.array(obs_cap), np.array(obs_tag), np.stack(corners)), CAUCHY, 3.0).cost
    s4 = prob.solve()
    print(f"re-added with Cauchy(3): setup_kind {s4['setup_kind']} initial_cost {s4['initial_cost']:.17g} numpy {ref:.17g}")
    assert abs(s4["initial_cost"] - ref) <= 1e-12 * ref
    # ... and with the default loss instead of a per-block one
    start = (camera.copy(), np.stack(caps).copy(), np.stack(tags).copy())
    prob.reset()
    prob.set_loss(SOFT_L_ONE, 3.0)
    for b in range(len(obs_cap)):
        prob.add_residual_block(corners[b], camera, caps[obs_cap[b]], tags[obs_tag[b]])
    ref = robust_terms(oracle, start + (np.array(obs_cap), np.array(obs_tag), np.stack(corners)), SOFT_L_ONE, 3.0).cost
    s5 = prob.solve()
    assert abs(s5["initial_cost"] - ref) <= 1e-12 * ref


# ---- two ranks on one GPU through the callback transport (as test_gpu_multirank.py) ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# medium splits over two ranks (108 and 92 captures); small, kvar and k24 leave rank 1 without captures
RANKS_GRAPH = "medium"


def _rank_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ar_slam_amd import lm
        g, _ = outliers(synth.config_graph(RANKS_GRAPH))

        def allreduce(a, op):
            dist.all_reduce(torch.from_numpy(a), op=dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.MAX)

        rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners,
                                comm=(rank, world, allreduce), device=0, obs_loss=_mixed_losses(g))
        s = rp.solve()
        own = rp.owned_captures()
        q.put((rank, rp.camera.copy(), own, rp.cap[own].copy(), rp.tag.copy(),
               [it["cost"] for it in s["iterations"]], s["termination"], s["rule"], s["final_cost"]))
    except Exception as e:   # noqa: BLE001 -- surface the failure in the parent
        q.put((rank, None, None, None, None, None, repr(e), None, None))
    finally:
        dist.destroy_process_group()


def test_two_ranks_carry_the_loss(lm, oracle):
    """Every observation has its own kind and scale and both ranks own captures, so a rank that took
    another observation's loss (unfiltered, or indexed by the whole problem's observation) or none
    shows in the cost from iteration 0 on."""
    pytest.importorskip("torch")
    import multiprocessing as mp
    g, _ = _graph(RANKS_GRAPH + "+outliers")
    one = _run(lm, RANKS_GRAPH + "+outliers", "mixed", record=False, elimination=lm.ELIM_CAPTURES)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    res.sort(key=lambda t: t[0])
    for r in res:
        assert r[1] is not None, r[6]
    assert res[0][5] == res[1][5]
    np.testing.assert_array_equal(res[0][1], res[1][1])
    rank, cam, _, _, tag, costs, term, rule, final = res[0]
    s1 = one["s"]
    assert (term, rule) == (s1["termination"], s1["rule"])
    costs1 = [it["cost"] for it in s1["iterations"]]
    assert abs(len(costs) - len(costs1)) <= 1
    for a, b in list(zip(costs, costs1))[:5]:
        assert abs(a - b) <= 1e-9 * abs(b)
    assert abs(final - s1["final_cost"]) <= 1e-8 * s1["final_cost"]
    assert abs(cam[0] - one["camera"][0]) <= 1e-8 * one["camera"][0]
    # iteration 0 against numpy, too: the cost of every rank's observations under their own losses
    ref0 = _terms_at(oracle, g, "mixed", pack(g.camera, g.cap, g.tag)).cost
    print(f"two ranks: iteration 0 cost {costs[0]:.17g} numpy {ref0:.17g}; captures per rank "
          f"{[len(r[2]) for r in res]}")
    assert abs(costs[0] - ref0) <= 1e-12 * ref0
    # the problem really is split: every rank owns captures, every capture is owned exactly once
    cap = np.full((g.n_cap, 6), np.nan)
    seen = np.zeros(g.n_cap, int)
    for r in res:
        assert len(r[2]) > 0, "a rank without captures: the losses' per-rank split is not exercised"
        cap[r[2]] = r[3]
        seen[r[2]] += 1
    assert np.all(seen == 1), "every capture is owned by exactly one rank"
    assert_poses_match(cap, tag, one["cap"], one["tag"], tags=np.unique(g.obs_tag))


# ---- the ArSlamSolver mirror ----
def _slam(lm, g, corners, loss=None):
    s = lm.SlamSolver()
    s.set_camera(g.camera)
    if loss is not None:
        s.set_loss(*loss)
    for c in range(g.n_cap):
        sel = g.obs_cap == c
        s.add_detections(f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], corners[sel])
    s.solve()
    return s


def test_slam_mirror_set_loss(lm, oracle):
    g = synth.config_graph("cfg1")
    plain = _slam(lm, g, g.corners)
    never = _slam(lm, g, g.corners, loss=(lm.LOSS_HUBER, 1e6))
    np.testing.assert_allclose(never.capture_poses(), plain.capture_poses(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(never.aruco_poses(), plain.aruco_poses(), rtol=0, atol=1e-9)
    # one misread detection, Huber(3): the last solve's cost is the robust cost of the mirror's blocks
    corners = np.array(g.corners, np.float64).copy()
    corners[5] += np.tile([40.0 * np.cos(0.7), 40.0 * np.sin(0.7)], 4)
    s = _slam(lm, g, corners, loss=(lm.LOSS_HUBER, 3.0))
    blocks = [s.block(b) for b in range(s.num_blocks)]
    assert all(b[3] for b in blocks) and len(blocks) == g.n_obs
    arrays = (s.camera()[0], s.capture_poses(), s.aruco_poses(), np.array([b[0] for b in blocks]),
              np.array([b[1] for b in blocks]), np.stack([b[2] for b in blocks]))
    ref = robust_terms(oracle, arrays, HUBER, 3.0)
    last = s.last_summary()
    print(f"mirror: final_cost {last['final_cost']:.17g} numpy {ref.cost:.17g}; largest s {ref.s.max():.1f}")
    assert ref.s.max() > 9.0   # (the loss bites: an observation past Huber's threshold)
    assert abs(last["final_cost"] - ref.cost) <= 1e-9 * ref.cost
    with pytest.raises(lm.LMError) as e:
        s.set_loss(7, 1.0)
    assert e.value.code == -1
