"""The elimination-order memory (csrc/host_layout.cpp OrderMemory) on the CPU, through
arslam_debug_order_memory: a sequence of problems passed through one memory as a first load and
then pointer-keyed reloads.  Each case derives what must happen from the rules as the struct
states them:
  * graph_outgrown: 10 * directed edges > 11 * the edges the order was computed at;
  * groups_outgrown: 4 * groups > 5 * the groups the order was computed at;
  * kHeightSlack: a kept order whose tile tree is more than one level taller than remembered is
    replaced by a fresh one;
  * a kept order needs the same free blocks (by index), or maps rows by original block (a mixed set
    after a mixed set); new blocks go after every kept row, before the camera's rows.
The graphs are a chain of 40 tags on a line, capture c seeing tags c and c + 1 (39 captures, 78
directed edges), grown in different ways; the layout ignores the corners.

What a fresh order is compared with: a reload's fresh nested dissection takes the faster separator
search (LayoutRequest::fast_order, as every order computed for a grown pointer-keyed problem does),
the one-off layout of debug_reduced_plan the full one, and the two may cut differently.  So the
one-off layout is the reference under reverse Cuthill-McKee, which has one search, and under nested
dissection the reference is the same problem reloaded with nothing remembered (fresh_reload)."""
import numpy as np
import pytest

from ar_slam_amd import lm, synth

NT = 40


def chain(extra=(), n_tag=NT, tag_const=None):
    """The chain plus one capture per pair in `extra`."""
    pairs = [(c, c + 1) for c in range(NT - 1)] + list(extra)
    tag = np.zeros((n_tag, 6))
    tag[:, 0] = 0.2 * np.arange(n_tag)
    return dict(camera=np.array([600.0, 0.0, 0.0]), cap=np.zeros((len(pairs), 6)), tag=tag,
                obs_cap=np.repeat(np.arange(len(pairs)), 2), obs_tag=np.array(pairs).reshape(-1),
                tag_const=tag_const)


def directed_edges(q):
    """Directed co-visibility edges among the free tags, as ReducedLayout::n_edges counts them."""
    free = np.ones(len(q["tag"]), bool) if q["tag_const"] is None else ~np.asarray(q["tag_const"], bool)
    e = set()
    for c in range(len(q["cap"])):
        ts = q["obs_tag"][q["obs_cap"] == c]
        e |= {(a, b) for a in ts for b in ts if a != b and free[a] and free[b]}
    return len(e)


RCM, ND = 1, 2


def fresh_rows(q, ordering):
    """The rows of a fresh order of q as a reload computes it, from outside the memory under test."""
    if ordering == ND:   # a reload with nothing remembered
        return lm.debug_order_memory([q, q], ordering=ND, forget_before=[0, 1])[1]["tag_row"]
    return lm.debug_reduced_plan(q["camera"], q["cap"], q["tag"], q["obs_cap"], q["obs_tag"],
                                 np.zeros((len(q["obs_cap"]), 8)), tag_const=q["tag_const"], ordering=ordering)[1]


def within_limits(a, b):
    """b against the order computed at a: neither the graph nor the groups outgrown."""
    return 10 * directed_edges(b) <= 11 * directed_edges(a) and 4 * len(b["cap"]) <= 5 * len(a["cap"])


def not_too_tall(s0, s1):
    return s1["etree_height"] <= s0["etree_height"] + 1


def test_same_problem_twice_is_reused():
    s = lm.debug_order_memory([chain(), chain()])
    assert (s[0]["order_reused"], s[1]["order_reused"]) == (0, 1)
    assert np.array_equal(s[0]["tag_row"], s[1]["tag_row"])
    one_off = lm.debug_reduced_plan(**{k: chain()[k] for k in ("camera", "cap", "tag", "obs_cap", "obs_tag")},
                                    corners=np.zeros((2 * (NT - 1), 8)))[1]
    assert np.array_equal(s[0]["tag_row"], one_off)   # (a first load: the full search, as the one-off layout)


def test_small_growth_keeps_every_row():
    # 9 more captures (39 -> 48: 4 * 48 <= 5 * 39), three of them new pairs (78 -> 84 edges: 840 <= 858)
    a, b = chain(), chain([(5, 6)] * 6 + [(0, 2), (10, 12), (20, 22)])
    assert len(b["cap"]) == 48 and directed_edges(a) == 78 and directed_edges(b) == 84 and within_limits(a, b)
    s = lm.debug_order_memory([a, b])
    assert not_too_tall(s[0], s[1])
    assert s[1]["order_reused"] == 1 and s[1]["recomputed"] == 0
    assert np.array_equal(s[0]["tag_row"], s[1]["tag_row"])


@pytest.mark.parametrize("ordering", [RCM, ND])
def test_a_quarter_more_groups_is_fresh(ordering):
    b = chain([(5, 6)] * 10)   # 49 captures: 4 * 49 = 196 > 195, no new edge
    assert directed_edges(b) == 78 and not within_limits(chain(), b)
    s = lm.debug_order_memory([chain(), b], ordering=ordering)
    assert s[1]["order_reused"] == 0 and s[1]["recomputed"] == 0
    assert np.array_equal(s[1]["tag_row"], fresh_rows(b, ordering))


@pytest.mark.parametrize("ordering", [RCM, ND])
def test_a_tenth_more_edges_is_fresh(ordering):
    b = chain([(i, i + 20) for i in range(4)])   # 43 captures (172 <= 195), 86 edges: 860 > 858
    assert 4 * len(b["cap"]) <= 5 * 39 and directed_edges(b) == 86 and not within_limits(chain(), b)
    s = lm.debug_order_memory([chain(), b], ordering=ordering)
    assert s[1]["order_reused"] == 0 and s[1]["recomputed"] == 0
    assert np.array_equal(s[1]["tag_row"], fresh_rows(b, ordering))


@pytest.mark.parametrize("ordering", [RCM, ND])
def test_a_changed_free_set_is_fresh(ordering):
    const = np.zeros(NT, np.uint8)
    const[7] = 1
    b = chain(tag_const=const)
    s = lm.debug_order_memory([chain(), b], ordering=ordering)
    assert s[1]["order_reused"] == 0
    assert s[1]["tag_row"][7] == -1
    assert np.array_equal(s[1]["tag_row"], fresh_rows(b, ordering))


def test_a_new_tag_goes_after_the_kept_rows():
    a, b = chain(), chain([(NT - 1, NT)], n_tag=NT + 1)   # one capture and one tag more, 80 edges
    assert within_limits(a, b)
    s = lm.debug_order_memory([a, b])
    assert not_too_tall(s[0], s[1])
    assert s[1]["order_reused"] == 1
    assert np.array_equal(s[1]["tag_row"][:NT], s[0]["tag_row"])
    assert s[1]["tag_row"][NT] == s[0]["tag_row"].max() + 6
    cam_row = 6 * (NT + 1) + s[1]["pad_rows"]   # the tag rows and their padding, then the camera
    assert s[1]["tag_row"][NT] + 6 <= cam_row


def test_a_kept_order_that_grew_too_tall_is_recomputed():
    """One capture coupling the two halves of the dissected chain: within both growth limits, so the
    order would be kept, but the tiles of the two halves then lie on one elimination path -- more
    than a level taller than the remembered tree."""
    a, b = chain(), chain([(2, NT - 3)])
    assert within_limits(a, b)
    s = lm.debug_order_memory([a, b])
    assert s[1]["recomputed"] == 1 and s[1]["order_reused"] == 0
    assert np.array_equal(s[1]["tag_row"], fresh_rows(b, ND))
    # the kept order's height is not reported; the fresh one's is what a first load gives
    assert s[1]["etree_height"] == lm.debug_order_memory([b])[0]["etree_height"]


def cfg2_prefix(g, k):
    """g's first k captures with g's own tag numbering (a tag no capture sees yet is not a parameter)."""
    sel = g.obs_cap < k
    return dict(camera=g.camera, cap=g.cap[:k], tag=g.tag, obs_cap=g.obs_cap[sel], obs_tag=g.obs_tag[sel])


def test_mixed_after_mixed_keeps_rows_by_block():
    """cfg2's first 229 and 230 captures, both past the point where Ceres' set mixes captures and
    tags.  The set re-chosen for one capture more moves a few blocks across (one leaves the reduced
    side, three join it): a handful of groups and edges against some 230 groups and thousands of
    edges, far inside both growth limits, so the order is kept and the rows are mapped by block."""
    g = synth.config_graph("cfg2")
    s = lm.debug_order_memory([cfg2_prefix(g, 229), cfg2_prefix(g, 230)], elimination=lm.ELIM_MIXED)
    assert s[0]["side"] == s[1]["side"] == lm.ELIM_MIXED
    assert not_too_tall(s[0], s[1])
    assert s[1]["order_reused"] == 1
    old = np.concatenate([s[0]["tag_row"], s[0]["cap_row"], [-1]])   # (capture 229 is new)
    new = np.concatenate([s[1]["tag_row"], s[1]["cap_row"]])
    both = (old >= 0) & (new >= 0)
    assert both.sum() > 100 and np.array_equal(old[both], new[both])
    left = (old >= 0) & (new < 0)
    joined = (old < 0) & (new >= 0)
    assert left.sum() >= 1 and joined.sum() >= 1
    assert s[1]["pad_rows"] == s[0]["pad_rows"] + 6 * left.sum()
    assert np.all(new[joined] > old[both].max())
    assert len(set(new[new >= 0])) == (new >= 0).sum()


def test_forget_makes_the_next_load_fresh():
    s = lm.debug_order_memory([chain(), chain()], forget_before=[0, 1])
    assert s[1]["order_reused"] == 0 and s[1]["recomputed"] == 0
    assert np.array_equal(s[0]["tag_row"], s[1]["tag_row"])
