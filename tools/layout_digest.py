"""Digest of everything the host structure code derives, one line per case, to compare two
libraries (ARSLAM_LIB selects one; nothing is built): per synth config x ordering x skip-zero-tiles
the sha256 of tag_row and every field of arslam_plan_info (debug_reduced_plan); the plan under
capture, tag and mixed elimination (debug_reduced_plan_side); the extended gather plan of medium at
two cuts; the rank split of cfg3 at 2, 4 and 8 ranks.  usage: layout_digest.py > listing.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ar_slam_amd import lm, synth  # noqa: E402

NAMES = ("tiny", "small", "medium", "wide", "kvar", "k24", "wall", "cfg1", "cfg2", "cfg3")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def fields(d):
    return " ".join(f"{k}={d[k]!r}" for k in d)


for name in NAMES:
    g = synth.config_graph(name)
    for ordering in (0, 1, 2):
        for skip in (0, 1):
            info, tag_row = lm.debug_reduced_plan(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners,
                                                  ordering=ordering, skip_zero_tiles=skip)
            print(f"plan {name} ordering={ordering} skip={skip} tag_row={sha(tag_row)} {fields(info)}", flush=True)
    for elim in (lm.ELIM_CAPTURES, lm.ELIM_TAGS, lm.ELIM_MIXED):
        try:
            side, info = lm.debug_reduced_plan_side(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, elim)
            print(f"side {name} elimination={elim} side={side} {fields(info)}", flush=True)
        except lm.LMError as e:   # (a side that does not fit one wave's local system)
            print(f"side {name} elimination={elim} error {e}", flush=True)
g = synth.config_graph("medium")
for c0 in (g.n_cap // 2, g.n_cap - 1):
    print(f"gather_extend medium c0={c0}",
          lm.debug_gather_extend(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, c0), flush=True)
g = synth.config_graph("cfg3")
for nranks in (2, 4, 8):
    for rank in range(nranks):
        info, owner = lm.debug_rank_split(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, nranks, rank)
        print(f"rank_split cfg3 nranks={nranks} rank={rank} cap_owner={sha(owner)} {fields(info)}", flush=True)
