"""k_schur's output-stage descriptor table (schur_store_table.h), read through
arslam_debug_schur_store_table: for every nblk the stored slots write each element of the capture's
block-packed slab exactly once, at the offset schur_block_off gives its (row, column).  No GPU."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


# the 16x16 tiles (r, cc) of the output product in the kernel's order: cc <= r + 1
TILES = [(r, cc) for r in range(4) for cc in range(4) if cc <= r + 1]


def blk(x, m):
    return 0 if x == 0 else (1 + (m - 1) // 6 if x == m else 1 + (x - 1) // 6)


def blk_size(U, nblk):
    return 1 if U in (0, nblk + 1) else 6


def blk_start(U, nblk):
    return 0 if U == 0 else (1 + 6 * (U - 1) if U <= nblk else 1 + 6 * nblk)


def block_off(U, V, nblk):
    """host_structure.h schur_block_off: the row blocks before U, then the blocks (U, V' < V)."""
    R = 0 if U == 0 else 1 + 6 * (U - 1) + 18 * U * (U - 1)
    return R + blk_size(U, nblk) * blk_start(V, nblk)


def slab_size(nblk):
    return 3 + 12 * nblk + 18 * nblk * (nblk + 1)


def test_tile_order():
    assert len(TILES) == 13 and TILES[:5] == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]


@pytest.mark.parametrize("nblk", range(1, 11))
def test_store_table_covers_slab_once(L, nblk):
    off, stored = L.debug_schur_store_table(nblk)
    assert off.shape == stored.shape == (13, 64, 4)
    m = 1 + 6 * nblk
    M = m + 1
    offs = off[stored != 0]
    assert offs.size == slab_size(nblk) == 3 + 12 * nblk + 18 * nblk * (nblk + 1)
    assert np.array_equal(np.sort(offs), np.arange(slab_size(nblk)))
    n = 0
    for t, (r, cc) in enumerate(TILES):
        for lane in range(64):
            li, lk = lane & 15, lane >> 4
            for reg in range(4):
                p, q = 16 * r + lk + 4 * reg, 16 * cc + li
                U, V = blk(min(p, m), m), blk(min(q, m), m)
                want = p < M and q < M and V <= U      # the lower block triangle, rhs row included
                assert bool(stored[t, lane, reg]) == want, (nblk, t, lane, reg)
                if want:
                    sV = blk_size(V, nblk)
                    exp = block_off(U, V, nblk) + (p - blk_start(U, nblk)) * sV + (q - blk_start(V, nblk))
                    assert off[t, lane, reg] == exp, (nblk, p, q)
                    n += 1
    assert n == slab_size(nblk)


@pytest.mark.parametrize("nblk", [0, 11, -3])
def test_store_table_rejects_other_nblk(L, nblk):
    with pytest.raises(L.LMError):
        L.debug_schur_store_table(nblk)
