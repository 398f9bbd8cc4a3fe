"""Records tests/golden/bsolve_parent.npz with the library ARSLAM_LIB names (the build whose results
tests/test_gpu_bsolve_prefetch.py then requires bit for bit): dense seeded SPD systems solved by the
persistent executor (arslam_debug_dense_llt_ex, executor=1), whose backward solve k_bsolve_dag gives
column k of a dense T-tile matrix a gather list of T-1-k items.  The file holds the sizes, the seeds
and the y vectors only.
usage: ARSLAM_LIB=... python tools/make_bsolve_golden.py out.npz"""
import sys

import numpy as np

sys.path.insert(0, ".")

# n -> T = (n + 1 + 63) // 64 tiles (the rhs is row n): 63: no gather, rhs row in the column's own
# tile; 64: rhs row alone in the last tile, lists 0 and 1; 100: a partial tile; 200: lists 0..3
# (empty, prologue only, one swap, steady state); 321: both register sets reused, partial tile
SIZES = (63, 64, 100, 200, 321)
SEED0 = 20240


def system(n):
    """(seed, A, b): A = M M^T + n I from the seeded generator, b from the same stream.  M and b
    are small integers over a power of two, so M M^T is exact in float64 whatever order the host's
    BLAS sums in: the recording host and the testing host build the same bits of A."""
    seed = SEED0 + n
    rng = np.random.default_rng(seed)
    M = rng.integers(-16, 17, size=(n, n)).astype(np.float64) / 8.0
    A = M @ M.T + n * np.eye(n)
    b = rng.integers(-1024, 1025, size=n).astype(np.float64) / 64.0
    return seed, A, b


def solve(lm, n):
    _, A, b = system(n)
    _, y, info = lm.debug_dense_llt(A, b, executor=1)
    assert info == 0, (n, info)
    return y


def residual(A, y, b):
    """||A y - b||_inf / (||A||_inf ||y||_inf + ||b||_inf)"""
    return np.abs(A @ y - b).max() / (np.abs(A).sum(axis=1).max() * np.abs(y).max() + np.abs(b).max())


if __name__ == "__main__":
    from ar_slam_amd import lm
    out = {"sizes": np.array(SIZES, np.int64), "seeds": np.array([system(n)[0] for n in SIZES], np.int64)}
    for n in SIZES:
        _, A, b = system(n)
        out[f"y_{n}"] = solve(lm, n)
        print(n, "residual", residual(A, out[f"y_{n}"], b), "numpy", residual(A, np.linalg.solve(A, b), b))
    np.savez_compressed(sys.argv[1], **out)
    print(lm.library_info())
