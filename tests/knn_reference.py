"""The float32 yardstick of include/gsr_knn.h: a chunked numpy brute force of exactly the header's definition.

    d2(i, j) = (dx * dx + dy * dy) + dz * dz in float32, in that order (numpy contracts nothing), for every j != i;
    candidates ordered by (d2, j); k = min(3, N - 1); nn_index = the first k of them, then -1;
    mean_dist2 = ((d2_0 + d2_1) + d2_2) / 3 in float32, over k terms and divided by k when k < 3, 0 when N = 1.

The value path takes the k smallest distances with np.partition (ties have equal values, so which of them it picks does not matter);
the index path keeps every candidate at or below the k-th smallest distance of its row and orders those few by (d2, j)."""
import numpy as np

K = 3


def _d2_rows(p, a, b):
    """d2 of the queries a .. b-1 against every point, (b - a, N) float32, the query itself at +inf."""
    q = p[a:b]
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    d[np.arange(b - a), np.arange(a, b)] = np.inf
    return d


def _mean(best, k):
    """best (M, k) float32 ascending -> the mean as the header sums and divides it."""
    s = best[:, 0]
    for c in range(1, k):
        s = s + best[:, c]
    return (s / np.float32(k)).astype(np.float32)


def knn_reference(points, want_indices=False, chunk=None):
    """(mean_dist2 (N,) float32, nn_index (N, 3) int32 or None) of an (N, 3) cloud."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    k = min(K, n - 1)
    mean = np.zeros(n, np.float32)
    idx = np.full((n, K), -1, np.int32) if want_indices else None
    if k == 0:
        return mean, idx
    chunk = chunk or max(1, min(n, (1 << 23) // n))          # about 8 M distances at a time
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        d = _d2_rows(p, a, b)
        best = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
        mean[a:b] = _mean(best, k)
        if want_indices:
            rows, cols = np.nonzero(d <= best[:, k - 1:k])    # every candidate that can be among the first k, ties included
            order = np.lexsort((cols, d[rows, cols], rows))   # by row, then (d2, j)
            rows, cols = rows[order], cols[order]
            first = np.searchsorted(rows, np.arange(b - a))
            for c in range(k):
                idx[a:b, c] = cols[first + c]
    return mean, idx
