"""The kNN yardstick (tests/knn_reference.py) against cases known in closed form: what the GPU test compares bit for bit must itself
be the definition of include/gsr_knn.h."""
import numpy as np

from knn_reference import knn_reference


def lattice(n=8, pitch=0.25):
    """n^3 points, x fastest: index = x + n y + n^2 z.  pitch 0.25 and its multiples are exact in float32."""
    g = np.arange(n, dtype=np.float32) * np.float32(pitch)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def test_lattice_is_exact_and_ties_go_to_the_lower_index():
    p = lattice()
    mean, idx = knn_reference(p, want_indices=True)
    assert mean.dtype == np.float32 and idx.dtype == np.int32
    assert (mean == np.float32(0.0625)).all()                  # every point has at least three neighbours at one pitch
    assert idx[0].tolist() == [1, 8, 64]
    assert idx[1].tolist() == [0, 2, 9]                        # x-1, x+1, y+1: four candidates at 0.0625, the lowest three indices
    assert idx[511].tolist() == [511 - 64, 511 - 8, 511 - 1]
    mean_only, none = knn_reference(p)
    assert none is None and mean_only.tobytes() == mean.tobytes()


def test_identical_points_are_neighbours_at_distance_zero():
    p = np.full((300, 3), 0.37, np.float32)
    mean, idx = knn_reference(p, want_indices=True)
    assert (mean == 0).all()
    assert idx[0].tolist() == [1, 2, 3] and idx[1].tolist() == [0, 2, 3] and idx[2].tolist() == [0, 1, 3] and idx[3].tolist() == [0, 1, 2]
    assert (idx[4:] == np.array([0, 1, 2])).all()


def test_fewer_than_three_neighbours():
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    mean, idx = knn_reference(one, want_indices=True)
    assert mean.tolist() == [0.0] and idx.tolist() == [[-1, -1, -1]]
    two = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], np.float32)
    mean, idx = knn_reference(two, want_indices=True)
    assert mean.tolist() == [9.0, 9.0]                         # the pair's d2, not a third of it
    assert idx.tolist() == [[1, -1, -1], [0, -1, -1]]
    three = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]], np.float32)
    mean, idx = knn_reference(three, want_indices=True)
    assert mean.tolist() == [5.0, 5.5, 9.5]                    # (1 + 9) / 2, (1 + 10) / 2, (9 + 10) / 2
    assert idx.tolist() == [[1, 2, -1], [0, 2, -1], [0, 1, -1]]


def test_float32_arithmetic_in_the_stated_order():
    # dx^2 + dy^2 = 2^24 exactly, + dz^2 = 1 is lost in float32; a float64 sum, or dz first, would keep it
    p = np.array([[0.0, 0.0, 0.0], [4096.0, 0.0, 1.0], [0.0, 4096.0, 1.0], [1e4, 1e4, 1e4], [-1e4, -1e4, -1e4]], np.float32)
    mean, _ = knn_reference(p)
    third = np.float32(3e8)
    assert mean[0] == (np.float32(2 ** 24) + np.float32(2 ** 24) + third) / np.float32(3)


def test_an_index_permutation_permutes_the_results():
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    mean, idx = knn_reference(p, want_indices=True, chunk=97)  # (a chunk size that does not divide N)
    perm = rng.permutation(len(p))
    mean_p, idx_p = knn_reference(p[perm], want_indices=True)
    assert mean_p.tobytes() == mean[perm].tobytes()
    # a random cloud has no ties (checked), so the neighbours are the same points: map the permuted run's indices back
    d = np.sort(((p[:, None, :] - p[None, :, :]).astype(np.float64) ** 2).sum(-1), axis=1)[:, 1:5]
    assert (np.diff(d, axis=1) > 0).all()
    assert (perm[idx_p] == idx[perm]).all()
