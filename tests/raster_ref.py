"""seq.kmer.raster restated in numpy (include/kmhgpu.h has the definition): the rows (i, j) of a
frame (i_lo, j_lo, bin_i, bin_j, n_i, n_j) counted per cell with np.add.at, nothing else.  The
tests' reference; its rows are crafted or the clean-room oracle's, never the code under test's."""
import numpy as np


def raster(rows, frame) -> np.ndarray:
    """int64 (n_i, n_j): M[bi, bj] = #{(i, j) : i >= i_lo, (i - i_lo) // bin_i == bi < n_i,
    j >= j_lo, (j - j_lo) // bin_j == bj < n_j}."""
    i_lo, j_lo, bin_i, bin_j, n_i, n_j = (int(x) for x in frame)
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    i, j = rows[:, 0], rows[:, 1]
    keep = (i >= i_lo) & (j >= j_lo)
    bi = (i[keep] - i_lo) // bin_i
    bj = (j[keep] - j_lo) // bin_j
    inside = (bi < n_i) & (bj < n_j)
    m = np.zeros((n_i, n_j), np.int64)
    np.add.at(m, (bi[inside], bj[inside]), 1)
    return m


def in_frame(rows, frame) -> int:
    """The rows inside the frame."""
    i_lo, j_lo, bin_i, bin_j, n_i, n_j = (int(x) for x in frame)
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    i, j = rows[:, 0], rows[:, 1]
    return int(((i >= i_lo) & (i < i_lo + n_i * bin_i) & (j >= j_lo) & (j < j_lo + n_j * bin_j)).sum())


def coarsen(m, fi: int, fj: int) -> np.ndarray:
    """Cells summed in groups of fi x fj (the last group of an axis may be short): the matrix of
    the same frame origin at bin widths fi and fj times as wide."""
    n_i, n_j = m.shape
    pi, pj = -(-n_i // fi) * fi, -(-n_j // fj) * fj
    p = np.zeros((pi, pj), np.int64)
    p[:n_i, :n_j] = m
    return p.reshape(pi // fi, fi, pj // fj, fj).sum(axis=(1, 3))


def window_counts(n: int, lo: int, width: int, bins: int) -> np.ndarray:
    """How many of the coordinates 1..n fall into each of `bins` bins of `width` from lo."""
    edges = lo + width * np.arange(bins + 1, dtype=np.int64)
    return np.clip(np.minimum(edges[1:], n + 1) - np.maximum(edges[:-1], 1), 0, None)
