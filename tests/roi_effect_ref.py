"""The yardstick of nm_roi_effect (own code, float64 / int64): per column of a table the pair counts of group X against
group Y, Cliff's delta, the ROC-AUC of the column as a patient score, the group sizes and means -- the columns of
metrics.ROI_EFFECT_COLUMNS, by the formulas of include/nmhip.h:

    n_more / n_less   pairs (i in X, j in Y) with x_i > y_j / x_i < y_j (a NaN compares false both ways: a tie)
    cliff_delta       (n_more - n_less) / (n_x n_y)              -- the integer difference, one float64 division
    auc               (2 n_more + ties) / (2 n_x n_y),  ties = n_x n_y - n_more - n_less
    mean_x / mean_y   np.mean of the group's rows (NaN propagates); an empty group: zero counts, NaN quotients and mean

Two forms of the counts: `counts_broadcast` compares every pair (n_x n_y D booleans at a time), `counts_sorted` looks every x up
in the sorted non-NaN y of its column (np.searchsorted, side left / right; a NaN x contributes nothing) for sizes where the
first does not fit.  `literal_delta` walks the pairs of one column one by one, as the reference's cliff_delta does (utils.py:97-109)."""
import numpy as np

COLUMNS = ("cliff_delta", "auc", "n_more", "n_less", "n_x", "n_y", "mean_x", "mean_y")


def split(x, group):
    x = np.asarray(x, dtype=np.float64)
    group = np.asarray(group)
    return x[group == 1], x[group == 0]


def counts_broadcast(X, Y):
    """(n_more, n_less) per column, int64, from every pair."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    more = (X[:, None, :] > Y[None, :, :]).sum((0, 1), dtype=np.int64)
    less = (X[:, None, :] < Y[None, :, :]).sum((0, 1), dtype=np.int64)
    return more, less


def counts_sorted(X, Y):
    """(n_more, n_less) per column, int64: y_j < x are the first searchsorted(.., 'left') of the sorted y, y_j > x the ones
    from searchsorted(.., 'right') on."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    D = X.shape[1]
    more, less = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    for c in range(D):
        ys = np.sort(Y[~np.isnan(Y[:, c]), c])
        xs = X[~np.isnan(X[:, c]), c]
        more[c] = np.searchsorted(ys, xs, side="left").sum(dtype=np.int64)
        less[c] = (len(ys) - np.searchsorted(ys, xs, side="right")).sum(dtype=np.int64)
    return more, less


def table(x, group, counts=counts_broadcast):
    """[D, 8] float64 in the order of COLUMNS for one set: x [rows, D], group [rows] (1 = X, 0 = Y, else left out)."""
    X, Y = split(x, group)
    nx, ny = X.shape[0], Y.shape[0]
    D = X.shape[1]
    more, less = counts(X, Y) if nx and ny else (np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64))
    pairs = np.int64(nx) * np.int64(ny)
    ties = pairs - more - less
    out = np.full((D, len(COLUMNS)), np.nan)
    if pairs:
        out[:, 0] = (more - less).astype(np.float64) / np.float64(pairs)
        out[:, 1] = (2 * more + ties).astype(np.float64) / np.float64(2 * pairs)
    out[:, 2], out[:, 3], out[:, 4], out[:, 5] = more, less, nx, ny
    with np.errstate(invalid="ignore"):
        if nx:
            out[:, 6] = X.mean(0)
        if ny:
            out[:, 7] = Y.mean(0)
    return out


def literal_delta(X, Y):
    """Cliff's delta pair by pair on 1-D X and Y, as the reference's double loop forms it: +1 for x > y, -1 for y > x, the
    sum over the number of pairs."""
    total = 0
    for xi in X:
        for yj in Y:
            if xi > yj:
                total += 1
            elif yj > xi:
                total -= 1
    return np.float64(total) / np.float64(len(X) * len(Y))
