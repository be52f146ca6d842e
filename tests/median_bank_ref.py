"""numpy restatement of the width-bank median (include/eat_median_bank.h): `detect_ref.median_ref` row by row, one width per
(slice, class).  Nothing here shares code with the package."""
import numpy as np

from tests.detect_ref import median_ref


def median_bank_ref(x, rec, widths):
    """x (K, G_total), rec rows (first, count, goff, G), widths (Mw, K) or (K,) odd integers -> (Mw, K, G_total) in the dtype
    of x: out[j, k] = row k of `median_ref(x, rec, widths[j, k])`, the running median of x[k] of that width per recording
    with periodic reflection.  median_ref treats the rows independently, so it runs once per distinct width on the rows that
    use it and its rows are dealt out."""
    x = np.asarray(x)
    widths = np.atleast_2d(np.asarray(widths))
    assert widths.shape[1] == x.shape[0]
    out = np.empty((widths.shape[0],) + x.shape, dtype=x.dtype)
    for m in np.unique(widths).tolist():
        rows = np.flatnonzero((widths == m).any(axis=0))
        filtered = median_ref(x[rows], rec, int(m))
        for j in range(widths.shape[0]):
            use = widths[j, rows] == m
            out[j, rows[use]] = filtered[use]
    return out
