"""Referee of the two scoring sub-commands, `similarity` (K8) and `findOutliers` (K9): plain numpy and Python, no import
of the engine (helper module, no tests in here).

- similarity_counts: include/sdice.h K8 on whole arrays (oracle_np.similarity_scores walks cell by cell);
- rowstats_rows / same_bits: np.nanmean, np.nanstd and the NaN count of every row as findOutliers.py:127-135 of the
  reference writes them, and the comparison that sees the sign of a zero;
- outlier_lines: findOutliers.py:120-152 line by line -> the text the reference prints;
- similarity_report: similarity.py:5-64 on Python floats of the text fields -> the report the reference writes.
"""
import warnings

import numpy as np


# ------------------------------------------------------------------------------ K8
def similarity_counts(ps, mid, sign):
    """-> (scores, counts) int64 [s]: over the rows with sign != 0, counts = non-NaN PS per column, scores = those below
    the row's midpoint where sign < 0, above it for any other non-zero sign"""
    ps, mid, sign = np.asarray(ps, np.float64), np.asarray(mid, np.float64), np.asarray(sign)
    counted = ~np.isnan(ps) & (sign != 0)[:, None]
    with np.errstate(invalid="ignore"):
        scored = np.where((sign < 0)[:, None], ps < mid[:, None], ps > mid[:, None]) & counted
    return scored.sum(axis=0, dtype=np.int64), counted.sum(axis=0, dtype=np.int64)


# ------------------------------------------------------------------------------ K9
def rowstats_rows(data, idx):
    """-> (mean, std in data.dtype, n_nan int32), one numpy call per 1-D row as the reference makes it"""
    data, idx = np.asarray(data), np.asarray(idx)
    mean, std = np.empty(len(data), data.dtype), np.empty(len(data), data.dtype)
    n_nan = np.empty(len(data), np.int32)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i, r in enumerate(data):
            vals = r[idx]
            mean[i], std[i], n_nan[i] = np.nanmean(vals), np.nanstd(vals), np.isnan(vals).sum()
    return mean, std, n_nan


def same_bits(got, want):
    """per cell: NaN where the reference has NaN (any payload), the reference's bit pattern everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise AssertionError(("dtype or shape", got.dtype, want.dtype, got.shape, want.shape))
    if got.dtype.kind != "f":
        return got == want
    word = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.where(np.isnan(want), np.isnan(got), got.view(word) == want.view(word))


# ------------------------------------------------------------------------------ findOutliers.py:120-152
def outlier_lines(matrix, cols, rows, samples, null, cutoff):
    """the reference's loop over the rows of `matrix` (any dtype numpy takes) -> the text it prints"""
    cols, rows = np.asarray(cols), np.asarray(rows)
    null_at = np.argwhere(np.isin(cols, null))[:, 0]
    sample_at = np.argwhere(np.isin(cols, samples))[:, 0]
    out = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for e, row in enumerate(matrix):
            null_vals = row[null_at]
            if np.sum(np.isnan(null_vals)) / len(null_vals) > 0.2:
                continue
            std = np.nanstd(null_vals)
            if std < 0.001:
                continue
            mean = np.nanmean(null_vals)
            vals = row[sample_at]
            z = (vals - mean) / std
            for pos, x in enumerate(z):
                if x >= cutoff and abs(x - mean) >= cutoff:
                    out.append("\t".join(str(v) for v in (rows[e], cols[sample_at[pos]], x, vals[pos], mean, std)) + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------ similarity.py:5-64
def similarity_report(comparison_path, allps_path, manifest_path=None):
    """-> (the report text, None), or (the lines written before it, the exception's type) where the reference raises"""
    midpoints, deltas = {}, {}
    with open(comparison_path) as table:
        table.readline()
        for line in table:
            row = line.rstrip().split("\t")
            if float(row[6]) > 0.05:
                continue
            delta = float(row[5])
            if delta == 0:
                continue
            midpoints[row[0]] = float(row[3]) - delta / 2
            deltas[row[0]] = delta
    with open(allps_path) as table:
        samples = table.readline().rstrip().split("\t")[1:]
        scores, counts = [0] * len(samples), [0] * len(samples)
        for line in table:
            row = line.rstrip().split("\t")
            delta = deltas.get(row[0])
            if delta is None or not (delta < 0 or delta > 0):
                continue
            for i, ps in enumerate(row[1:]):
                if ps != "nan":
                    counts[i] += 1
                    scores[i] += float(ps) < midpoints[row[0]] if delta < 0 else float(ps) > midpoints[row[0]]
    groups = None
    if manifest_path:
        groups = {}
        with open(manifest_path) as manifest:
            for line in manifest:
                name, _path, group1, group2 = line.rstrip().split("\t")
                groups[name] = (group1, group2)
    out = []
    try:
        for score, sample, count in sorted(zip(scores, samples, counts), reverse=True):
            if groups and sample in groups:
                out.append(f"{sample}\t{groups[sample][0]}\t{groups[sample][1]}\t{score / count:0.03f}\t{score}\t{count}\n")
            elif not groups:
                out.append(f"{sample}\t{score / count:0.03f}\t{score}\t{count}\n")
    except ZeroDivisionError as e:
        return "".join(out), type(e)
    return "".join(out), None
