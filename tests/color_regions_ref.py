"""Test-side restatement of the region-wise colour transfer (nerfstyle_amd/color_match.py, csrc/color_regions.hip), written from
the definitions in include/nsr.h, on top of color_match_ref.py:

region_of:       explicit integer labels: l when 0 <= l < K, else K.  Float labels (the fourth float of a row): k when the value
                 equals the integer k exactly, 0 <= k < K (-0.0 is 0); negative, >= K, fractional, NaN and inf -> K.
region_moments:  [K+1, 10] fp64: count and color_match_ref.moments of every region's rows; an empty region is ten zeros.
solve_regions:   color_match_ref.solve per matched (class, cluster) pair with at least min_rows rows on both sides; the fallback
                 (all rows against all rows, or the identity) for every other class and for slot Kc.
apply_regions:   color_match_ref.apply per region."""
import numpy as np

import color_match_ref as R

F32, F64 = np.float32, np.float64


def region_of(labels, K):
    """labels [n] integer or floating -> [n] int64 in 0..K"""
    l = np.asarray(labels)
    if np.issubdtype(l.dtype, np.floating):
        with np.errstate(invalid='ignore'):
            ok = (l >= 0) & (l < K) & (np.floor(l) == l)              # all False for NaN; inf fails l < K
        return np.where(ok, np.where(ok, l, 0).astype(np.int64), K)
    l = l.astype(np.int64)
    return np.where((l >= 0) & (l < K), l, K)


def region_moments(rows, regions, K):
    """rows [n, >=3], regions [n] in 0..K (region_of) -> [K+1, 10] fp64"""
    rows = np.asarray(rows)
    out = np.zeros((K + 1, 10), F64)
    for k in range(K + 1):
        sel = regions == k
        out[k, 0] = sel.sum()
        if out[k, 0]:
            out[k, 1:] = R.moments(rows[sel])
    return out


def region_scale(rows, regions, K):
    """[K+1, 10] fp64: sum of |term| per entry (the count's is the count)"""
    return region_moments(np.abs(np.asarray(rows)[:, :3].astype(F64)), regions, K)


def solve_regions(content_m, style_m, matching, min_rows=256, fallback='global'):
    """[Kc+1, 10], [Ks+1, 10], matching [Kc] -> [Kc+1, 4, 4] float32"""
    content_m, style_m = np.asarray(content_m, F64), np.asarray(style_m, F64)
    Kc, Ks = content_m.shape[0] - 1, style_m.shape[0] - 1
    assert len(matching) == Kc and fallback in ('global', 'identity')
    base = np.eye(4, dtype=F32)
    if fallback == 'global':
        tc, ts = content_m.sum(0), style_m.sum(0)
        base = R.solve(tc[1:], tc[0], ts[1:], ts[0])
    tfs = np.repeat(base[None], Kc + 1, 0)
    for i, j in enumerate(matching):
        if 0 <= j < Ks and content_m[i, 0] >= max(1, min_rows) and style_m[j, 0] >= max(1, min_rows):
            tfs[i] = R.solve(content_m[i, 1:], content_m[i, 0], style_m[j, 1:], style_m[j, 0])
    return tfs


def apply_regions(rows, regions, tfs, clamp=True):
    """rows [n, 3 or 4] f32 -> the rows, each mapped by tfs[its region]; a fourth column is carried over"""
    rows = np.asarray(rows, F32)
    out = rows.copy()
    for k in range(len(tfs)):
        sel = regions == k
        if sel.any():
            out[sel] = R.apply(rows[sel], tfs[k], clamp)
    return out


def apply_bound(rows, regions, tfs):
    """[n, 3] fp64: color_match_ref.apply_bound of every row under its own region's transform"""
    rows = np.asarray(rows)
    out = np.zeros((rows.shape[0], 3), F64)
    for k in range(len(tfs)):
        sel = regions == k
        if sel.any():
            out[sel] = R.apply_bound(rows[sel], tfs[k])
    return out


def match_by_region(content_rows, content_regions, Kc, style_rows, style_regions, Ks, matching, min_rows=256, fallback='global',
                    clamp=True):
    """-> (rows' f32, tfs [Kc+1,4,4] f32): the whole restatement"""
    tfs = solve_regions(region_moments(content_rows, content_regions, Kc), region_moments(style_rows, style_regions, Ks), matching,
                        min_rows, fallback)
    return apply_regions(content_rows, content_regions, tfs, clamp), tfs
