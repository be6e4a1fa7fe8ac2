"""Test-side restatement of the colour transfer (nerfstyle_amd/color_match.py, csrc/color_match.hip), written from ARF's
definition, not from the reference code: with mu, C the mean and covariance of the content rows and mu_s, C_s those of the
style rows, x -> A x + b with A = C_s^(1/2) C^(-1/2) (symmetric square roots, eigenvalues clamped to [1e-8, 1e8]) and
b = mu_s - A mu.

moments:  the nine fp64 sums the kernel writes.
solve:    moments -> the [4,4] float32 transform, numpy fp64.
apply:    the kernel's f32 fma chain.  Each fmaf is emulated as an fp64 product (exact for two f32) plus an fp64 add, rounded to
          fp64 and then to f32: the sum is rounded twice where the hardware rounds once, so a result may differ from the kernel's
          by one f32 ulp of that step (apply_bound)."""
import numpy as np

F32, F64 = np.float32, np.float64


def moments(rows):
    """rows [n, >=3] (only the first three columns are read) -> [9] fp64: sum r, g, b, rr, rg, rb, gg, gb, bb"""
    x = np.asarray(rows)[:, :3].astype(F64)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    return np.array([r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(), (g * b).sum(),
                     (b * b).sum()], F64)


def moment_scale(rows):
    """[9] fp64: sum of |term| per moment, what a relative bound on a reordered sum is relative to"""
    x = np.abs(np.asarray(rows)[:, :3].astype(F64))
    return moments(x)


def mean_cov(m, n):
    m = np.asarray(m, F64)
    mu = m[:3] / n
    second = np.array([[m[3], m[4], m[5]], [m[4], m[6], m[7]], [m[5], m[7], m[8]]], F64)
    return mu, second / n - np.outer(mu, mu)


def solve(content_moments, n_c, style_moments, n_s):
    """-> [4,4] float32: A in [:3,:3], b in [:3,3], last row 0 0 0 1"""
    mu_c, cov_c = mean_cov(content_moments, n_c)
    mu_s, cov_s = mean_cov(style_moments, n_s)
    e_c, u_c = np.linalg.eigh(cov_c)
    e_s, u_s = np.linalg.eigh(cov_s)
    inv_sqrt_c = (u_c / np.sqrt(np.clip(e_c, 1e-8, 1e8))) @ u_c.T
    sqrt_s = (u_s * np.sqrt(np.clip(e_s, 1e-8, 1e8))) @ u_s.T
    A = sqrt_s @ inv_sqrt_c
    tf = np.eye(4, dtype=F64)
    tf[:3, :3] = A
    tf[:3, 3] = mu_s - A @ mu_c
    return tf.astype(F32)


def _fma(a, x, c):
    return (np.asarray(a, F32).astype(F64) * x.astype(F64) + c.astype(F64)).astype(F32)


def apply(rows, tf, clamp=True):
    """rows [n, 3 or 4] f32 -> the rows mapped; a fourth column is carried over"""
    rows = np.asarray(rows, F32)
    tf = np.asarray(tf, F32)
    out = rows.copy()
    r, g, b = rows[:, 0], rows[:, 1], rows[:, 2]
    for c in range(3):
        v = _fma(tf[c, 2], b, _fma(tf[c, 1], g, _fma(tf[c, 0], r, np.full_like(r, tf[c, 3]))))
        out[:, c] = np.minimum(np.maximum(v, F32(0)), F32(1)) if clamp else v
    return out


def apply_bound(rows, tf):
    """[n, 3] fp64: 2^-23 (|tf[c,3]| + sum_k |tf[c,k]| |x_k|), the distance allowed between apply() and the kernel"""
    x = np.abs(np.asarray(rows)[:, :3].astype(F64))
    t = np.abs(np.asarray(tf, F32).astype(F64))
    return 2.0 ** -23 * (t[:3, 3][None, :] + x @ t[:3, :3].T)


def match(image_set, style_img):
    """image_set [N,H,W,3], style_img [H,W,3] f32 -> (image_set' f32 clamped, color_tf [4,4] f32): the whole restatement"""
    rows = np.asarray(image_set, F32).reshape(-1, 3)
    srows = np.asarray(style_img, F32).reshape(-1, 3)
    tf = solve(moments(rows), rows.shape[0], moments(srows), srows.shape[0])
    return apply(rows, tf).reshape(np.asarray(image_set).shape), tf
