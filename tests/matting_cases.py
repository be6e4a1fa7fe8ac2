"""Inputs, shapes and references for the edge tests of the matting-Laplacian kernel (csrc/matting.hip): NumPy only, no GPU.

Shared by test_gpu_matting_edges.py and test_matting_cpu.py, which measures on the reference side alone how far the two fp64
restatements of matting_ref.py disagree on every case below: the noise floor under the bars of the GPU file.

The kernel works on TX x TY = 32 x 8 pixel tiles with a 2r halo; D = 2r+1 is the window's side.  edge_shapes(r) puts the
image's right and bottom borders at every distance from a tile seam at which the last tile changes what it holds: pixels but
no window centre, a centre whose window reaches into the neighbour's halo, a full halo."""
import functools

import numpy as np

from matting_ref import matting_dense, matting_fast

TX, TY = 32, 8
EPS = 1e-7
DENSE_LIMIT = 4096                    # pixels up to which the per-window dense restatement is the reference
# conditioned_case(r): largest per-element difference of matting_dense and matting_fast over max |gradient|, as measured
# (test_matting_cpu.py prints it and holds the measurement to this record)
COND_FLOOR = {1: 4.64e-11, 2: 1.98e-11}


def edge_shapes(r):
    """(H, W) pairs, in a fixed order, without repeats"""
    D = 2 * r + 1
    out = [(D, D), (D, D + 1), (D + 1, D), (D, 97), (61, D)]                                   # one window, one row, one column
    out += [(11, W) for W in (31, 32, 33, 32 + r, 32 + r + 1, 32 + 2 * r, 32 + 2 * r + 1, 63, 64, 65)]      # width seam
    out += [(H, 37) for H in (7, 8, 9, 8 + r, 8 + r + 1, 8 + 2 * r, 8 + 2 * r + 1, 16, 17)]                   # height seam
    out += [(8 + r + 1, 32 + r + 1), (17, 65), (8 + 2 * r + 1, 64 + 2 * r + 1)]                # both seams at once
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def inputs(r, H, W):
    """float32 target, uniform in [0, 1), and a style map that partly follows it; seeded per (r, H, W)"""
    rng = np.random.default_rng([r, H, W])
    t = rng.random((3, H, W)).astype(np.float32)
    v = (0.6 * t[::-1] + 0.4 * rng.random((3, H, W))).astype(np.float32)
    return t, v


def conditioned_inputs(r, noise=1e-3, H=17, W=65):
    """A step of height 0.5 on the x = TX tile seam in all three channels plus `noise` of uniform noise: the windows that
    straddle the seam have a Sigma of rank one plus noise^2 / 12."""
    rng = np.random.default_rng([r, H, W, 1])
    t = np.full((3, H, W), 0.25)
    t[:, :, TX:] += 0.5
    t = (t + noise * rng.random((3, H, W))).astype(np.float32)
    v = (0.6 * t[::-1] + 0.4 * rng.random((3, H, W))).astype(np.float32)
    return t, v


def reference(t, v, r, eps=EPS):
    """fp64 (value, gradient): per-window dense up to DENSE_LIMIT pixels, vectorised above"""
    if t.shape[1] * t.shape[2] <= DENSE_LIMIT:
        val, g = matting_dense(t, v, r, eps)
        return float(val), g
    return matting_fast(t, v, r, eps)


@functools.lru_cache(maxsize=None)
def edge_case(r, H, W):
    """(target, v, value, gradient) of one edge shape, computed once; callers must not modify the arrays"""
    t, v = inputs(r, H, W)
    val, g = reference(t, v, r)
    for a in (t, v, g):
        a.setflags(write=False)
    return t, v, val, g


@functools.lru_cache(maxsize=None)
def conditioned_case(r, noise=1e-3):
    t, v = conditioned_inputs(r, noise)
    val, g = reference(t, v, r)
    for a in (t, v, g):
        a.setflags(write=False)
    return t, v, val, g


def floor(t, v, r, eps=EPS):
    """How far the two fp64 restatements disagree: (largest per-element gradient difference / max |gradient|, relative
    value difference)"""
    vd, gd = matting_dense(t, v, r, eps)
    vf, gf = matting_fast(t, v, r, eps)
    return float(np.abs(gd - gf).max() / np.abs(gd).max()), abs(float(vd) - vf) / abs(float(vd))


def window_count(H, W, r):
    """[H,W] number of (2r+1)^2 windows inside the image that contain each pixel, in closed form"""
    y, x = np.arange(H), np.arange(W)
    ny = np.minimum(y + r, H - 1 - r) - np.maximum(y - r, r) + 1
    nx = np.minimum(x + r, W - 1 - r) - np.maximum(x - r, r) + 1
    return ny[:, None] * nx[None, :]


def window_count_brute(H, W, r):
    n = np.zeros((H, W), np.int64)
    for cy in range(r, H - r):
        for cx in range(r, W - r):
            n[cy - r:cy + r + 1, cx - r:cx + r + 1] += 1
    return n


def count_gradient(v, r):
    """The gradient as eps -> infinity, where Sigma^-1 vanishes and only the window means are left:
    2 (n_p v_p - sum over the windows that contain p of mean_w(v)), with n_p from window_count.  fp64."""
    v = np.asarray(v, np.float64)
    _, H, W = v.shape
    d = 2 * r + 1
    h, w = H - 2 * r, W - 2 * r
    mean = sum(v[:, dy:dy + h, dx:dx + w] for dy in range(d) for dx in range(d)) / float(d * d)
    acc = np.zeros_like(v)
    for dy in range(d):
        for dx in range(d):
            acc[:, dy:dy + h, dx:dx + w] += mean
    return 2.0 * (window_count(H, W, r)[None] * v - acc)
