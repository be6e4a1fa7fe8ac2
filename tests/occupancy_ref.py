"""Reference for the occupancy-grid update (NumPy, CPU): nsr_occ_num_points, nsr_occ_sample_points (k_occ_sample with its Philox
counter and key layout, the occupied-cell list as flatnonzero) and nsr_occ_update (scatter, decay/max, mean, packbits) restated,
plain and sequential where that is clearest; and the error bound tests/test_gpu_occupancy.py holds the device mean to.

Cells are flat indices cas * H^3 + morton(x, y, z).  Every fp32 expression is written with float32 operands, one NumPy
operation per rounding, so no product is fused with a sum."""
import functools

import numpy as np

from frame_batch_ref import philox, umulhi

F32 = np.float32
M32 = 0xffffffff


def num_points(C, H, full):
    H3 = H ** 3
    return C * H3 if full else C * 2 * (H3 // 4)


def _expand_bits(v):
    v = np.asarray(v, np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0xFF0000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0F00F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0xC30C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x49249249)
    return v


def morton(x, y, z):
    """bit i of x -> bit 3i, of y -> bit 3i+1, of z -> bit 3i+2 (coordinates below 1024)"""
    return _expand_bits(x) | (_expand_bits(y) << np.uint32(1)) | (_expand_bits(z) << np.uint32(2))


def _compact_bits(v):
    v = np.asarray(v, np.uint32) & np.uint32(0x49249249)
    v = (v | (v >> np.uint32(2))) & np.uint32(0xC30C30C3)
    v = (v | (v >> np.uint32(4))) & np.uint32(0x0F00F00F)
    v = (v | (v >> np.uint32(8))) & np.uint32(0xFF0000FF)
    v = (v | (v >> np.uint32(16))) & np.uint32(0x0000FFFF)
    return v


def morton_invert(m):
    """-> uint32 [N,3]"""
    m = np.asarray(m, np.uint32)
    return np.stack([_compact_bits(m), _compact_bits(m >> np.uint32(1)), _compact_bits(m >> np.uint32(2))], axis=-1)


@functools.lru_cache(maxsize=16)
def _words(P, k0, k1, seq, which):
    """the four Philox words of counter (p, seq, which, 0) for p < P, as read-only uint32 arrays (they do not depend on the grid,
    so the cases of one shape share them)"""
    out = tuple(w.astype(np.uint32) for w in philox(np.arange(P, dtype=np.uint64), seq, which, 0, k0, k1))
    for w in out:
        w.setflags(write=False)
    return out


def occupied(grid_cas):
    """ascending Morton indices of one cascade's occupied cells: nonzero(grid > 0) -- NaN, -1, -0.0 and +0.0 are not occupied,
    the smallest denormal is"""
    with np.errstate(invalid='ignore'):
        return np.flatnonzero(np.asarray(grid_cas, F32) > F32(0))


def cascade_scales(cas, H, bound):
    """-> (span, half) of occ_position in fp32: b = min(2^cas, bound), half = b / H, span = b - half"""
    b = np.minimum(np.asarray(2.0 ** np.asarray(cas, np.float64), F32), F32(bound))
    half = b / F32(H)
    return b - half, half


def positions(cas, m, u, H, bound):
    """occ_position: cas [P], Morton index m [P], jitter u f32 [P,3] in [0,1) -> f32 [P,3], one rounding per operation"""
    span, half = cascade_scales(cas, H, bound)
    c = morton_invert(m).astype(F32)
    xn = F32(2) * c / F32(H - 1) - F32(1)
    v = xn * span[:, None]
    v = v + (np.asarray(u, F32) * F32(2) - F32(1)) * half[:, None]
    assert v.dtype == F32
    return v


def sample_points(grid, C, H, bound, full, seed, seq, noise=None):
    """-> (xyzs f32 [P,3], idx i32 [P]) of nsr_occ_sample_points at the summed sequence `seq` (taken mod 2^32)"""
    H3 = H ** 3
    P = num_points(C, H, full)
    k0, k1, seq = seed & M32, (seed >> 32) & M32, seq & M32
    p = np.arange(P, dtype=np.int64)
    if noise is None:
        r = _words(P, k0, k1, seq, 0)
        u = np.stack([(r[d] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) for d in range(3)], axis=1)
    else:
        u = np.asarray(noise, F32).reshape(P, 3)
    if full:
        cas, m, idx = p // H3, p % H3, p.copy()
    else:
        grid = np.asarray(grid, F32).reshape(C, H3)
        n_rand = H3 // 4
        per = 2 * n_rand
        cas, j = p // per, p % per
        q = _words(P, k0, k1, seq, 1)
        m = morton(umulhi(q[0], H), umulhi(q[1], H), umulhi(q[2], H)).astype(np.int64)
        idx = cas * H3 + m
        for c in range(C):
            occ = occupied(grid[c])
            sel = np.flatnonzero((cas == c) & (j >= n_rand))
            if occ.size == 0:
                m[sel], idx[sel] = 0, -1                      # the kernel still writes a position: that of cell 0
            else:
                m[sel] = occ[umulhi(q[3][sel], occ.size).astype(np.int64)]
                idx[sel] = c * H3 + m[sel]
    return positions(cas, m, u, H, bound), idx.astype(np.int32)


def update(grid, sigmas, idx, C, H, full, decay, thresh=None):
    """-> (grid' f32 [C*H^3], mean64, tmp f32 [C*H^3]).  Partial: tmp = -1, then scattered; among several writers of one cell the
    largest non-negative sigma wins (k_occ_scatter), -0.0 never writes (its bit pattern loses the integer max against -1), and a
    negative or NaN sigma is stored as it is -- defined only where such a point is its cell's single writer.  Full: tmp = sigmas.
    `thresh` does not enter (the threshold is min(device mean, thresh), applied by packbits)."""
    cells = C * H ** 3
    g = np.array(grid, F32).reshape(cells)
    s = np.asarray(sigmas, F32).reshape(-1)
    if full:
        assert s.size == cells
        tmp = s.copy()
    else:
        idx = np.asarray(idx, np.int64).reshape(-1)
        assert s.size == idx.size and idx.max(initial=-1) < cells
        tmp = np.full(cells, -1, F32)
        with np.errstate(invalid='ignore'):
            nonneg = (s >= 0) & ~np.signbit(s) & (idx >= 0)
            other = ~(s >= 0) & (idx >= 0)
        tmp[idx[other]] = s[other]
        best = np.full(cells, -np.inf, F32)
        np.maximum.at(best, idx[nonneg], s[nonneg])
        tmp[best >= 0] = best[best >= 0]
    with np.errstate(invalid='ignore'):
        both = (g >= 0) & (tmp >= 0)
        g[both] = np.fmax(g[both] * F32(decay), tmp[both])
        mean64 = float(np.where(g > 0, g, F32(0)).astype(np.float64).mean())      # fmaxf(g, 0): NaN counts 0
    return g, mean64, tmp


def packbits(grid, thr):
    """bit i of byte n = (cell 8n+i > thr), strict"""
    with np.errstate(invalid='ignore'):
        bits = np.asarray(grid, F32).reshape(-1, 8) > F32(thr)
    return np.packbits(bits, axis=1, bitorder='little').reshape(-1)


def mean_bound(C, H):
    """relative error bound of the device mean, counted: along any value's path there are k = ceil(cells / (nblk * 256)) + 6 + 4
    fp32 additions (the thread's strided adds, six shuffle steps, four wave totals; nblk = min(ceil(cells / 256), 2048)) and one
    rounding in the final cast; the sum of the block totals and the division run in double.  All addends are >= 0, so the error
    is at most (k + 1) * 2^-24 of the mean to first order; doubled for the second-order terms and the double arithmetic."""
    cells = C * H ** 3
    nblk = min(-(-cells // 256), 2048)
    k = -(-cells // (nblk * 256)) + 6 + 4
    return 2.0 * (k + 1) * 2.0 ** -24
