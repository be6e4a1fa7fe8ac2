"""NumPy fp64 restatement of nsr_occ_mark_untrained (csrc/occ_untrained.hip, include/nsr.h "Untrained cells"): the same IEEE
operations in the same order -- NumPy never contracts a multiply and an add -- so counts, the grid, the bitfield and the totals
are compared exactly.  Also the host frustum computation of Renderer.mark_untrained_grid, restated apart from the product's, and
the march's cell index (rm_probe.h) for the tests that ask which cells a point falls into."""
import numpy as np

F32, F64 = np.float32, np.float64


def morton_invert(m):
    x = np.asarray(m, np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xc30c30c3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0f00f00f)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xff0000ff)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000ffff)
    return x


def _expand_bits(v):
    v = np.asarray(v, np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0xFF0000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0F00F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0xC30C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x49249249)
    return v


def morton(x, y, z):
    return _expand_bits(x) | (_expand_bits(y) << np.uint32(1)) | (_expand_bits(z) << np.uint32(2))


def flips(camera_flip):
    """(f0, f1, f2) as k_generate_rays decodes them: bits 2, 1, 0"""
    return tuple(-1.0 if (camera_flip >> s) & 1 else 1.0 for s in (2, 1, 0))


def cell_centres(C, H, bound):
    """-> (X [C, H^3, 3] fp64 in flat-index order, half [C] fp64)"""
    m = np.arange(H ** 3, dtype=np.uint32)
    idx = np.stack([morton_invert(m), morton_invert(m >> np.uint32(1)), morton_invert(m >> np.uint32(2))], 1).astype(np.int64)
    X, half = np.empty((C, H ** 3, 3), F64), np.empty(C, F64)
    for cas in range(C):
        b = min(F64(2.0 ** cas), F64(F32(bound)))
        half[cas] = b / F64(H)
        X[cas] = b * (2 * idx + 1 - H).astype(F64) / F64(H)
    return X, half


def counts(C, H, bound, poses, frustum, camera_flip, margin_cells):
    """-> int32 [C * H^3]: the number of frames that see each cell"""
    x_lo, x_hi, y_lo, y_hi = (F64(v) for v in frustum)
    f0, f1, f2 = (F64(f) for f in flips(camera_flip))
    P = np.asarray(poses, F32)[:, :3, :].astype(F64)
    X, half = cell_centres(C, H, bound)
    kx_hi, kx_lo = np.sqrt(F64(1) + x_hi * x_hi), np.sqrt(F64(1) + x_lo * x_lo)
    ky_hi, ky_lo = np.sqrt(F64(1) + y_hi * y_hi), np.sqrt(F64(1) + y_lo * y_lo)
    out = np.zeros((C, H ** 3), np.int32)
    for cas in range(C):
        rho = (F64(margin_cells) * half[cas]) * np.sqrt(F64(3.0))
        for R in P:
            d0, d1, d2 = X[cas, :, 0] - R[0, 3], X[cas, :, 1] - R[1, 3], X[cas, :, 2] - R[2, 3]
            xc = ((R[0, 0] * d0 + R[1, 0] * d1) + R[2, 0] * d2) * f0
            yc = ((R[0, 1] * d0 + R[1, 1] * d1) + R[2, 1] * d2) * f1
            zc = ((R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2) * f2
            seen = ((zc + rho > 0) & (xc - x_hi * zc <= rho * kx_hi) & (x_lo * zc - xc <= rho * kx_lo)
                    & (yc - y_hi * zc <= rho * ky_hi) & (y_lo * zc - yc <= rho * ky_lo))
            out[cas] += seen
    return out.reshape(-1)


def mark(grid, bitfield, C, H, bound, poses, frustum, camera_flip, margin_cells, min_views):
    """-> (counts i32 [C*H^3], grid after f32 [C*H^3], bitfield after u8 [C*H^3/8] or None, n_untrained u32 [C])"""
    cnt = counts(C, H, bound, poses, frustum, camera_flip, margin_cells)
    g = np.array(grid, F32).reshape(-1).copy()
    unseen = cnt < min_views
    with np.errstate(invalid='ignore'):
        reopen = ~unseen & (g < 0)
    g[unseen] = F32(-1)
    g[reopen] = F32(0)
    bits = None
    if bitfield is not None:
        clear = np.packbits(unseen.reshape(-1, 8)[:, ::-1], axis=1).reshape(-1)          # bit i of byte n = cell 8 n + i
        bits = np.asarray(bitfield, np.uint8).reshape(-1) & ~clear
    return cnt, g, bits, unseen.reshape(C, -1).sum(1).astype(np.uint32)


# ---- host frustum (Renderer.mark_untrained_grid) ------------------------------------------------------------------------------
def pinhole_frustum(w, h, fx, fy, cx, cy):
    """the frame's outer pixel edges in pinhole coordinates, fp64"""
    fx, fy, cx, cy = F64(fx), F64(fy), F64(cx), F64(cy)
    return float((F64(0) - cx) / fx), float((F64(w) - cx) / fx), float((F64(0) - cy) / fy), float((F64(h) - cy) / fy)


def lens_frustum(w, h, lens):
    """lens = (fx, fy, cx, cy, k1, k2): the bounding rectangle of (x s, y s), s = 1 + r2 (k1 + r2 k2), over the four corners of
    every border pixel, i.e. every integer corner on the frame's outline and one pixel inside it"""
    fx, fy, cx, cy, k1, k2 = (F64(v) for v in lens)
    if k1 == 0 and k2 == 0:
        return pinhole_frustum(w, h, fx, fy, cx, cy)
    U, V = np.meshgrid(np.arange(w + 1, dtype=F64), np.arange(h + 1, dtype=F64))
    ring = (U <= 1) | (U >= w - 1) | (V <= 1) | (V >= h - 1)
    x, y = (U[ring] - cx) / fx, (V[ring] - cy) / fy
    r2 = x * x + y * y
    s = F64(1) + r2 * (k1 + r2 * k2)
    return float((x * s).min()), float((x * s).max()), float((y * s).min()), float((y * s).max())


# ---- the march's cell of a point (rm_probe.h, fp32) ----------------------------------------------------------------------------
def march_cells(xyz, C, H, bound):
    """flat cell indices [n, C - m1 ...] flattened: for every point, the cell rm_probe would read at every level from the point's
    own mip level up to C - 1 (the march takes max(m1, m2), and m2 depends on the step length alone).  xyz fp32 [n,3] inside the
    box.  -> int64 [k]"""
    xyz = np.asarray(xyz, F32)
    bound32 = F32(bound)
    mx = np.abs(xyz).max(1)
    _, e = np.frexp(mx)
    m1 = np.clip(e, 0, C - 1)
    out = []
    for level in range(C):
        sel = m1 <= level
        p = xyz[sel]
        mip_pow = F32(2.0 ** level)
        rb = F32(1) / mip_pow if mip_pow < bound32 else F32(1) / bound32
        n = np.clip((p * rb + F32(1)) * F32(0.5 * H), F32(0), F32(H - 1)).astype(np.int64)
        out.append(level * H ** 3 + morton(n[:, 0], n[:, 1], n[:, 2]).astype(np.int64))
    return np.concatenate(out)
