"""Builders and references for the per-axis bounding box of the field kernels and for the two position-derivative kernels
(nsr_field_density_gradient, nsr_field_position_gradient).  NumPy / CPU torch only; the CPU tests prove what the builders
claim, the GPU tests use them.

Two boxes:
  * EXACT_*: sizes 4 * 2^e with e = (-2, 1, 0) and a minimum on a 2^-4 grid.  A point x' of the +-2 cube on a 2^-16 grid and
    x_k = min_k + (x'_k + 2) * 2^e_k give the same fp32 value (x - min) / size == (x' + 2) / 4, because x, x - min and x' + 2
    are all exact in fp32: from field_unit on, a call on the box at x and a call on the cube at x' are one computation.
  * ODD_*: the sample order's box, sizes (3, 4, 1.75): u rounds differently from the cube's, so kernels are held to the
    rounding-emulating restatement (oracle.torch_port.Field) evaluated at x' = 4 (x - min) / size - 2 (float64), with the
    gradient multiplied by 4 / size_k.

"Outside" is the encoder's rule: u = ((x - min) / size + 1) / 2 must lie in [0, 1], i.e. x in [min - size, min + size]; the
box proper is u in [0.5, 1].
"""
import numpy as np
import torch

import grid_encode_ref as GE
from sample_order_ref import BOX_MIN as ODD_MIN, BOX_SIZE as ODD_SIZE

EXACT_E = (-2, 1, 0)
EXACT_SIZE = tuple(4.0 * 2.0 ** e for e in EXACT_E)          # (1, 8, 4)
EXACT_MIN = (0.4375, -6.25, -2.0)
CUBE_MIN, CUBE_SIZE = (-2.0, -2.0, -2.0), (4.0, 4.0, 4.0)
GRID = 2.0 ** -16
FACE_WINDOW = 2.0 ** -10                                     # odd box: no kept point has u * res_l this close to an integer


def _specials_cube():
    """cube coordinates of the edge points, on the 2^-16 grid: (points [n,3], dead [n])"""
    inside = np.array([0.40625, -1.21875, 1.0625])
    pts, dead = [], []

    def add(p, d):
        pts.append(np.asarray(p, np.float64))
        dead.append(d)
    add([0.3125, np.nan, -0.1875], True)
    add([np.inf, 0.125, 0.25], True)
    add([0.5, -0.75, -np.inf], True)
    for k in range(3):
        for v, d in ((2.0 + GRID, True), (-6.0 - GRID, True), (2.0, False), (-6.0, False)):   # u just above 1, just below 0, == 1, == 0
            p = inside.copy()
            p[k] = v
            add(p, d)
    add([-2.0, -2.0, -2.0], False)                           # the box's two extreme corners
    add([2.0, 2.0, 2.0], False)
    add([-6.0, -6.0, -6.0], False)                           # and the encoder's own low corner, u = (0, 0, 0)
    return np.array(pts), np.array(dead)


def special_slots(M, n):
    """slots for n edge points in a buffer of M: slots 0, 7 and 15 of tiles first (from tile 1 on), then every fourth slot"""
    if M > 33 + 4 * (n - 4):
        s = [16, 23, 31] + [33 + 4 * j for j in range(n - 3)]
    else:
        s = list(np.linspace(0, M - 1, n).astype(int)) if M >= n else list(range(M))
    return np.asarray(s[:min(n, M)], np.int64)


def exact_points(M, seed=0):
    """(x_cube [M,3] f32, x_box [M,3] f32, dead [M] bool) for the EXACT box; every sixteenth random point has one coordinate in
    the encoded shell below the box (u < 0.5)"""
    rng = np.random.default_rng(seed)
    xc = rng.integers(-2 ** 17, 2 ** 17 + 1, size=(M, 3)).astype(np.float64) * GRID
    shell = np.arange(M) % 16 == 5
    ax = rng.integers(0, 3, size=M)
    xc[shell, ax[shell]] -= 4.0
    dead = np.zeros(M, bool)
    sp, sd = _specials_cube()
    slots = special_slots(M, len(sp))
    xc[slots] = sp[:len(slots)]
    dead[slots] = sd[:len(slots)]
    with np.errstate(invalid='ignore'):
        xb = np.asarray(EXACT_MIN)[None] + (xc + 2.0) * (2.0 ** np.asarray(EXACT_E, np.float64))[None]
    return xc.astype(np.float32), xb.astype(np.float32), dead


def exactness_report(M, seed=0):
    """float64 evidence for exact_points: per point and axis, are x, x - min and x' + 2 exact in fp32, and do the box and
    the cube then give the same fp32 normalised coordinate?  Non-finite coordinates must be the same non-finite value."""
    xc, xb, _ = exact_points(M, seed)
    xc64, xb64 = xc.astype(np.float64), xb.astype(np.float64)
    mn, e = np.asarray(EXACT_MIN)[None], np.asarray(EXACT_E, np.float64)[None]
    fin = np.isfinite(xc64)
    with np.errstate(invalid='ignore'):
        x_true = mn + (xc64 + 2.0) * 2.0 ** e                # float64: exact for these magnitudes
        d_box, d_cube = xb64 - mn, xc64 + 2.0

        def f32_exact(v):
            return v.astype(np.float32).astype(np.float64) == v
        ok = f32_exact(x_true) & (x_true == xb64) & f32_exact(d_box) & f32_exact(d_cube)
        same_u = (xb - np.asarray(EXACT_MIN, np.float32)[None]) / np.asarray(EXACT_SIZE, np.float32)[None] == \
                 (xc - np.float32(-2.0)) / np.float32(4.0)
        same_nonfinite = (np.isnan(xc) & np.isnan(xb)) | (xc == xb)
    return np.where(fin, ok & same_u, same_nonfinite & ~np.isfinite(xb64))


# ---- the kernels' encoder input, fp32, operation for operation (field_unit) --------------------------------------------------
def unit_f32(x, bmin, bsize):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        xn = (x - np.asarray(bmin, np.float32)[None]) / np.asarray(bsize, np.float32)[None]
        return (xn + np.float32(1.0)) / np.float32(2.0)


def unit_f64(x, bmin, bsize):
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return ((x - np.asarray(bmin, np.float64)[None]) / np.asarray(bsize, np.float64)[None] + 1.0) / 2.0


def grid_S(min_res=16, bound=2.0):
    return GE.grid_S(float(np.exp2(np.log2(1024 * (2 * bound) / min_res) / 15)))


def resolutions(min_res=16, bound=2.0):
    return np.array(GE.resolutions(16, grid_S(min_res, bound), min_res), np.int64)


def fast_levels(offsets, min_res=16, bound=2.0):
    """field_fill_args' mask from grid_encode_ref.fill_levels (nsr_fill_levels' rule): bit l set when level l is hashed and its
    size is a power of two"""
    mask = 0
    for l, lv in enumerate(GE.fill_levels(offsets, grid_S(min_res, bound), min_res, 0)):
        if lv['use_hash'] and lv['size'] & (lv['size'] - 1) == 0:
            mask |= 1 << l
    return mask


def model_cfg(bsize, min_res=16):
    """NetworkConfig under which a StyleTCNerf on a box of sides `bsize` has the grid of the +-2 cube: the model scales its
    finest resolution by the box's largest side, 1024 * 4 here"""
    from nerfstyle_amd.config import NetworkConfig, PosEncConfig
    coeff = 1024.0 * 4.0 / float(max(bsize))
    return NetworkConfig(pos_enc=PosEncConfig(min_res=min_res, max_res_coeff=coeff))


def make_model(dev, ref, bmin, bsize, table_half=True, dt='f16', min_res=16):
    """a StyleTCNerf on the box (bmin, bsize) holding the parameters of the oracle field `ref`"""
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.style_nerf import StyleTCNerf
    mn, sz = np.asarray(bmin, np.float64), np.asarray(bsize, np.float64)
    m = StyleTCNerf(model_cfg(bsize, min_res), BBox(mn, mn + sz), ref.nc, enc_dtype=None if table_half else torch.float32,
                    use_dir=False, compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16)
    assert m.rows == int(ref.offsets[-1]) and m.S == float(np.float32(np.log2(ref.pls)))
    sd = m.state_dict()
    sd.update({'x_density_embedder.embeddings': ref.emb_density.detach(), 'x_color_embedder.embeddings': ref.emb_color.detach(),
               'density_net.params': ref.p_density.detach(), 'color1_net.params': ref.p_color1.detach(),
               'color2_net.params': ref.p_color2.detach(), 'class_net.params': ref.p_class.detach()})
    m.load_state_dict(sd)
    return m.to(dev)


def cells(u, res, dtype):
    """[M,16,3] cell of every level: floor(u * res) clamped to res - 1, in `dtype` arithmetic (nsr_grid_locate)"""
    u = np.asarray(u, dtype)
    pos = u[:, None, :] * res.astype(dtype)[None, :, None]
    return np.minimum(np.floor(pos), (res - 1).astype(dtype)[None, :, None]).astype(np.int64)


def near_face(u32, res):
    """[M] bool: some u * res_l (fp32 product of the kernel's fp32 u) within FACE_WINDOW of an integer"""
    pos = u32.astype(np.float32)[:, None, :] * res.astype(np.float32)[None, :, None]
    return (np.abs(pos - np.rint(pos)) < FACE_WINDOW).any(axis=(1, 2))


def to_cube_f64(x, bmin, bsize):
    """x' = 4 (x - min) / size - 2 in float64 from the fp32 positions"""
    x = np.asarray(x, np.float32).astype(np.float64)
    return (x - np.asarray(bmin, np.float64)[None]) / np.asarray(bsize, np.float64)[None] * 4.0 - 2.0


def odd_points(M, seed=0, min_res=16):
    """(x [M,3] f32 in the ODD box, dead [M] bool, redrawn: int).  Live points are uniform over the encoded range of the box
    (seven in eight inside the box proper, one in eight with a coordinate in the shell below it); a point near a cell face
    of any level (near_face) is drawn again.  Dead points: NaN, +-inf, outside on either side of every axis; u == 0 and
    u == 1 on each axis are live and exempt from the redraw (they sit on a face by construction and are clamped)."""
    rng = np.random.default_rng(seed)
    mn, sz = np.asarray(ODD_MIN, np.float64), np.asarray(ODD_SIZE, np.float64)
    res = resolutions(min_res)

    def draw(n):
        r = rng.random((n, 3))
        shell = rng.random(n) < 0.125
        ax = rng.integers(0, 3, size=n)
        r[shell, ax[shell]] -= 1.0
        return (mn[None] + sz[None] * r).astype(np.float32)
    x = draw(M)
    redrawn = 0
    for _ in range(64):
        bad = near_face(unit_f32(x, ODD_MIN, ODD_SIZE), res)
        if not bad.any():
            break
        redrawn += int(bad.sum())
        x[bad] = draw(int(bad.sum()))
    assert not near_face(unit_f32(x, ODD_MIN, ODD_SIZE), res).any()
    dead = np.zeros(M, bool)
    sp = []
    inside = (mn + sz * np.array([0.61, 0.27, 0.83])).astype(np.float32)
    sp.append((np.array([inside[0], np.nan, inside[2]], np.float32), True))
    sp.append((np.array([np.inf, inside[1], inside[2]], np.float32), True))
    sp.append((np.array([inside[0], inside[1], -np.inf], np.float32), True))
    for k in range(3):
        for v, d in ((mn[k] + sz[k] * 1.001, True), (mn[k] - sz[k] * 1.001, True), (mn[k] + sz[k], False), (mn[k] - sz[k], False)):
            p = inside.copy()
            p[k] = np.float32(v)
            sp.append((p, d))
    slots = special_slots(M, len(sp))
    for s, (p, d) in zip(slots, sp):
        x[s], dead[s] = p, d
    return x, dead, redrawn


# ---- float64 restatement of both derivative kernels, with the mutations a test must notice -----------------------------------
MUTATIONS = ('size0_everywhere', 'out_scale_swapped', 'min_wrong_axis', 'cell_scale_level_x2', 'perm_bound_dropped')
MUT_LEVEL = 6                                               # the level whose cell_scale the fourth mutation doubles


def _unit_mut(pts, bmin, bsize, mut):
    mn, sz = np.asarray(bmin, np.float64).copy(), np.asarray(bsize, np.float64).copy()
    if mut == 'size0_everywhere':
        sz[:] = sz[0]
    if mut == 'min_wrong_axis':
        mn = mn[[1, 0, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        u = ((np.asarray(pts, np.float64) - mn[None]) / sz[None] + 1.0) / 2.0
    dudx = 1.0 / (2.0 * sz)
    if mut == 'out_scale_swapped':
        dudx = dudx[[0, 2, 1]]
    return u, dudx


def _partials(u, live, emb, offsets, res):
    """features x [M,32] and their partials t [3,M,32] with respect to u (res_l included), float64; emb [rows, 2]"""
    from oracle import torch_port as TP
    M = u.shape[0]
    x, t = np.zeros((M, 32)), np.zeros((3, M, 32))
    uu = np.where(live[:, None], u, 0.5)
    for l in range(16):
        size = int(offsets[l + 1] - offsets[l])
        pos = uu * float(res[l])
        c = np.minimum(np.floor(pos), float(res[l] - 1))
        f = pos - c
        ci = torch.from_numpy(c.astype(np.int64))[:, None, :] + TP._CORNERS[None]
        rows = (TP._row_index(ci, int(res[l]), size) + int(offsets[l])).numpy()
        v = emb[rows]                                                                          # [M, 8, 2]
        w1 = np.stack([1 - f, f], axis=-1)                                                      # [M, axis, bit]
        for idx in range(8):
            w = w1[:, 0, idx & 1] * w1[:, 1, (idx >> 1) & 1] * w1[:, 2, idx >> 2]
            x[:, 2 * l:2 * l + 2] += w[:, None] * v[:, idx]
        for gd in range(3):
            d0, d1 = [d for d in range(3) if d != gd]
            for j in range(4):
                b0, b1 = j & 1, j >> 1
                w = w1[:, d0, b0] * w1[:, d1, b1]
                left = (b0 << d0) | (b1 << d1)
                t[gd, :, 2 * l:2 * l + 2] += float(res[l]) * w[:, None] * (v[:, left | (1 << gd)] - v[:, left])
    x[~live] = 0
    t[:, ~live] = 0
    return x, t


def density_gradient_f64(ref, pts, bmin, bsize, density_scale=1.0, mut=None):
    """(sigma [M], grad [M,3]) of k_field_density_grad's chain in float64 without operand rounding, for positions in the box
    (bmin, bsize); `ref` is an oracle.torch_port.Field (its tables, first MLP and grid)"""
    emb = ref.emb_density.detach().numpy().astype(np.float64)
    p = ref.p_density.detach().numpy().astype(np.float64)
    W1, W2 = p[:2048].reshape(64, 32), p[2048:3072].reshape(16, 64)[0]
    res = resolutions(ref.min_res, ref.bound)
    u, dudx = _unit_mut(pts, bmin, bsize, mut)
    with np.errstate(invalid='ignore'):
        live = np.all((u >= 0) & (u <= 1), axis=1)
    x, t = _partials(u, live, emb, ref.offsets, res)
    if mut == 'cell_scale_level_x2':
        t[:, :, 2 * MUT_LEVEL:2 * MUT_LEVEL + 2] *= 2.0
    h = x @ W1.T
    logit = np.maximum(h, 0) @ W2
    grad = np.zeros((len(u), 3))
    for k in range(3):
        grad[:, k] = density_scale * np.exp(np.clip(logit, -15, 15)) * (((t[k] @ W1.T) * (h > 0)) @ W2) * dudx[k]
    grad[~live] = 0
    return density_scale * np.exp(logit), grad


def position_gradient_f64(ref, pts, eg, bmin, bsize, count=None, perm=None, mut=None, table_half=False):
    """k_field_xgrad in float64: grad [M,3] = sum over levels and the four channels of eg [M,16,4] * d feature / d x; zero for
    dead samples and for slots at or past `count`.  The fifth mutation walks perm without the bound m < count: a slot past
    the count is then computed from whatever `eg` holds there (NaN in the tests) and written."""
    M = len(pts)
    count = M if count is None else int(min(max(count, 0), M))
    res = resolutions(ref.min_res, ref.bound)
    u, dudx = _unit_mut(pts, bmin, bsize, mut)
    with np.errstate(invalid='ignore'):
        live = np.all((u >= 0) & (u <= 1), axis=1)
    walked = np.zeros(M, bool)
    order = np.arange(count) if perm is None else np.asarray(perm[:count]).astype(np.int64)
    ok = order < (M if mut == 'perm_bound_dropped' else count)
    walked[order[ok]] = True
    out = np.zeros((M, 3))
    for e, sl in ((ref.emb_density, slice(0, 2)), (ref.emb_color, slice(2, 4))):
        emb = e.detach()
        emb = (emb.to(torch.float16) if table_half else emb).to(torch.float64).numpy()
        _, t = _partials(u, live & walked, emb, ref.offsets, res)
        if mut == 'cell_scale_level_x2':
            t[:, :, 2 * MUT_LEVEL:2 * MUT_LEVEL + 2] *= 2.0
        g = np.where((live & walked)[:, None], np.asarray(eg, np.float64)[:, :, sl].reshape(M, 32), 0.0)
        for k in range(3):
            out[:, k] += (t[k] * g).sum(axis=1) * dudx[k]
    return out


# ---- the rounding-emulating reference (autograd of oracle.torch_port.Field), evaluated through x' ---------------------------
def field_ref(nc=5, table_scale=1.0, min_res=16):
    from oracle import torch_port as TP
    return TP.Field(num_classes=nc, table_scale=table_scale, min_res=min_res)


def density_gradient_ref(ref, x, good, bmin, bsize, dt, table_half, density_scale=1.0, own_unit=False):
    """d sigma / d x [M,3] float32 of the restatement with the kernel's operand roundings; rows outside `good` are zero.
    Default: evaluated at x' = to_cube_f64(x), times 4 / size_k.  own_unit: evaluated on u = unit_f32(x, bmin, bsize), the
    fp32 operations of field_unit on the box itself, times 1 / (2 size_k)."""
    g = np.zeros((len(x), 3), np.float32)
    if own_unit:
        u = torch.tensor(unit_f32(x, bmin, bsize)[good], requires_grad=True)
        ref.encoder_input = lambda pts: u
        try:
            ref(u, sigma_only=True, half=dt, table_half=table_half).sum().backward()
        finally:
            del ref.encoder_input
        g[good] = u.grad.numpy() * np.float32(density_scale) * (1.0 / (2.0 * np.asarray(bsize, np.float64)))[None].astype(np.float32)
        return g
    xp = to_cube_f64(x, bmin, bsize)[good].astype(np.float32)
    pt = torch.tensor(xp, requires_grad=True)
    ref(pt, sigma_only=True, half=dt, table_half=table_half).sum().backward()
    g[good] = pt.grad.numpy() * np.float32(density_scale) * (4.0 / np.asarray(bsize, np.float64))[None].astype(np.float32)
    return g


def position_gradient_ref(ref, x, eg, good, bmin, bsize, table_half, dtype):
    """d / d x of sum(eg * encode(u)) over both tables through torch_port.grid_encode, u = (x' + 2) / 8 + 1/2 formed in `dtype`
    from x' = to_cube_f64(x) (fp32 when dtype is float32); [good rows, 3] float64"""
    from oracle import torch_port as TP
    xp = to_cube_f64(x, bmin, bsize)[good]
    if dtype == torch.float32:
        xp32 = xp.astype(np.float32)
        u0 = ((xp32 - np.float32(-2.0)) / np.float32(4.0) + np.float32(1.0)) / np.float32(2.0)
    else:
        u0 = ((xp + 2.0) / 4.0 + 1.0) / 2.0
    u = torch.tensor(u0, dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(eg)[good], dtype=dtype)
    tot = 0
    for emb, sl in ((ref.emb_density, slice(0, 2)), (ref.emb_color, slice(2, 4))):
        e = emb.detach()
        e = (e.to(torch.float16) if table_half else e).to(dtype)
        enc = TP.grid_encode(u, e, ref.offsets, ref.pls, base_resolution=ref.min_res)
        tot = tot + (enc.view(-1, 16, 2) * g[:, :, sl]).sum()
    tot.backward()
    return u.grad.numpy().astype(np.float64) / (2.0 * np.asarray(bsize, np.float64))[None]


def keep_level(ref, emb0, level):
    """in place: ref's two tables = emb0 (pair of tensors) with every row outside `level` zeroed"""
    a, b = int(ref.offsets[level]), int(ref.offsets[level + 1])
    with torch.no_grad():
        for p, e in ((ref.emb_density, emb0[0]), (ref.emb_color, emb0[1])):
            p.zero_()
            p[a:b] = e[a:b]


def bad_mask(M):
    """(outside, nan) of tests/test_gpu_field_bwd_gout_exact.py::_bad_mask: slots 0, 7 and 15 of alternating tiles and one
    sample in eight of the rest, from M = 63 on"""
    i = np.arange(M)
    dead = (i % 8 == 3) & (M >= 63)
    nan = (i % 8 == 6) & (M >= 63)
    if M >= 63:
        for k, slot in enumerate((0, 7, 15)):
            if 32 * k + slot < M:
                dead[32 * k + slot], nan[32 * k + slot] = True, False
            if 32 * k + 16 + slot < M:
                nan[32 * k + 16 + slot], dead[32 * k + 16 + slot] = True, False
    return dead, nan


def edge_points(M, seed=0):
    """cube positions for the derivative kernels' shape cases: (x [M,3] f32, good [M] bool).  From M = 63 on the bad samples
    of bad_mask: NaN, +-inf and points outside on either side of every axis in turn; u == 0 and u == 1 samples on each axis
    from M = 15 on (fewer where M is smaller)."""
    rng = np.random.default_rng(900 + M + seed)
    x = (rng.random((M, 3)) * 3.6 - 1.8).astype(np.float32)
    dead, nan = bad_mask(M)
    kinds = [np.nan, np.inf, -np.inf]
    for n, i in enumerate(np.flatnonzero(nan)):
        x[i, n % 3] = kinds[n % 3] if (n // 3) % 2 == 0 else kinds[(n + 1) % 3]
    outs = [(0, 2.5), (0, -6.5), (1, 2.0 * (1 + 2.0 ** -20)), (1, -6.00001), (2, 9.0), (2, -7.0)]
    for n, i in enumerate(np.flatnonzero(dead)):
        ax, v = outs[n % 6]
        x[i, ax] = v
    good = ~(dead | nan)
    faces = [(0, 2.0), (0, -6.0), (1, 2.0), (1, -6.0), (2, 2.0), (2, -6.0)]
    free = np.flatnonzero(good)
    if M >= 15:
        for n, (ax, v) in enumerate(faces):
            x[free[1 + 2 * n], ax] = v
    return x, good
