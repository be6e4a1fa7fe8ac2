"""float64 NumPy restatement of the stand-alone hash-grid encoder (csrc/gridenc.hip): forward, table backward and input
backward, for C in {1, 2, 4, 8}, any L <= 32, gridtype hash | tiled, both align_corners settings, any style, both layouts.

Cell and fraction come from the same fp32 products as nsr_grid_locate (x * scale, + 0.5f, floor, min, p - cell, each rounded
to fp32); rows from the rule of nsr_fill_levels and nsr_grid_row written again in NumPy unsigned 32-bit arithmetic.
Everything after that -- weights, interpolation, sums -- is float64.  Inputs outside [0, 1] and NaN give zero output rows, zero
input-gradient rows and no table gradient.

Exact lattice probes: per_level_scale = 2 and H = 16 make S = 1 and the resolutions 16 * 2^l; inputs on multiples of 1/16 make
x * scale exact, the fractions 0 or 1 (align_corners) or multiples of 1/16 (not), the weights multiples of 2^-12; integer tables
and gradients then make every term of every sum a multiple of 2^-12, and with sum |terms| < 2^24 / 4096 every partial sum in
any order is an fp32 number: the kernels must give the bytes of this reference.  `Case.conditions` asserts that.
"""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
PRIMES = (1, 2654435761, 805459861)
STYLE_PRIME = 3674653429


def grid_S(per_level_scale):
    return np.float32(np.log2(per_level_scale))


def resolutions(L, S, H):
    """floor(exp2f(l * S) * H) in fp32 (nsr_fill_levels)"""
    return [int(np.floor(np.exp2(np.float32(l) * np.float32(S), dtype=np.float32) * np.float32(H))) for l in range(L)]


def offsets_for(L, per_level_scale, H, log2_hashmap_size, align_corners):
    """GridEncoder's level sizes (gridencoder.py)"""
    off, o = [], 0
    for i in range(L):
        res = int(np.ceil(H * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (res if align_corners else res + 1) ** 3)
        off.append(o)
        o += int(np.ceil(n / 8) * 8)
    off.append(o)
    return np.array(off, np.int32)


def fill_levels(offsets, S, H, gridtype):
    """nsr_fill_levels: per level (offset, size, resolution, use_hash, mul[3], style_mul), strides in wrapping u32"""
    lv = []
    for l, res in enumerate(resolutions(len(offsets) - 1, S, H)):
        size = int(offsets[l + 1] - offsets[l])
        stride, mul = 1, [0, 0, 0]
        for d in range(3):
            if stride > size:
                break
            mul[d] = stride
            stride = (stride * (res + 1)) & 0xFFFFFFFF
        style_mul = 0
        if stride <= size:
            style_mul = stride
            stride = (stride * 512) & 0xFFFFFFFF
        lv.append(dict(offset=int(offsets[l]), size=size, res=res, use_hash=int(gridtype == 0 and stride > size), mul=mul,
                       style_mul=style_mul))
    return lv


def grid_row(lv, p, style):
    """nsr_grid_row for integer corners p [..., 3] (uint64 holding u32 values) -> level-relative rows"""
    p = p.astype(np.uint64)
    if lv['use_hash']:
        idx = np.uint64((style * STYLE_PRIME) & 0xFFFFFFFF) * np.ones(p.shape[:-1], np.uint64)
        for d in range(3):
            idx = idx ^ ((p[..., d] * np.uint64(PRIMES[d])) & U32)
    else:
        idx = np.uint64((style * lv['style_mul']) & 0xFFFFFFFF) * np.ones(p.shape[:-1], np.uint64)
        for d in range(3):
            idx = (idx + p[..., d] * np.uint64(lv['mul'][d])) & U32
    return (idx % np.uint64(lv['size'])).astype(np.int64)


def locate(x, res, align_corners):
    """nsr_grid_locate in fp32: x [B, 3] f32 -> (cell int64 [B, 3], frac f32 [B, 3])"""
    scale = np.float32(res - (0 if align_corners else 1))
    p = (x.astype(np.float32) * scale).astype(np.float32)
    if not align_corners:
        p = (p + np.float32(0.5)).astype(np.float32)
    c = np.minimum(np.floor(p), np.float32(res - 1)).astype(np.float32)
    return c.astype(np.int64), (p - c).astype(np.float32)


_CORNERS = np.array([[(i >> d) & 1 for d in range(3)] for i in range(8)], np.int64)      # bit d = the upper corner on axis d


def inside(x):
    return np.all((x >= 0) & (x <= 1), axis=1)                                           # NaN compares false


def corners(x, lv, align_corners, style):
    """-> ok [B] bool, rows [B, 8] int64 (level-relative), w [B, 8] f64, frac [B, 3] f64, wd [B, 8, 3] f64; samples that are not
    inside are located at 0.5 so that the arrays are well defined -- callers mask them with ok"""
    ok = inside(x)
    xs = np.where(ok[:, None], x, np.float32(0.5)).astype(np.float32)
    cell, frac = locate(xs, lv['res'], align_corners)
    f = frac.astype(np.float64)
    wd = np.where(_CORNERS[None] == 1, f[:, None, :], 1.0 - f[:, None, :])
    rows = grid_row(lv, (cell[:, None, :] + _CORNERS[None]).astype(np.uint64), style)
    return ok, rows, wd.prod(axis=2), f, wd


def _blc(a, B, L, C, blc):
    """a user array in the layout blc selects -> [B, L, C] float64"""
    a = np.asarray(a, np.float64)
    return a.reshape(B, L, C) if blc else a.reshape(L, B, C).transpose(1, 0, 2)


def forward(x, emb, offsets, S, H, gridtype, align_corners, style=0, out_blc=1, terms=None):
    """-> [B, L*C] (out_blc) or [L, B, C], float64.  terms: a list that receives (sum |terms|, all terms) per level"""
    lvs = fill_levels(offsets, S, H, gridtype)
    B, L, C = x.shape[0], len(lvs), emb.shape[1]
    emb = np.asarray(emb, np.float64)
    out = np.zeros((B, L, C))
    for l, lv in enumerate(lvs):
        ok, rows, w, _, _ = corners(x, lv, align_corners, style)
        t = w[:, :, None] * emb[lv['offset'] + rows]                                      # [B, 8, C]
        t[~ok] = 0
        out[:, l] = t.sum(axis=1)
        if terms is not None:
            terms.append((np.abs(t).sum(axis=1).max(initial=0), t))
    out = out + 0.0
    return out.reshape(B, L * C) if out_blc else np.ascontiguousarray(out.transpose(1, 0, 2))


def backward(grad, x, offsets, n_rows, C, S, H, gridtype, align_corners, style=0, grad_blc=1, terms=None):
    """-> grad_embeddings [n_rows, C] float64 (the sum this call adds) and touched [n_rows] bool"""
    lvs = fill_levels(offsets, S, H, gridtype)
    B, L = x.shape[0], len(lvs)
    g = _blc(grad, B, L, C, grad_blc)
    ge, ge_abs = np.zeros((n_rows, C)), np.zeros((n_rows, C))
    touched = np.zeros(n_rows, bool)
    for l, lv in enumerate(lvs):
        ok, rows, w, _, _ = corners(x, lv, align_corners, style)
        t = (w[:, :, None] * g[:, l][:, None, :])[ok]                                     # [n, 8, C]
        r = (lv['offset'] + rows[ok]).reshape(-1)
        np.add.at(ge, r, t.reshape(-1, C))
        np.add.at(ge_abs, r, np.abs(t).reshape(-1, C))
        touched[r] = True
        if terms is not None:
            terms.append((0.0, t))
    if terms is not None:
        terms.append((ge_abs.max(initial=0), np.zeros(0)))
    return ge + 0.0, touched


def input_backward(grad, x, emb, offsets, S, H, gridtype, align_corners, style=0, grad_blc=1, terms=None, dtype=np.float64):
    """-> grad_inputs [B, 3] float64: sum over levels, channels and corner pairs of grad * d out / d x (k_grid_input_bwd).
    dtype = np.float32 runs the same statements in float32 from the same cells and fractions: the float32 restatement that
    the kernel's error is measured against (4 x its error, the rule of test_gpu_grid_input_grad.py)."""
    lvs = fill_levels(offsets, S, H, gridtype)
    B, L, C = x.shape[0], len(lvs), emb.shape[1]
    g = _blc(grad, B, L, C, grad_blc).astype(dtype)
    emb = np.asarray(emb, dtype)
    gi, gi_abs = np.zeros((B, 3), dtype), np.zeros((B, 3), dtype)
    for l, lv in enumerate(lvs):
        ok, rows, _, f, wd = corners(x, lv, align_corners, style)
        wd = wd.astype(dtype)
        scale = dtype(lv['res'] - (0 if align_corners else 1))
        gv = (emb[lv['offset'] + rows] * g[:, l][:, None, :]).sum(axis=2)                 # [B, 8]
        for gd in range(3):
            others = [d for d in range(3) if d != gd]
            for idx in range(8):
                if (idx >> gd) & 1:
                    continue
                w = scale * wd[:, idx, others[0]] * wd[:, idx, others[1]]
                t = np.where(ok, w * (gv[:, idx | (1 << gd)] - gv[:, idx]), dtype(0))
                gi[:, gd] += t
                gi_abs[:, gd] += np.abs(t)
                if terms is not None:
                    terms.append((0.0, np.concatenate([t, np.where(ok, w, 0.0), np.where(ok, scale * wd[:, idx, others[0]], 0.0)])))
    if terms is not None:
        terms.append((gi_abs.max(initial=0), np.zeros(0)))
    return gi.astype(np.float64) + 0.0


def dyadic_ok(terms, frac_bits):
    """every recorded term is a multiple of 2^-frac_bits and every recorded sum |terms| is below 2^24 * 2^-frac_bits: every
    partial sum in any order is then an integer multiple of the unit below 2^24 units, i.e. an fp32 number"""
    unit = 2.0 ** -frac_bits
    for s, t in terms:
        q = np.asarray(t) / unit
        if not (np.all(q == np.rint(q)) and np.abs(q).max(initial=0) < 2 ** 24 and s / unit < 2 ** 24):
            return False
    return True


# ---------------------------------------------------------------------------------------------
# exact lattice cases
# ---------------------------------------------------------------------------------------------
PLS_EXACT, H_EXACT = 2.0, 16
BAD_ROWS = ([1.25, 0.5, 0.5], [0.5, -0.0625, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nan])


class Case:
    """One exact probe.  dup: 4096 samples drawn from 8 distinct lattice points.  small: tables and gradients in {-1, 0, 1}
    (the L = 16 cases, whose input gradient sums terms scaled by the resolution, up to 2^19)."""

    def __init__(self, C, gridtype, align, style, L=3, B=257, emb_half=False, grad_half=False, blc=1, dup=False, small=False,
                 log2=13, seed=0, tag='main'):
        self.C, self.gridtype, self.align, self.style, self.L, self.B = C, gridtype, align, style, L, B
        self.emb_half, self.grad_half, self.blc, self.dup, self.small, self.log2, self.seed, self.tag = \
            emb_half, grad_half, blc, dup, small, log2, seed, tag

    @property
    def id(self):
        return '%s-C%d-%s-%s-style%d-L%d-B%d' % (self.tag, self.C, self.gridtype, 'align' if self.align else 'noalign', self.style,
                                                   self.L, self.B)

    @property
    def gt(self):
        return 0 if self.gridtype == 'hash' else 1

    @property
    def S(self):
        return grid_S(PLS_EXACT)

    def offsets(self):
        return offsets_for(self.L, PLS_EXACT, H_EXACT, self.log2, self.align)

    def data(self):
        """x [B, 3] f32 on the 1/16 lattice, with rows outside [0, 1] or NaN first, last and at threads 255 / 256 where the
        batch reaches them; emb [rows, C] and grad [B, L, C] small integers (as fp32); pre: an integer pre-fill of the table
        gradient.  grad is returned in [B, L, C]; `layout` brings it to the case's."""
        rng = np.random.default_rng(1000 + self.seed)
        B, L, C = self.B, self.L, self.C
        if self.dup:
            pts = rng.integers(0, 17, (8, 3))
            assert len(np.unique(pts, axis=0)) == 8
            x = (pts[rng.integers(0, 8, B)] / 16.0).astype(np.float32)
        else:
            x = (rng.integers(0, 17, (B, 3)) / 16.0).astype(np.float32)
            if B >= 4:
                x[1], x[2] = [0, 0, 0], [1, 1, 1]
        bad = [i for i in (0, 255, 256, B - 1) if i < B] if B > 1 else []
        for k, i in enumerate(bad):
            x[i] = BAD_ROWS[k % 4]
        hi = 1 if (self.small or self.dup) else (8 if not self.emb_half else 4)
        n_rows = int(self.offsets()[-1])
        emb = rng.integers(-hi, hi + 1, (n_rows, C)).astype(np.float32)
        gmax = 1 if (self.small or self.dup) else 2
        grad = rng.integers(-gmax, gmax + 1, (B, L, C)).astype(np.float32)
        pre = rng.integers(-3, 4, (n_rows, C)).astype(np.float32)
        return x, emb, grad, pre, sorted(set(bad))

    def layout(self, a):
        """[B, L, C] -> the layout the case passes to the kernel ([B, L*C] or [L, B, C])"""
        return np.ascontiguousarray(a.reshape(self.B, self.L * self.C) if self.blc else a.transpose(1, 0, 2))

    def reference(self, check=False):
        x, emb, grad, pre, bad = self.data()
        off = self.offsets()
        tf, tb, ti = ([], [], []) if check else (None, None, None)
        a = (off, self.S, H_EXACT, self.gt, self.align, self.style)
        out = forward(x, emb, *a, out_blc=self.blc, terms=tf)
        ge, touched = backward(self.layout(grad), x, off, emb.shape[0], self.C, *a[1:], grad_blc=self.blc, terms=tb)
        gi = input_backward(self.layout(grad), x, emb, *a, grad_blc=self.blc, terms=ti)
        ref = dict(x=x, emb=emb, grad=self.layout(grad), pre=pre, bad=bad, off=off, out=out, ge=ge, touched=touched, gi=gi)
        if check:
            ref['terms'] = (tf, tb, ti)
        return ref

    def conditions(self, ref):
        """the exactness conditions of the module docstring; the table gradient is also called twice into one buffer and once
        into the pre-fill, so its bound is taken on 2 x the sums plus the pre-fill"""
        tf, tb, ti = ref['terms']
        assert dyadic_ok(tf, 12), 'forward'
        assert dyadic_ok([(2 * s + 3, t) for s, t in tb], 12), 'table backward'
        assert dyadic_ok(ti, 0 if self.align else 8), 'input backward'
        x = ref['x'][inside(ref['x'])]
        assert np.array_equal(x * 16, np.rint(x * 16))


def exact_cases():
    cases = []
    for C in (1, 2, 4, 8):
        for gridtype in ('hash', 'tiled'):
            for align in (True, False):
                for style in (0, 3):
                    cases.append(Case(C, gridtype, align, style, seed=len(cases)))
    k = 0
    for C in (2, 8):
        for gridtype in ('hash', 'tiled'):
            v = dict(C=C, gridtype=gridtype)
            for tag, kw in (('embf16', dict(emb_half=True, align=False, style=3)),
                            ('gradf16', dict(grad_half=True, align=False, style=0)),
                            ('bothf16', dict(emb_half=True, grad_half=True, align=True, style=3)),
                            ('lbc', dict(blc=0, align=False, style=3)),
                            ('L1', dict(L=1, align=False, style=3)),
                            ('L2', dict(L=2, align=True, style=0)),
                            ('L16', dict(L=16, align=True, style=3, small=True)),
                            ('B1', dict(B=1, align=False, style=0)),
                            ('B255', dict(B=255, align=True, style=3)),
                            ('B256', dict(B=256, align=False, style=3)),
                            ('dup', dict(B=4096, dup=True, align=False, style=3))):
                k += 1
                cases.append(Case(seed=100 + k, tag=tag, **v, **kw))
    return cases


def round_f16(a):
    """float64 -> nearest-even f16, as float32"""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float32)
