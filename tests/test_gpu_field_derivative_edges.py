"""GPU: nsr_field_density_gradient (field_normal.hip) and nsr_field_position_gradient (field_xgrad.hip) at their edges, on the
+-2 cube.  Inputs and references: tests/field_box_ref.py (proved on the CPU in tests/test_field_box_cpu.py).

  * shapes: M in {1, 15, 16, 17, 63, 64, 65, 513, 4609} (one sample, ragged and full tiles, one tile past a wave's and a
    workgroup's share, 10 workgroups: field_logical_block with nb % 8 = 2) on the grids min_res = 16 and min_res = 2 (levels
    whose size is no power of two next to fast ones: both instantiations of the row helpers); from M = 63 on NaN, +-inf and
    outside samples at slots 0, 7 and 15 of tiles, u == 0 and u == 1 samples on each axis.  Bars: density gradient rel-L2
    5e-3 (f16) / 3e-2 (bf16) against autograd of the rounding-emulating restatement, position gradient at most 4x the error
    of the same restatement in fp32, against fp64;
  * every level alone (the other fifteen levels' table rows zeroed), M = 65, against the same bars;
  * the device count: inside a tile, 0, M, above M, negative -- zero gradients from the count on, sigmas there untouched,
    a NaN guard band behind 3 M floats untouched;
  * the position gradient's perm: identity, reversed, the sample order's, and one naming slots at or past the count, with
    NaN in every enc_grad slot the kernel promises not to read;
  * M = 16 * 2048 * 32 + 17 (the 2048-workgroup cap, nine tiles per wave) against the same buffer in chunks of 4096, bit for bit;
  * the normaliser with gradients of order 1e-25 and 1e+25, and with finite components whose length is above FLT_MAX;
  * sigmas == NULL and a captured graph replayed twice, equal to the eager call bit for bit.

Measured on an MI355X: this module takes 20 s (the slowest case 2.7 s); figures in DESIGN.md "Per-axis box and the derivative
kernels' edges"."""
import ctypes

import numpy as np
import pytest
import torch

import field_box_ref as FB
from helpers import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = (1, 15, 16, 17, 63, 64, 65, 513, 4609)
DG_CONFIGS = [('f16', True), ('f16', False), ('bf16', True)]
DG_BAR = {'f16': 5e-3, 'bf16': 3e-2}
M_CAP = 16 * 2048 * 32 + 17

_MODELS, _REFS = {}, {}


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def _ref(min_res):
    if min_res not in _REFS:
        _REFS[min_res] = FB.field_ref(5, 1.0, min_res)
    return _REFS[min_res]


def _model(dev, min_res, dt, table_half):
    key = (min_res, dt, table_half)
    if key not in _MODELS:
        _MODELS[key] = FB.make_model(dev, _ref(min_res), FB.CUBE_MIN, FB.CUBE_SIZE, table_half, dt, min_res)
    return _MODELS[key]


def _dg(m, pts, cnt=None, sig=True, normalize=False, density_scale=1.0, guard=0):
    """(sigmas [M] pre-filled with -7 | None, grads [M,3], guard band)"""
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    sigmas = torch.full((M,), -7.0, device=pts.device) if sig else None
    buf = torch.full((3 * M + guard,), float('nan'), device=pts.device)
    desc = m._desc(density_scale)
    L.check(L.lib().nsr_field_density_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(m._mlp_flat()), L.p(pts), M, L.p(cnt),
                                               L.p(sigmas), L.p(buf), int(normalize), L.stream()), 'field_density_gradient')
    return sigmas, buf[:3 * M].view(M, 3), buf[3 * M:]


def _xg(m, pts, eg, cnt=None, perm=None, guard=0, fill=float('nan')):
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    buf = torch.full((3 * M + guard,), fill, device=pts.device)
    desc = m._desc(1.0)
    L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(pts), M, L.p(cnt), L.p(eg), L.p(perm),
                                                L.p(buf), L.stream()), 'field_position_gradient')
    return buf[:3 * M].view(M, 3), buf[3 * M:]


def _eg(M, good, seed=0):
    """(enc_grad for the reference, the same with NaN wherever the kernel must not look)"""
    eg = np.random.default_rng(70 + M + seed).standard_normal((M, 16, 4)).astype(np.float32)
    eg_in = eg.copy()
    eg_in[~good] = np.nan
    return eg, eg_in


def test_level_tables_have_fast_and_general_levels(dev):
    for min_res in (16, 2):
        m = _model(dev, min_res, 'f16', True)
        fast = FB.fast_levels(m._offsets_np, min_res)
        assert fast != 0 and fast != 0xFFFF, hex(fast)


@pytest.mark.parametrize('min_res', [16, 2])
@pytest.mark.parametrize('dt,table_half', DG_CONFIGS, ids=['%s-%s' % (c[0], 'tab16' if c[1] else 'tab32') for c in DG_CONFIGS])
@pytest.mark.parametrize('M', SHAPES)
def test_density_gradient_shapes(dev, M, dt, table_half, min_res):
    m, ref = _model(dev, min_res, dt, table_half), _ref(min_res)
    x, good = FB.edge_points(M)
    pts = T(x, dev)
    sig, g, _ = _dg(m, pts)
    with torch.no_grad():
        want_sig = m.field(pts, sigma_only=True)
    assert torch.equal(bits(sig), bits(want_sig))                                # the forward's bits, dead samples included
    g = g.cpu().numpy()
    assert np.isfinite(g).all() and not g[~good].any()
    want = FB.density_gradient_ref(ref, x, good, FB.CUBE_MIN, FB.CUBE_SIZE, dt, table_half)
    assert np.linalg.norm(want) > 0
    r = rel_l2(g, want)
    print('density gradient M=%d min_res=%d %s tables %s: rel-L2 %.3e (bar %g)' % (M, min_res, dt, 'f16' if table_half else 'f32', r, DG_BAR[dt]))
    assert r <= DG_BAR[dt]
    _, n, _ = _dg(m, pts, normalize=True)
    n = n.cpu().numpy()
    zero = np.all(n == 0, axis=1)
    assert np.array_equal(zero, np.all(g == 0, axis=1)) and not np.signbit(n[zero]).any()
    assert np.all(np.abs(np.linalg.norm(n[~zero].astype(np.float64), axis=1) - 1) <= 1e-5)


@pytest.mark.parametrize('min_res', [16, 2])
@pytest.mark.parametrize('table_half', [True, False], ids=['tab16', 'tab32'])
@pytest.mark.parametrize('M', SHAPES)
def test_position_gradient_shapes(dev, M, table_half, min_res):
    m, ref = _model(dev, min_res, 'f16', table_half), _ref(min_res)
    x, good = FB.edge_points(M)
    eg, eg_in = _eg(M, good)
    pts, eg_d = T(x, dev), T(eg_in, dev)
    got, _ = _xg(m, pts, eg_d)
    again, _ = _xg(m, pts, eg_d)
    perm = m.sample_order(pts)
    via_perm, _ = _xg(m, pts, eg_d, perm=perm)
    assert torch.equal(bits(got), bits(again)) and torch.equal(bits(got), bits(via_perm))
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and not g[~good].any()
    w64, w32 = (FB.position_gradient_ref(ref, x, eg, good, FB.CUBE_MIN, FB.CUBE_SIZE, table_half, d) for d in (torch.float64, torch.float32))
    e_k, e_32 = rel_l2(g[good], w64), rel_l2(w32, w64)
    print('position gradient M=%d min_res=%d tables %s: rel-L2 %.3e, fp32 restatement %.3e' % (M, min_res, 'f16' if table_half else 'f32', e_k, e_32))
    assert np.linalg.norm(w64) > 0 and e_32 > 0 and e_k <= 4 * e_32


@pytest.mark.parametrize('min_res', [16, 2])
def test_every_level_alone(dev, min_res):
    """level l's rows of the tables, the rest zero: a wrong cell_scale[l], level-to-lane map or corner pairing of one level
    has no fifteen good levels to hide behind"""
    M = 65
    m, ref = _model(dev, min_res, 'f16', False), _ref(min_res)
    x, good = FB.edge_points(M)
    eg, eg_in = _eg(M, good)
    pts, eg_d = T(x, dev), T(eg_in, dev)
    emb0 = (ref.emb_density.detach().clone(), ref.emb_color.detach().clone())
    te = m.table_elems
    saved = m.arena.detach()[:te].clone()
    try:
        for l in range(16):
            FB.keep_level(ref, emb0, l)
            a, b = int(ref.offsets[l]) * 4, int(ref.offsets[l + 1]) * 4
            with torch.no_grad():
                m.arena[:te] = 0
                m.arena[a:b] = saved[a:b]
            _, g, _ = _dg(m, pts)
            g = g.cpu().numpy()
            want = FB.density_gradient_ref(ref, x, good, FB.CUBE_MIN, FB.CUBE_SIZE, 'f16', False)
            assert np.all(np.abs(want).max(axis=0) > 0), l
            r = rel_l2(g, want)
            xg = _xg(m, pts, eg_d)[0].cpu().numpy()
            w64, w32 = (FB.position_gradient_ref(ref, x, eg, good, FB.CUBE_MIN, FB.CUBE_SIZE, False, d) for d in (torch.float64, torch.float32))
            e_k, e_32 = rel_l2(xg[good], w64), rel_l2(w32, w64)
            print('min_res=%d level %2d alone: density gradient rel-L2 %.3e (bar 5e-3), position gradient %.3e (fp32 restatement %.3e)'
                  % (min_res, l, r, e_k, e_32))
            assert np.isfinite(g).all() and np.isfinite(xg).all() and not g[~good].any() and not xg[~good].any()
            assert r <= DG_BAR['f16'], l
            assert np.all(np.abs(w64).max(axis=0) > 0) and e_k <= 4 * e_32, l
    finally:
        with torch.no_grad():
            m.arena[:te] = saved
            ref.emb_density.copy_(emb0[0])
            ref.emb_color.copy_(emb0[1])


@pytest.mark.parametrize('count', [37, 0, 100, 150, -3])
def test_device_count(dev, count):
    M, guard = 100, 64
    m = _model(dev, 16, 'f16', True)
    x, good = FB.edge_points(M)
    pts = T(x, dev)
    n = min(max(count, 0), M)
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
    live = good & (np.arange(M) < n)
    sig, g, band = _dg(m, pts, cnt, guard=guard)
    full_sig, full_g, _ = _dg(m, pts)
    assert torch.all(sig[n:] == -7.0) and torch.equal(bits(sig[:n]), bits(full_sig[:n]))
    assert torch.equal(bits(g[:n]), bits(full_g[:n])) and not g[n:].any() and not torch.signbit(g[n:]).any()
    assert torch.isnan(band).all() and band.numel() == guard
    assert n == 0 or float(g[:n].abs().sum()) > 0
    eg, eg_in = _eg(M, live)
    eg_d = T(eg_in, dev)
    xg, band = _xg(m, pts, eg_d, cnt, guard=guard)
    full_xg, _ = _xg(m, pts, T(_eg(M, good)[1], dev))
    assert torch.isfinite(xg).all() and torch.equal(bits(xg[:n]), bits(full_xg[:n])) and not xg[n:].any()
    assert torch.isnan(band).all() and band.numel() == guard


def test_position_gradient_perms(dev):
    M, count = 117, 101
    m = _model(dev, 16, 'f16', True)
    x, good = FB.edge_points(M)
    pts = T(x, dev)
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
    live = good & (np.arange(M) < count)
    eg, eg_in = _eg(M, live)
    eg_d = T(eg_in, dev)
    base, _ = _xg(m, pts, eg_d, cnt)
    assert torch.isfinite(base).all() and not base[T(~live, dev)].any() and float(base.abs().sum()) > 0
    tail = np.arange(count, M)
    ident = np.arange(M)
    rev = np.concatenate([np.arange(count)[::-1], tail])
    order = m.sample_order(pts, cnt)
    for name, p in (('identity', ident), ('reversed', rev), ('sample order', order)):
        p_d = p if torch.is_tensor(p) else T(p.astype(np.int32), dev)
        got, _ = _xg(m, pts, eg_d, cnt, p_d)
        assert torch.equal(bits(got), bits(base)), name
        assert torch.equal(bits(_xg(m, pts, eg_d, cnt, p_d)[0]), bits(base)), name
    # entries that name slots at or past the count (and past M): skipped, their own slots keep what the buffer held
    past = rev.copy()
    hit = [0, 7, 15, 16, 50, 100]
    past[hit] = [count, count + 1, M - 1, M, 2 ** 31 - 1, count + 3]
    got, _ = _xg(m, pts, eg_d, cnt, T(past.astype(np.int64).astype(np.uint32).view(np.int32), dev), fill=7.0)
    skipped = rev[hit]
    keep = np.ones(M, bool)
    keep[skipped] = False
    assert torch.all(got[T(skipped, dev)] == 7.0)
    assert torch.equal(bits(got[T(keep, dev)]), bits(base[T(keep, dev)]))
    assert not got[count:].any()


def test_chunks_equal_the_whole_buffer_at_the_workgroup_cap(dev):
    M, C = M_CAP, 4096
    assert (M + 15) // 16 > 2048 * 32                                            # 2048 workgroups, 33 tiles each: nine per wave
    m = _model(dev, 16, 'f16', True)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    pts = (torch.rand(M, 3, device=dev, generator=g) * 4.2 - 2.2).contiguous()   # a few per cent outside
    pts[5::1001, 1] = float('nan')
    pts[9::2003, 2] = float('inf')
    eg = torch.randn(M, 16, 4, device=dev, generator=g)
    sig, dg, _ = _dg(m, pts)
    xg, _ = _xg(m, pts, eg)
    assert torch.isfinite(dg).all() and torch.isfinite(xg).all() and float(dg.abs().sum()) > 0 and float(xg.abs().sum()) > 0
    sig_c, dg_c, xg_c = torch.empty_like(sig), torch.empty_like(dg), torch.empty_like(xg)
    for a in range(0, M, C):
        b = min(a + C, M)
        s, d, _ = _dg(m, pts[a:b])
        sig_c[a:b], dg_c[a:b] = s, d
        xg_c[a:b] = _xg(m, pts[a:b], eg[a:b])[0]
    assert torch.equal(bits(sig), bits(sig_c)) and torch.equal(bits(dg), bits(dg_c)) and torch.equal(bits(xg), bits(xg_c))


@pytest.mark.parametrize('order', [1e-25, 1e+25])
def test_normaliser_range(dev, order):
    """the `big` rescaling of the normaliser: the squares of components of order 1e-25 or 1e+25 leave the fp32 range"""
    M = 513
    m = _model(dev, 16, 'f16', True)
    x, good = FB.edge_points(M)
    pts = T(x, dev)
    _, g1, _ = _dg(m, pts)
    typical = float(g1.abs().max(dim=1).values[T(good, dev)].median())
    ds = order / typical
    _, g, _ = _dg(m, pts, density_scale=ds)
    _, n, _ = _dg(m, pts, density_scale=ds, normalize=True)
    g, n = g.cpu().numpy(), n.cpu().numpy()
    med = float(np.median(np.abs(g[good]).max(axis=1)))
    print('density_scale %.3e: median largest component %.3e' % (ds, med))
    assert order / 10 < med < order * 10
    assert np.isfinite(g).all() and np.isfinite(n).all()
    zero = np.all(g == 0, axis=1)
    assert np.array_equal(zero[~good], np.ones((~good).sum(), bool)) and zero.sum() < M // 3
    assert not n[zero].any() and not np.signbit(n[zero]).any()
    length = np.linalg.norm(n[~zero].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() <= 1e-5
    lg = np.linalg.norm(g[~zero].astype(np.float64), axis=1)
    assert np.abs(n[~zero] + g[~zero].astype(np.float64) / lg[:, None]).max() <= 1e-5


def test_normaliser_where_the_length_overflows(dev):
    """components that fp32 holds while |grad| is above FLT_MAX: density_scale puts one sample's largest component at 0.99 FLT_MAX
    (its second component is at least 0.15 of that, so |grad| > FLT_MAX); samples with a larger gradient are left out"""
    M = 513
    m = _model(dev, 16, 'f16', True)
    x, good = FB.edge_points(M)
    g1 = _dg(m, T(x, dev))[1].cpu().numpy().astype(np.float64)
    a = np.sort(np.abs(g1), axis=1)
    cand = good & (a[:, 2] > 0) & (a[:, 1] >= 0.2 * a[:, 2])
    i = int(np.flatnonzero(cand)[np.argmax(a[cand, 2])])
    keep = np.flatnonzero(a[:, 2] <= a[i, 2])
    j = int(np.flatnonzero(keep == i)[0])
    fmax = float(np.finfo(np.float32).max)
    ds = 0.99 * fmax / a[i, 2]
    pts = T(x[keep], dev)
    _, g, _ = _dg(m, pts, density_scale=ds)
    _, n, _ = _dg(m, pts, density_scale=ds, normalize=True)
    g, n = g.cpu().numpy().astype(np.float64), n.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(n).all()
    assert 0.98 * fmax < np.abs(g[j]).max() <= fmax and np.linalg.norm(g[j]) > fmax
    zero = np.all(g == 0, axis=1)
    assert not n[zero].any()
    assert np.abs(np.linalg.norm(n[~zero], axis=1) - 1).max() <= 1e-5
    assert np.abs(n[~zero] + g[~zero] / np.linalg.norm(g[~zero], axis=1)[:, None]).max() <= 1e-5


def test_null_sigmas_and_graph_replay(dev):
    M = 513
    m = _model(dev, 2, 'f16', True)
    x, good = FB.edge_points(M)
    pts = T(x, dev)
    cnt = torch.tensor([M - 9, 0], dtype=torch.int32, device=dev)
    eg_d = T(_eg(M, good & (np.arange(M) < M - 9))[1], dev)
    perm = m.sample_order(pts, cnt)
    sig_e, g_e, _ = _dg(m, pts, cnt)
    x_e, _ = _xg(m, pts, eg_d, cnt, perm)
    _, g_null, _ = _dg(m, pts, cnt, sig=False)
    assert torch.equal(bits(g_null), bits(g_e))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _dg(m, pts, cnt)
        _xg(m, pts, eg_d, cnt, perm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sig_g, g_g, _ = _dg(m, pts, cnt)
        x_g, _ = _xg(m, pts, eg_d, cnt, perm)
    for _ in range(2):
        sig_g.fill_(-7.0)
        g_g.fill_(7.0)
        x_g.fill_(7.0)
        graph.replay()
        assert torch.equal(bits(sig_g), bits(sig_e)) and torch.equal(bits(g_g), bits(g_e)) and torch.equal(bits(x_g), bits(x_e))
