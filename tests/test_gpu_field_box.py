"""GPU: the per-axis bounding box of nsr_field_desc (bbox_min[3], bbox_size[3]) through every field kernel but the streaming
render: sample order, forward (plain gather, sigma-only, lattice gather, with directions), both backwards (gradients-out +
lattice scatter with perm, run tracker without, colour-only), the density gradient and the position gradient.

1. Exact.  On the box EXACT_MIN / EXACT_SIZE of tests/field_box_ref.py (sizes 1, 8, 4: powers of two times the cube's 4) a
   call at x and a call on the +-2 cube at x' are the same computation from field_unit on (proved on the CPU:
   tests/test_field_box_cpu.py).  Two models with one state_dict must give: equal perm; bit-identical sigmas, rgbs, saved
   feats and enc_grad; table gradients per level and encoder within rel-L2 2e-5 and zero exactly where the other is zero,
   the four MLP blocks within 1.73e-6 / 1.59e-6 / 1.51e-6 / 1.52e-6 (the bars of test_gpu_table_scatter_carry.py and
   test_gpu_field_bwd_gout_exact.py: the same products, summed in an order the atomics choose); density and position
   gradients with grads_box[:, k] * (size_k / 4) == grads_cube[:, k] bit for bit.  M = 117 and M = 4609 (289 tiles, 10
   workgroups: field_logical_block with nb % 8 = 2), a device count 9 below M.
2. On the sample order's box (3, 4, 1.75), where u rounds differently from the cube's: forward and position gradient
   against the restatement at x' = 4 (x - min) / size - 2 (float64), gradients times 4 / size_k, with the bars of
   test_field_forward and test_position_gradient_kernel.  Backward and density gradient with the bars of
   test_field_backward and test_density_gradient against the same restatement on field_unit's own fp32 u of the box
   (NumPy, from bbox_min / bbox_size): evaluated at x' the reference is up to 1.2e-2 away from itself on that u -- a
   last-bit change of u flips a handful of ReLU masks, in plain fp32 too, see the comment in the test -- so no kernel can
   meet 5e-3 there; the distance to the x' evaluation is printed.  Every gradient against a reference whose y and z factors are exchanged must
   miss its bar tenfold.

Measured on an MI355X: this module takes 18 s; figures in DESIGN.md "Per-axis box and the derivative kernels' edges"."""
import ctypes

import numpy as np
import pytest
import torch

import field_box_ref as FB
from helpers import rel_l2

pytestmark = pytest.mark.gpu

TABLE_BAR = 2e-5
MLP_BAR = {'density_net': 1.73e-6, 'color1_net': 1.59e-6, 'color2_net': 1.51e-6, 'class_net': 1.52e-6}
DENSITY_SCALE = 1.5
EXACT_CASES = [('f16', True, 5), ('f16', False, 1), ('bf16', True, 13), ('bf16', False, 5)]
RATIO = (np.asarray(FB.EXACT_SIZE) / 4.0).astype(np.float32)[None]            # (1/4, 2, 1): exact factors

_PAIRS = {}


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def _pair(dev, dt, table_half, nc):
    key = (dt, table_half, nc)
    if key not in _PAIRS:
        ref = FB.field_ref(nc, 0.5)
        cube = FB.make_model(dev, ref, FB.CUBE_MIN, FB.CUBE_SIZE, table_half, dt)
        box = FB.make_model(dev, ref, FB.EXACT_MIN, FB.EXACT_SIZE, table_half, dt)
        sd_c, sd_b = cube.state_dict(), box.state_dict()
        assert all(torch.equal(sd_c[k], sd_b[k]) for k in sd_c)
        _PAIRS[key] = (cube, box)
    return _PAIRS[key]


def _forward(m, pts, cnt, perm=None, rgbs=True, feats=True):
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    sig = torch.full((M,), -7.0, device=pts.device)
    rgb = torch.full((M, m.out_channels), -7.0, device=pts.device) if rgbs else None
    f = torch.zeros(((M + 15) // 16) * 512, dtype=torch.int32, device=pts.device) if feats else None
    desc = m._desc(DENSITY_SCALE)
    L.check(L.lib().nsr_field_forward(ctypes.byref(desc), L.p(m._gather_tables()), L.p(m._mlp_flat()), L.p(pts), M, L.p(cnt), L.p(sig),
                                      L.p(rgb), L.p(f), L.p(perm), L.stream()), 'field_forward')
    return sig, rgb, f


def _backward(m, pts, cnt, perm, gs, gr):
    m.arena.grad = None
    m.grad_arena = None
    sig, rgb = m.field(pts, False, cnt, density_scale=DENSITY_SCALE, perm=perm)
    torch.autograd.backward([sig, rgb], [gs, gr])
    assert not m._spatial_scatter_unsupported
    return m.arena.grad.detach().cpu().numpy().copy()


def _compare_grads(m, tag, g_box, g_cube, mlp=True):
    from nerfstyle_amd.style_nerf import MLP_LAYOUT
    te, off = m.table_elems, m._offsets_np
    tb, tc = g_box[:te].reshape(m.rows, 2, 2), g_cube[:te].reshape(m.rows, 2, 2)
    assert np.isfinite(g_box).all() and np.isfinite(g_cube).all()
    assert np.array_equal(tb == 0, tc == 0), tag                                 # where one side is exactly zero, so is the other
    worst = 0.0
    for l in range(16):
        for e in range(2):
            w, g = tc[off[l]:off[l + 1], e], tb[off[l]:off[l + 1], e]
            if float(np.abs(w).sum()) == 0.0:
                assert not g.any()
                continue
            r = rel_l2(g, w)
            worst = max(worst, r)
            assert r <= TABLE_BAR, (tag, l, e, r)
    line = '%s | tables worst level rel-L2 %.3g (bar %g)' % (tag, worst, TABLE_BAR)
    for name, o, n in MLP_LAYOUT:
        w, g = g_cube[te + o: te + o + n], g_box[te + o: te + o + n]
        if not mlp:
            assert not w.any() and not g.any()
            continue
        assert float(np.abs(w).sum()) > 0
        r = rel_l2(g, w)
        line += ' %s %.3g' % (name, r)
        assert r <= MLP_BAR[name], (tag, name, r)
    print(line)


def _position_gradient(m, pts, cnt, ws, perm):
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    out = torch.full((M, 3), 7.0, device=pts.device)
    desc = m._desc(DENSITY_SCALE)
    L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(pts), M, L.p(cnt), L.p(ws), L.p(perm),
                                                L.p(out), L.stream()), 'field_position_gradient')
    return out


@pytest.mark.parametrize('M', [117, 4609])
@pytest.mark.parametrize('dt,table_half,nc', EXACT_CASES, ids=['%s-%s-nc%d' % (c[0], 'tab16' if c[1] else 'tab32', c[2]) for c in EXACT_CASES])
def test_box_equals_cube_exactly(dev, dt, table_half, nc, M):
    from nerfstyle_amd import _lib as L
    cube, box = _pair(dev, dt, table_half, nc)
    xc_h, xb_h, dead = FB.exact_points(M)
    xc, xb = T(xc_h, dev), T(xb_h, dev)
    count = M - 9
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
    live = ~dead & (np.arange(M) < count)
    tag = 'M=%d %s tables %s nc=%d' % (M, dt, 'f16' if table_half else 'f32', nc)

    # sample order
    perm = cube.sample_order(xc, cnt)
    assert torch.equal(perm, box.sample_order(xb, cnt))
    ph = perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(ph[:count]), np.arange(count))

    # forward: plain gather, sigma-only, with perm (the lattice gather on 16-bit tables)
    for m_, x_ in ((cube, xc), (box, xb)):
        d = m_._desc(DENSITY_SCALE)
        assert L.lib().nsr_field_forward_uses_lattice(ctypes.byref(d), 1, 0) == int(table_half)
    for p_, rgbs, feats in ((None, True, True), (None, False, False), (perm, True, True)):
        sc, rc, fc = _forward(cube, xc, cnt, p_, rgbs, feats)
        sb, rb, fb = _forward(box, xb, cnt, p_, rgbs, feats)
        assert torch.equal(bits(sc), bits(sb)), tag
        assert torch.all(sc[count:] == -7.0) and torch.isfinite(sc[:count]).all()
        if rgbs:
            assert torch.equal(bits(rc), bits(rb)), tag
            assert torch.isfinite(rc[:count]).all() and float(rc[:count, :3].std()) > 0
        if feats:
            assert torch.equal(fc, fb) and int((fc != 0).sum()) > 0, tag
        if p_ is None and rgbs:
            sig_plain, rgb_plain = sc, rc
        elif rgbs:
            assert torch.equal(bits(sc), bits(sig_plain)) and torch.equal(bits(rc), bits(rgb_plain))     # per sample, whatever the walk

    # backward with perm: gradients-out kernel + lattice scatter
    g = torch.Generator(device=dev)
    g.manual_seed(M + nc)
    gs = torch.randn(M, device=dev, generator=g) * 1e-2
    gr = torch.randn(M, 3 + nc, device=dev, generator=g)
    gc = _backward(cube, xc, cnt, perm, gs, gr)
    gb = _backward(box, xb, cnt, perm, gs, gr)
    eg_c, eg_b = cube._bwd_ws[:M * 64].view(M, 64), box._bwd_ws[:M * 64].view(M, 64)
    # every slot below the count is written: perm[:count] is a bijection of them, and the kernel stores zeros for a dead sample
    assert torch.equal(bits(eg_c[:count]), bits(eg_b[:count])), tag
    rows = torch.as_tensor(np.flatnonzero(live), device=dev)
    dead_rows = torch.as_tensor(np.flatnonzero(dead & (np.arange(M) < count)), device=dev)
    assert torch.isfinite(eg_c[:count]).all() and float(eg_c[rows].abs().sum()) > 0 and not eg_c[dead_rows].any()
    _compare_grads(cube, tag + ' perm', gb, gc)

    # position gradient on the encoder gradients just compared, with and without perm
    for p_ in (perm, None):
        pc = _position_gradient(cube, xc, cnt, cube._bwd_ws, p_).cpu().numpy()
        pb = _position_gradient(box, xb, cnt, box._bwd_ws, p_).cpu().numpy()
        assert np.isfinite(pc).all() and np.abs(pc[live]).sum() > 0
        assert not pc[~live].any() and not pb[~live].any()
        assert np.array_equal((pb * RATIO).view(np.uint32), pc.view(np.uint32)), tag
        nz = np.abs(pc[pc != 0])
        assert nz.min() > 2.0 ** -122 and nz.max() < 2.0 ** 120                # the factor is exact only inside the normal range

    # backward without perm: the run tracker
    _compare_grads(cube, tag + ' tracker', _backward(box, xb, cnt, None, gs, gr), _backward(cube, xc, cnt, None, gs, gr))

    # colour-only backward: perm, saved feats, no density table, no nets
    res = []
    for m_, x_ in ((cube, xc), (box, xb)):
        m_.train_density_table, m_.train_mlps = False, False
        try:
            res.append(_backward(m_, x_, cnt, perm, gs, gr))
            eg = m_._bwd_ws[:M * 64].view(M, 16, 4)
            assert not eg[:count, :, :2].any() and float(eg[rows][:, :, 2:].abs().sum()) > 0
            res.append(m_._bwd_ws[:M * 64].view(M, 64)[:count].clone())
        finally:
            m_.train_density_table, m_.train_mlps = True, True
    assert torch.equal(bits(res[1]), bits(res[3])), tag
    te = cube.table_elems
    assert not res[0][:te].reshape(-1, 2, 2)[:, 0].any() and not res[2][:te].reshape(-1, 2, 2)[:, 0].any()
    _compare_grads(cube, tag + ' colour-only', res[2], res[0], mlp=False)

    # density gradient
    sc, dc = cube.density_gradient(xc, m_dev=cnt, density_scale=DENSITY_SCALE)
    sb, db = box.density_gradient(xb, m_dev=cnt, density_scale=DENSITY_SCALE)
    assert torch.equal(bits(sc[:count]), bits(sb[:count])) and torch.equal(bits(sc[:count]), bits(sig_plain[:count]))
    dc, db = dc.cpu().numpy(), db.cpu().numpy()
    assert np.isfinite(dc).all() and not dc[~live].any() and not db[~live].any()
    assert (np.abs(dc[live]).max(axis=1) > 0).mean() > 0.99
    assert np.array_equal((db * RATIO).view(np.uint32), dc.view(np.uint32)), tag
    nz = np.abs(dc[dc != 0])
    assert nz.min() > 2.0 ** -122 and nz.max() < 2.0 ** 120
    # normals of the box: the normalisation of the BOX's gradient (the box is anisotropic: they are not the cube's)
    _, nb = box.density_gradient(xb, m_dev=cnt, density_scale=DENSITY_SCALE, normalize=True)
    nb = nb.cpu().numpy()
    zero = np.all(nb == 0, axis=1)
    assert np.array_equal(zero, np.all(db == 0, axis=1))
    lg = np.linalg.norm(db.astype(np.float64), axis=1)
    assert np.abs(np.linalg.norm(nb[~zero].astype(np.float64), axis=1) - 1).max() <= 1e-5
    assert np.abs(nb[~zero] + db[~zero] / lg[~zero, None]).max() <= 1e-5
    _, nc_ = cube.density_gradient(xc, m_dev=cnt, density_scale=DENSITY_SCALE, normalize=True)
    assert np.abs(nb - nc_.cpu().numpy()).max() > 1e-2                            # ... and they do differ from the cube's


def test_box_equals_cube_with_directions(dev):
    """nsr_field_forward_dirs (view-dependent colour) on the box and the cube: the same bits"""
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.style_nerf import StyleTCNerf
    M = 117
    xc_h, xb_h, dead = FB.exact_points(M)
    cube = StyleTCNerf(FB.model_cfg(FB.CUBE_SIZE), BBox.from_radius(2.0), 5, view_dependent=True)
    mn, sz = np.asarray(FB.EXACT_MIN), np.asarray(FB.EXACT_SIZE)
    box = StyleTCNerf(FB.model_cfg(FB.EXACT_SIZE), BBox(mn, mn + sz), 5, view_dependent=True)
    sd = cube.state_dict()
    g = torch.Generator().manual_seed(5)
    for k in ('x_density_embedder.embeddings', 'x_color_embedder.embeddings'):
        sd[k] = torch.rand(sd[k].shape, generator=g) - 0.5
    cube.load_state_dict(sd)
    box.load_state_dict(sd)
    cube, box = cube.to(dev), box.to(dev)
    d = np.random.default_rng(2).standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dirs = T(d, dev)
    cnt = torch.tensor([M - 9, 0], dtype=torch.int32, device=dev)
    with torch.no_grad():
        sc, rc = cube.field(T(xc_h, dev), m_dev=cnt, dirs=dirs)
        sb, rb = box.field(T(xb_h, dev), m_dev=cnt, dirs=dirs)
        _, r2 = cube.field(T(xc_h, dev), m_dev=cnt, dirs=-dirs)
    n = M - 9
    assert torch.equal(bits(sc[:n]), bits(sb[:n])) and torch.equal(bits(rc[:n]), bits(rb[:n]))
    assert torch.isfinite(rc[:n]).all() and not torch.equal(rc[:n], r2[:n])      # the directions do reach the colour


# ---- 2. the box that is not a power of two, against float64 -------------------------------------------------------------------
ODD_CASES = [('f16', True), ('f16', False), ('bf16', True)]
M_ODD = 4099                 # the sample count the bars of test_field_backward are stated at
_ODD = {}


def _odd(O, dev, dt, table_half):
    key = (dt, table_half)
    if key not in _ODD:
        ref = FB.field_ref(5, 0.5)
        m = FB.make_model(dev, ref, FB.ODD_MIN, FB.ODD_SIZE, table_half, dt)
        _ODD[key] = (m, ref)
    if 'pts' not in _ODD:
        x, dead, _ = FB.odd_points(M_ODD)
        _ODD['pts'] = (x, dead, FB.to_cube_f64(x, FB.ODD_MIN, FB.ODD_SIZE))
    return _ODD[key] + _ODD['pts']


@pytest.mark.parametrize('dt,table_half', ODD_CASES, ids=['%s-%s' % (c[0], 'tab16' if c[1] else 'tab32') for c in ODD_CASES])
def test_odd_box_against_the_restatement(O, dev, dt, table_half):
    m, ref, x, dead, xp = _odd(O, dev, dt, table_half)
    good = ~dead
    xp32 = np.where(np.isfinite(xp), xp, 3.0).astype(np.float32)                # the oracle's stand-in for NaN / inf: outside
    pts = T(x, dev)
    tag = 'odd box %s tables %s' % (dt, 'f16' if table_half else 'f32')
    factor = (4.0 / np.asarray(FB.ODD_SIZE))[None]
    swap = factor[:, [0, 2, 1]] / factor

    # forward: the bars of test_field_forward
    fp = O.FieldParams(ref.emb_density.detach().numpy(), ref.emb_color.detach().numpy(), ref.p_density.detach().numpy(),
                       ref.p_color1.detach().numpy(), ref.p_color2.detach().numpy(), ref.p_class.detach().numpy(), ref.offsets,
                       ref.pls, num_classes=ref.nc)
    out_e, _, logit_e = O.field_forward(fp, xp32, half=dt, table_half=table_half)
    out_f, _, _ = O.field_forward(fp, xp32, half=None, table_half=table_half)
    gs_h = (np.random.default_rng(14).standard_normal(M_ODD) * 1e-2).astype(np.float32)
    gr_h = np.random.default_rng(15).standard_normal((M_ODD, 8)).astype(np.float32)
    gs_h[dead], gr_h[dead] = 0, 0
    perm = m.sample_order(pts)
    m.arena.grad = None
    m.grad_arena = None
    sig, rgb = m.field(pts, False, perm=perm)
    rn, sn = rgb.detach().cpu().numpy(), sig.detach().cpu().numpy()
    tol_e, tol_f = (2e-3, 5e-3) if dt == 'f16' else (1e-2, 3e-2)
    e1, e2, e3 = rel_l2(rn[good], out_e[good]), rel_l2(rn[good], out_f[good]), float(np.abs(np.log(sn[good]) - logit_e[good]).max())
    print('%s | forward rel-L2 %.3g (bar %g), against fp32 %.3g (bar %g), logit %.3g' % (tag, e1, tol_e, e2, tol_f, e3))
    assert e1 < tol_e and e2 < tol_f and e3 < (2e-2 if dt == 'f16' else 1e-1)

    # backward (gradients-out + scatter).  The reference at x' forms its encoder input from x' in fp32; on one coordinate in
    # ten that differs from field_unit's u on the box by one unit of 2^-24.  Times the finest resolution, 4096, and a table
    # difference of order 0.5 that moves a finest-level feature by about 1e-4, which is enough to change the sign of a hidden
    # pre-activation that close to zero: a handful of the 64 x 4099 units per net.  Each flip changes its sample's gradient by a
    # whole term, tens of per cent, and one sample of 4099 changing by 30 % is 5e-3 in rel-L2.  Measured on the CPU on these
    # points WITHOUT any operand rounding (half=None, fp32 tables): the reference at x' differs from itself on field_unit's u
    # by 2.7e-3 .. 6.2e-3 per block, the same at every level of the tables (level 0: 8.7e-3, where the fractions move by
    # 1e-6), and five samples carry all of the density chain's difference; with the f16 emulation 2.2e-3 .. 1.2e-2.  It is
    # ReLU's discontinuity under a last-bit change of the position, in fp32 as much as in the emulation: no reference
    # evaluated at x' -- emulating, plain fp32 or float64 -- can hold a kernel that is handed x to test_field_backward's
    # 5e-3, whose reference forms u with the kernel's own operations.  The bars are therefore applied, as they stand, against
    # the restatement on field_unit's u, formed in NumPy from bbox_min / bbox_size with the kernel's three fp32 operations
    # (independent of the kernel: a wrong axis, size or minimum in the kernel still shows).  The distance to the x'
    # evaluation and the reference's own spread are printed beside it, not asserted.
    torch.autograd.backward([sig, rgb], [T(gs_h, dev), T(gr_h, dev)])
    assert not m._spatial_scatter_unsupported
    params = (ref.emb_density, ref.emb_color, ref.p_density, ref.p_color1, ref.p_color2, ref.p_class)

    def reference(u):
        for p_ in params:
            p_.grad = None
        if u is not None:
            ref.encoder_input = lambda pts_: u
        try:
            out_r, sig_r = ref(torch.tensor(xp32[good]), half=dt, table_half=table_half)
        finally:
            if u is not None:
                del ref.encoder_input
        ((sig_r[:, 0] * torch.tensor(gs_h[good])).sum() + (out_r * torch.tensor(gr_h[good])).sum()).backward()
        return [p_.grad.numpy().copy() for p_ in params]
    want_u = reference(torch.tensor(FB.unit_f32(x, FB.ODD_MIN, FB.ODD_SIZE)[good]))
    want_x = reference(None)
    ga = m.arena.grad.cpu().numpy()
    gt = ga[:m.table_elems].reshape(m.rows, 2, 2)
    gm = ga[m.table_elems:]
    tol = 5e-3 if dt == 'f16' else 3e-2
    got_all = [gt[:, 0], gt[:, 1], gm[0:3072], gm[3072:6144], gm[6144:12288], gm[12288:15360]]
    for name, got, wu, wx in zip(('density table', 'colour table', 'density', 'color1', 'color2', 'class'), got_all, want_u, want_x):
        r_u, r_x, spread = rel_l2(got, wu), rel_l2(got, wx), rel_l2(wu, wx)
        print('%s | backward %-13s rel-L2 %.3g (bar %g); at x\' %.3g, the reference against itself %.3g' % (tag, name, r_u, tol, r_x, spread))
        assert r_u < tol, name
    assert not np.any((gt[:, 0] != 0) & (want_u[0] == 0)) and not np.any((gt[:, 1] != 0) & (want_u[1] == 0))

    # density gradient
    bar = 5e-3 if dt == 'f16' else 3e-2
    _, dg = m.density_gradient(pts)
    dg = dg.cpu().numpy()
    # (as for the backward: at x' the reference differs from itself on field_unit's u by 6.7e-3 without any emulation and by
    # 2.4e-3 (f16 tables) / 6.9e-3 (fp32 tables) with it, so the bar is applied against the restatement on field_unit's u)
    want = FB.density_gradient_ref(ref, x, good, FB.ODD_MIN, FB.ODD_SIZE, dt, table_half)
    want_u = FB.density_gradient_ref(ref, x, good, FB.ODD_MIN, FB.ODD_SIZE, dt, table_half, own_unit=True)
    assert np.isfinite(dg).all() and not dg[dead].any()
    r_u, r, spread, rs = rel_l2(dg, want_u), rel_l2(dg, want), rel_l2(want_u, want), rel_l2(dg, want * swap)
    print('%s | density gradient rel-L2 %.3g (bar %g); at x\' %.3g, the reference against itself %.3g; against swapped factors %.3g'
          % (tag, r_u, bar, r, spread, rs))
    assert r_u <= bar and rel_l2(dg, want_u * swap) > 10 * bar and rs > 10 * bar

    # position gradient
    eg = np.random.default_rng(5).standard_normal((M_ODD, 16, 4)).astype(np.float32)
    eg_in = eg.copy()
    eg_in[dead] = np.nan
    from nerfstyle_amd import _lib as L
    out = torch.full((M_ODD, 3), 7.0, device=dev)
    desc = m._desc(1.0)
    L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(pts), M_ODD, None, L.p(T(eg_in, dev)),
                                                L.p(perm), L.p(out), L.stream()), 'field_position_gradient')
    xg = out.cpu().numpy()
    assert np.isfinite(xg).all() and not xg[dead].any()
    w64, w32 = (FB.position_gradient_ref(ref, x, eg, good, FB.ODD_MIN, FB.ODD_SIZE, table_half, d) for d in (torch.float64, torch.float32))
    e_k, e_32 = rel_l2(xg[good], w64), rel_l2(w32, w64)
    print('%s | position gradient rel-L2 %.3g (bar 4 x %.3g), against swapped factors %.3g' % (tag, e_k, e_32, rel_l2(xg[good], w64 * swap)))
    assert e_32 > 0 and e_k <= 4 * e_32 and rel_l2(xg[good], w64 * swap) > 10 * 4 * e_32
