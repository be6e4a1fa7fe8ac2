"""GPU: error-map importance sampling -- nsr_draw_frame_batch_error, nsr_error_map_accumulate / _rebuild and
nsr_recon_loss_weighted against the NumPy restatement of tests/error_map_ref.py, through the C ABI and through ErrorMap.

Bars.  Everything integer (seg_frame, pix, rows, accumulators, prefixes) and err (a stated operation order) compare exactly.
weights: 1e-6 relative (five fp32 operations, two of them divisions).  Weighted loss against torch: 2e-6, the bar of the plain
loss; against nsr_recon_loss with weights 1: bit for bit; ray_err: 1 ulp of the per-ray sum."""
import numpy as np
import pytest
import torch

import error_map_ref as ER
import frame_batch_ref as FR
from helpers import render_setup, room_cameras

pytestmark = pytest.mark.gpu
SEED = 0x9e3779b97f4a7c15
W, H, CELL = 40, 27, 16                              # 3 x 2 cells, the edge cells 8 wide and 11 high
GUARD = 64


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class DevMap:
    """the device state of one ER.Map, driven through the C ABI"""

    def __init__(self, m, dev, guard=False):
        self.m, self.dev = m, dev
        self.bufs = {}
        for name, arr in (('err', m.err), ('acc_sum', m.acc_sum.view(np.int64)), ('acc_cnt', m.acc_cnt.view(np.int32)),
                          ('prefix', np.zeros((m.F, m.G), np.int64)), ('frame_prefix', np.zeros(m.F, np.int64))):
            t = T(arr, dev).reshape(-1)
            if guard:                               # garbage on both sides: 0x5a bytes
                buf = torch.full((t.numel() + 2 * GUARD,), 0, dtype=t.dtype, device=dev)
                buf.view(torch.uint8).fill_(0x5a)
                buf[GUARD:GUARD + t.numel()] = t
                self.bufs[name] = buf
                t = buf[GUARD:GUARD + t.numel()]
            setattr(self, name, t)

    def guards_intact(self):
        return all(bool((b[:GUARD].view(torch.uint8) == 0x5a).all()) and bool((b[-GUARD:].view(torch.uint8) == 0x5a).all())
                   for b in self.bufs.values())

    def grid(self):
        return self.m.F, self.m.w, self.m.h, self.m.cell

    def rebuild(self):
        from nerfstyle_amd import _lib as L
        L.check(L.lib().nsr_error_map_rebuild(*self.grid(), float(self.m.decay), float(self.m.quant_scale), L.p(self.err), L.p(self.acc_sum),
                                              L.p(self.acc_cnt), L.p(self.prefix), L.p(self.frame_prefix), L.stream()), 'rebuild')
        return self

    def accumulate(self, seg, pix, err, S, K):
        from nerfstyle_amd import _lib as L
        L.check(L.lib().nsr_error_map_accumulate(*self.grid(), L.p(seg), L.p(pix), L.p(err), S, K, L.p(self.acc_sum), L.p(self.acc_cnt),
                                                 L.stream()), 'accumulate')

    def draw(self, S, K, seq, fixed=None, frames_by_error=False, stream_id=0):
        from nerfstyle_amd import _lib as L
        dev = self.dev
        out = (torch.full((S,), -9, dtype=torch.int32, device=dev), torch.full((S * K,), -9, dtype=torch.int32, device=dev),
               torch.full((S * K,), -9, dtype=torch.int64, device=dev), torch.full((S * K,), -9.0, device=dev))
        L.check(L.lib().nsr_draw_frame_batch_error(*self.grid(), L.p(self.prefix), L.p(self.frame_prefix), float(self.m.uniform_mix),
                                                   int(frames_by_error), S, K, SEED, seq, None, stream_id, L.p(fixed), 0, L.p(out[0]),
                                                   L.p(out[1]), L.p(out[2]), L.p(out[3]), L.stream()), 'draw_frame_batch_error')
        return tuple(t.cpu().numpy() for t in out)

    def same_state(self):
        m = self.m
        return (np.array_equal(self.err.cpu().numpy().view(np.uint32), m.err.reshape(-1).view(np.uint32))
                and np.array_equal(_u64(self.acc_sum), m.acc_sum.reshape(-1)) and np.array_equal(self.acc_cnt.cpu().numpy().view(np.uint32), m.acc_cnt.reshape(-1))
                and np.array_equal(_u64(self.prefix), m.prefix.reshape(-1)) and np.array_equal(_u64(self.frame_prefix), m.frame_prefix))


def _decades_map(uniform_mix=0.1, zero_frame=1):
    """F = 3, masses spanning three decades, one frame's total 0"""
    m = ER.Map(3, W, H, CELL, uniform_mix=uniform_mix)
    rng = np.random.default_rng(0)
    m.err[:] = (10.0 ** rng.uniform(-3.0, 0.0, m.err.shape)).astype(np.float32)
    m.err[:, 0], m.err[:, -1] = 1.0, 1e-3
    if zero_frame is not None:
        m.err[zero_frame] = 0.0
    ER.rebuild(m)
    return m


def _check_draw(m, got, want, K):
    seg, pix, rows, weights = got
    w_seg, w_pix, w_rows, w_weights, by_cell, cell = want
    assert np.array_equal(seg, w_seg) and np.array_equal(pix, w_pix) and np.array_equal(rows, w_rows)
    rel = np.abs(weights.astype(np.float64) - w_weights) / w_weights
    print('weights: max relative difference %.3e' % rel.max())
    assert rel.max() <= 1e-6
    assert pix.min() >= 0 and pix.max() < m.P and rows.min() >= 0 and rows.max() < m.F * m.P
    # a pixel of the cell branch lies inside its cell's real extent
    x, y = pix[by_cell] % m.w, pix[by_cell] // m.w
    gx, gy = cell[by_cell] % m.gw, cell[by_cell] // m.gw
    assert np.all((x >= gx * m.cell) & (x < gx * m.cell + m.cw[gx]) & (y >= gy * m.cell) & (y < gy * m.cell + m.ch[gy]))
    return by_cell


# ---- 1. the draw -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,K', [(5, 64), (257, 1), (2, 1000)])
def test_draw_is_the_restated_draw(dev, S, K):
    m = _decades_map()
    d = DevMap(m, dev).rebuild()
    assert d.same_state() and int(m.prefix[1, -1]) == 0
    n_cell = 0
    for fbe in (False, True):
        got = d.draw(S, K, 11, frames_by_error=fbe)
        by_cell = _check_draw(m, got, ER.draw(m, S, K, SEED, 11, frames_by_error=fbe), K)
        n_cell += int(by_cell.sum())
        frame = np.repeat(got[0], K)
        assert not by_cell[frame == 1].any()                                 # the frame without mass: uniform pixels ...
        if not fbe:
            assert np.all(got[3][frame == 1] == 1.0)                         # ... of weight exactly 1
        if fbe:
            assert np.any(got[3] != d.draw(S, K, 11)[3])                     # the frame factor is in the weights
    assert n_cell > 0                                                        # the cell branch was taken
    # fixed frames with an invalid entry: its rays are uniform with weight 1 and rows of frame 0
    fixed = np.resize(np.asarray([2, 7, 0, 1, 2, -1], np.int32), S)
    for fbe in (False, True):
        got = d.draw(S, K, 12, fixed=T(fixed, dev), frames_by_error=fbe)
        _check_draw(m, got, ER.draw(m, S, K, SEED, 12, fixed_frames=fixed, frames_by_error=fbe), K)
        assert np.array_equal(got[0], fixed)
        bad = np.repeat((fixed < 0) | (fixed >= m.F), K)
        assert bad.any() and np.all(got[3][bad] == 1.0) and np.all(got[2][bad] == got[1][bad])
    # another rank draws another batch
    other = d.draw(S, K, 11, stream_id=1)
    _check_draw(m, other, ER.draw(m, S, K, SEED, 11, stream_id=1), K)
    assert not np.array_equal(other[1], d.draw(S, K, 11)[1])


# ---- 2. uniform_mix = 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frames_by_error', [False, True])
def test_uniform_mix_one_is_draw_frame_batch(dev, frames_by_error):
    from nerfstyle_amd import _lib as L
    m = _decades_map(uniform_mix=1.0)
    d = DevMap(m, dev).rebuild()
    for S, K, stream_id in ((5, 64, 0), (257, 1, 3)):
        seg, pix, rows = (torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S * K, dtype=torch.int32, device=dev),
                          torch.empty(S * K, dtype=torch.int64, device=dev))
        L.check(L.lib().nsr_draw_frame_batch(m.F, m.P, S, K, SEED, 21, None, stream_id, None, 0, L.p(seg), L.p(pix), L.p(rows), L.stream()),
                'draw_frame_batch')
        got = d.draw(S, K, 21, frames_by_error=frames_by_error, stream_id=stream_id)
        assert np.array_equal(got[0], seg.cpu().numpy()) and np.array_equal(got[1], pix.cpu().numpy()) and np.array_equal(got[2], rows.cpu().numpy())
        assert np.all(got[3] == 1.0)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], FR.draw(m.F, m.P, S, K, SEED, 21, stream_id=stream_id)))


# ---- 3. uniform_mix = 0, one cell with mass ----------------------------------------------------------------------------------------
def test_uniform_mix_zero_single_cell(dev):
    m = ER.Map(2, W, H, CELL, uniform_mix=0.0)
    m.err[:] = 0.0
    m.err[0, 5] = m.err[1, 2] = 0.37                                         # the ragged corner cell; the ragged column's top cell
    ER.rebuild(m)
    d = DevMap(m, dev).rebuild()
    fixed = np.asarray([0, 1, 1, 0], np.int32)
    got = d.draw(4, 300, 5, fixed=T(fixed, dev))
    want = ER.draw(m, 4, 300, SEED, 5, fixed_frames=fixed)
    by_cell = _check_draw(m, got, want, 300)
    assert by_cell.all()
    cells = m.cell_of(got[1])
    frame = np.repeat(fixed, 300)
    assert np.all(cells[frame == 0] == 5) and np.all(cells[frame == 1] == 2)
    assert len(np.unique(got[1][frame == 0])) > 70                           # 600 draws over the 88 pixels of the corner cell
    # the whole mass in 88 (128) of 1080 pixels: weights 88 / 1080 and 128 / 1080
    assert np.allclose(got[3][frame == 0], 88.0 / 1080.0, rtol=1e-6) and np.allclose(got[3][frame == 1], 128.0 / 1080.0, rtol=1e-6)


# ---- 4. prefix across scan chunks and past 32 bits ---------------------------------------------------------------------------------
def test_prefix_over_chunks_and_past_32_bits(dev):
    m = ER.Map(1, 504, 378, 8)
    assert m.G == 63 * 48 == 3024 and m.G % 256 != 0
    m.err[:] = 3.0
    m.err[0, 700] = np.nan
    m.err[0, 2900] = -2.0
    ER.rebuild(m)
    assert int(m.prefix[0, -1]) > 2 ** 32 and int(m.mass[0, 700]) == 0 and int(m.mass[0, 2900]) == 0
    d = DevMap(m, dev, guard=True).rebuild()
    assert np.array_equal(_u64(d.prefix), m.prefix.reshape(-1)) and np.array_equal(_u64(d.frame_prefix), m.frame_prefix)
    assert d.guards_intact()
    # several frames: the second launch's prefix of the totals, more frames than one chunk of it
    m2 = ER.Map(300, 24, 16, 8)
    m2.err[:] = np.random.default_rng(1).uniform(0.0, 4.0, m2.err.shape).astype(np.float32)
    ER.rebuild(m2)
    d2 = DevMap(m2, dev).rebuild()
    assert d2.same_state()


# ---- 5. accumulate and fold --------------------------------------------------------------------------------------------------------
def _rays_for_accumulate():
    """S = 20 segments of K = 1000 rays over frames 0..2 of 4: segment 3 names no frame; segments 4 to 6 sit whole in one cell
    (thousands of rays, every lane of a wave on one address), the rest is spread; NaN, negative and above-the-clamp errors throughout"""
    rng = np.random.default_rng(2)
    S, K = 20, 1000
    seg = rng.integers(0, 3, S).astype(np.int32)
    seg[3] = 5
    seg[4:7] = 2
    pix = rng.integers(0, W * H, S * K).astype(np.int32)
    one_cell = (rng.integers(16, 27, 3 * K) * W + rng.integers(32, 40, 3 * K)).astype(np.int32)           # the corner cell
    pix[4 * K:7 * K] = one_cell
    pix[7 * K:7 * K + 128] = 40 * 3 + np.arange(128) % 16                                                 # whole waves in cell 0
    err = (rng.random(S * K) ** 4 * 3.0).astype(np.float32)
    err[rng.integers(0, S * K, 300)] = np.nan
    err[rng.integers(0, S * K, 300)] = -0.5
    err[rng.integers(0, S * K, 300)] = 17.0
    err[rng.integers(0, S * K, 50)] = np.inf
    return S, K, seg, pix, err


def test_accumulate_and_fold(dev):
    S, K, seg, pix, err = _rays_for_accumulate()
    m = ER.Map(4, W, H, CELL, decay=0.3)
    m.err[:] = np.random.default_rng(3).uniform(0.1, 2.0, m.err.shape).astype(np.float32)
    ER.rebuild(m)
    start = m.err.copy()
    d = DevMap(m, dev, guard=True).rebuild()
    seg_d, pix_d, err_d = T(seg, dev), T(pix, dev), T(err, dev)
    d.accumulate(seg_d, pix_d, err_d, S, K)
    ER.accumulate(m, seg, pix, err, K)
    assert int(m.acc_cnt.max()) > 2000 and int(m.acc_cnt.sum()) < S * K - K
    assert d.same_state()                                                    # the accumulators before the fold
    acc = (d.acc_sum.clone(), d.acc_cnt.clone())
    touched = m.acc_cnt > 0
    d.rebuild()
    ER.rebuild(m)
    assert d.same_state() and d.guards_intact()
    assert not bool(d.acc_cnt.any()) and not bool(d.acc_sum.any())
    assert np.array_equal(m.err[~touched].view(np.uint32), start[~touched].view(np.uint32)) and (~touched).any()
    assert np.any(m.err[touched] != start[touched]) and not touched[3].any()
    err_1 = d.err.clone()
    # the same rays in another order (whole segments and the rays inside them): the same accumulators, bit for bit
    perm_s = np.random.default_rng(4).permutation(S)
    order = np.concatenate([s * K + np.random.default_rng(5 + s).permutation(K) for s in perm_s])
    d_p = DevMap(ER.Map(4, W, H, CELL, decay=0.3), dev)
    d_p.err.copy_(T(start, dev).reshape(-1))
    d_p.accumulate(T(seg[perm_s], dev), T(pix[order], dev), T(err[order], dev), S, K)
    assert torch.equal(d_p.acc_sum, acc[0]) and torch.equal(d_p.acc_cnt, acc[1])
    d_p.rebuild()
    assert torch.equal(d_p.err.view(torch.int32), err_1.view(torch.int32)) and torch.equal(d_p.prefix, d.prefix)
    # a second step on top of the first
    err2 = np.roll(err, 777)
    d.accumulate(seg_d, pix_d, T(err2, dev), S, K)
    d.rebuild()
    ER.accumulate(m, seg, pix, err2, K)
    ER.rebuild(m)
    assert d.same_state() and d.guards_intact()


# ---- 6. weighted loss --------------------------------------------------------------------------------------------------------------
def _loss_call(dev, rgb, cls, t_rgb, t_cls, pix, weight, want_err, ce_lambda=1e-3, plain=False):
    from nerfstyle_amd import _lib as L
    N, nc = rgb.shape[0], 0 if cls is None else cls.shape[1]
    g_rgb = torch.full_like(rgb, 7.0)
    g_cls = None if cls is None else torch.full_like(cls, 7.0)
    out = torch.full((3,), 7.0, device=dev)
    ray_err = torch.full((N,), 7.0, device=dev) if want_err else None
    ws = torch.empty(int(L.lib().nsr_recon_loss_workspace_bytes(N)) // 4, device=dev)
    if plain:
        L.check(L.lib().nsr_recon_loss(L.p(rgb), L.p(cls), N, nc, L.p(t_rgb), L.p(t_cls), L.p(pix), ce_lambda, 1.0, None, L.p(g_rgb),
                                       L.p(g_cls), L.p(out), L.p(ws), L.stream()), 'recon_loss')
    else:
        L.check(L.lib().nsr_recon_loss_weighted(L.p(rgb), L.p(cls), N, nc, L.p(t_rgb), L.p(t_cls), L.p(pix), L.p(weight), ce_lambda, 1.0,
                                                None, L.p(g_rgb), L.p(g_cls), L.p(ray_err), L.p(out), L.p(ws), L.stream()), 'recon_loss_weighted')
    return out, g_rgb, g_cls, ray_err


@pytest.mark.parametrize('with_classes', [True, False])
def test_weighted_loss(dev, with_classes):
    N, nc, P = 1000, 5, 3000
    g = torch.Generator().manual_seed(3)
    rgb = torch.rand(N, 3, generator=g).to(dev)
    cls = (torch.randn(N, nc, generator=g) * 2).to(dev) if with_classes else None
    t_rgb = torch.rand(P, 3, generator=g).to(dev)
    t_cls = torch.randint(0, nc, (P,), generator=g).to(dev) if with_classes else None
    pix = torch.randint(0, P, (N,), generator=g).to(dev)
    weight = (0.05 + 8.0 * torch.rand(N, generator=g) ** 3).to(dev)
    out, g_rgb, g_cls, ray_err = _loss_call(dev, rgb, cls, t_rgb, t_cls, pix, weight, True)
    # torch, fp64
    r64 = rgb.double().requires_grad_()
    c64 = cls.double().requires_grad_() if with_classes else None
    per_ray = ((r64 - t_rgb[pix].double()) ** 2).sum(1)
    exact = ((rgb - t_rgb[pix]).double() ** 2).sum(1)                        # of the fp32 differences the kernel forms
    want = (weight.double() * per_ray).sum() / (3 * N)
    if with_classes:
        ce = torch.logsumexp(c64, 1) - c64.gather(1, t_cls[pix][:, None])[:, 0]
        want = want + 1e-3 * (weight.double() * ce).sum() / N
    want.backward()
    want = want.detach()
    print('weighted loss %.6f, |got - want| %.3e, gradients %.3e' % (float(want.detach()), abs(float(out[0]) - float(want.detach())),
                                                                    float((g_rgb.double() - r64.grad).abs().max())))
    assert abs(float(out[0]) - float(want)) <= 2e-6
    assert float((g_rgb.double() - r64.grad).abs().max()) <= 2e-6
    if with_classes:
        assert float((g_cls.double() - c64.grad).abs().max()) <= 2e-6
        assert abs(float(out[1] + out[2]) - float(want)) <= 2e-6
    else:
        assert float(out[2]) == 0.0
    # ray_err: the unweighted per-ray sum to 1 ulp
    ulp = torch.abs(torch.nextafter(exact.float(), torch.full((N,), 9.0, device=dev)) - exact.float())
    print('ray_err: max |got - sum| / ulp %.3f' % float(((ray_err.double() - exact).abs() / ulp.double()).max()))
    assert bool(((ray_err.double() - exact).abs() <= ulp.double()).all()) and bool((ray_err != 7.0).all())
    # weights of exactly 1 (given, or absent): the plain loss bit for bit
    p_out, p_rgb, p_cls, _ = _loss_call(dev, rgb, cls, t_rgb, t_cls, pix, None, False, plain=True)
    for w1 in (torch.ones(N, device=dev), None):
        o, gr, gc, re = _loss_call(dev, rgb, cls, t_rgb, t_cls, pix, w1, w1 is None)
        assert torch.equal(o, p_out) and torch.equal(gr, p_rgb)
        assert gc is None and p_cls is None or torch.equal(gc, p_cls)
        assert re is None or torch.equal(re, ray_err)
    assert not torch.equal(out, p_out)


def test_recon_loss_host_layer(dev):
    from nerfstyle_amd.recon_loss import recon_loss
    N, P = 1000, 3000
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand(N, 3, generator=g).to(dev).requires_grad_()
    t_rgb = torch.rand(P, 3, generator=g).to(dev)
    pix = torch.randint(0, P, (N,), generator=g).to(dev)
    weight = (0.05 + 4.0 * torch.rand(N, generator=g)).to(dev)
    err = torch.empty(N, device=dev)
    loss = recon_loss(rgb, None, t_rgb, pix=pix, ray_weight=weight, ray_err_out=err)
    loss.backward()
    per_ray = ((rgb.detach() - t_rgb[pix]) ** 2).sum(1)
    assert abs(float(loss.detach()) - float((weight * per_ray).sum() / (3 * N))) <= 2e-6
    assert float((err - per_ray).abs().max()) <= 1e-6
    want_g = 2.0 * weight[:, None] * (rgb.detach() - t_rgb[pix]) / (3 * N)
    assert float((rgb.grad - want_g).abs().max()) <= 2e-6


# ---- 7. ErrorMap, and the captured loop --------------------------------------------------------------------------------------------
def _dataset(dev, intr, poses, F=4):
    from nerfstyle_amd.dataset import ResidentDataset
    rng = np.random.default_rng(8)
    images = np.broadcast_to(rng.random((F, 3, 1, 1)).astype(np.float32), (F, 3, intr.h, intr.w)).copy()
    images[:, :, ::7, ::5] = 0.9                                             # not flat: the per-ray errors differ
    return ResidentDataset(images, np.asarray(poses, np.float32)[:F], intr, 2.0, dev)


def test_error_map_object(dev):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ErrorMap, ResidentDataset
    rng = np.random.default_rng(9)
    F = 3
    ds = ResidentDataset(rng.random((F, 3, H, W)).astype(np.float32), np.asarray(room_cameras()['poses'], np.float32)[:F],
                         Intrinsics(H, W, 30.0, 30.0, 20.0, 13.5), 2.0, dev)
    em = ErrorMap(ds, cell=CELL, decay=0.2, uniform_mix=0.25)
    m = ER.Map(F, W, H, CELL, decay=0.2, uniform_mix=0.25)
    assert (em.gw, em.gh, em.G) == (m.gw, m.gh, m.G) and np.array_equal(_u64(em.prefix), m.prefix)
    assert em.acc_sum.dtype == torch.int64 and em.acc_cnt.dtype == torch.int32
    em.err.copy_(T((10.0 ** rng.uniform(-3, 0, (F, m.G))).astype(np.float32), dev))
    m.err[:] = em.err.cpu().numpy()
    em.rebuild()
    ER.rebuild(m)
    for f in range(F):
        assert np.allclose(em.pdf(f).numpy().reshape(-1), ER.pdf(m, f), rtol=1e-12, atol=0)
    seqdev = torch.tensor([4], dtype=torch.int32, device=dev)
    batch, wts = em.draw(5, 65, SEED, sequence=2, sequence_dev=seqdev, advance=True, frames_by_error=True, stream_id=1)
    want = ER.draw(m, 5, 65, SEED, 6, stream_id=1, frames_by_error=True)
    assert int(seqdev[0]) == 5 and (batch.S, batch.K) == (5, 65)
    assert np.array_equal(batch.seg_frame.cpu().numpy(), want[0]) and np.array_equal(batch.pix.cpu().numpy(), want[1])
    assert np.array_equal(batch.rows.cpu().numpy(), want[2]) and np.allclose(wts.cpu().numpy(), want[3], rtol=1e-6, atol=0)
    ptrs = [t.data_ptr() for t in (*batch[:3], wts)]
    again = em.draw(5, 65, SEED, sequence=2, sequence_dev=seqdev, frames=T(np.asarray([2, 2, 0, 1, 0], np.int32), dev), out=(batch, wts))
    assert again[0] is batch and again[1] is wts and ptrs == [t.data_ptr() for t in (*batch[:3], wts)]
    want = ER.draw(m, 5, 65, SEED, 7, fixed_frames=[2, 2, 0, 1, 0])
    assert np.array_equal(batch.pix.cpu().numpy(), want[1]) and np.allclose(wts.cpu().numpy(), want[3], rtol=1e-6, atol=0)
    ray_err = T(rng.random(5 * 65).astype(np.float32), dev)
    em.update(batch, ray_err)
    ER.accumulate(m, want[0], want[1], ray_err.cpu().numpy(), 65)
    ER.rebuild(m)
    assert np.array_equal(em.err.cpu().numpy().view(np.uint32), m.err.view(np.uint32)) and np.array_equal(_u64(em.prefix), m.prefix)
    # the state round trip
    em2 = ErrorMap(ds, cell=CELL)
    em2.load_state_dict(em.state_dict())
    assert torch.equal(em2.err, em.err) and torch.equal(em2.prefix, em.prefix) and torch.equal(em2.frame_prefix, em.frame_prefix)
    assert (em2.decay, em2.uniform_mix) == (0.2, 0.25)
    with pytest.raises(ValueError, match='another grid'):
        ErrorMap(ds, cell=8).load_state_dict(em.state_dict())


def test_captured_loop_replays_equal_eager(dev):
    """draw (advance) -> render_frames (no grad) -> weighted loss -> update, captured as one graph on one stream and replayed three
    times, against the same three steps run eagerly from the same state; no optimiser runs, so the render is a function of the batch"""
    from nerfstyle_amd.dataset import ErrorMap
    from nerfstyle_amd.graph import _ready_for_capture
    from nerfstyle_amd.recon_loss import recon_loss
    r, _, poses, intr, _ = render_setup(dev, nc=5, compute_dtype=torch.float16, contrast=16.0)
    r.cfg.density_scale = 40.0
    ds = _dataset(dev, intr, poses)
    P = ds.poses[:, :3, :].contiguous()
    S, K, init = 4, 96, 0.5
    em = ErrorMap(ds, cell=32, decay=0.5, uniform_mix=0.2, init=init)
    start = em.state_dict()
    seq = torch.zeros(1, dtype=torch.int32, device=dev)
    out = em.draw(S, K, SEED, sequence_dev=seq)
    err_buf = torch.zeros(S * K, device=dev)
    _ready_for_capture(r.model)

    def step():
        batch, wts = em.draw(S, K, SEED, sequence=3, sequence_dev=seq, advance=True, frames_by_error=True, out=out)
        with torch.no_grad(), r.occupancy_frozen():
            o = r.render_frames(P, batch)
            loss = recon_loss(o['rgb_map'], None, ds.target_rgb_rows, pix=batch.rows, ray_weight=wts, ray_err_out=err_buf)
        em.update(batch, err_buf)
        return loss

    def snapshot():
        return [t.clone() for t in (out[0].seg_frame, out[0].pix, out[1], em.err, em.prefix, em.frame_prefix)]
    eager, losses = [], []
    for _ in range(3):
        losses.append(float(step()))
        eager.append(snapshot())
    assert int(seq[0]) == 3 and not torch.equal(eager[0][1], eager[1][1])
    # the map moved only where rays fell
    touched = torch.zeros_like(em.err, dtype=torch.bool)
    for snap in eager:
        frame = snap[0].long().repeat_interleave(K)
        cellid = (snap[1].long() // intr.w // 32) * em.gw + (snap[1].long() % intr.w) // 32
        touched[frame, cellid] = True
    assert bool((em.err[~touched] == init).all()) and bool((~touched).any()) and bool((em.err[touched] != init).any())
    assert all(np.isfinite(v) and v > 0 for v in losses)
    # back to the start, capture (the warm-up step runs on a side stream and is undone), replay
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = step()
    em.load_state_dict(start)
    seq.zero_()
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(), eager[k]):
            assert torch.equal(got, want)
        assert float(loss_g) == losses[k]
