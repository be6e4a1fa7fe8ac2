"""The spatially ordered table scatter (table_scatter.hip) on the block sequences its shift-carry has to get right.

Every case runs nsr_field_backward twice on identical inputs: with `perm` from nsr_sample_order (gradients-out MLP
kernel + lattice scatter) and without (the fused run-tracker kernel, which is the reference here), and compares the
table gradient PER LEVEL AND PER ENCODER:
  * rel-L2 <= 2e-5 where the reference's norm is non-zero (both sides sum the same fp32 products, in different orders);
  * exactly zero where the reference is zero;
  * the MLP gradients (the part of the arena behind the tables) agree to rel-L2 < 2e-5, the bar of
    test_gpu_field.py::test_sample_order_and_sorted_walk_equal_buffer_order.
Reference LLFF grid (16 levels, 16 .. 4096), f16 tables, f16 compute, nc = 5; case 1 once more with bf16 compute and
fp32 tables.

The synthetic cases are also checked against an fp64 NumPy trilinear scatter of a KNOWN per-sample encoder gradient:
only the colour table is trained, with unit upstream gradients on the colours, and the encoder gradient is the
[M][16] float4 buffer the gradients-out kernel hands to the scatter.  The NumPy scatter takes cell and fraction from
the same fp32 products as the kernels and sums in fp64; against the oracle's own fp32 encoder backward it stays within
rel-L2 1e-5 on every level (checked on the CPU on these positions: 1.2e-7 .. 2.4e-6, the largest where 1 500 samples
share one block and the oracle's fp32 sums are longest), and the kernel's fp32 sums carry the same kind of error (a
random walk of at most 1 500 roundings of 6e-8 each: ~2e-6), so the bar is the 2e-5 of the comparison above.

A launch gives every wave ONE 16-sample tile until the batch exceeds 262 144 samples, so a wave meets a block change
only where blocks hold fewer than 16 samples: the synthetic blocks hold 1 .. 5.  Of this file only test_marched_patch goes
past that size (its waves walk more than one tile), with one aggregate per level.  The walk of two and three tiles a wave --
the key, the lattices and the prefetches carried across a tile boundary -- is test_gpu_table_scatter_walk.py's; the
position builders and the fp64 scatter are shared with it (table_scatter_cases.py)."""
import numpy as np
import pytest
import torch

from helpers import rel_l2, room_cameras, small_scene
from table_scatter_cases import SYNTHETIC, np_trilinear_scatter, unit_of

pytestmark = pytest.mark.gpu

BAR = 2e-5
NC = 5


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _model(dev, dt='f16', table_dtype=None):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    from oracle import torch_port as TP
    ref = TP.Field(num_classes=NC, table_scale=0.5)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), NC, enc_dtype=table_dtype, use_dir=False,
                    compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16)
    sd = m.state_dict()
    sd.update({'x_density_embedder.embeddings': ref.emb_density.detach(), 'x_color_embedder.embeddings': ref.emb_color.detach(),
               'density_net.params': ref.p_density.detach(), 'color1_net.params': ref.p_color1.detach(),
               'color2_net.params': ref.p_color2.detach(), 'class_net.params': ref.p_class.detach()})
    m.load_state_dict(sd)
    return m.to(dev)


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev)


# ---------------------------------------------------------------------------------------------
# the two calls and their comparison
# ---------------------------------------------------------------------------------------------
def _backward(m, xyzs, counter, perm, gs, gr):
    m.arena.grad = None
    m.grad_arena = None
    sig, rgb = m.field(xyzs, False, counter, perm=perm)
    torch.autograd.backward([sig, rgb], [gs, gr])
    return m.arena.grad.detach().cpu().numpy().copy()


def _upstream(M, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    gs = torch.randn(M, device=dev, generator=g) * 1e-2
    gr = torch.randn(M, 3 + NC, device=dev, generator=g)
    return gs, gr


def _levels(m):
    off = m._offsets_np
    return [(l, int(off[l]), int(off[l + 1])) for l in range(16)]


def _check_per_level(m, got, want, what):
    """got / want: [rows, 2 encoders, 2 features]"""
    for l, a, b in _levels(m):
        for e in range(want.shape[1]):
            w, g = want[a:b, e], got[a:b, e]
            nw = float(np.linalg.norm(w.astype(np.float64)))
            if nw == 0.0:
                print('%s level %2d encoder %d: reference zero, |sorted| max %g' % (what, l, e, float(np.abs(g).max())))
                assert not g.any(), (what, l, e)
            else:
                r = rel_l2(g, w)
                print('%s level %2d encoder %d: rel-L2 %.3g' % (what, l, e, r))
                assert r <= BAR, (what, l, e, r)


def _sorted_vs_tracker(m, xyzs, counter, seed):
    M = xyzs.shape[0]
    gs, gr = _upstream(M, xyzs.device, seed)
    perm = m.sample_order(xyzs, m_dev=counter)
    g_tracker = _backward(m, xyzs, counter, None, gs, gr)
    g_sorted = _backward(m, xyzs, counter, perm, gs, gr)
    te = m.table_elems
    assert float(np.abs(g_tracker[:te]).sum()) > 0
    _check_per_level(m, g_sorted[:te].reshape(m.rows, 2, 2), g_tracker[:te].reshape(m.rows, 2, 2), 'sorted vs tracker')
    r = rel_l2(g_sorted[te:], g_tracker[te:])
    print('MLP gradients: rel-L2 %.3g' % r)
    assert r < 2e-5
    return perm


def _vs_numpy(O, m, pts, dev):
    """colour table only, unit upstream gradients; the encoder gradient is what the gradients-out kernel wrote"""
    xyzs = T(pts, dev)
    M = pts.shape[0]
    gs = torch.zeros(M, device=dev)
    gr = torch.ones(M, 3 + NC, device=dev)
    perm = m.sample_order(xyzs)
    m.train_density_table = False
    try:
        g = _backward(m, xyzs, None, perm, gs, gr)
        genc = m._bwd_ws[:M * 64].view(M, 16, 4).cpu().numpy()[:, :, 2:4].copy()
    finally:
        m.train_density_table = True
    u = unit_of(pts)
    live = np.all((u >= 0) & (u <= 1), axis=1)
    want = np_trilinear_scatter(O, u, live, genc, m._offsets_np, m.rows)
    got = g[:m.table_elems].reshape(m.rows, 2, 2)
    assert not got[:, 0].any()                                   # the density table is not trained
    assert float(np.abs(want).sum()) > 0
    _check_per_level(m, got[:, 1:2], want[:, None, :], 'sorted vs fp64 scatter')


@pytest.mark.parametrize('name', sorted(SYNTHETIC))
def test_synthetic_blocks(O, dev, model, name):
    """cases 1 - 5: x-runs (even -> odd carry, odd -> even flush, two carries in a row; interior, at u = 0, at u = 1),
    gaps of 2 and 5 blocks, the 2 x 2 Morton group (x moves while y changed: no carry), one block alone (also exactly
    16 and 17 samples), dead samples between x neighbours"""
    pts = SYNTHETIC[name]()
    assert pts.shape[0] < 8000
    u = unit_of(pts)
    assert np.all((u >= 0) & (u <= 1), axis=1).sum() >= min(16, pts.shape[0])
    if name == 'dead_between':
        assert (u[:, 0] > 1).sum() > 100
    if name in ('one_block_16', 'one_block_17'):
        assert pts.shape[0] == int(name[-2:])
    _sorted_vs_tracker(model, T(pts, dev), None, 11)
    _vs_numpy(O, model, pts, dev)


def test_x_runs_bf16_compute_fp32_tables(O, dev):
    m = _model(dev, 'bf16', torch.float32)
    pts = SYNTHETIC['x_runs']()
    _sorted_vs_tracker(m, T(pts, dev), None, 12)


@pytest.fixture(scope='module')
def marched_patch(O, dev):
    """64 x 64 pixels of room pose 0 through the real march: real block populations"""
    from nerfstyle_amd import raymarching as R
    c = room_cameras()
    _, bits = small_scene()
    ys, xs = np.meshgrid(np.arange(157, 221), np.arange(220, 284), indexing='ij')
    pix = (ys * c['w'] + xs).reshape(-1)
    ro, rd = O.generate_rays(np.asarray(c['poses'][0], np.float32), c['w'], c['h'], c['fl_x'], c['fl_y'], c['cx'], c['cy'], 3,
                             pix_indices=pix)[:2]
    aabb = T(np.array([-2, -2, -2, 2, 2, 2], np.float32), dev)
    near, far = R.near_far_from_aabb(T(ro, dev), T(rd, dev), aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    xyzs = R.march_rays_train_nosync(T(ro, dev), T(rd, dev), 2.0, T(bits, dev), 2, 128, near, far, 4096 * 160, counter, 0., 1024)[0]
    cnt = int(counter[0])
    assert 4096 * 8 < cnt < xyzs.shape[0]
    xyzs[cnt:] = float('nan')                                   # capacity tail: never read
    return xyzs, counter, cnt


def test_marched_patch(O, dev, model, marched_patch):
    """case 6: the same comparison on a dense patch"""
    xyzs, counter, cnt = marched_patch
    _sorted_vs_tracker(model, xyzs, counter, 13)


def test_device_count_below_capacity(O, dev, model):
    """case 7: m_dev below M -- the slots behind the count hold live positions with gradients and must not be walked"""
    pts = SYNTHETIC['x_runs']()
    M = pts.shape[0]
    cnt = (M - 333) // 16 * 16 - 5                              # ends inside a tile
    assert cnt % 16 != 0
    xyzs = T(pts, dev)
    counter = torch.tensor([cnt, 0], dtype=torch.int32, device=dev)
    perm = _sorted_vs_tracker(model, xyzs, counter, 14)
    ph = perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(ph[:cnt]), np.arange(cnt))
    # ... and the result is the one of the truncated batch
    gs, gr = _upstream(M, dev, 14)
    g_full = _backward(model, xyzs, counter, perm, gs, gr)
    g_cut = _backward(model, xyzs[:cnt].contiguous(), None, model.sample_order(xyzs[:cnt].contiguous()), gs[:cnt].contiguous(),
                      gr[:cnt].contiguous())
    te = model.table_elems
    _check_per_level(model, g_full[:te].reshape(model.rows, 2, 2), g_cut[:te].reshape(model.rows, 2, 2), 'count vs truncated')
