"""GPU: the fused SSIM metric and D-SSIM loss (nsr_ssim, nerfstyle_amd/ssim.py) against the fp64 restatement of the definition
(tests/ssim_ref.py): value, per-channel means, map and gradient at the shapes where the kernel can go wrong, both paddings,
strides and pitches read in place; determinism, graph capture, untouched memory, the autograd plumbing, the term inside
StyleCriterion and one training render end to end.

Tolerances.  They are not taken from the kernel: the restatement itself, evaluated in f32 instead of fp64 on the CPU (torch
conv2d), differs from fp64 over these image kinds at 37x21, 64x64 and 378x504 by at most
    value 4.1e-7      gradient, relative L2 1.7e-5      map, absolute 2.2e-4 (the near-identical pair; 'constant' 1.3e-4,
                                                             'partly' 3.8e-5)
(ssim_ref.ssim_ref(dtype=torch.float32) against dtype=torch.float64).  The map is the hardest of the three: G*(x x) - mu_x^2
cancels to ~1e-3 between numbers of size ~0.4, each carrying a few 1e-8.  The bounds below were fixed before the kernel existed; it meets
the map bound because it forms the variances from the window sums of x - 1/2 (csrc/ssim.hip, ss_eval)."""
import functools

import numpy as np
import pytest
import torch

import ssim_ref as R
from helpers import small_scene

pytestmark = pytest.mark.gpu

VALUE_TOL, MAP_TOL, GRAD_TOL = 1e-5, 1e-4, 3e-4          # absolute, absolute, relative L2


def _T():
    from nerfstyle_amd.ssim import TILE
    return TILE


def _shapes():
    T = _T()
    return [(1, 1), (3, 4), (5, 16), (11, 11), (T, T), (T + 1, T - 1), (37, 21), (2 * T + 5, 3 * T + 11), (378, 504)]


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """[(kind, img, target, {padding: fp64 restatement})], computed once and shared"""
    out = []
    for kind, x, y in R.image_pairs(H, W, seed=H * 1000 + W):
        pads = ['same'] + (['valid'] if H >= 11 and W >= 11 else [])
        out.append((kind, x, y, {p: R.ssim_ref(x, y, p) for p in pads}))
    return out


def _compare(tag, ref, value, channels, smap, grad):
    dv = abs(float(value) - float(ref['value']))
    dc = float(np.abs(np.asarray(channels, np.float64) - ref['channels']).max())
    dm = float(np.abs(np.asarray(smap, np.float64) - ref['map']).max())
    dg = R.rel_l2(grad, ref['grad'])
    print('{:40s} value {:.6f} |dv| {:.2e} |dch| {:.2e} |dmap| {:.2e} grad rel L2 {:.2e}'.format(tag, float(value), dv, dc, dm, dg))
    assert dv <= VALUE_TOL and dc <= VALUE_TOL, tag
    assert dm <= MAP_TOL, tag
    assert dg <= GRAD_TOL, tag


def _run(dev, x, y, padding, H=None, W=None):
    from nerfstyle_amd import ssim as S
    xt = (x if torch.is_tensor(x) else torch.tensor(x, device=dev)).requires_grad_(True)
    yt = y if torch.is_tensor(y) else torch.tensor(y, device=dev)
    value, smap = S.ssim(xt, yt, H, W, padding=padding, return_map=True)
    assert value.dtype == torch.float64 and value.dim() == 0 and value.device.type == 'cuda'
    channels = S.channel_means(value)
    value.backward()
    return value.detach().cpu(), channels.cpu().numpy(), smap.cpu().numpy(), xt.grad


def test_shapes_cover_the_tile_edges():
    T = _T()
    assert T == 32 and (T, T) in _shapes() and (T + 1, T - 1) in _shapes() and (2 * T + 5, 3 * T + 11) in _shapes()


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: '{}x{}'.format(*s))
def test_against_the_fp64_restatement(dev, shape):
    H, W = shape
    for kind, x, y, refs in _case(H, W):
        for padding, ref in refs.items():
            value, channels, smap, grad = _run(dev, x, y, padding)
            assert smap.shape == (H, W, 3) and grad.shape == (H, W, 3) and grad.dtype == torch.float32
            if padding == 'valid':
                border = np.ones((H, W), bool)
                border[5:H - 5, 5:W - 5] = False
                assert np.count_nonzero(smap[border]) == 0 and np.count_nonzero(smap[~border]) == 3 * (H - 10) * (W - 10)
            _compare('{}x{} {} {}'.format(H, W, kind, padding), ref, value, channels, smap, grad.cpu().numpy())
    if shape == (11, 11):
        assert np.count_nonzero(_case(11, 11)[0][3]['valid']['map']) == 3          # one counted pixel per channel
    near = [c for c in _case(H, W) if c[0] == 'near'][0]
    if H * W >= 37 * 21:
        assert 0.95 < float(near[3]['same']['value']) < 0.995              # the near-identical pair is one


def test_strides_and_a_pitched_target_read_in_place(dev):
    """126x168: img as the renderer's rows [H*W,3], target a patch of a larger stride-4 frame, frame.view(Hf,Wf,4)[y0:y1, x0:x1]"""
    from nerfstyle_amd import ssim as S
    H, W, Hf, Wf, y0, x0 = 126, 168, 140, 200, 9, 17
    for kind, x, y, refs in _case(H, W):
        frame = torch.full((Hf * Wf, 4), -7.0, device=dev)
        patch = frame.view(Hf, Wf, 4)[y0:y0 + H, x0:x0 + W]
        patch[:, :, :3] = torch.tensor(y, device=dev)
        before = frame.clone()
        t, h, w, stride, pitch = S._geometry('target', patch, None, None)
        assert (h, w, stride, pitch) == (H, W, 4, Wf) and t.data_ptr() == patch.data_ptr()      # in place
        rows = torch.tensor(x, device=dev).view(H * W, 3)
        assert S._geometry('img', rows, H, W)[3:] == (3, W)
        for padding, ref in refs.items():
            value, channels, smap, grad = _run(dev, rows.clone(), patch, padding, H, W)
            assert grad.shape == (H * W, 3)
            _compare('126x168 pitched {} {}'.format(kind, padding), ref, value, channels, smap, grad.view(H, W, 3).cpu().numpy())
        # and the other way round: a stride-4 pitched img (its gradient has a zero fourth float), a stride-3 target
        img4 = torch.full((Hf, Wf, 4), 3.0, device=dev)
        img4[y0:y0 + H, x0:x0 + W, :3] = torch.tensor(x, device=dev)
        leaf = img4.clone().requires_grad_(True)
        v = S.ssim(leaf[y0:y0 + H, x0:x0 + W], torch.tensor(y, device=dev).view(-1, 3), H, W)
        v.backward()
        ref = refs['same']
        assert abs(float(v.detach()) - float(ref['value'])) <= VALUE_TOL
        g = leaf.grad
        assert R.rel_l2(g[y0:y0 + H, x0:x0 + W, :3].cpu().numpy(), ref['grad']) <= GRAD_TOL
        assert float(g[..., 3].abs().max()) == 0 and float(g[:y0].abs().max()) == 0 and float(g[:, :x0].abs().max()) == 0
        # untouched: the fourth floats and everything outside the patch keep their bits
        assert torch.equal(frame, before)


def test_identical_images(dev):
    """value within 1e-6 of 1; the gradient, zero in exact arithmetic, is bounded by FACTOR = 4 times what the f32 restatement
    leaves at the same input (max abs)"""
    FACTOR = 4.0
    for H, W in ((37, 21), (2 * _T() + 5, 3 * _T() + 11)):
        x = R.pattern(H, W, 5)
        f32 = R.ssim_ref(x, x, 'same', dtype=torch.float32)
        for padding in ('same', 'valid'):
            value, channels, smap, grad = _run(dev, x, x.copy(), padding)
            bound = FACTOR * float(np.abs(R.ssim_ref(x, x, padding, dtype=torch.float32)['grad']).max())
            print('identical {}x{} {}: 1 - value {:.2e}, max |grad| {:.2e} (f32 restatement x {}: {:.2e})'.format(
                H, W, padding, 1.0 - float(value), float(grad.abs().max()), FACTOR, bound))
            assert abs(float(value) - 1.0) <= 1e-6 and np.abs(channels - 1.0).max() <= 1e-6
            assert float(grad.abs().max()) <= bound
        assert float(np.abs(f32['grad']).max()) > 0


def test_two_calls_are_bit_identical(dev):
    H, W = 2 * _T() + 5, 3 * _T() + 11
    _, x, y, _ = _case(H, W)[0]
    for padding in ('same', 'valid'):
        a, b = _run(dev, x, y, padding), _run(dev, x, y, padding)
        assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert float(a[3].abs().max()) > 0


def _direct(dev, x_rows, y_rows, H, W, coef, scale, valid=0):
    """nsr_ssim itself with a guarded gradient buffer -> (out [4], grad [H*W,3])"""
    from nerfstyle_amd import _lib as L
    guard = 64
    buf = torch.full((H * W * 3 + 2 * guard,), 123.0, device=dev)
    grad = buf[guard:guard + H * W * 3]
    out = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib().nsr_ssim_workspace_bytes(H, W, 1)) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().nsr_ssim(x_rows.data_ptr(), x_rows.shape[1], W, y_rows.data_ptr(), y_rows.shape[1], W, H, W, valid, coef,
                             L.p(scale), L.p(out), None, grad.data_ptr(), L.p(ws), L.stream()), 'ssim')
    torch.cuda.synchronize()
    assert float(buf[:guard].min()) == 123.0 == float(buf[:guard].max()) and float(buf[-guard:].min()) == 123.0 == float(buf[-guard:].max())
    return out, grad.view(H * W, 3).clone()


def test_grad_carries_exactly_coef_times_scale_and_spares_the_fourth_float(dev):
    H, W = 37, 21
    _, x, y, _ = _case(H, W)[0]
    x4 = torch.tensor(R.pack(x, 4, fill=9.0), device=dev).view(H * W, 4)
    y3 = torch.tensor(y, device=dev).view(H * W, 3)
    before = x4.clone()
    out1, unit = _direct(dev, x4, y3, H, W, 1.0, None)
    scale = torch.tensor(1.7, device=dev)
    out2, scaled = _direct(dev, x4, y3, H, W, -0.37, scale)
    assert torch.equal(out1, out2)
    cs = torch.tensor(-0.37, dtype=torch.float32, device=dev) * scale
    assert torch.equal(scaled, cs * unit) and float(unit.abs().max()) > 0
    assert torch.equal(x4, before) and float(x4[:, 3].min()) == 9.0
    assert abs(float(out1[0]) - float(out1[1:].mean())) < 1e-15


def test_graph_capture_replays_with_new_contents_and_scale(dev):
    from nerfstyle_amd.ssim import dssim_loss
    H, W = 37, 53
    pairs = R.image_pairs(H, W, seed=7)
    tgt = torch.tensor(pairs[0][2], device=dev).view(-1, 3)
    p = torch.tensor(pairs[0][1], device=dev).view(-1, 3).requires_grad_(True)
    p.grad = torch.zeros_like(p)
    scale = torch.tensor(2.0, device=dev)

    def body():
        return dssim_loss(p.view(H, W, 3), tgt.view(H, W, 3), lam=0.2, factor=0.5, scale=scale, backward=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = body()
    # new image contents and a changed scale, through the same graph
    with torch.no_grad():
        p.copy_(torch.tensor(pairs[1][1], device=dev).view(-1, 3))
        scale.fill_(3.0)
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    q = torch.tensor(pairs[1][1], device=dev).view(-1, 3).requires_grad_(True)
    loss_e = dssim_loss(q.view(H, W, 3), tgt.view(H, W, 3), lam=0.2, factor=0.5, scale=torch.tensor(3.0, device=dev), backward=True)
    assert loss_e.dtype == torch.float32 and not loss_e.requires_grad
    assert torch.equal(loss_g, loss_e) and torch.equal(p.grad, q.grad) and float(q.grad.abs().max()) > 0
    ref = R.ssim_ref(pairs[1][1], pairs[1][2], 'same')
    assert abs(float(loss_e) - 0.5 * 3.0 * 0.2 * (1.0 - float(ref['value']))) <= 0.3 * VALUE_TOL + 1e-7
    assert R.rel_l2(q.grad.view(H, W, 3).cpu().numpy(), -0.5 * 3.0 * 0.2 * ref['grad']) <= GRAD_TOL


def test_autograd_plumbing(dev):
    from nerfstyle_amd import ssim as S
    H, W = 37, 21
    _, x, y, refs = _case(H, W)[0]
    ref = refs['same']
    yt = torch.tensor(y, device=dev)
    # a renderer-style [N,3] leaf
    rows = torch.tensor(x, device=dev).view(-1, 3).requires_grad_(True)
    v = S.ssim(rows, yt.view(-1, 3), H, W)
    v.backward()
    assert rows.grad.shape == (H * W, 3) and R.rel_l2(rows.grad.view(H, W, 3).cpu().numpy(), ref['grad']) <= GRAD_TOL
    g1 = rows.grad.clone()
    rows.grad = None
    (S.ssim(rows, yt.view(-1, 3), H, W) * 3.0).backward()
    assert torch.allclose(rows.grad, 3.0 * g1, rtol=1e-6, atol=0)
    # no gradient wanted: no gradient buffer, the same value
    v0 = S.ssim(rows.detach(), yt.view(-1, 3), H, W)
    assert v0.grad_fn is None and torch.equal(v0, v.detach())
    # half-precision images get a gradient of their own dtype (the kernel reads their f32 conversion)
    for dt in (torch.bfloat16, torch.float16):
        xh = torch.tensor(x, device=dev).to(dt).requires_grad_(True)
        S.ssim(xh, yt).backward()
        assert xh.grad.dtype == dt and xh.grad.shape == (H, W, 3)
        r16 = R.ssim_ref(xh.detach().float().cpu().numpy(), y, 'same')
        assert R.rel_l2(xh.grad.float().cpu().numpy(), r16['grad']) <= (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11)
    # the map
    _, smap = S.ssim(torch.tensor(x, device=dev), yt, return_map=True)
    assert smap.shape == (H, W, 3) and smap.dtype == torch.float32 and not smap.requires_grad
    # the loss and its module
    leaf = torch.tensor(x, device=dev).requires_grad_(True)
    loss = S.DSSIM(lam=0.2)(leaf, yt)
    assert loss.dtype == torch.float32 and abs(float(loss) - 0.2 * (1.0 - float(ref['value']))) <= VALUE_TOL
    loss.backward()
    assert R.rel_l2(leaf.grad.cpu().numpy(), -0.2 * ref['grad']) <= GRAD_TOL
    # metrics: PSNR from torch's MSE, SSIM of the 'valid' form
    m = S.frame_metrics(torch.tensor(x, device=dev), yt)
    mse = torch.mean((torch.tensor(x, device=dev) - yt) ** 2)
    assert m.shape == (2,) and m.dtype == torch.float64 and m.device.type == 'cuda'
    assert abs(float(m[0]) - float(-10.0 * torch.log(mse) / np.log(10.0))) < 1e-4
    assert abs(float(m[1]) - float(refs['valid']['value'])) <= VALUE_TOL
    with pytest.raises(ValueError, match='valid'):
        S.ssim(torch.rand(10, 12, 3, device=dev), torch.rand(10, 12, 3, device=dev), padding='valid')


def test_style_criterion_ssim_lambda(dev):
    """ssim_lambda = 0: totals and gradient bit-identical to a criterion built without the argument; 0.5 adds
    0.5 * (1 - SSIM) (kept as crit.last_ssim) and its gradient reaches rgb_hw3.grad"""
    from nerfstyle_amd.losses import SemanticStyleLoss
    from nerfstyle_amd.ssim import ssim
    from nerfstyle_amd.stylize import StyleCriterion
    from nerfstyle_amd.vgg import VGG16FeatureExtractor
    H, W = 48, 64
    g = torch.Generator().manual_seed(9)
    target = torch.rand(3, H, W, generator=g).to(dev)
    style = torch.rand(3, H, W, generator=g).to(dev)
    seg = torch.randint(0, 5, (H, W), generator=g)
    rgb0 = torch.rand(H, W, 3, generator=g).to(dev)
    classes = torch.randn(H, W, 5, generator=g).to(dev)
    fx = VGG16FeatureExtractor(['relu3']).to(dev)

    def run(**kw):
        crit = StyleCriterion(fx, SemanticStyleLoss(['relu3'], clusters=seg), content_lambda=0.001, style_lambda=1.0, **kw)
        crit.init_style(style, num_classes=5)
        rgb = rgb0.clone().requires_grad_(True)
        total, content, style_v = crit(rgb, target, classes, frame_key=0)
        total.backward()
        return crit, total.detach(), content, style_v, rgb.grad

    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _, t_old, c_old, s_old, g_old = run()
        crit0, t0, c0, s0, g0 = run(ssim_lambda=0.0)
        crit1, t1, c1, s1, g1 = run(ssim_lambda=0.5)
    finally:
        torch.backends.cudnn.deterministic = det
    assert crit0.last_ssim is None
    assert torch.equal(t0, t_old) and torch.equal(g0, g_old) and torch.equal(c0, c_old) and torch.equal(s0, s_old)
    assert torch.equal(c1, c0) and torch.equal(s1, s0)
    x = rgb0.clone().requires_grad_(True)
    v = ssim(x, target.permute(1, 2, 0))
    v.backward()
    ref = R.ssim_ref(rgb0.cpu().numpy(), target.permute(1, 2, 0).cpu().numpy(), 'same')
    assert abs(float(v) - float(ref['value'])) <= VALUE_TOL
    assert crit1.last_ssim.dtype == torch.float64 and crit1.last_ssim.device.type == 'cuda'
    assert torch.equal(crit1.last_ssim, (1.0 - v.detach()) * 0.5)
    assert abs(float(crit1.last_ssim) - 0.5 * (1.0 - float(ref['value']))) <= VALUE_TOL
    assert torch.equal(t1, t0 + crit1.last_ssim.to(t0.dtype))
    assert torch.allclose(g1, g0 - 0.5 * x.grad, rtol=1e-5, atol=1e-7 * float(g0.abs().max()))
    assert float((g1 - g0).abs().max()) > 0


def test_end_to_end_training_render_with_dssim(dev):
    """one training render of a patch of the small scene, then dssim_loss against the resident target's patch view, in place"""
    from nerfstyle_amd.common import BBox, Box2D, Intrinsics
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.dataset import ResidentDataset
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.ssim import dssim_loss
    from nerfstyle_amd.style_nerf import StyleTCNerf
    nc = 5
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=torch.float32, use_dir=False)
    poses, intr, _ = load_room_cameras()
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=3 + nc, samples_per_ray_cap=256).to(dev)
    grid, bits = small_scene()
    r.density_grid = torch.tensor(grid, device=dev)
    r.density_bitfield = torch.tensor(bits, device=dev)
    r.update_occ = False
    Hf, Wf = 48, 64
    r.intr = Intrinsics(Hf, Wf, intr.fx * Wf / intr.w, intr.fy * Wf / intr.w, Wf / 2.0, Hf / 2.0)
    images = np.random.default_rng(3).random((2, 3, Hf, Wf), np.float32)
    ds = ResidentDataset(images, np.asarray(poses[:2], np.float32), r.intr, 2.0, dev)
    f, box = 1, Box2D(8, 6, 40, 30)
    out = r.render(ds.poses[f], None, patch=box, training=True)
    assert out['rgb_map'].shape == (box.w * box.h, 3) and out['rgb_map'].requires_grad
    tgt = ds.targets[f].view(Hf, Wf, -1)[box.y:box.y + box.h, box.x:box.x + box.w]
    if m.arena.grad is not None:
        m.arena.grad.zero_()
    loss = dssim_loss(out['rgb_map'], tgt, box.h, box.w, lam=0.2, backward=True)
    g = m.arena.grad
    assert 0.0 < float(loss) <= 0.4 and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    want = R.ssim_ref(out['rgb_map'].detach().view(box.h, box.w, 3).cpu().numpy(), tgt.cpu().numpy(), 'same')
    assert abs(float(loss) - 0.2 * (1.0 - float(want['value']))) <= VALUE_TOL
