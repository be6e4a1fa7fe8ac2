"""GPU: the matting-Laplacian photorealism loss (nsr_matting_laplacian, nerfstyle_amd/matting.py) against the reference's
recorded outputs (tests/golden/matting_reference.npz) and a full-frame fp64 restatement; determinism, autograd, refusals,
and the photo term inside the stylisation iteration (StyleCriterion(photo_lambda), deferred and resident back-propagation)."""
import numpy as np
import pytest
import torch

from helpers import rel_l2, small_scene
from matting_ref import fixture_cases, matting_fast, rel_err

pytestmark = pytest.mark.gpu

VALUE_TOL, GRAD_TOL = 1e-9, 1e-6          # value: relative; gradient: relative L2 (f32 output rounding)


@pytest.fixture(scope='module')
def fixture():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return fixture_cases(np.load(os.path.join(root, 'tests', 'golden', 'matting_reference.npz')))


def _run(dev, t, v, r=1, eps=1e-7, v_dtype=torch.float32):
    from nerfstyle_amd.matting import MattingLaplacian
    vt = torch.tensor(np.asarray(v), device=dev).to(v_dtype).requires_grad_(True)
    loss = MattingLaplacian(dev, win_rad=r, eps=eps)(torch.tensor(np.asarray(t), device=dev), vt)
    loss.backward()
    return loss, vt.grad


def test_hip_matches_reference_fixtures(dev, fixture):
    for name, r, eps, t, v, value, g64, g32 in fixture:
        loss, g = _run(dev, t, v, r, eps)
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.device.type == 'cuda'
        assert g.dtype == torch.float32 and g.shape == v.shape
        assert rel_err(float(loss.detach()), value) <= VALUE_TOL, (name, float(loss.detach()), value)
        assert rel_l2(g.cpu().numpy(), g64) <= GRAD_TOL, name
        # a float64 style_map (what the reference's forward converts to) gets a float64 gradient of the same values
        loss64, g_64 = _run(dev, t, v, r, eps, v_dtype=torch.float64)
        assert g_64.dtype == torch.float64 and torch.equal(loss64.detach(), loss.detach())
        assert rel_l2(g_64.cpu().numpy(), g64) <= GRAD_TOL, name
        assert rel_l2(g.cpu().numpy(), g32) <= GRAD_TOL, name


@pytest.mark.parametrize('r', [1, 2])
def test_full_frame_1008x756_matches_fp64_restatement(dev, r):
    from nerfstyle_amd.matting import matting_laplacian
    H, W = 756, 1008
    rng = np.random.default_rng(11 + r)
    # a smooth image with edges and noise, and a style map that partly follows it
    yy, xx = np.mgrid[0:H, 0:W] / 97.0
    t = np.stack([0.5 + 0.3 * np.sin(xx + c) * np.cos(yy * (c + 1)) for c in range(3)]) + 0.02 * rng.random((3, H, W))
    t[:, :, W // 3:] += 0.2
    t = t.astype(np.float32)
    v = (0.6 * t[::-1] + 0.4 * rng.random((3, H, W))).astype(np.float32)
    value, grad = matting_fast(t, v, r, 1e-7)
    vt = torch.tensor(v, device=dev, requires_grad=True)
    loss = matting_laplacian(torch.tensor(t, device=dev), vt, r, 1e-7)
    loss.backward()
    assert rel_err(float(loss.detach()), value) <= VALUE_TOL, (float(loss.detach()), value)
    assert rel_l2(vt.grad.cpu().numpy(), grad) <= GRAD_TOL


def test_two_calls_are_bit_identical(dev):
    from nerfstyle_amd.matting import matting_laplacian
    g = torch.Generator(device='cpu').manual_seed(4)
    t = torch.rand(3, 378, 504, generator=g).to(dev)
    v = torch.rand(3, 378, 504, generator=g).to(dev)
    out = []
    for _ in range(2):
        vt = v.clone().requires_grad_(True)
        loss = matting_laplacian(t, vt)
        loss.backward()
        out.append((loss.detach().clone(), vt.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][1].abs().max()) > 0


def test_autograd_scales_and_reaches_hw3_rgb_through_permute(dev):
    from nerfstyle_amd.matting import MattingLaplacian
    g = torch.Generator(device='cpu').manual_seed(5)
    t = torch.rand(3, 40, 52, generator=g).to(dev)
    rgb = torch.rand(40, 52, 3, generator=g).to(dev).requires_grad_(True)
    m = MattingLaplacian(dev)
    m(t, rgb.permute(2, 0, 1)).backward()
    g1 = rgb.grad.clone()
    assert g1.shape == (40, 52, 3) and float(g1.abs().sum()) > 0
    rgb.grad = None
    (3.0 * m(t, rgb.permute(2, 0, 1))).backward()
    assert torch.allclose(rgb.grad, 3.0 * g1, rtol=1e-6, atol=0)
    # the same gradient as a contiguous [3,H,W] style map
    v = rgb.detach().permute(2, 0, 1).contiguous().requires_grad_(True)
    m(t, v).backward()
    assert torch.equal(v.grad.permute(1, 2, 0), g1)


def test_refusals(dev):
    from nerfstyle_amd.matting import MattingLaplacian
    t = torch.rand(3, 16, 16, device=dev)
    v = torch.rand(3, 16, 16, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match='target'):
        MattingLaplacian(dev)(t.clone().requires_grad_(True), v)
    with pytest.raises(RuntimeError, match='invalid argument'):
        MattingLaplacian(dev)(t[:, :2].contiguous(), v[:, :2].detach().contiguous().requires_grad_(True))
    with pytest.raises(RuntimeError, match='invalid argument'):
        MattingLaplacian(dev, win_rad=2)(t[:, :, :4].contiguous(), v[:, :, :4].detach().contiguous().requires_grad_(True))
    with pytest.raises(RuntimeError, match='unsupported'):
        MattingLaplacian(dev, win_rad=3)(t, v)


# ---- the photo term in the stylisation iteration ---------------------------------------------------------------------

def _renderer(dev):
    """The seeded oracle checkpoint on the small synthetic scene, a 96x128 frame of the LLFF room camera."""
    from nerfstyle_amd.common import BBox, Intrinsics
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    from oracle import torch_port as TP
    nc = 5
    ref = TP.Field(num_classes=nc, table_scale=0.5)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=torch.float32, use_dir=False)
    sd = m.state_dict()
    sd.update({'x_density_embedder.embeddings': ref.emb_density.detach(), 'x_color_embedder.embeddings': ref.emb_color.detach(),
               'density_net.params': ref.p_density.detach(), 'color1_net.params': ref.p_color1.detach(),
               'color2_net.params': ref.p_color2.detach(), 'class_net.params': ref.p_class.detach()})
    m.load_state_dict(sd)
    poses, intr, _ = load_room_cameras()
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=3 + nc, samples_per_ray_cap=256).to(dev)
    grid, bits = small_scene()
    r.density_grid = torch.tensor(grid, device=dev)
    r.density_bitfield = torch.tensor(bits, device=dev)
    r.update_occ = False
    r.intr = Intrinsics(96, 128, intr.fx * 128 / intr.w, intr.fy * 128 / intr.w, 64., 48.)
    return r, torch.tensor(poses[2], device=dev)


def test_photo_term_through_deferred_and_resident_backprop(dev):
    """A loss made of the photo term only: the deferred iteration gives the gradient of one direct full-frame backward
    (the bars of test_deferred_backprop_equals_direct_and_trains_only_colour_table), only the colour table moves, and the
    resident iteration gives the deferred gradient."""
    from nerfstyle_amd.matting import MattingLaplacian
    from nerfstyle_amd.optim import FusedAdam
    from nerfstyle_amd.stylize import deferred_backprop_step, resident_backprop_step
    r, pose = _renderer(dev)
    m = r.model
    g = torch.Generator().manual_seed(8)
    target = torch.rand(3, 96, 128, generator=g).to(dev)
    photo = MattingLaplacian(dev)

    def image_loss(rgb):
        return photo(target, rgb.permute(2, 0, 1))

    opt = FusedAdam(m, lr=0.1, keywords=['x_color_embedder'])
    SCALE = 1024.0              # f16 MFMA operands in the field backward (see the test named above)
    loss, _ = deferred_backprop_step(r, pose, image_loss, patch_size=50, loss_scale=SCALE)
    assert loss.dtype == torch.float64 and float(loss) > 0
    g_def = m.arena.grad.clone()
    m.arena.grad.zero_()
    out = r.render(pose, None, training=True)
    (image_loss(out['rgb_map'].view(96, 128, 3)) * SCALE).backward()
    g_dir = m.arena.grad.clone()
    m.arena.grad.zero_()
    assert float(g_dir.abs().sum()) > 0
    assert rel_l2(g_def.cpu().numpy(), g_dir.cpu().numpy()) < 2e-3
    loss_res, _ = resident_backprop_step(r, pose, image_loss, loss_scale=SCALE)
    g_res = m.arena.grad.clone()
    assert rel_err(float(loss_res), float(loss)) < 1e-5
    assert rel_l2(g_res.cpu().numpy(), g_def.cpu().numpy()) < 2e-3
    gt = g_def[:m.table_elems].view(m.rows, 2, 2)
    assert float(gt[:, 0, :].abs().max()) == 0.0 and float(gt[:, 1, :].abs().max()) > 0.0
    m.arena.grad.copy_(g_def)
    before = m.arena.detach().clone()
    opt.step(grad_scale=SCALE)
    after = m.arena.detach()
    tb, ta = before[:m.table_elems].view(m.rows, 2, 2), after[:m.table_elems].view(m.rows, 2, 2)
    assert torch.equal(tb[:, 0, :], ta[:, 0, :]) and torch.equal(before[m.table_elems:], after[m.table_elems:])
    assert not torch.equal(tb[:, 1, :], ta[:, 1, :])


def test_style_criterion_photo_lambda(dev):
    """photo_lambda = 0: the criterion's total and gradient are bit-identical to content + style computed as before the
    photo term existed; photo_lambda = 1e-4 adds exactly 1e-4 * L (kept as crit.last_photo, a device tensor)."""
    import torch.nn.functional as F
    from nerfstyle_amd.losses import SemanticStyleLoss
    from nerfstyle_amd.matting import matting_laplacian
    from nerfstyle_amd.stylize import StyleCriterion
    from nerfstyle_amd.vgg import VGG16FeatureExtractor
    H, W = 96, 128
    g = torch.Generator().manual_seed(9)
    target = torch.rand(3, H, W, generator=g).to(dev)
    style = torch.rand(3, H, W, generator=g).to(dev)
    seg = torch.randint(0, 5, (H, W), generator=g)
    rgb0 = torch.rand(H, W, 3, generator=g).to(dev)
    classes = torch.randn(H, W, 5, generator=g).to(dev)
    fx = VGG16FeatureExtractor(['relu3']).to(dev)

    def run(photo_lambda):
        crit = StyleCriterion(fx, SemanticStyleLoss(['relu3'], clusters=seg), content_lambda=0.001, style_lambda=1.0,
                              photo_lambda=photo_lambda)
        crit.init_style(style, num_classes=5)
        rgb = rgb0.clone().requires_grad_(True)
        total, content, style_v = crit(rgb, target, classes, frame_key=0)
        total.backward()
        return crit, total.detach(), content, style_v, rgb.grad

    # the criterion as it was before photo_lambda: content + style
    def old_criterion():
        sl = SemanticStyleLoss(['relu3'], clusters=seg)
        with torch.no_grad():
            sl.init_feats(fx(style), num_classes=5)
            tgt = fx(target)['relu3']
        rgb = rgb0.clone().requires_grad_(True)
        feats = fx(rgb.permute(2, 0, 1))
        old = F.mse_loss(feats['relu3'], tgt) * 0.001 + sl(feats, None, torch.argmax(classes, dim=-1), 0) * 1.0
        old.backward()
        return old.detach(), rgb.grad

    # bit-for-bit comparisons of the VGG backward need the deterministic convolution algorithms
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        t_old, g_old = old_criterion()
        crit0, t0, c0, s0, g0 = run(0.0)
        lam = 1e-4
        crit1, t1, c1, s1, g1 = run(lam)
    finally:
        torch.backends.cudnn.deterministic = det
    assert crit0.photo_loss is None and crit0.last_photo is None
    assert torch.equal(t0, t_old) and torch.equal(g0, g_old)
    assert torch.equal(c1, c0) and torch.equal(s1, s0)
    vp = rgb0.permute(2, 0, 1).clone().requires_grad_(True)
    L = matting_laplacian(target, vp)
    L.backward()
    assert crit1.last_photo.dtype == torch.float64 and crit1.last_photo.device.type == 'cuda'
    assert torch.equal(crit1.last_photo, L.detach() * lam)
    assert float(L.detach()) * lam > 1e-3 * abs(float(t0))             # the term is visible in the total
    assert torch.equal(t1, t0 + (L.detach() * lam).to(t0.dtype))
    assert torch.allclose(g1, g0 + lam * vp.grad.permute(1, 2, 0), rtol=1e-5, atol=1e-7 * float(g0.abs().max()))
