"""View-dependent colour through the renderer: the samples' directions reach the field in every render mode."""
import numpy as np
import pytest
import torch

import sh_ref as SH
from helpers import rel_l2, render_setup

pytestmark = pytest.mark.gpu


def _setup(dev, nc=5, cap=None, contrast=16.0):
    ref = SH.FieldDirs(num_classes=nc)
    with torch.no_grad():                          # colours and densities that vary across the image (helpers.render_setup)
        ref.p_density[2048:] *= contrast
        ref.p_color2[-1024:] *= contrast
        ref.p_sh *= 4.0                            # and a colour that really depends on the direction
    r, _, poses, intr, _ = render_setup(dev, nc=nc, table_dtype=None, cap=cap, ref=ref, view_dependent=True,
                                        state={'color2_net.params': ref.color2_params().detach()})
    r.cfg.density_scale = 40.0
    return r, poses, intr


def test_training_render_equals_hand_driven_pipeline(dev):
    """64x48 patch: render_train of a view_dependent model == march (want_dirs) -> model.field(pts, dirs) -> composite by hand;
    and the directions matter: the same samples shaded with another direction set give another image."""
    from nerfstyle_amd import raymarching
    from nerfstyle_amd.common import Box2D
    from nerfstyle_amd.rays import generate_rays
    from nerfstyle_amd.renderer import _render_train
    r, poses, intr = _setup(dev)
    m = r.model
    pose = torch.tensor(poses[0], device=dev)
    patch = Box2D(300, 200, 64, 48)
    with torch.no_grad():
        out = r.render(pose, None, patch=patch, training=True)
        rays, _ = generate_rays(pose, intr, None, patch=patch, camera_flip=r.cfg.flip_camera, device=dev)
        N = rays.origins.shape[0]
        assert N == 64 * 48 and out['rgb_map'].shape == (N, 3)
        nears, fars = raymarching.near_far_from_aabb(rays.origins, rays.dirs, r.aabb, r.cfg.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        M = r.sample_capacity(N)
        xyzs, dirs, deltas, rinfo = raymarching.march_rays_train_nosync(
            rays.origins, rays.dirs, r.bound, r.march_bitfield, r.cascade, r.cfg.grid_size, nears, fars, M, counter, 0.,
            r.cfg.max_steps, want_dirs=True)
        cnt = int(counter[0])
        assert cnt > N
        # the march hands every sample a direction of the batch (its ray's)
        assert bool(((dirs[:cnt].norm(dim=1) - 1).abs() < 1e-3).all())
        sig, rgbs = m.field(xyzs, sigma_only=False, m_dev=counter, density_scale=r.cfg.density_scale, dirs=dirs)
        image, depth, classes, _ = _render_train(sig, rgbs, deltas, rinfo, nears, fars, r.cfg.t_thresh)
        assert torch.equal(image, out['rgb_map']) and torch.equal(classes, out['classes']) and torch.equal(depth, out['trans_map'])
        assert float(image.min()) < 0.9 and float(image.std()) > 0.05             # something was rendered
        sig2, rgbs2 = m.field(xyzs, sigma_only=False, m_dev=counter, density_scale=r.cfg.density_scale, dirs=-dirs)
        image2, _, classes2, _ = _render_train(sig2, rgbs2, deltas, rinfo, nears, fars, r.cfg.t_thresh)
        assert torch.equal(classes2, classes) and float((image2 - image).abs().max()) > 1e-2


def test_inference_paths_against_training_path(dev):
    """render_test and the reference's inference loop against the training path on a patch: > 45 dB, the existing bar."""
    from nerfstyle_amd.common import Box2D
    r, poses, intr = _setup(dev)
    pose = torch.tensor(poses[5], device=dev)
    patch = Box2D(100, 60, 128, 96)
    with torch.no_grad():
        train = r.render(pose, None, patch=patch, training=True)['rgb_map']
        fast = r.render(pose, None, patch=patch, training=False)['rgb_map']
        r.reference_inference_loop = True
        loop = r.render(pose, None, patch=patch, training=False)['rgb_map']
    for name, img in (('render_test', fast), ('loop', loop)):
        mse = float(((img - train) ** 2).mean())
        psnr = 10.0 * np.log10(1.0 / max(mse, 1e-30))
        print(name, 'PSNR against the training path', psnr)
        assert psnr > 45.0, (name, psnr)
    assert float(train.min()) < 0.9
    # the streaming kernel has no direction input: a clear refusal
    r.reference_inference_loop = False
    r.fused_inference = True
    with pytest.raises(NotImplementedError, match='direction'):
        r.render(pose, None, patch=patch, training=False)


def test_graph_captured_step_equals_eager_steps(dev):
    """A captured GraphedRenderStep at 256 rays (static dirs buffer), replayed three times with new contents, against eager
    steps: the bar of test_gpu_render.test_graph_captured_step_equals_eager_step."""
    from nerfstyle_amd.graph import GraphedRenderStep
    r, poses, intr = _setup(dev, cap=192)
    m = r.model
    n = 256
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    target = torch.rand(intr.w * intr.h, 3, device=dev, generator=g)

    def loss_fn(out, pix):
        return torch.mean((out['rgb_map'] - target[pix]) ** 2) + 1e-3 * out['classes'].square().mean()

    step = GraphedRenderStep(r, n, loss_fn)
    pose_t = torch.tensor(poses, device=dev)
    step.capture(pose_t[0], torch.randperm(intr.w * intr.h, device=dev, generator=g)[:n])
    for k in (1, 5, 9):
        pix = torch.randperm(intr.w * intr.h, device=dev, generator=g)[:n]
        m.arena.grad.zero_()
        loss_g = step(pose_t[k], pix).clone()
        grad_g = m.arena.grad.clone()
        m.arena.grad.zero_()
        out = r.render(pose_t[k], None, training=True, pix_subset=pix)
        loss_e = loss_fn(out, pix)
        loss_e.backward()
        assert abs(float(loss_g) - float(loss_e.detach())) <= 1e-6 * abs(float(loss_e.detach()))
        sh = slice(m.table_elems + 15360, m.table_elems + 16384)
        assert float(grad_g[sh].abs().max()) > 0
        assert rel_l2(grad_g.cpu().numpy(), m.arena.grad.cpu().numpy()) < 1e-4


def test_loss_scaler_step_moves_the_sh_block(dev):
    """LossScaler + FusedAdam.step(scaler=...) on the larger arena, through the renderer."""
    from nerfstyle_amd.optim import FusedAdam, LossScaler
    r, poses, intr = _setup(dev, cap=192)
    m = r.model
    opt = FusedAdam(m, lr=1e-2)
    sc = LossScaler(init_scale=128.0)
    opt.zero_grad()
    before = m.arena.detach()[m.table_elems + 15360:].clone()
    pix = torch.arange(0, 512, device=dev) * 997 % (intr.w * intr.h)
    out = r.render(torch.tensor(poses[2], device=dev), None, training=True, pix_subset=pix)
    sc.scale(out['rgb_map'].square().mean()).backward()
    sc.step(opt, lr_decay_steps=100.0)
    after = m.arena.detach()[m.table_elems + 15360:]
    assert (after != before).float().mean() > 0.9 and bool(torch.isfinite(after).all())
