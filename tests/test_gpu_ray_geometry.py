"""Per-ray geometry terms on the GPU (k_geom_fwd / k_geom_bwd in composite.hip, raymarching.ray_geometry,
Renderer.geometry_terms): differentiable depth and the mip-NeRF 360 distortion on the weights of the training composite.

Inputs are helpers.edge_rays with nears = 0.2 and fars = 2.2 (ray_geometry_ref.geometry_case): rays of 0 to 200 samples whose
stop lands on chosen lanes, no transmittance within 10 % of the threshold, a dropped ray, an empty ray, a ray without a range,
slots no ray owns, a shuffled index.  The reference is the fp64 restatement of the definitions with autograd gradients.

Bars: depth 2e-4 (the project's depth bar), distortion 2e-5 max(1, max|ref|) (the composite bar), gradient 1e-4 max|ref|.
tests/test_ray_geometry_cpu.py holds the serial fp32 evaluation of the formula to a quarter of each on these inputs (it is at
4e-7, 1.4e-7 and 8e-8), so none of them needed the fallback; none is derived from the kernel's output."""
import numpy as np
import pytest
import torch

import ray_geometry_ref as G
from helpers import rel_l2, render_setup

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.as_tensor(np.array(a), device=dev)          # (a copy: the cached arrays are read-only)


def _inputs(c, dev):
    return [T(c[k], dev) for k in ('sig', 'deltas', 'rays', 'nears', 'fars')]


def _forward(c, dev):
    """the C entry point -> (depth, distortion, totals) tensors"""
    from nerfstyle_amd import _lib as L
    sig, deltas, rays, nears, fars = _inputs(c, dev)
    depth, dist = torch.full((c['N'],), float('nan'), device=dev), torch.full((c['N'],), float('nan'), device=dev)
    totals = torch.full((c['N'], 4), float('nan'), device=dev)
    L.check(L.lib().nsr_ray_geometry_forward(L.p(sig), L.p(deltas), L.p(rays), L.p(nears), L.p(fars), c['M'], c['N'], c['T_thresh'],
                                             int(c['is_ndc']), L.p(depth), L.p(dist), L.p(totals), L.stream()), 'ray_geometry_forward')
    return depth, dist, totals


@pytest.mark.parametrize('is_ndc', [False, True])
def test_forward_on_edge_rays(dev, is_ndc):
    from nerfstyle_amd import _lib as L
    c = G.geometry_case(is_ndc)
    depth_t, dist_t, _ = _forward(c, dev)
    depth, dist = depth_t.cpu().numpy(), dist_t.cpu().numpy()
    assert np.isfinite(depth).all() and np.isfinite(dist).all()
    # depth_norm of nsr_render_train_forward on the same buffers.  That entry point has no is_ndc argument and reads the delta
    # columns 0 and 1, so for is_ndc it is handed the rows with the column pairs exchanged: the same kernel on the same numbers.
    sig, deltas, rays, nears, fars = _inputs(c, dev)
    if is_ndc:
        deltas = deltas[:, [2, 3, 0, 1]].contiguous()
    N, M, C = c['N'], c['M'], 3
    rgbs = torch.rand(M, C, device=dev)
    outs = [torch.empty(s, device=dev) for s in ((N,), (N,), (N, C), (N, 3), (N,))]
    L.check(L.lib().nsr_render_train_forward(L.p(sig), L.p(rgbs), L.p(deltas), L.p(rays), L.p(nears), L.p(fars), M, N, C, c['T_thresh'],
                                             *[L.p(o) for o in outs], None, L.stream()), 'render_train_forward')
    depth_norm = outs[4].cpu().numpy()
    v = c['valid']
    e_depth = np.abs(depth[v] - depth_norm[v]).max()
    e_ref = np.abs(depth[v] - c['depth'][v]).max()
    e_dist = np.abs(dist - c['dist']).max()
    print(is_ndc, 'depth vs depth_norm', e_depth, 'vs fp64', e_ref, 'distortion vs fp64', e_dist, 'max|ref|', c['dist'].max())
    assert e_depth <= 2e-4 and e_ref <= 2e-4
    assert (depth[v] > 0).sum() >= 20 and (depth[v] == 0).sum() >= 20
    assert e_dist <= 2e-5 * max(1.0, np.abs(c['dist']).max())
    assert dist[v].min() > 0
    # exact zeros: the dropped ray, the empty ray, the ray with near == far == FLT_MAX (where depth_norm is 0 / 0)
    r = c['rays']
    for row in (len(r) - 1, int(np.nonzero(r[:, 2] == 0)[0][0]), c['miss']):
        assert depth[r[row, 0]] == 0 and dist[r[row, 0]] == 0, row
    assert np.isnan(depth_norm[r[c['miss'], 0]])


@pytest.mark.parametrize('is_ndc', [False, True])
@pytest.mark.parametrize('which', G.UPSTREAM)
def test_backward_on_edge_rays(dev, is_ndc, which):
    """The C entry point into a NaN-filled grad_sigmas with a guard behind M, then the same through the autograd wrapper."""
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import raymarching as R
    c = G.geometry_case(is_ndc)
    M, N, owned, ref = c['M'], c['N'], c['owned'], c['grads'][which]
    gd, gx = G.upstream(c, which)
    gd_t, gx_t = (None if gd is None else T(gd, dev)), (None if gx is None else T(gx, dev))
    sig, deltas, rays, nears, fars = _inputs(c, dev)
    _, _, totals = _forward(c, dev)
    gs_t = torch.full((M + 4096,), float('nan'), device=dev)
    L.check(L.lib().nsr_ray_geometry_backward(L.p(gd_t), L.p(gx_t), L.p(sig), L.p(deltas), L.p(rays), L.p(nears), L.p(fars),
                                              L.p(totals), M, N, c['T_thresh'], int(is_ndc), L.p(gs_t), L.stream()),
            'ray_geometry_backward')
    gs = gs_t.cpu().numpy()
    assert np.isnan(gs[M:]).all()                               # nothing behind the M samples
    gs = gs[:M]
    assert np.array_equal(np.isnan(gs), ~owned)                 # NaN exactly on the slots no ray owns
    scale = np.abs(ref).max()
    err = np.abs(gs[owned] - ref[owned]).max()
    print(is_ndc, which, 'max|ref|', scale, 'max abs error', err, 'relative', err / scale)
    assert err <= 1e-4 * scale
    n_stop = 0
    for row, (index, offset, steps) in enumerate(c['rays']):
        stop = c['stop'][row]
        seg, rseg = gs[offset:offset + steps], ref[offset:offset + steps]
        if row == len(c['rays']) - 1 or row == c['miss']:
            assert (seg == 0).all()                             # the dropped ray; the ray without a range
        elif stop < steps:
            assert (seg[stop + 1:] == 0).all() and (rseg[stop + 1:] == 0).all()       # behind the stop: exactly 0
            if rseg[stop] != 0:                                 # the stopping sample itself has a gradient
                assert seg[stop] != 0, (row, stop)
                n_stop += 1
    assert n_stop >= (60 if which != 'depth' else 10)           # (G_depth alone: only where the clamp passes a gradient)
    # the wrapper: same bits in the owned slots, zeros elsewhere
    s_t = sig.clone().requires_grad_()
    depth, dist = R.ray_geometry(s_t, deltas, rays, nears, fars, c['T_thresh'], is_ndc)
    loss = sum((o * g).sum() for o, g in ((depth, gd_t), (dist, gx_t)) if g is not None)
    loss.backward()
    g_w = s_t.grad.cpu().numpy()
    assert np.array_equal(g_w[owned], gs[owned]) and (g_w[~owned] == 0).all()


@pytest.mark.parametrize('is_ndc', [False, True])
def test_totals_have_the_bits_of_the_composite(dev, is_ndc):
    """totals[:, 0] and totals[:, 1] (sum w, sum w t) are weights_sum and depth of nsr_composite_rays_train_forward on the same
    samples, to the bit: the claim above GeomArgs in composite.hip.  Rays with a range that are neither dropped nor empty."""
    from nerfstyle_amd import _lib as L
    c = G.geometry_case(is_ndc)
    _, _, totals_t = _forward(c, dev)
    sig, deltas, rays, _, _ = _inputs(c, dev)
    N, M, C = c['N'], c['M'], 3
    rgbs = torch.rand(M, C, device=dev)
    ws_t, depth_t, image_t = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, C, device=dev)
    L.check(L.lib().nsr_composite_rays_train_forward(L.p(sig), L.p(rgbs), L.p(deltas), L.p(rays), M, N, C, c['T_thresh'], int(is_ndc),
                                                     L.p(ws_t), L.p(depth_t), L.p(image_t), L.stream()), 'composite_rays_train_forward')
    totals, ws, depth = totals_t.cpu().numpy(), ws_t.cpu().numpy(), depth_t.cpu().numpy()
    v = c['valid']
    assert v.sum() >= 50
    assert np.array_equal(totals[v, 0], ws[v])
    assert np.array_equal(totals[v, 1], depth[v])


def test_two_runs_give_the_same_bits(dev):
    from nerfstyle_amd import raymarching as R
    c = G.geometry_case(False)

    def run():
        sig, deltas, rays, nears, fars = _inputs(c, dev)
        sig.requires_grad_()
        depth, dist = R.ray_geometry(sig, deltas, rays, nears, fars, c['T_thresh'])
        ((depth * T(c['g_depth'], dev)).sum() + (dist * T(c['g_dist'], dev)).sum()).backward()
        return [x.detach().cpu().numpy() for x in (depth, dist, sig.grad)]
    for a, b in zip(run(), run()):
        assert np.array_equal(a, b)


# ---- through the renderer -------------------------------------------------------------------------------------------
N_RAYS = 256


def _renderer(dev):
    r, _, poses, intr, _ = render_setup(dev, table_dtype=None, cap=192, contrast=16.0)
    r.cfg.density_scale = 40.0
    return r, poses, intr


def _pix(intr, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randperm(intr.w * intr.h, device=dev, generator=g)[:N_RAYS]


def _geo_loss(out):
    return out['distortion'].mean() + ((out['depth'] - 0.5) ** 2).mean()


def test_renderer_switch_outputs_and_gradient(dev):
    from nerfstyle_amd import raymarching
    from nerfstyle_amd.rays import generate_rays
    r, poses, intr = _renderer(dev)
    m = r.model
    pose, pix = torch.tensor(poses[0], device=dev), _pix(intr, dev, 11)
    with torch.no_grad():
        off = r.render(pose, None, training=True, pix_subset=pix)
    assert 'depth' not in off and 'distortion' not in off
    r.geometry_terms = True
    with torch.no_grad():
        test = r.render(pose, None, training=False, pix_subset=pix)
    assert 'depth' not in test and 'distortion' not in test                 # render_test ignores the switch
    m._ensure_grad()
    m.arena.grad.zero_()
    out = r.render(pose, None, training=True, pix_subset=pix)
    for k in ('rgb_map', 'classes', 'trans_map'):
        assert torch.equal(out[k], off[k]), k
    assert out['depth'].shape == out['distortion'].shape == (N_RAYS,)
    fin = torch.isfinite(out['trans_map'])
    assert int(fin.sum()) > N_RAYS // 2
    e = float((out['depth'].detach()[fin] - out['trans_map'][fin]).abs().max())
    print('depth vs trans_map', e, 'finite', int(fin.sum()), 'distortion max', float(out['distortion'].detach().max()))
    assert e <= 2e-4
    assert bool(torch.isfinite(out['depth']).all()) and bool(torch.isfinite(out['distortion']).all())
    assert bool((out['depth'][~fin] == 0).all()) and bool((out['distortion'][~fin] == 0).all())
    assert float(out['distortion'].detach().max()) > 0 and float(out['depth'].detach().max()) > 0
    _geo_loss(out).backward()
    grad = m.arena.grad.detach().clone()
    parts = {k: v.cpu().numpy() for k, v in m.views_of(grad).items()}
    for k in ('x_density_embedder.embeddings', 'density_net.params'):
        assert np.abs(parts[k]).max() > 0, k
    for k in ('x_color_embedder.embeddings', 'color1_net.params', 'color2_net.params', 'class_net.params'):
        assert (parts[k] == 0).all(), k
    # the hand-driven pipeline: march -> field -> d loss / d sigmas from the fp64 restatement -> sigmas.backward
    rays, _ = generate_rays(pose, intr, None, camera_flip=r.cfg.flip_camera, pix_subset=pix, device=dev)
    nears, fars = raymarching.near_far_from_aabb(rays.origins, rays.dirs, r.aabb, r.cfg.min_near)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    M = r.sample_capacity(N_RAYS)
    xyzs, _, deltas, rinfo = raymarching.march_rays_train_nosync(rays.origins, rays.dirs, r.bound, r.march_bitfield, r.cascade,
                                                                 r.cfg.grid_size, nears, fars, M, counter, 0., r.cfg.max_steps)
    m.arena.grad.zero_()
    sigmas, _ = m.field(xyzs, sigma_only=False, m_dev=counter, density_scale=r.cfg.density_scale)
    cnt = int(counter[0])
    s64 = sigmas.detach().double().cpu()
    s64[cnt:] = 0.0                                                          # (slots past the count are not written)
    s64.requires_grad_()
    depth, dist = G.geometry_torch(s64, deltas.cpu().numpy(), rinfo.cpu().numpy(), nears.cpu().numpy(), fars.cpu().numpy(),
                                   r.cfg.t_thresh)
    (dist.mean() + ((depth - 0.5) ** 2).mean()).backward()
    assert float((depth.detach() - out['depth'].detach().double().cpu()).abs().max()) <= 2e-4
    sigmas.backward(s64.grad.to(torch.float32).to(dev))
    e = rel_l2(grad.cpu().numpy(), m.arena.grad.cpu().numpy())
    print('arena gradient against the hand-driven fp64 pipeline: rel-L2', e)
    assert e < 1e-4


def test_graph_captured_step_with_both_terms(dev):
    """GraphedRenderStep whose loss holds both terms: captured once, replayed on two other pixel sets, against eager steps
    (the bar of test_graph_captured_step_equals_eager_steps)."""
    from nerfstyle_amd.graph import GraphedRenderStep
    r, poses, intr = _renderer(dev)
    r.geometry_terms = True
    m = r.model
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    target = torch.rand(intr.w * intr.h, 3, device=dev, generator=g)

    def loss_fn(out, pix):
        return torch.mean((out['rgb_map'] - target[pix]) ** 2) + 0.1 * _geo_loss(out)

    step = GraphedRenderStep(r, N_RAYS, loss_fn)
    pose_t = torch.tensor(poses, device=dev)
    step.capture(pose_t[0], _pix(intr, dev, 20))
    for k in (4, 8):
        pix = _pix(intr, dev, 20 + k)
        m.arena.grad.zero_()
        loss_g = step(pose_t[k], pix).clone()
        grad_g = m.arena.grad.clone()
        m.arena.grad.zero_()
        out = r.render(pose_t[k], None, training=True, pix_subset=pix)
        loss_e = loss_fn(out, pix)
        loss_e.backward()
        print(k, 'loss', float(loss_g), float(loss_e.detach()), 'grad rel-L2', rel_l2(grad_g.cpu().numpy(), m.arena.grad.cpu().numpy()))
        assert abs(float(loss_g) - float(loss_e.detach())) <= 1e-6 * abs(float(loss_e.detach()))
        assert rel_l2(grad_g.cpu().numpy(), m.arena.grad.cpu().numpy()) < 1e-4
