"""GPU: the fused forward-mode density gradient (nsr_field_density_gradient, StyleTCNerf.density_gradient) and the normal
map built on it (Renderer.render_normals).

Gradient reference: autograd of oracle.torch_port.Field(sigma_only=True) with the kernel's operand roundings emulated
(straight-through), in float32 -- the restatement then forms the encoder input, the cells and the fractions with the kernel's
own fp32 operations.  Bars: rel-L2 <= 5e-3 (f16 compute) / 3e-2 (bf16), the project's bars for gradients through rounded
operands, on a fresh checkpoint (tables +-1e-4) and on tables x1e4 -- the two ends of the f16 range the
tangents have to survive.  Measured values: DESIGN.md "Position gradients".
"""
import numpy as np
import pytest
import torch

from helpers import rel_l2, room_rays, small_scene

pytestmark = pytest.mark.gpu

M_TOTAL = 16 * 7 + 5       # seven full tiles and a ragged one
M_DEV = M_TOTAL - 9        # device-side count: the last tile it reaches is ragged too
I_NAN, I_OUT, I_CORNER, I_LOW = 3, 20, 40, 41
DENSITY_SCALE = 1.5


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _march(O, dev, n_rays, cap):
    from nerfstyle_amd import raymarching as R
    grid, bits = small_scene()
    ro, rd = room_rays(O, n_rays, seed=3)
    aabb = T(np.array([-2, -2, -2, 2, 2, 2], np.float32), dev)
    near, far = R.near_far_from_aabb(T(ro, dev), T(rd, dev), aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    xyzs, _, deltas, rays = R.march_rays_train_nosync(T(ro, dev), T(rd, dev), 2.0, T(bits, dev), 2, 128, near, far, n_rays * cap,
                                                      counter, 0., 1024)
    return xyzs, int(counter[0])


@pytest.fixture(scope='module')
def positions(O, dev):
    """[M_TOTAL, 3] float32: a marched patch with a NaN, an out-of-box, a box-corner and a low-corner sample injected"""
    xyzs, cnt = _march(O, dev, 64, 256)
    assert cnt >= M_TOTAL + 100
    pts = xyzs[100:100 + M_TOTAL].cpu().numpy().copy()
    pts[I_NAN] = [0.3, np.nan, -0.2]
    pts[I_OUT] = [2.5, 0.1, 0.2]
    pts[I_CORNER] = [2.0, 2.0, 2.0]
    pts[I_LOW] = [-2.0, -2.0, -2.0]
    return pts


def _pair(dev, dt, table_half, table_scale):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    from oracle import torch_port as TP
    ref = TP.Field(num_classes=5, table_scale=table_scale)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None if table_half else torch.float32, use_dir=False,
                    compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16)
    sd = m.state_dict()
    sd['x_density_embedder.embeddings'] = ref.emb_density.detach()
    sd['x_color_embedder.embeddings'] = ref.emb_color.detach()
    for k, p in (('density_net', ref.p_density), ('color1_net', ref.p_color1), ('color2_net', ref.p_color2), ('class_net', ref.p_class)):
        sd[k + '.params'] = p.detach()
    m.load_state_dict(sd)
    return m.to(dev), ref


_REF = {}


def _reference_grad(ref, pts, dt, table_half, table_scale):
    """d sigma / d position of the restatement, computed once per configuration"""
    key = (dt, table_half, table_scale)
    if key not in _REF:
        good = np.ones(M_TOTAL, bool)
        good[I_NAN] = False                                        # a NaN row would only put NaN into its own gradient
        pt = torch.tensor(pts[good], requires_grad=True)
        ref(pt, sigma_only=True, half=dt, table_half=table_half).sum().backward()
        g = np.zeros((M_TOTAL, 3), np.float32)
        g[good] = pt.grad.numpy() * np.float32(DENSITY_SCALE)
        g[M_DEV:] = 0
        _REF[key] = g
    return _REF[key]


@pytest.mark.parametrize('table_scale', [1e-4, 1.0])
@pytest.mark.parametrize('dt,table_half', [('f16', False), ('bf16', False), ('f16', True), ('bf16', True)])
def test_density_gradient(dev, positions, dt, table_half, table_scale):
    m, ref = _pair(dev, dt, table_half, table_scale)
    pts = T(positions, dev)
    m_dev = torch.tensor([M_DEV, 0], dtype=torch.int32, device=dev)
    with torch.no_grad():
        want_sig = m.field(pts, sigma_only=True, m_dev=m_dev, density_scale=DENSITY_SCALE)
    sig, grads = m.density_gradient(pts, m_dev=m_dev, density_scale=DENSITY_SCALE)
    assert sig.shape == (M_TOTAL,) and grads.shape == (M_TOTAL, 3) and not grads.requires_grad
    # sigma: the forward's bits
    assert torch.equal(sig[:M_DEV], want_sig[:M_DEV])
    g = grads.cpu().numpy()
    assert np.all(np.isfinite(g))
    # dead, NaN and out-of-box rows: exactly zero
    assert np.all(g[M_DEV:] == 0) and np.all(g[I_NAN] == 0) and np.all(g[I_OUT] == 0)
    assert np.any(g[I_CORNER] != 0) and np.any(g[I_LOW] != 0)
    want = _reference_grad(ref, positions, dt, table_half, table_scale)
    assert np.all(want[I_OUT] == 0) and np.linalg.norm(want) > 0
    err = rel_l2(g, want)
    print('density gradient %s table_half=%d tables +-%g: rel-L2 %.3e' % (dt, table_half, table_scale, err))
    assert err <= (5e-3 if dt == 'f16' else 3e-2)
    # unit normals: -grad / |grad|, or exactly zero
    sig_n, nrm = m.density_gradient(pts, m_dev=m_dev, density_scale=DENSITY_SCALE, normalize=True)
    assert torch.equal(sig_n[:M_DEV], sig[:M_DEV])
    n = nrm.cpu().numpy()
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    zero = np.all(n == 0, axis=1)
    assert np.all(zero | (np.abs(length - 1) <= 1e-5))
    assert np.array_equal(zero, np.all(g == 0, axis=1))
    lg = np.linalg.norm(g.astype(np.float64), axis=1)
    assert np.abs(n[~zero] + g[~zero] / lg[~zero, None]).max() <= 1e-5
    # entry point without the sigma output
    import ctypes
    from nerfstyle_amd import _lib as L
    g2 = torch.full_like(grads, 7.0)
    desc = m._desc(DENSITY_SCALE)
    L.check(L.lib().nsr_field_density_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(m._mlp_flat()), L.p(pts), M_TOTAL,
                                               L.p(m_dev), None, L.p(g2), 0, L.stream()), 'field_density_gradient')
    assert torch.equal(g2, grads)


def test_density_gradient_graph_replays_equal_eager(dev, positions):
    m, _ = _pair(dev, 'f16', True, 1.0)
    pts = T(positions, dev)
    m_dev = torch.tensor([M_DEV, 0], dtype=torch.int32, device=dev)
    sig_e, g_e = m.density_gradient(pts, m_dev=m_dev, normalize=False)
    sig_e, g_e = sig_e.clone(), g_e.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.density_gradient(pts, m_dev=m_dev)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sig_g, g_g = m.density_gradient(pts, m_dev=m_dev)
    for _ in range(2):
        sig_g.zero_()
        g_g.fill_(7.0)
        graph.replay()
        assert torch.equal(g_g, g_e) and torch.equal(sig_g[:M_DEV], sig_e[:M_DEV])


def test_render_normals(O, dev):
    """A 32 x 24 frame: the normal map is the existing training composite of the kernel's per-sample unit normals over the
    same marched samples, rays that miss the box are zero, |normal_map| <= weights_sum, and the occupancy schedule does
    not move."""
    from nerfstyle_amd import raymarching as R
    from nerfstyle_amd.common import RayBatch
    from nerfstyle_amd.config import RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    m, _ = _pair(dev, 'f16', True, 1.0)
    _, intr, _ = load_room_cameras()
    cfg = RendererConfig.llff()
    cfg.density_scale = 40.0                                       # opaque enough for weights_sum to be far from zero
    r = Renderer(m, cfg, intr, 2.0, raymarch_channels=8).to(dev)
    grid, bits = small_scene()
    r.density_bitfield = T(bits, dev)
    c = __import__('helpers').room_cameras()
    W, H = 32, 24
    ys, xs = np.meshgrid(np.arange(H) * (c['h'] // H), np.arange(W) * (c['w'] // W), indexing='ij')
    pix = (ys * c['w'] + xs).reshape(-1)
    ro, rd = O.generate_rays(np.asarray(c['poses'][0], np.float32), c['w'], c['h'], c['fl_x'], c['fl_y'], c['cx'], c['cy'], 3,
                             pix_indices=pix)
    ro, rd = ro.copy(), rd.copy()
    ro[:5] = [10.0, 10.0, 10.0]                                    # five rays that start outside and look away: they miss the box
    rd[:5] = [0.0, 0.0, 1.0]
    rays = RayBatch.__new__(RayBatch)
    rays.origins, rays.dirs = T(ro, dev), T(rd, dev)
    r.local_step = 5
    ring = r.step_counter.clone()
    out = r.render_normals(rays)
    assert r.local_step == 5 and torch.equal(r.step_counter, ring)
    N = W * H
    nm, ws = out['normal_map'], out['weights_sum']
    assert nm.shape == (N, 3) and ws.shape == (N,) and out['depth'].shape == (N,)
    # the same samples through the pieces
    near, far = R.near_far_from_aabb(rays.origins, rays.dirs, r.aabb, r.cfg.min_near)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    xyzs, _, deltas, rinfo = R.march_rays_train_nosync(rays.origins, rays.dirs, r.bound, r.march_bitfield, r.cascade, r.cfg.grid_size,
                                                       near, far, r.sample_capacity(N), counter, 0., r.cfg.max_steps)
    assert int(counter[0]) > 16 * N // 4
    sig, nrm = m.density_gradient(xyzs, m_dev=counter, density_scale=r.cfg.density_scale, normalize=True)
    ws_ref, _, img_ref = R.composite_rays_train(sig, nrm, deltas, rinfo, r.cfg.t_thresh)
    assert float(ws_ref.max()) > 0.1
    assert float((nm - img_ref).abs().max()) <= 2e-5 and float((ws - ws_ref).abs().max()) <= 2e-5
    assert torch.all(nm[:5] == 0) and torch.all(ws[:5] == 0)
    assert torch.all(nm.norm(dim=1) <= ws + 1e-5)
