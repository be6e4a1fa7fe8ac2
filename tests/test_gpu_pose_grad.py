"""GPU: camera pose gradients through the training render -- the three kernels alone (nsr_field_position_gradient,
nsr_rays_position_backward, nsr_generate_rays_backward), the chain through the fused field, the end-to-end pose gradient of
Renderer.render against tests/pose_ref.py, the switch's off state, and the three kernels under graph capture.

Bars.  Kernel 1: the one tests/test_gpu_grid_input_grad.py holds nsr_grid_encode_input_backward to (rel-L2 against fp64
autograd at most 4x that of the same restatement in fp32; the same arithmetic per level).  Kernels 2 and 3: the bound of any
fp32 summation order with the product's rounding, n * 2^-23 * sum |term| per output.  Chain and end to end: rel-L2 5e-3 (f16) /
3e-2 (bf16), the project's bars for gradients through rounded operands."""
import ctypes

import numpy as np
import pytest
import torch

import pose_ref
from helpers import rel_l2, render_setup, room_cameras, room_rays, small_scene

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


# ---- kernel 1 --------------------------------------------------------------------------------------------------------------
_MODELS, _K1REF = {}, {}


def _model(dev, table_half, table_scale, dt='f16'):
    key = (table_half, table_scale, dt)
    if key not in _MODELS:
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
        m.load_state_dict(sd)
        _MODELS[key] = (m.to(dev), ref)
    return _MODELS[key]


def _k1_inputs(M):
    rng = np.random.default_rng(40 + M)
    pts = (rng.random((M, 3)) * 4 - 2).astype(np.float32)
    bad = []
    if M >= 15:
        pts[3] = [0.3, np.nan, -0.2]
        pts[5] = [2.5, 0.1, 0.2]                       # outside the box
        pts[7] = [2.0, -0.7, 1.1]                      # exactly on a box face: the last cell, fraction 1
        bad = [3, 5]
    m_dev = M - max(1, M // 8)                         # < M; M = 1: nothing is live
    eg = rng.standard_normal((M, 16, 4)).astype(np.float32)
    perm = np.arange(M, dtype=np.int32)
    perm[:m_dev] = rng.permutation(m_dev)
    return pts, bad, m_dev, eg, perm


def _k1_reference(ref, pts, eg, good, table_half, dtype):
    """d / d position of sum(enc_grad * encode(u)) over both tables, through torch_port.grid_encode from the fp32 encoder input"""
    from oracle import torch_port as TP
    u32 = ((pts[good] - np.float32(-2.0)) / np.float32(4.0) + np.float32(1.0)) / np.float32(2.0)      # field_unit, fp32
    u = torch.tensor(u32, dtype=dtype, requires_grad=True)
    g = torch.tensor(eg[good], dtype=dtype)
    tot = 0
    for emb, sl in ((ref.emb_density, slice(0, 2)), (ref.emb_color, slice(2, 4))):
        e = emb.detach()
        e = (e.to(torch.float16) if table_half else e).to(dtype)
        enc = TP.grid_encode(u, e, ref.offsets, ref.pls, base_resolution=ref.min_res)
        tot = tot + (enc.view(-1, 16, 2) * g[:, :, sl]).sum()
    tot.backward()
    return u.grad.numpy().astype(np.float64) / (2 * 4.0)


def _run_k1(m, dev, pts, m_dev, eg_d, perm, M):
    from nerfstyle_amd import _lib as L
    out = torch.full((M, 3), 7.0, device=dev)
    desc = m._desc(1.0)
    cnt = torch.tensor([m_dev, 0], dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(m._gather_tables()), L.p(pts), M, L.p(cnt), L.p(eg_d),
                                                L.p(perm), L.p(out), L.stream()), 'field_position_gradient')
    return out


@pytest.mark.parametrize('table_scale', [1e-4, 1.0])
@pytest.mark.parametrize('table_half', [False, True])
@pytest.mark.parametrize('M', [1, 15, 17, 117])
def test_position_gradient_kernel(dev, M, table_half, table_scale):
    m, ref = _model(dev, table_half, table_scale)
    pts, bad, m_dev, eg, perm = _k1_inputs(M)
    good = np.ones(M, bool)
    good[bad] = False
    good[m_dev:] = False
    # the workspace arrives with NaN bytes wherever the kernel must not look: invalid samples and slots past the count
    eg_in = eg.copy()
    eg_in[~good] = np.nan
    pts_d, eg_d, perm_d = T(pts, dev), T(eg_in, dev), T(perm, dev)
    got = _run_k1(m, dev, pts_d, m_dev, eg_d, None, M)
    assert torch.equal(got, _run_k1(m, dev, pts_d, m_dev, eg_d, None, M))               # two calls: the same bits
    assert torch.equal(got, _run_k1(m, dev, pts_d, m_dev, eg_d, perm_d, M))             # with perm: the same bits per sample
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g)) and np.all(g[~good] == 0)
    if not good.any():
        return
    want, w32 = (_k1_reference(ref, pts, eg, good, table_half, d) for d in (torch.float64, torch.float32))
    e_kernel, e_f32 = rel_l2(g[good], want), rel_l2(w32, want)
    print('M=%d half=%d tables +-%g: kernel %.3e  float32 restatement %.3e' % (M, table_half, table_scale, e_kernel, e_f32))
    assert np.linalg.norm(want) > 0 and e_f32 > 0
    if M >= 15:
        assert np.any(g[7] != 0)
    assert e_kernel <= 4 * e_f32


# ---- kernel 2 --------------------------------------------------------------------------------------------------------------
def _k2_inputs():
    rng = np.random.default_rng(7)
    counts = [63, 0, 1, 130, 64, 65, 5]                # the last one is dropped: it ends at the buffer's end
    offs, off = [], 0
    for i, c in enumerate(counts):
        offs.append(off)
        off += c + (2 if i == 3 else 0)                # two slots no ray owns
    M = off
    N = len(counts)
    rays = np.stack([rng.permutation(N), offs, counts], 1).astype(np.int32)
    deltas = np.zeros((M, 4), np.float32)
    deltas[:, 0] = rng.uniform(0.002, 0.006, M)
    deltas[:, 1] = deltas[:, 0] * rng.uniform(1.0, 3.0, M).astype(np.float32)
    g = rng.standard_normal((M, 3)).astype(np.float32)
    nears = rng.uniform(0.2, 1.5, N).astype(np.float32)
    return rays, deltas, g, nears, M, N


@pytest.mark.parametrize('with_nears', [False, True])
def test_rays_position_backward(dev, with_nears):
    from nerfstyle_amd import raymarching as R
    rays, deltas, g, nears, M, N = _k2_inputs()
    args = (T(g, dev), T(deltas, dev), T(rays, dev), M, T(nears, dev) if with_nears else None)
    go, gd = R.rays_position_backward(*args)
    go2, gd2 = R.rays_position_backward(*args)
    assert torch.equal(go, go2) and torch.equal(gd, gd2)
    go, gd = go.cpu().numpy().astype(np.float64), gd.cpu().numpy().astype(np.float64)
    for n, (idx, off, cnt) in enumerate(rays):
        if cnt == 0 or off + cnt >= M:
            assert np.all(go[idx] == 0) and np.all(gd[idx] == 0)
            continue
        gi = g[off:off + cnt].astype(np.float64)
        t = np.cumsum(deltas[off:off + cnt, 1].astype(np.float64))
        # with nears: the sample's own parameter; its two extra fp32 operations are two more roundings of t per term
        extra = 0
        if with_nears:
            t, extra = np.float64(nears[idx]) + t - deltas[off:off + cnt, 0], 2
        term = t[:, None] * gi
        assert np.all(np.abs(go[idx] - gi.sum(0)) <= cnt * U23 * np.abs(gi).sum(0))
        err, bound = np.abs(gd[idx] - term.sum(0)), (cnt + extra) * U23 * np.abs(term).sum(0)
        print('count %3d: d/d dir err / bound %s' % (cnt, err / bound))
        assert np.all(err <= bound)
    with pytest.raises(RuntimeError, match='unsupported'):
        R.rays_position_backward(args[0], args[1], args[2], M, None, is_ndc=True)


# ---- kernel 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('N', [1, 255, 257, 5000])
def test_generate_rays_backward(dev, N, camera_flip):
    from nerfstyle_amd import _lib as L
    c = room_cameras()
    rng = np.random.default_rng(N + camera_flip)
    pix = rng.choice(c['w'] * c['h'], size=N, replace=False).astype(np.int32)
    pose = np.asarray(c['poses'][2], np.float32)[:3]
    fx, fy, cx, cy = (float(np.float32(c[k])) for k in ('fl_x', 'fl_y', 'cx', 'cy'))
    g_o, g_d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    ws = torch.full((int(L.lib().nsr_generate_rays_backward_workspace_bytes(N)) // 8,), float('nan'), dtype=torch.float64, device=dev)
    pose_d, pix_d, go_d, gd_d = T(pose, dev), T(pix, dev), T(g_o, dev), T(g_d, dev)

    def run():
        out = torch.full((3, 4), 7.0, device=dev)
        L.check(L.lib().nsr_generate_rays_backward(L.p(pose_d), c['w'], c['h'], fx, fy, cx, cy, camera_flip, L.p(pix_d), N, L.p(go_d),
                                                   L.p(gd_d), L.p(ws), L.p(out), L.stream()), 'generate_rays_backward')
        return out
    got = run()
    assert torch.equal(got, run())
    p = torch.tensor(pose, dtype=torch.float64, requires_grad=True)
    o, d = pose_ref.generate_rays(p, c['w'], fx, fy, cx, cy, camera_flip, pix)
    ((o * torch.tensor(g_o, dtype=torch.float64)).sum() + (d * torch.tensor(g_d, dtype=torch.float64)).sum()).backward()
    want = p.grad.numpy()
    # sum |term| per entry, from the formula: h_n c_n^T with h = (I - d d^T) g_d / |v|, and |g_o| for the translation
    cd = pose_ref.camera_dirs(c['w'], fx, fy, cx, cy, camera_flip, pix, torch.float64).numpy()
    v = cd @ pose[:, :3].astype(np.float64).T
    nv = np.linalg.norm(v, axis=1, keepdims=True)
    dn = v / nv
    h = (g_d - dn * (dn * g_d).sum(1, keepdims=True)) / nv
    terms = np.concatenate((h[:, :, None] * cd[:, None, :], g_o.astype(np.float64)[:, :, None]), axis=2)      # [N,3,4]
    assert np.abs(terms.sum(0) - want).max() <= 1e-11 * np.abs(terms).sum(0).max()
    err, bound = np.abs(got.cpu().numpy() - want), N * U23 * np.abs(terms).sum(0)
    print('N=%d flip=%d: max err / bound %.3f' % (N, camera_flip, float((err / bound).max())))
    assert np.all(err <= bound)


# ---- chain through the field ----------------------------------------------------------------------------------------------------
DENSITY_SCALE = 40.0
M_CHAIN, M_CHAIN_DEV = 117, 108


def _marched(O, dev, n_rays=64, cap=256):
    from nerfstyle_amd import raymarching as R
    _, bits = small_scene()
    ro, rd = room_rays(O, n_rays, seed=3)
    aabb = T(np.array([-2, -2, -2, 2, 2, 2], np.float32), dev)
    near, far = R.near_far_from_aabb(T(ro, dev), T(rd, dev), aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    xyzs, _, _, _ = R.march_rays_train_nosync(T(ro, dev), T(rd, dev), 2.0, T(bits, dev), 2, 128, near, far, n_rays * cap, counter, 0., 1024)
    assert int(counter[0]) >= M_CHAIN + 100
    return xyzs[100:100 + M_CHAIN].contiguous()


@pytest.mark.parametrize('dt,table_half', [('f16', False), ('f16', True), ('bf16', True)])
def test_position_gradient_through_the_field(O, dev, dt, table_half):
    r, ref, _, _, _ = render_setup(dev, nc=5, table_dtype=None if table_half else torch.float32,
                                   compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16, contrast=16.0)
    m = r.model
    pts = _marched(O, dev).requires_grad_()
    cnt = torch.tensor([M_CHAIN_DEV, 0], dtype=torch.int32, device=dev)
    rng = np.random.default_rng(11)
    gs, gr = rng.standard_normal(M_CHAIN).astype(np.float32), rng.standard_normal((M_CHAIN, 8)).astype(np.float32)
    perm = m.sample_order(pts.detach(), cnt)
    sig, rgb = m.field(pts, m_dev=cnt, density_scale=DENSITY_SCALE, perm=perm, pos_grad=True)
    ((sig * T(gs, dev))[:M_CHAIN_DEV].sum() + (rgb * T(gr, dev))[:M_CHAIN_DEV].sum()).backward()
    got = pts.grad.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(got[M_CHAIN_DEV:] == 0)
    assert not m._spatial_scatter_unsupported and m.arena.grad is not None
    pt = torch.tensor(pts.detach().cpu().numpy()[:M_CHAIN_DEV], requires_grad=True)
    out, s = ref(pt, half=dt, table_half=table_half)
    ((s[:, 0] * DENSITY_SCALE * torch.tensor(gs[:M_CHAIN_DEV])).sum() + (out * torch.tensor(gr[:M_CHAIN_DEV])).sum()).backward()
    want = pt.grad.numpy()
    err = rel_l2(got[:M_CHAIN_DEV], want)
    print('field chain %s table_half=%d: rel-L2 %.3e (|want| %.3e)' % (dt, table_half, err, np.linalg.norm(want)))
    assert np.linalg.norm(want) > 0
    assert err <= (5e-3 if dt == 'f16' else 3e-2)
    # a field call without the switch: positions stay constants
    p2 = pts.detach().clone().requires_grad_()
    sig2, _ = m.field(p2, m_dev=cnt, density_scale=DENSITY_SCALE, perm=perm)
    sig2[:M_CHAIN_DEV].sum().backward()
    assert p2.grad is None


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _e2e_render(r, pose, image, patch):
    out = r.render(pose, image, patch=patch, training=True)
    loss = ((out['rgb_map'] - out['target']) ** 2).mean()
    loss.backward()
    return out, loss


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_pose_gradient_end_to_end(dev, dt):
    from nerfstyle_amd.common import Box2D, RayBatch
    from nerfstyle_amd.rays import generate_rays, pixel_ids
    cd = torch.float16 if dt == 'f16' else torch.bfloat16
    r, ref, poses, intr, _ = render_setup(dev, nc=5, compute_dtype=cd, contrast=16.0)
    r.cfg.density_scale = DENSITY_SCALE
    patch = Box2D(480, 360, 24, 16)
    W, H = intr.size()
    image = torch.tensor(np.random.default_rng(2).random((3, H, W)).astype(np.float32), device=dev)
    pose0 = np.asarray(poses[0], np.float32)[:3]
    pose = torch.tensor(pose0, device=dev, requires_grad=True)
    r.pose_gradients = True
    out, loss = _e2e_render(r, pose, image, patch)
    assert pose.grad is not None and pose.grad.shape == (3, 4)
    got = pose.grad.cpu().numpy()

    # the reference on the same marched samples
    with torch.no_grad():
        rays, _ = generate_rays(pose.detach(), intr, None, patch=patch, camera_flip=r.cfg.flip_camera, device=dev)
        mt = r.march_train(rays)
    n = int(mt['counter'][0])
    assert 1000 < n < mt['M']
    pix = pixel_ids(intr, patch)[0].numpy()
    cam = (W, float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy), int(r.cfg.flip_camera))
    xyzs, deltas, rinfo = (mt[k].cpu().numpy() for k in ('xyzs', 'deltas', 'rays_info'))
    p = torch.tensor(pose0, requires_grad=True)
    t = pose_ref.march_parameters(p.detach(), cam, pix, xyzs[:n], rinfo)
    ref_loss, ref_rgb = pose_ref.render_loss(p, cam, pix, t, deltas[:n], rinfo, mt['M'], ref, out['target'].cpu().numpy(),
                                             density_scale=DENSITY_SCALE, T_thresh=r.cfg.t_thresh, half=dt, table_half=False)
    ref_loss.backward()
    want = p.grad.numpy()
    print('rgb_map: max |kernel - reference| %.3e' % float((ref_rgb.detach() - out['rgb_map'].detach().cpu()).abs().max()))
    # non-trivial: far above the rounding noise of the loss itself
    assert np.linalg.norm(want) > 1e3 * np.finfo(np.float32).eps * float(ref_loss)
    bar = 5e-3 if dt == 'f16' else 3e-2
    err = rel_l2(got, want)
    flipped = want.copy()
    flipped[:, 3] *= -1
    print('pose gradient %s: rel-L2 %.3e, |want| %.3e, loss %.3e, with the translation negated %.3e' % (
        dt, err, np.linalg.norm(want), float(ref_loss), rel_l2(got, flipped)))
    assert rel_l2(got, flipped) > bar               # sensitivity: a wrong sign of the translation column does not pass
    assert err <= bar

    # off: the switch off, or a pose that does not require grad -- the bits of a renderer that never had the switch set
    base, _, _, _, _ = render_setup(dev, nc=5, compute_dtype=cd, contrast=16.0)
    base.cfg.density_scale = DENSITY_SCALE
    b_out, _ = _e2e_render(base, torch.tensor(pose0, device=dev), image, patch)
    # The field backward accumulates arena.grad with fp32 atomics whose order is not fixed: two runs of one renderer differ in
    # the last bits (measured: 5.6e-9 on gradients of order 1).  The reference's own run-to-run difference is therefore the
    # yardstick for arena.grad: bit-identical when the reference repeats itself bit for bit, else within 4x that difference.
    base_grad = base.model.arena.grad.clone()
    base.model.arena.grad.zero_()
    _e2e_render(base, torch.tensor(pose0, device=dev), image, patch)
    spread = float((base.model.arena.grad - base_grad).abs().max())
    print('never-set renderer, two runs: max |arena.grad difference| %.3e' % spread)
    for switch, req in ((False, True), (True, False)):
        r.model.arena.grad.zero_()
        r.pose_gradients = switch
        p2 = torch.tensor(pose0, device=dev, requires_grad=req)
        o2, _ = _e2e_render(r, p2, image, patch)
        assert p2.grad is None
        for k in ('rgb_map', 'trans_map', 'classes'):
            assert torch.equal(o2[k], b_out[k])
        d = float((r.model.arena.grad - base_grad).abs().max())
        print('switch=%s requires_grad=%s: max |arena.grad difference| %.3e' % (switch, req, d))
        assert torch.equal(r.model.arena.grad != 0, base_grad != 0)
        # (the floor 2^-20 max|grad| keeps a by-chance small spread of two runs from failing a third: 16 ulps of the largest entry)
        assert torch.equal(r.model.arena.grad, base_grad) if spread == 0 else d <= max(4 * spread, 2.0 ** -20 * float(base_grad.abs().max()))


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_three_kernels_graph_replays_equal_eager(dev):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import raymarching as R
    m, _ = _model(dev, True, 1.0)
    M = 117
    pts, bad, m_dev, eg, perm = _k1_inputs(M)
    rng = np.random.default_rng(3)
    counts = [40, 0, 64, 12]                           # 116 samples in four rays, the last slot unowned
    rays = np.stack([[2, 0, 3, 1], np.cumsum([0] + counts[:-1]), counts], 1).astype(np.int32)
    deltas = np.zeros((M, 4), np.float32)
    deltas[:, 0] = rng.uniform(0.002, 0.006, M)
    deltas[:, 1] = deltas[:, 0] * np.float32(1.5)
    c = room_cameras()
    pose = T(np.asarray(c['poses'][0], np.float32)[:3], dev)
    pix = T(rng.choice(c['w'] * c['h'], size=4, replace=False).astype(np.int32), dev)
    fx, fy, cx, cy = (float(c[k]) for k in ('fl_x', 'fl_y', 'cx', 'cy'))
    pts_d, perm_d, rays_d, deltas_d = T(pts, dev), T(perm, dev), T(rays, dev), T(deltas, dev)
    nears = T(rng.uniform(0.2, 1.0, 4).astype(np.float32), dev)
    eg_d = T(eg, dev)
    desc = m._desc(1.0)
    cnt = torch.tensor([m_dev, 0], dtype=torch.int32, device=dev)
    tables = m._gather_tables()
    ws = torch.empty(int(L.lib().nsr_generate_rays_backward_workspace_bytes(4)) // 8, dtype=torch.float64, device=dev)

    def chain():
        gx = torch.empty(M, 3, device=dev)
        L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(tables), L.p(pts_d), M, L.p(cnt), L.p(eg_d), L.p(perm_d),
                                                    L.p(gx), L.stream()), 'field_position_gradient')
        go, gd = R.rays_position_backward(gx, deltas_d, rays_d, M, nears)
        gp = torch.empty(3, 4, device=dev)
        L.check(L.lib().nsr_generate_rays_backward(L.p(pose), c['w'], c['h'], fx, fy, cx, cy, 3, L.p(pix), 4, L.p(go), L.p(gd), L.p(ws),
                                                   L.p(gp), L.stream()), 'generate_rays_backward')
        return gx, gp
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx_g, gp_g = chain()
    for k in range(2):
        eg_d.copy_(T(np.random.default_rng(50 + k).standard_normal((M, 16, 4)).astype(np.float32), dev))
        gx_e, gp_e = (t.clone() for t in chain())
        gx_g.fill_(7.0)
        gp_g.fill_(7.0)
        graph.replay()
        assert torch.equal(gx_g, gx_e) and torch.equal(gp_g, gp_e)
        assert float(gp_e.abs().sum()) > 0
