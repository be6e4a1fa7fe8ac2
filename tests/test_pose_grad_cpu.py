"""Host side of the camera pose gradients: the reference chain of tests/pose_ref.py is trustworthy (its rays are the golden
ones, its fp64 gradient passes gradcheck), PoseRefiner, the new entry points' symbols, signatures and argument checks, the
refusals of Renderer.pose_gradients and its default."""
import ctypes

import numpy as np
import pytest
import torch

import pose_ref
from helpers import room_cameras, small_scene


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _cam(c):
    return (c['w'], c['fl_x'], c['fl_y'], c['cx'], c['cy'], 3)


def test_restated_generate_rays_matches_the_goldens(golden):
    c = room_cameras()
    pose = torch.tensor(golden['pose0'], dtype=torch.float32)
    o, d = pose_ref.generate_rays(pose, *_cam(c), golden['rays_rand_idx'])
    assert np.abs(d.numpy()[:512] - golden['rays_rand_d']).max() <= 1.2e-7      # test_oracle_cpu.py's bar
    assert np.array_equal(o.numpy()[:512], golden['rays_rand_o'])
    sel = golden['rays_full_sel']
    o, d = pose_ref.generate_rays(pose, *_cam(c), np.arange(c['w'] * c['h'])[sel])
    assert np.abs(d.numpy() - golden['rays_full_d']).max() <= 1.2e-7


def _small_frame(O, W=6, H=4):
    """a W x H grid of pixels of room frame 0 marched by the CPU oracle through the seeded occupancy"""
    c = room_cameras()
    ys, xs = np.meshgrid(np.arange(H) * (c['h'] // H) + 7, np.arange(W) * (c['w'] // W) + 5, indexing='ij')
    pix = (ys * c['w'] + xs).reshape(-1)
    pose = np.asarray(c['poses'][0], np.float64)[:3]
    o, d = pose_ref.generate_rays(torch.tensor(pose, dtype=torch.float32), *_cam(c), pix)
    _, bits = small_scene()
    near, far = O.near_far_from_aabb(o.numpy(), d.numpy(), np.array([-2, -2, -2, 2, 2, 2], np.float32), 0.2)
    xyzs, _, deltas, rays, counter = O.march_rays_train(o.numpy(), d.numpy(), 2.0, bits, 2, 128, near, far, max_steps=64)
    return c, pix, pose, xyzs, deltas, rays, W * H * 64


def test_reference_chain_passes_gradcheck_in_float64(O):
    from oracle import torch_port as TP
    c, pix, pose, xyzs, deltas, rays, cap = _small_frame(O)
    assert 50 < xyzs.shape[0] < cap
    field = TP.Field(num_classes=2, table_scale=0.5).double()
    with torch.no_grad():
        field.p_density[2048:] *= 16
        field.p_color2[-1024:] *= 16
    target = np.random.default_rng(0).random((len(pix), 3))

    p = torch.tensor(pose, dtype=torch.float64, requires_grad=True)
    t = pose_ref.march_parameters(p.detach(), _cam(c), pix, xyzs, rays)

    def loss(p):
        return pose_ref.render_loss(p, _cam(c), pix, t, deltas, rays, cap, field, target, density_scale=40.0)[0]
    g, = torch.autograd.grad(loss(p), p)
    assert float(g.norm()) > 0
    # the rays, t and the live set are held fixed by construction (t is detached, the march is not re-run); the hash grid is
    # piecewise trilinear, so the step stays far below a finest cell (4 / 4096) and kinks under it show up as a loose atol
    assert torch.autograd.gradcheck(loss, (p,), eps=1e-7, atol=1e-5 * float(g.abs().max()), rtol=1e-3, nondet_tol=0.0)


def test_sample_parameter_is_the_marchs(O):
    """xyz = o + t d with t recovered from the marched positions; the composite's running sum of deltas[:, 1] is that
    parameter PLUS the step minus near -- what nsr_rays_position_backward corrects for when it is given nears."""
    c, pix, pose, xyzs, deltas, rays, cap = _small_frame(O)
    p32 = torch.tensor(pose, dtype=torch.float32)
    t = pose_ref.march_parameters(p32, _cam(c), pix, xyzs, rays)
    pts = pose_ref.positions(p32, _cam(c), pix, t, rays)
    assert np.abs(pts.numpy() - xyzs).max() <= 1e-5
    o, d = pose_ref.generate_rays(p32, *_cam(c), pix)
    near, _ = O.near_far_from_aabb(o.numpy(), d.numpy(), np.array([-2, -2, -2, 2, 2, 2], np.float32), 0.2)
    for n, off, cnt in rays:
        if cnt:
            run = np.cumsum(deltas[off:off + cnt, 1].astype(np.float64))
            assert np.abs(near[n] + run - deltas[off:off + cnt, 0] - t.numpy()[off:off + cnt]).max() <= 2e-5


# ---- PoseRefiner ------------------------------------------------------------------------------------------------------
def test_pose_refiner_zero_correction_is_the_stored_pose():
    from nerfstyle_amd.pose import PoseRefiner
    poses = torch.tensor(room_cameras()['poses'], dtype=torch.float32)
    pr = PoseRefiner(poses)
    assert pr.delta.shape == (poses.shape[0], 6) and float(pr.delta.abs().sum()) == 0
    assert [n for n, _ in pr.named_parameters()] == ['delta'] and 'poses' in dict(pr.named_buffers())
    for f in (0, 3, poses.shape[0] - 1):
        out = pr(f)
        assert out.shape == (3, 4) and out.requires_grad
        assert torch.equal(out.detach(), poses[f, :3, :])


def test_pose_refiner_exp_is_a_rotation_and_passes_gradcheck():
    from nerfstyle_amd.pose import PoseRefiner, se3_exp
    rng = np.random.default_rng(1)
    for scale in (0.0, 1e-6, 1e-3, 0.3, 2.5):
        R, _ = se3_exp(torch.tensor(rng.standard_normal(6) * scale, dtype=torch.float32))
        R = R.double()
        assert float((R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
        assert abs(float(torch.linalg.det(R)) - 1) <= 1e-6
    poses = torch.tensor(room_cameras()['poses'], dtype=torch.float64)[:3]
    pr = PoseRefiner(poses).double()
    for scale in (0.0, 1e-5, 0.2):
        d0 = torch.tensor(rng.standard_normal((3, 6)) * scale, dtype=torch.float64, requires_grad=True)

        def f(d):
            pr.delta.data = d.data
            R, t = se3_exp(d[1])
            P = pr.poses[1]
            return torch.cat((R @ P[:, :3], (R @ P[:, 3] + t)[:, None]), dim=1)
        assert torch.autograd.gradcheck(f, (d0,), eps=1e-6, atol=1e-7)
        with torch.no_grad():
            pr.delta.copy_(d0)
        assert torch.allclose(pr(1), f(d0), rtol=0, atol=0)
    # at zero: d pose / d translation part is the identity, d / d axis-angle the generators applied to the pose
    pr = PoseRefiner(poses).double()
    out = pr(0)
    g, = torch.autograd.grad(out[:, 3].sum(), pr.delta)
    assert torch.equal(g[0, 3:], torch.ones(3, dtype=torch.float64)) and float(g[1:].abs().sum()) == 0


# ---- entry points --------------------------------------------------------------------------------------------------------
def _desc(Lv=16):
    from nerfstyle_amd import _lib
    offsets = (np.arange(17, dtype=np.int32) * 4096).copy()
    d = _lib.FieldDesc()
    d.L, d.H, d.S, d.num_classes = Lv, 16, 0.5, 5
    d.table_dtype, d.compute_dtype = _lib.NSR_F16, _lib.NSR_F16
    for i in range(3):
        d.bbox_min[i], d.bbox_size[i] = -2.0, 4.0
    d.density_scale = 1.0
    d.offsets = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return d, offsets


def test_symbols_signatures_and_host_side_checks(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    want = {'nsr_field_position_gradient': 9, 'nsr_rays_position_backward': 10, 'nsr_generate_rays_backward': 15,
            'nsr_generate_rays_backward_workspace_bytes': 1}
    for name, nargs in want.items():
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == nargs
    with open(_lib.LIB_PATH.replace('nerfstyle_amd/libnsr_hip.so', 'include/nsr.h')) as f:
        header = f.read()
    assert all(name + '(' in header for name in want)
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)
    desc, keep = _desc()

    def xgrad(d=ctypes.byref(desc), M=8, out=fake, tables=fake, eg=fake):
        return L.nsr_field_position_gradient(d, tables, fake, M, None, eg, None, out, None)
    assert xgrad(M=0) == 0 and xgrad(d=None, M=0, out=None) == 0            # empty work is a no-op success
    assert xgrad(d=None) == -1 and xgrad(out=None) == -1 and xgrad(eg=None) == -1
    assert xgrad(tables=ctypes.c_void_p(4100)) == -1 and xgrad(eg=ctypes.c_void_p(4104)) == -1
    desc8, keep8 = _desc(Lv=8)
    assert xgrad(d=ctypes.byref(desc8)) == -2                              # NSR_ERR_UNSUPPORTED: 16 levels or nothing

    def rays(N=4, ndc=0, go=fake, deltas=fake):
        return L.nsr_rays_position_backward(fake, deltas, fake, None, 64, N, ndc, go, fake, None)
    assert rays(N=0) == 0 and rays(N=0, go=None) == 0
    assert rays(ndc=1) == -2 and rays(N=0, ndc=1) == -2
    assert rays(go=None) == -1 and rays(deltas=ctypes.c_void_p(4100)) == -1

    def gen(N=4, pix=fake, ws=fake, out=fake, w=8, h=8):
        return L.nsr_generate_rays_backward(fake, w, h, 1.0, 1.0, 0.0, 0.0, 0, pix, N, fake, fake, ws, out, None)
    assert gen(N=0) == 0 and gen(N=0, out=None, ws=None) == 0
    assert gen(out=None) == -1 and gen(ws=None) == -1 and gen(w=0) == -1
    assert gen(pix=None, N=63) == -1                                        # no pixel list: N must be the whole frame
    assert L.nsr_generate_rays_backward_workspace_bytes(1) >= 12 * 8
    assert L.nsr_generate_rays_backward_workspace_bytes(1 << 20) == L.nsr_generate_rays_backward_workspace_bytes(5000)


# ---- the switch ----------------------------------------------------------------------------------------------------------
def _renderer(ndc=False, view_dependent=False):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=view_dependent, view_dependent=view_dependent)
    poses, intr, _ = load_room_cameras()
    cfg = RendererConfig.llff()
    cfg.use_ndc = ndc
    r = Renderer(m, cfg, intr, 2.0, raymarch_channels=5)
    r.update_occ = False
    return r, torch.tensor(np.asarray(poses[0], np.float32)[:3], requires_grad=True)


def test_switch_defaults_to_off_and_refusals_name_their_reason(built):
    from nerfstyle_amd.common import Box2D
    r, pose = _renderer()
    assert r.pose_gradients is False
    patch = Box2D(8, 8, 4, 4)

    def refuses(r, word, **kw):
        with pytest.raises(NotImplementedError, match=word):
            r.render(pose, patch=patch, training=True, **kw)
    r.pose_gradients = True
    r.model._spatial_scatter_unsupported = True
    refuses(r, 'spatial table scatter')
    r.model._spatial_scatter_unsupported = False
    r.model.train_density_table = False
    refuses(r, 'colour-only')
    r.model.train_density_table, r.model.train_mlps = True, False
    refuses(r, 'colour-only')
    r.model.train_mlps = True
    r.fused_nograd_train = True
    refuses(r, 'fused')
    r.fused_nograd_train, r.fused_inference = False, True
    refuses(r, 'fused')
    r.fused_inference = False
    r.model.train_density_table = False
    with pytest.raises(NotImplementedError, match='pose_gradients'):           # the two-halves entry refuses as well
        r.begin_train(pose, torch.arange(16, dtype=torch.int32))
    r.model.train_density_table = True
    r2, _ = _renderer(ndc=True)
    r2.pose_gradients = True
    refuses(r2, 'use_ndc')
    r3, _ = _renderer(view_dependent=True)
    r3.pose_gradients = True
    refuses(r3, 'view_dependent')
    # everything servable, but the tensors live on the CPU: the library's usual answer
    with pytest.raises(RuntimeError, match='HIP device'):
        r.render(pose, patch=patch, training=True)
    # the field's own door
    with pytest.raises(NotImplementedError, match='perm'):
        r.model.field(torch.zeros(4, 3, requires_grad=True), pos_grad=True)
