"""GPU: lens refinement -- nsr_generate_rays_lens against nsr_generate_rays_frames (k = 0, bit for bit) and against the fp64
restatement of tests/lens_ref.py (k != 0), nsr_generate_rays_lens_backward against the fp64 closed form, both under graph capture
with the lens changed between replays, the gradient through generate_rays_frames / Renderer into LensRefiner's parameters, and the
recovery of a true lens from ray directions.

Bars.  Forward with distortion: 4 x the largest error of the fp32 restatement (the kernel's operations in the kernel's order)
against fp64 on the same inputs, measured in the test -- the convention of k_field_xgrad's test.  Backward: the bound of any
fp32 summation order with the product's rounding, count * 2^-23 * sum |term| per entry, as tests/test_gpu_frame_batch.py.
Recovery: 2 x the final loss of the same loop on the fp64 restatement (lens_ref.REC_*; the factor allows for the fp32 forward)."""
import numpy as np
import pytest
import torch

import lens_ref as LR
from helpers import render_setup, room_cameras

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
W, H = 24, 16
CAM = (20.0, 21.0, 11.5, 8.25)                       # fx, fy, cx, cy
KD = (-0.12, 0.03)                                   # r2 <= 0.5 at this size: s stays in [0.94, 1] (test_lens_cpu.py)
SEG = [2, 0, 2, 1, 2]
GUARD = 64
KS = [1, 63, 64, 65, 257]
# the backward's mapping is the mixed-frame one: a thread per segment below K = 64, then ceil(K / 256) blocks per segment, at
# most 64: 1000 is four blocks with a partial last one, 16500 is 65 blocks' worth on 64
KS_BWD = KS + [1000, 16500]


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _poses(F=3):
    return np.ascontiguousarray(np.asarray(room_cameras()['poses'], np.float32)[:F, :3, :])


def _lens(k=(0.0, 0.0), cam=CAM):
    return np.asarray(tuple(cam) + tuple(k), np.float32)


def _guarded(n, dev, dtype=torch.float32, fill=7.0, inner=None):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    if inner is not None:
        buf[GUARD:GUARD + n] = inner
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=7.0):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


# ---- 1. / 2. forward -------------------------------------------------------------------------------------------------------------
def _forward(dev, poses_d, lens_d, seg_d, pix_d, S, K, flip, F):
    from nerfstyle_amd import _lib as L
    N = S * K
    bo, ro = _guarded(N * 3, dev)
    bd, rd = _guarded(N * 3, dev)
    L.check(L.lib().nsr_generate_rays_lens(L.p(poses_d), F, W, H, L.p(lens_d), flip, L.p(seg_d), L.p(pix_d), S, K, L.p(ro), L.p(rd),
                                           L.stream()), 'generate_rays_lens')
    assert _guards_intact(bo, N * 3) and _guards_intact(bd, N * 3)
    return ro.view(N, 3).clone(), rd.view(N, 3).clone()


@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('K', KS)
def test_forward_without_distortion_is_generate_rays_frames(dev, K, camera_flip):
    from nerfstyle_amd import _lib as L
    poses, S, F = _poses(), len(SEG), 3
    pix = np.random.default_rng(100 * K + camera_flip).integers(0, W * H, S * K).astype(np.int32)
    poses_d, pix_d, seg_d, lens_d = T(poses, dev), T(pix, dev), T(np.asarray(SEG, np.int32), dev), T(_lens(), dev)
    want_o, want_d = torch.empty(S * K, 3, device=dev), torch.empty(S * K, 3, device=dev)
    L.check(L.lib().nsr_generate_rays_frames(L.p(poses_d), F, W, H, *CAM, camera_flip, L.p(seg_d), L.p(pix_d), S, K, L.p(want_o),
                                             L.p(want_d), L.stream()), 'generate_rays_frames')
    got_o, got_d = _forward(dev, poses_d, lens_d, seg_d, pix_d, S, K, camera_flip, F)
    assert torch.equal(got_o, want_o) and torch.equal(got_d, want_d) and bool(torch.isfinite(got_d).all())
    # a segment that names no frame: NaN rows for it, the others untouched
    for bad_s, bad in ((3, F), (0, -1)):
        seg = np.asarray(SEG, np.int32)
        seg[bad_s] = bad
        o, d = _forward(dev, poses_d, lens_d, T(seg, dev), pix_d, S, K, camera_flip, F)
        sel = torch.zeros(S * K, dtype=torch.bool, device=dev)
        sel[bad_s * K:(bad_s + 1) * K] = True
        assert bool(torch.isnan(o[sel]).all()) and bool(torch.isnan(d[sel]).all())
        assert torch.equal(o[~sel], want_o[~sel]) and torch.equal(d[~sel], want_d[~sel])


@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('K', KS)
def test_forward_with_distortion(dev, K, camera_flip):
    """Measured on an MI355X: the kernel's directions are the fp32 restatement's bit for bit at every shape; the restatement's
    largest error against fp64 is 3.2e-8 (K = 1) .. 1.384e-7 (K = 63)."""
    poses, S, F = _poses(), len(SEG), 3
    pix = np.random.default_rng(200 * K + camera_flip).integers(0, W * H, S * K).astype(np.int32)
    lens = _lens(KD)
    got_o, got_d = _forward(dev, T(poses, dev), T(lens, dev), T(np.asarray(SEG, np.int32), dev), T(pix, dev), S, K, camera_flip, F)
    o64, d64 = LR.rays(poses, W, lens, camera_flip, SEG, pix, K)
    o32, d32 = LR.rays(poses, W, lens, camera_flip, SEG, pix, K, dtype=np.float32)
    own = float(np.abs(d32 - d64).max())
    err = float(np.abs(got_d.cpu().numpy().astype(np.float64) - d64).max())
    print('K=%d flip=%d: fp32 restatement against fp64 %.3e, kernel against fp64 %.3e (bar %.3e), kernel == restatement: %s'
          % (K, camera_flip, own, err, 4 * own, np.array_equal(got_d.cpu().numpy(), d32)))
    assert own > 0 and err <= 4 * own
    assert np.array_equal(got_o.cpu().numpy(), o32) and np.array_equal(o32, o64.astype(np.float32))
    assert float((got_d.double().norm(dim=1) - 1).abs().max()) < 1e-6


# ---- 3. backward -----------------------------------------------------------------------------------------------------------------
def _backward(dev, poses_d, lens_d, seg_d, pix_d, go_d, gd_d, S, K, flip, F, with_poses=True, ws=None):
    """-> (grad_poses [F,3,4] or None, grad_lens [6]); the workspace arrives as NaN between guard bands unless one is handed in"""
    from nerfstyle_amd import _lib as L
    n_ws = int(L.lib().nsr_generate_rays_lens_backward_workspace_bytes(F, S, K)) // 8
    wbuf = None
    if ws is None:
        wbuf, ws = _guarded(n_ws, dev, dtype=torch.float64, inner=float('nan'))
    pbuf, gp = _guarded(F * 12, dev)
    lbuf, gl = _guarded(6, dev)
    L.check(L.lib().nsr_generate_rays_lens_backward(L.p(poses_d), F, W, H, L.p(lens_d), flip, L.p(seg_d), L.p(pix_d), S, K, L.p(go_d),
                                                    L.p(gd_d), L.p(ws), L.p(gp) if with_poses else None, L.p(gl), L.stream()),
            'generate_rays_lens_backward')
    assert _guards_intact(pbuf, F * 12) and _guards_intact(lbuf, 6) and (wbuf is None or _guards_intact(wbuf, n_ws))
    if not with_poses:
        assert bool((gp == 7.0).all())
    return (gp.view(F, 3, 4).clone() if with_poses else None), gl.clone()


def _frames_backward(dev, poses_d, seg_d, pix_d, go_d, gd_d, S, K, flip, F):
    from nerfstyle_amd import _lib as L
    ws = torch.full((int(L.lib().nsr_generate_rays_frames_backward_workspace_bytes(F, S, K)) // 8,), float('nan'), dtype=torch.float64,
                    device=dev)
    out = torch.empty(F, 3, 4, device=dev)
    L.check(L.lib().nsr_generate_rays_frames_backward(L.p(poses_d), F, W, H, *CAM, flip, L.p(seg_d), L.p(pix_d), S, K, L.p(go_d), L.p(gd_d),
                                                      L.p(ws), L.p(out), L.stream()), 'generate_rays_frames_backward')
    return out


@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('K', KS_BWD)
def test_backward(dev, K, camera_flip):
    """Measured on an MI355X: err / bound prints as 0.000 at every shape, for the pose rows and the lens row (the sums are fp64)."""
    F, S = 4, len(SEG)                                  # frame 3 is in no segment
    poses = _poses(F)
    rng = np.random.default_rng(7 * K + camera_flip)
    pix = rng.integers(0, W * H, S * K).astype(np.int32)
    g_o, g_d = rng.standard_normal((S * K, 3)).astype(np.float32), rng.standard_normal((S * K, 3)).astype(np.float32)
    poses_d, lens = T(poses, dev), _lens(KD)
    lens_d = T(lens, dev)

    def run(seg, pix, g_o, g_d, lens_d=lens_d):
        a = (T(np.asarray(seg, np.int32), dev), T(pix, dev), T(g_o, dev), T(g_d, dev))
        gp, gl = _backward(dev, poses_d, lens_d, *a, S, K, camera_flip, F)
        gp2, gl2 = _backward(dev, poses_d, lens_d, *a, S, K, camera_flip, F)
        assert torch.equal(gp, gp2) and torch.equal(gl, gl2)                             # two calls: the same bits
        only = _backward(dev, poses_d, lens_d, *a, S, K, camera_flip, F, with_poses=False)
        assert only[0] is None and torch.equal(only[1], gl)                              # grad_poses = NULL: the lens row unchanged
        return gp.cpu().numpy(), gl.cpu().numpy()

    def check(got, seg, pix, g_o, g_d, what, lens=lens):
        gp, gl = got
        want, mag, count = LR.pose_gradient(poses, W, lens, camera_flip, seg, pix, K, g_o, g_d)
        err, bound = np.abs(gp - want), count[:, None, None] * U23 * mag
        for f in range(F):
            if count[f]:
                print('K=%d flip=%d %s frame %d (%d rays): max err / bound %.3f' % (K, camera_flip, what, f, count[f],
                                                                                     float((err[f] / bound[f]).max())))
                assert np.any(gp[f] != 0)
            else:
                assert np.all(gp[f] == 0)                 # exact zeros
        assert np.all(np.isfinite(gp)) and np.all(err <= bound)
        want_l, mag_l, n = LR.lens_gradient(poses, W, lens, camera_flip, seg, pix, K, g_o, g_d)
        err_l, bound_l = np.abs(gl - want_l), n * U23 * mag_l
        print('K=%d flip=%d %s lens (%d rays): err / bound %s' % (K, camera_flip, what, n, ' '.join('%.3f' % v for v in err_l / bound_l)))
        assert np.all(np.isfinite(gl)) and np.all(err_l <= bound_l) and np.all(gl != 0)

    got = run(SEG, pix, g_o, g_d)
    assert list(LR.pose_gradient(poses, W, lens, camera_flip, SEG, pix, K, g_o, g_d)[2]) == [K, K, 3 * K, 0]
    check(got, SEG, pix, g_o, g_d, 'as drawn')
    # segments 0 and 1 (frames 2 and 0) trade places with their rays: the same sums in another order
    order = np.concatenate([np.arange(s * K, (s + 1) * K) for s in (1, 0, 2, 3, 4)])
    seg2 = [SEG[1], SEG[0]] + SEG[2:]
    got2 = run(seg2, pix[order], g_o[order], g_d[order])
    check(got2, seg2, pix[order], g_o[order], g_d[order], 'swapped')
    check(got2, SEG, pix, g_o, g_d, 'swapped, against the unswapped reference')
    # a segment naming no frame adds nothing, to either result
    seg3 = list(SEG)
    seg3[2] = -1
    check(run(seg3, pix, g_o, g_d), seg3, pix, g_o, g_d, 'one segment out of range')
    # without distortion the pose rows are the mixed-frame backward's, bit for bit
    plain = _lens()
    gp0, gl0 = run(SEG, pix, g_o, g_d, lens_d=T(plain, dev))
    frames = _frames_backward(dev, poses_d, T(np.asarray(SEG, np.int32), dev), T(pix, dev), T(g_o, dev), T(g_d, dev), S, K, camera_flip, F)
    assert np.array_equal(gp0, frames.cpu().numpy())
    check((gp0, gl0), SEG, pix, g_o, g_d, 'k = 0', lens=plain)


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [5, 257])
def test_graph_replays_read_the_lens_on_the_device(dev, K):
    from nerfstyle_amd import _lib as L
    F, S, N, flip = 4, len(SEG), len(SEG) * K, 3
    poses_d = T(_poses(F), dev)
    rng = np.random.default_rng(K)
    seg_d, pix_d = T(np.asarray(SEG, np.int32), dev), T(rng.integers(0, W * H, N).astype(np.int32), dev)
    go_d, gd_d = T(rng.standard_normal((N, 3)).astype(np.float32), dev), T(rng.standard_normal((N, 3)).astype(np.float32), dev)
    lens_d = T(_lens(KD), dev)
    ws = torch.empty(int(L.lib().nsr_generate_rays_lens_backward_workspace_bytes(F, S, K)) // 8, dtype=torch.float64, device=dev)
    out = [torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev), torch.empty(F, 3, 4, device=dev), torch.empty(6, device=dev)]

    def call():
        L.check(L.lib().nsr_generate_rays_lens(L.p(poses_d), F, W, H, L.p(lens_d), flip, L.p(seg_d), L.p(pix_d), S, K, L.p(out[0]),
                                               L.p(out[1]), L.stream()), 'generate_rays_lens')
        L.check(L.lib().nsr_generate_rays_lens_backward(L.p(poses_d), F, W, H, L.p(lens_d), flip, L.p(seg_d), L.p(pix_d), S, K, L.p(go_d),
                                                        L.p(gd_d), L.p(ws), L.p(out[2]), L.p(out[3]), L.stream()),
                'generate_rays_lens_backward')
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = []
    for lens in (_lens(KD), _lens((0.05, -0.02), cam=(20.6, 21.63, 12.2, 7.85))):
        lens_d.copy_(T(lens, dev))                          # outside the graph: what an optimiser step does
        eager = _forward(dev, poses_d, lens_d, seg_d, pix_d, S, K, flip, F) + _backward(dev, poses_d, lens_d, seg_d, pix_d, go_d, gd_d, S, K,
                                                                                       flip, F)
        for t in out:
            t.fill_(7.0)
        ws.fill_(float('nan'))
        graph.replay()
        for got, want in zip(out, eager):
            assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and float(want.abs().sum()) > 0
        seen.append([t.clone() for t in out])
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[0][3], seen[1][3])


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------------
DENSITY_SCALE = 40.0
S_R, K_R = 4, 96
FRAMES_R = [0, 1, 1, 0]


def _renderer_and_batch(dev):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd.dataset import FrameBatch
    r, _, poses, intr, _ = render_setup(dev, nc=5, compute_dtype=torch.float16, contrast=16.0)
    r.cfg.density_scale = DENSITY_SCALE
    r.pose_gradients = True
    Wf, Hf = intr.size()
    seg = torch.empty(S_R, dtype=torch.int32, device=dev)
    pix = torch.empty(S_R * K_R, dtype=torch.int32, device=dev)
    rows = torch.empty(S_R * K_R, dtype=torch.int64, device=dev)
    L.check(L.lib().nsr_draw_frame_batch(2, Wf * Hf, S_R, K_R, 1234, 0, None, 0, L.p(T(np.asarray(FRAMES_R, np.int32), dev)), 0, L.p(seg),
                                         L.p(pix), L.p(rows), L.stream()), 'draw_frame_batch')
    return r, np.asarray(poses, np.float32)[:3, :3, :], intr, FrameBatch(seg, pix, rows, S_R, K_R)


def _refiner(intr, dev):
    from nerfstyle_amd.lens import LensRefiner
    Lr = LensRefiner(intr).to(dev)
    with torch.no_grad():                                   # off zero, so that forward()'s Jacobian is not the identity
        Lr.log_focal.copy_(torch.tensor([0.01, -0.005]))
        Lr.center.copy_(torch.tensor([0.7, -0.4]))
        Lr.dist.copy_(torch.tensor([-0.05, 0.01]))
    return Lr


def _grads(Lr):
    return [getattr(Lr, k).grad.clone() for k in ('log_focal', 'center', 'dist')]


def test_lens_gradient_through_the_renderer(dev):
    """The bound of test_backward carried through forward()'s Jacobian (diag(fx, fy, 1, 1, 1, 1)); torch's two roundings in that
    product are below it: count >= 2 and sum |term| >= |sum|."""
    from nerfstyle_amd.rays import generate_rays_frames
    r, poses, intr, batch = _renderer_and_batch(dev)
    N, Wf = S_R * K_R, intr.size()[0]
    target = torch.tensor(np.random.default_rng(4).random((N, 3)).astype(np.float32), device=dev)

    def loss_of(rgb):
        return ((rgb - target) ** 2).sum() * (1.0 / N)

    # (a) rays made by hand, their gradients kept
    La, Pa = _refiner(intr, dev), T(poses, dev).clone().requires_grad_()
    lens_a = La()
    rays = generate_rays_frames(Pa, batch.seg_frame, batch.pix, batch.K, intr, camera_flip=r.cfg.flip_camera, pose_grad=True, lens=lens_a)
    assert rays.origins.requires_grad and rays.dirs.requires_grad
    rays.origins.retain_grad()
    rays.dirs.retain_grad()
    rgb_a, trans_a, cls_a = r.render_train(rays, dense=False)
    assert float(trans_a.min()) < 0.5                                                    # the rays do hit the seeded scene
    loss_of(rgb_a).backward()
    g_o, g_d = rays.origins.grad.cpu().numpy(), rays.dirs.grad.cpu().numpy()
    lens_v = lens_a.detach().cpu().numpy()
    want, mag, n = LR.lens_gradient(poses, Wf, lens_v, r.cfg.flip_camera, FRAMES_R, batch.pix.cpu().numpy(), K_R, g_o, g_d)
    jac = np.asarray([lens_v[0], lens_v[1], 1.0, 1.0, 1.0, 1.0], np.float64)
    got = torch.cat(_grads(La)).cpu().numpy()
    err, bound = np.abs(got - want * jac), n * U23 * mag * jac
    print('log_focal, center, dist: |grad| %s, err / bound %s' % (' '.join('%.3e' % v for v in got), ' '.join('%.3f' % v for v in err / bound)))
    assert n == N and np.all(got != 0) and np.all(err <= bound)
    want_p, mag_p, count = LR.pose_gradient(poses, Wf, lens_v, r.cfg.flip_camera, FRAMES_R, batch.pix.cpu().numpy(), K_R, g_o, g_d)
    assert np.all(np.abs(Pa.grad.cpu().numpy() - want_p) <= count[:, None, None] * U23 * mag_p) and np.all(Pa.grad[2].cpu().numpy() == 0)

    # (b) the same through render_frames: bit for bit
    Lb, Pb = _refiner(intr, dev), T(poses, dev).clone().requires_grad_()
    out = r.render_frames(Pb, batch, lens=Lb())
    loss_of(out['rgb_map']).backward()
    assert torch.equal(out['rgb_map'], rgb_a) and torch.equal(out['trans_map'], trans_a) and torch.equal(out['classes'], cls_a)
    assert all(torch.equal(a, b) for a, b in zip(_grads(La), _grads(Lb))) and torch.equal(Pa.grad, Pb.grad)
    # the lens alone: no pose gradient is asked for, the lens gradient is the same
    Lc = _refiner(intr, dev)
    out = r.render_frames(T(poses, dev), batch, lens=Lc())
    loss_of(out['rgb_map']).backward()
    assert all(torch.equal(a, c) for a, c in zip(_grads(La), _grads(Lc)))
    # renders without a gradient take the refined rays: the single-pose call makes the batch's rows, a test render sees the lens
    with torch.no_grad(), r.occupancy_frozen():
        lens_c, P0, first = Lc(), T(poses[0], dev), batch.pix[:K_R]                      # segment 0 is frame 0
        rows = r.render_frames(T(poses, dev), batch, lens=lens_c)
        one = r.render(P0, pix_subset=first, training=True, lens=lens_c)
        assert all(torch.equal(one[k], rows[k][:K_R]) for k in ('rgb_map', 'trans_map', 'classes'))
        seen, blind = r.render(P0, pix_subset=first, lens=lens_c), r.render(P0, pix_subset=first)
        assert not seen['rgb_map'].requires_grad and not torch.equal(seen['rgb_map'], blind['rgb_map'])

    # (d) NDC reads the focal length of the fixed intrinsics
    r.cfg.use_ndc = True
    with pytest.raises(NotImplementedError, match='use_ndc.*focal length'):
        r.render_frames(Pb, batch, lens=Lb())
    r.cfg.use_ndc = False

    # (c) lens=None on this renderer: the renderer that was never given a lens
    def plain(rr):
        P = T(poses, dev).clone().requires_grad_()
        o = rr.render_frames(P, batch)
        loss_of(o['rgb_map']).backward()
        return [o[k].detach() for k in ('rgb_map', 'trans_map', 'classes')] + [P.grad]
    fresh = _renderer_and_batch(dev)[0]
    for a, b in zip(plain(r), plain(fresh)):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    assert not torch.equal(plain(r)[0], rgb_a.detach())                                  # and the lens did change the picture


def test_single_pose_is_one_frame_one_segment(dev):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.rays import generate_rays, generate_rays_frames
    intr, poses = Intrinsics(H, W, *CAM), T(_poses(), dev)
    pix = T(np.random.default_rng(1).integers(0, W * H, 300).astype(np.int32), dev)
    seg = torch.zeros(1, dtype=torch.int32, device=dev)
    plain, _ = generate_rays(poses[1], intr, pix_subset=pix, camera_flip=5)
    same, _ = generate_rays(poses[1], intr, pix_subset=pix, camera_flip=5, lens=T(_lens(), dev))
    assert torch.equal(plain.origins, same.origins) and torch.equal(plain.dirs, same.dirs) and not same.dirs.requires_grad
    g = torch.tensor(np.random.default_rng(2).standard_normal((2, 300, 3)).astype(np.float32), device=dev)
    grads = []
    for one in (True, False):
        P, Ln = poses[1].clone().requires_grad_(), T(_lens(KD), dev).requires_grad_()
        if one:
            rays, _ = generate_rays(P, intr, pix_subset=pix, camera_flip=5, pose_grad=True, lens=Ln)
        else:
            rays = generate_rays_frames(P[None], seg, pix, 300, intr, camera_flip=5, pose_grad=True, lens=Ln)
        ((rays.origins * g[0]).sum() + (rays.dirs * g[1]).sum()).backward()
        grads.append((rays.dirs.detach(), P.grad, Ln.grad))
    assert all(torch.equal(a, b) and float(a.abs().sum()) > 0 for a, b in zip(*grads))
    # pose_grad off: constants, as without a lens
    rays, _ = generate_rays(poses[1].clone().requires_grad_(), intr, pix_subset=pix, lens=T(_lens(KD), dev).requires_grad_())
    assert not rays.dirs.requires_grad


# ---- 6. recovery -----------------------------------------------------------------------------------------------------------------
def test_recovery(dev):
    """From LensRefiner zero towards lens_ref.REC_TRUE (focal +3 %, centre (+0.7, -0.4) px, k = (-0.08, 0.02)) on 5 x 257 rays
    over 3 frames: torch Adam, rates log_focal 2e-3 / center 5e-2 / dist 5e-3, 37 steps -- on the fp64 restatement the loss
    sum |d - d*|^2 falls from 1.856717 to 1.455943e-2 in those steps, below 1 % of its start for the first time
    (tests/test_lens_cpu.py::test_recovery_on_the_restatement).  The GPU run must end at or below twice that."""
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.lens import LensRefiner
    from nerfstyle_amd.rays import generate_rays_frames
    assert (LR.REC_STEPS, LR.REC_LOSS_CPU, LR.REC_RATES) == (37, 1.455943470e-02, {'log_focal': 2e-3, 'center': 5e-2, 'dist': 5e-3})
    poses = _poses()
    pix, target = LR.recovery_problem(poses)
    intr = Intrinsics(LR.REC_H, LR.REC_W, *LR.REC_CAM)
    P, seg_d, pix_d = T(poses, dev), T(np.asarray(LR.REC_SEG, np.int32), dev), T(pix, dev)
    refiner = LensRefiner(intr).to(dev)
    losses = LR.recovery_loop(refiner, lambda lens: generate_rays_frames(P, seg_d, pix_d, LR.REC_K, intr, camera_flip=LR.REC_FLIP,
                                                                         pose_grad=True, lens=lens).dirs, T(target, dev), LR.REC_STEPS)
    print('loss %.6e -> %.6e after %d steps (fp64 restatement on the CPU: %.6e -> %.6e); lens %s' % (
        losses[0], losses[-1], LR.REC_STEPS, LR.REC_LOSS_START, LR.REC_LOSS_CPU, refiner().detach().cpu().numpy()))
    assert abs(losses[0] - LR.REC_LOSS_START) <= 1e-4 * LR.REC_LOSS_START
    assert losses[-1] <= 2 * LR.REC_LOSS_CPU
