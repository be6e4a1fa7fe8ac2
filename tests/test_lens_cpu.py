"""Host side of the lens refinement: the closed-form gradients of tests/lens_ref.py against torch fp64 autograd of the restated
forward, the restatement at k = 0 against the mixed-frame reference, its fp32 form against its fp64 form, LensRefiner, the
argument checks of generate_rays / generate_rays_frames / Renderer, the new entry points' symbols and host-side checks, and the
recovery loop whose step count and final loss tests/test_gpu_lens.py holds the GPU to."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frame_batch_ref as FR
import lens_ref as LR
import pose_ref as PR
from helpers import room_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 16
CAM = (20.0, 21.0, 11.5, 8.25)
SEG = [2, 0, 2, 1, 2]
KD = (-0.12, 0.03)


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _poses(F=4):
    return np.ascontiguousarray(np.asarray(room_cameras()['poses'], np.float32)[:F, :3, :])


def _batch(K, seed):
    rng = np.random.default_rng(seed)
    n = len(SEG) * K
    return (rng.integers(0, W * H, n).astype(np.int32), rng.standard_normal((n, 3)).astype(np.float32),
            rng.standard_normal((n, 3)).astype(np.float32))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('k', [(0.0, 0.0), KD])
def test_closed_form_gradients_are_autograd_of_the_forward(k, camera_flip):
    """1e-10 of sum |term| per entry: both sides are fp64 (2^-53 per operation, a few dozen operations per ray, 85 rays)"""
    K = 17
    pix, g_o, g_d = _batch(K, 3)
    poses, lens = _poses(), np.asarray(CAM + k, np.float64)
    P = torch.tensor(poses, dtype=torch.float64, requires_grad=True)
    Ln = torch.tensor(lens, requires_grad=True)
    o, d = LR.rays_torch(P, Ln, W, camera_flip, SEG, pix, K)
    ((o * torch.tensor(g_o, dtype=torch.float64)).sum() + (d * torch.tensor(g_d, dtype=torch.float64)).sum()).backward()
    want_p, mag_p, count = LR.pose_gradient(poses, W, lens, camera_flip, SEG, pix, K, g_o, g_d)
    want_l, mag_l, n = LR.lens_gradient(poses, W, lens, camera_flip, SEG, pix, K, g_o, g_d)
    assert list(count) == [K, K, 3 * K, 0] and n == 5 * K and np.all(want_p[3] == 0)
    assert np.all(np.abs(P.grad.numpy() - want_p) <= 1e-10 * mag_p)
    assert np.all(np.abs(Ln.grad.numpy() - want_l) <= 1e-10 * mag_l) and np.all(mag_l > 0)
    if k == KD:
        assert np.all(want_l != 0)
    # the fp64 rays are the differentiable forward's
    o64, d64 = LR.rays(poses, W, lens, camera_flip, SEG, pix, K)
    assert np.abs(o64 - o.detach().numpy()).max() == 0 and np.abs(d64 - d.detach().numpy()).max() <= 1e-15


@pytest.mark.parametrize('camera_flip', [0, 5])
def test_without_distortion_it_is_the_mixed_frame_reference(camera_flip):
    """k = 0: s is exactly 1, so rays and pose gradient are those of frame_batch_ref / pose_ref up to the association of fp64
    sums (1e-13 of sum |term|)"""
    K = 17
    pix, g_o, g_d = _batch(K, 4)
    poses, lens = _poses(), CAM + (0.0, 0.0)
    o, d = LR.rays(poses, W, lens, camera_flip, SEG, pix, K)
    for s, f in enumerate(SEG):
        sl = slice(s * K, (s + 1) * K)
        wo, wd = PR.generate_rays(torch.tensor(poses[f], dtype=torch.float64), W, *CAM, camera_flip, pix[sl])
        assert np.array_equal(o[sl], wo.numpy()) and np.abs(d[sl] - wd.numpy()).max() <= 1e-15
    got, mag, count = LR.pose_gradient(poses, W, lens, camera_flip, SEG, pix, K, g_o, g_d)
    want, wmag, wcount = FR.pose_gradient(poses, W, *CAM, camera_flip, SEG, pix, K, g_o, g_d)
    assert np.array_equal(count, wcount) and np.all(np.abs(got - want) <= 1e-13 * wmag) and np.all(np.abs(mag - wmag) <= 1e-13 * wmag)
    # a segment naming no frame: NaN rows, nothing in either gradient
    seg = [2, 0, -1, 1, 4]
    o, d = LR.rays(poses, W, lens, camera_flip, seg, pix, K)
    bad = np.repeat(np.asarray(seg), K)
    bad = (bad < 0) | (bad >= 4)
    assert np.isnan(o[bad]).all() and np.isnan(d[bad]).all() and np.isfinite(o[~bad]).all() and np.isfinite(d[~bad]).all()
    assert list(LR.pose_gradient(poses, W, lens, camera_flip, seg, pix, K, g_o, g_d)[2]) == [K, K, K, 0]
    assert LR.lens_gradient(poses, W, lens, camera_flip, seg, pix, K, g_o, g_d)[2] == 3 * K


def test_fp32_restatement_stays_fp32_and_close():
    """about ten fp32 roundings on values of order one: 1e-6, against differences of 1e-2 that the distortion makes"""
    K = 65
    pix = _batch(K, 5)[0]
    poses, lens = _poses(), CAM + KD
    o32, d32 = LR.rays(poses, W, lens, 5, SEG, pix, K, dtype=np.float32)
    o64, d64 = LR.rays(poses, W, lens, 5, SEG, pix, K)
    assert o32.dtype == np.float32 and d32.dtype == np.float32
    assert np.array_equal(o32, o64.astype(np.float32)) and np.abs(d32 - d64).max() <= 1e-6
    assert np.abs(np.linalg.norm(d64, axis=1) - 1).max() <= 1e-15
    plain = LR.rays(poses, W, CAM + (0.0, 0.0), 5, SEG, pix, K)[1]
    assert np.abs(plain - d64).max() > 1e-3
    # r2 <= 0.5 at this size, so s stays in [0.94, 1]
    i, j = LR.pixel_centres(W, np.arange(W * H))
    r2 = ((i - CAM[2]) / CAM[0]) ** 2 + ((j - CAM[3]) / CAM[1]) ** 2
    s = 1 + r2 * (KD[0] + r2 * KD[1])
    assert r2.max() <= 0.5 and s.min() >= 0.94 and s.max() <= 1.0


# ---- LensRefiner ---------------------------------------------------------------------------------------------------------------
def _intr(cam=CAM):
    from nerfstyle_amd.common import Intrinsics
    return Intrinsics(H, W, *cam)


def test_refiner_at_zero_is_the_intrinsics():
    from nerfstyle_amd.lens import LensRefiner
    from nerfstyle_amd.scene import load_room_cameras
    for intr in (_intr(), load_room_cameras()[1]):
        L = LensRefiner(intr)
        assert sorted(n for n, _ in L.named_parameters()) == ['center', 'dist', 'log_focal']
        assert all(p.shape == (2,) and p.dtype == torch.float32 and float(p.detach().abs().sum()) == 0 for p in L.parameters())
        out = L()
        want = torch.tensor([float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy), 0.0, 0.0], dtype=torch.float32)
        assert out.shape == (6,) and out.dtype == torch.float32 and out.requires_grad and torch.equal(out.detach(), want)
        got = L.intrinsics()
        assert got.size() == intr.size()
        assert [got.fx, got.fy, got.cx, got.cy] == [float(v) for v in want[:4]]


def test_refiner_forward_under_autograd():
    from nerfstyle_amd.lens import LensRefiner
    L = LensRefiner(_intr()).double()
    with torch.no_grad():
        L.log_focal.copy_(torch.tensor([0.03, -0.02], dtype=torch.float64))
        L.center.copy_(torch.tensor([0.7, -0.4], dtype=torch.float64))
        L.dist.copy_(torch.tensor([-0.08, 0.02], dtype=torch.float64))
    out = L()
    want = np.array([20.0 * np.exp(0.03), 21.0 * np.exp(-0.02), 11.5 + 0.7, 8.25 - 0.4, -0.08, 0.02])
    assert np.abs(out.detach().numpy() - want).max() <= 1e-14
    lin = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=torch.float64)
    (out * lin).sum().backward()
    assert np.abs(L.log_focal.grad.numpy() - want[:2] * [1.0, 2.0]).max() <= 1e-13           # d exp = exp
    assert L.center.grad.tolist() == [3.0, 4.0] and L.dist.grad.tolist() == [5.0, 6.0]
    got = L.intrinsics()
    assert abs(got.fx - want[0]) <= 1e-13 and abs(got.cy - want[3]) <= 1e-13


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_lens_of_the_wrong_shape_or_dtype_is_rejected():
    from nerfstyle_amd.rays import generate_rays, generate_rays_frames
    poses = torch.tensor(_poses(3))
    seg, pix = torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    for bad in (torch.zeros(5), torch.zeros(6, dtype=torch.float64), torch.zeros(1, 6), [20.0, 21.0, 11.5, 8.25, 0.0, 0.0]):
        with pytest.raises(ValueError, match='lens'):
            generate_rays_frames(poses, seg, pix, 4, _intr(), lens=bad)
        with pytest.raises(ValueError, match='lens'):
            generate_rays(poses[0], _intr(), pix_subset=pix, lens=bad)
    # a well-formed lens on the host reaches the library's refusal: there is no CPU path
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        generate_rays_frames(poses, seg, pix, 4, _intr(), lens=torch.zeros(6))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        generate_rays(poses[0], _intr(), pix_subset=pix, lens=torch.zeros(6))


def test_renderer_refuses_a_lens_under_ndc(built):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.dataset import FrameBatch
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=False)
    poses, intr, _ = load_room_cameras()
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=5)
    r.update_occ = False
    batch = FrameBatch(torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), 2, 4)
    P = torch.tensor(np.asarray(poses, np.float32)[:3, :3])
    lens = torch.zeros(6)
    r.cfg.use_ndc = True
    with pytest.raises(NotImplementedError, match='use_ndc.*focal length'):
        r.render_frames(P, batch, lens=lens)
    with pytest.raises(NotImplementedError, match='use_ndc.*focal length'):
        r.render(P[0], pix_subset=batch.pix, training=True, lens=lens)
    r.cfg.use_ndc = False
    # a camera tensor like the pose: the pose-gradient refusals apply to a lens that requires grad
    r.pose_gradients = True
    r.model.train_density_table = False
    with pytest.raises(NotImplementedError, match='pose_gradients'):
        r.render_frames(P, batch, lens=lens.clone().requires_grad_())


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_host_side_checks(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    want = {'nsr_generate_rays_lens': 13, 'nsr_generate_rays_lens_backward': 16, 'nsr_generate_rays_lens_backward_workspace_bytes': 3}
    with open(os.path.join(ROOT, 'include', 'nsr.h')) as f:
        header = f.read()
    for name, nargs in want.items():
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert name + '(' in header
    assert 'NOT OpenCV' in header
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)

    def fwd(S=2, K=4, poses=fake, lens=fake, seg=fake, out=fake, w=8, F=3):
        return L.nsr_generate_rays_lens(poses, F, w, 8, lens, 0, seg, fake, S, K, out, fake, None)
    assert fwd(S=0) == 0 and fwd(K=0, out=None) == 0                          # empty work is a no-op success
    assert fwd(poses=None) == -1 and fwd(lens=None) == -1 and fwd(seg=None) == -1 and fwd(out=None) == -1
    assert fwd(w=0) == -1 and fwd(F=0) == -1 and fwd(S=1 << 20, K=1 << 20) == -1

    def bwd(S=2, K=4, ws=fake, lens=fake, out=fake, w=8, F=3):
        return L.nsr_generate_rays_lens_backward(fake, F, w, 8, lens, 0, fake, fake, S, K, fake, fake, ws, None, out, None)
    assert bwd(out=None) == -1 and bwd(lens=None) == -1 and bwd(ws=None) == -1 and bwd(w=0) == -1
    assert bwd(ws=ctypes.c_void_p(4100)) == -1 and bwd(S=1 << 20, K=1 << 20) == -1
    wsb, fsb = L.nsr_generate_rays_lens_backward_workspace_bytes, L.nsr_generate_rays_frames_backward_workspace_bytes
    for K in (1, 63, 64, 257, 16500, 1 << 22):                                # the mixed-frame mapping, 18 sums for its 12
        assert wsb(3, 5, K) * 12 == fsb(3, 5, K) * 18
    assert wsb(3, 5, 63) == 5 * 18 * 8 and wsb(3, 5, 257) == 5 * 2 * 18 * 8 and wsb(3, 0, 7) >= 8


# ---- recovery --------------------------------------------------------------------------------------------------------------------
def test_recovery_on_the_restatement():
    """The loop of tests/test_gpu_lens.py::test_recovery on the fp64 restatement: with lens_ref.REC_RATES the loss is below 1 % of
    its start for the first time after REC_STEPS steps, at REC_LOSS_CPU -- the figures the GPU run is held to."""
    from nerfstyle_amd.lens import LensRefiner
    poses = np.asarray(room_cameras()['poses'], np.float64)[:3, :3, :]
    pix, target = LR.recovery_problem(poses)
    P = torch.tensor(poses)
    refiner = LensRefiner(_intr(LR.REC_CAM)).double()
    losses = LR.recovery_loop(refiner, lambda lens: LR.rays_torch(P, lens, LR.REC_W, LR.REC_FLIP, LR.REC_SEG, pix, LR.REC_K)[1],
                              torch.tensor(target, dtype=torch.float64), LR.REC_STEPS)
    print('start %.9e, after %d steps %.9e' % (losses[0], LR.REC_STEPS, losses[-1]))
    assert abs(losses[0] - LR.REC_LOSS_START) <= 1e-6 * LR.REC_LOSS_START
    assert all(v >= 0.01 * losses[0] for v in losses[:-1]) and losses[-1] < 0.01 * losses[0]
    assert abs(losses[-1] - LR.REC_LOSS_CPU) <= 1e-6 * LR.REC_LOSS_CPU
    # towards the true lens, not merely downhill
    got, zero, true = refiner().detach().numpy(), np.asarray(LR.REC_CAM + (0.0, 0.0)), np.asarray(LR.REC_TRUE)
    assert np.all(np.abs(got[:4] - true[:4]) < np.abs(zero[:4] - true[:4]))
