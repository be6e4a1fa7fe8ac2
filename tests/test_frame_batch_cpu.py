"""Host side of the mixed-frame batches: the restated Philox against the Random123 known answers, the batched se(3)
exponential against the per-frame one, the dataset's row tables, the new entry points' symbols and signatures, and the answers
of render_frames and draw to CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frame_batch_ref as FR
from helpers import room_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


# ---- Philox --------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(x[0]) for x in FR.philox(*ctr, *key))
        assert got == want, [hex(g) for g in got]
    # vectorised over the first counter word: the same words as one call each
    many = FR.philox(np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344]),
                     np.array([0, 0xa4093822]), np.array([0, 0x299f31d0]))
    assert tuple(int(x[0]) for x in many) == KAT[0][2] and tuple(int(x[1]) for x in many) == KAT[2][2]


def test_restated_draw_is_in_range_and_keyed():
    seg, pix, rows = FR.draw(7, 384, 5, 64, seed=0x123456789abcdef, seq=3)
    assert seg.shape == (5,) and pix.shape == rows.shape == (320,)
    assert seg.min() >= 0 and seg.max() < 7 and pix.min() >= 0 and pix.max() < 384
    assert np.array_equal(rows, np.repeat(seg.astype(np.int64), 64) * 384 + pix)
    assert len(np.unique(pix)) > 150                                           # 320 uniform draws of 384: 217 distinct expected
    for other in (dict(seed=0x123456789abcdef, seq=4), dict(seed=0x123456789abcdee, seq=3), dict(seed=0x123456789abcdef, seq=3, stream_id=1)):
        assert not np.array_equal(FR.draw(7, 384, 5, 64, **other)[1], pix)
    fixed = FR.draw(7, 384, 5, 64, seed=0x123456789abcdef, seq=3, fixed_frames=[6, 6, 0, 1, 2])
    assert list(fixed[0]) == [6, 6, 0, 1, 2] and np.array_equal(fixed[1], pix)


# ---- batched se(3) ---------------------------------------------------------------------------------------------------------
def _deltas(kind, F, rng):
    if kind == 'zero':
        return np.zeros((F, 6))
    if kind == 'small':                       # |w|^2 below the series threshold 1e-8, translations ordinary
        d = rng.standard_normal((F, 6))
        d[:, :3] *= 3e-5
        return d
    if kind == 'mixed':                       # rows on both sides of the threshold, and a zero row
        d = rng.standard_normal((F, 6)) * 0.3
        d[0, :3] *= 1e-5
        d[1] = 0
        return d
    return rng.standard_normal((F, 6)) * 0.3


@pytest.mark.parametrize('kind', ['zero', 'small', 'mixed', 'ordinary'])
def test_forward_all_is_forward_per_frame(kind):
    """1e-12: a few dozen fp64 operations (2^-53 each) on magnitudes <= 10 -- derived, not measured"""
    from nerfstyle_amd.pose import PoseRefiner, se3_exp, se3_exp_many
    rng = np.random.default_rng(5)
    poses = torch.tensor(room_cameras()['poses'], dtype=torch.float64)[:5]
    F = poses.shape[0]
    pr = PoseRefiner(poses).double()
    with torch.no_grad():
        pr.delta.copy_(torch.tensor(_deltas(kind, F, rng)))
    if kind == 'small':
        assert float((pr.delta[:, :3] ** 2).sum(1).max()) < 1e-8
    allp = pr.forward_all()
    assert allp.shape == (F, 3, 4) and allp.dtype == torch.float64 and allp.requires_grad
    lin = torch.tensor(rng.standard_normal((F, 3, 4)))
    g_all, = torch.autograd.grad((allp * lin).sum(), pr.delta)
    g_one = torch.zeros_like(g_all)
    for f in range(F):
        one = pr(f)
        assert float((allp[f] - one).abs().max()) <= 1e-12
        g_one += torch.autograd.grad((one * lin[f]).sum(), pr.delta)[0]
        R, t = se3_exp(pr.delta[f])
        Rm, tm = se3_exp_many(pr.delta)
        assert float((Rm[f] - R).abs().max()) <= 1e-12 and float((tm[f] - t).abs().max()) <= 1e-12
    assert torch.isfinite(g_all).all() and float(g_all.abs().max()) > 0
    assert float((g_all - g_one).abs().max()) <= 1e-12
    if kind == 'zero':
        assert torch.equal(allp.detach(), pr.poses)
    if kind == 'mixed':
        assert torch.equal(allp[1].detach(), pr.poses[1])


def test_forward_all_at_zero_is_the_stored_poses_in_float32():
    from nerfstyle_amd.pose import PoseRefiner
    poses = torch.tensor(room_cameras()['poses'], dtype=torch.float32)          # [F,4,4]
    pr = PoseRefiner(poses)
    out = pr.forward_all()
    assert out.shape == (poses.shape[0], 3, 4) and out.requires_grad
    assert torch.equal(out.detach(), poses[:, :3, :])


# ---- dataset rows ----------------------------------------------------------------------------------------------------------
def _cpu_dataset(seg=True):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    rng = np.random.default_rng(9)
    images = rng.random((3, 3, 4, 6)).astype(np.float32)
    seg_maps = rng.integers(0, 5, (3, 4, 6)) if seg else None
    poses = np.asarray(room_cameras()['poses'], np.float32)[:3]
    return ResidentDataset(images, poses, Intrinsics(4, 6, 5.0, 5.0, 3.0, 2.0), 2.0, 'cpu', seg_maps=seg_maps, num_classes=5)


def test_dataset_row_tables():
    ds = _cpu_dataset()
    rgb, cls = ds.target_rgb_rows, ds.target_cls_rows
    assert rgb.shape == (3 * 24, 3) and rgb.dtype == torch.float32 and rgb.is_contiguous()
    assert cls.shape == (3 * 24,) and cls.dtype == torch.int64 and cls.is_contiguous()
    for f in range(3):
        for p in range(24):
            assert torch.equal(rgb[f * 24 + p], ds.targets[f, p, :3])
            assert int(cls[f * 24 + p]) == int(ds.targets[f, p, 3])
    assert ds.target_rgb_rows is rgb and ds.target_cls_rows is cls             # built once
    # sample() is untouched by them
    pose, tgt = ds.sample(1, torch.tensor([5, 0]))
    assert torch.equal(tgt, ds.targets[1][[5, 0]]) and pose.shape == (4, 4)
    plain = _cpu_dataset(seg=False)
    assert plain.target_rgb_rows.shape == (72, 3)
    with pytest.raises(AttributeError, match='segment maps'):
        plain.target_cls_rows


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_host_side_checks(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    want = {'nsr_generate_rays_frames': 16, 'nsr_generate_rays_frames_backward': 18,
            'nsr_generate_rays_frames_backward_workspace_bytes': 3, 'nsr_draw_frame_batch': 14}
    with open(os.path.join(ROOT, 'include', 'nsr.h')) as f:
        header = f.read()
    for name, nargs in want.items():
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert name + '(' in header
    assert 'UNIFORM WITH REPLACEMENT' in header
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION == 6
    fake = ctypes.c_void_p(4096)

    def fwd(S=2, K=4, poses=fake, seg=fake, out=fake, w=8, F=3):
        return L.nsr_generate_rays_frames(poses, F, w, 8, 1.0, 1.0, 0.0, 0.0, 0, seg, fake, S, K, out, fake, None)
    assert fwd(S=0) == 0 and fwd(K=0, out=None) == 0                          # empty work is a no-op success
    assert fwd(poses=None) == -1 and fwd(seg=None) == -1 and fwd(out=None) == -1 and fwd(w=0) == -1 and fwd(F=0) == -1
    assert fwd(S=1 << 20, K=1 << 20) == -1                                    # S * K past 32 bits

    def bwd(S=2, K=4, ws=fake, out=fake, w=8, F=3):
        return L.nsr_generate_rays_frames_backward(fake, F, w, 8, 1.0, 1.0, 0.0, 0.0, 0, fake, fake, S, K, fake, fake, ws, out, None)
    assert bwd(F=0) == 0 and bwd(F=0, out=None) == 0
    assert bwd(out=None) == -1 and bwd(ws=None) == -1 and bwd(w=0) == -1 and bwd(ws=ctypes.c_void_p(4100)) == -1
    wsb = L.nsr_generate_rays_frames_backward_workspace_bytes
    assert wsb(3, 5, 1) == wsb(3, 5, 63) == 5 * 12 * 8                        # a thread per segment
    assert wsb(3, 5, 64) == 5 * 12 * 8 and wsb(3, 5, 257) == 5 * 2 * 12 * 8   # blocks per segment
    assert wsb(3, 5, 1 << 20) == wsb(3, 5, 1 << 22)                           # capped
    assert wsb(3, 0, 7) >= 8

    def drw(S=2, K=4, seqdev=None, advance=0, pix=fake, F=3, P=64):
        return L.nsr_draw_frame_batch(F, P, S, K, 1, 0, seqdev, 0, None, advance, fake, pix, fake, None)
    assert drw(S=0) == 0
    assert drw(pix=None) == -1 and drw(F=0) == -1 and drw(P=0) == -1
    assert drw(advance=1) == -1 and drw(S=0, advance=1) == -1                # advance needs the device word


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_inference_are_refused(built):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.dataset import FrameBatch
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    ds = _cpu_dataset()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds.draw(2, 4, seed=1)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=False)
    poses, intr, _ = load_room_cameras()
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=5)
    r.update_occ = False
    batch = FrameBatch(torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), 2, 4)
    P = torch.tensor(np.asarray(poses, np.float32)[:3, :3])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        r.render_frames(P, batch)
    with pytest.raises(NotImplementedError, match='training render'):
        r.render_frames(P, batch, training=False)
    # the pose-gradient refusals are the single-pose path's
    r.pose_gradients = True
    r.model.train_density_table = False
    with pytest.raises(NotImplementedError, match='pose_gradients'):
        r.render_frames(P.clone().requires_grad_(), batch)
