"""Host side of per-frame exposure: the NumPy restatement (tests/exposure_ref.py) differentiates its own value correctly;
ExposureRefiner fixes the gauge as documented; the two entry points' symbols and host-side checks; recon_loss refuses what the
host layer promises to refuse.

Bars.  Finite differences: central, step 1e-5, in fp64, 1e-6 relative per element -- the value is quadratic in rgb_map (a central
difference is exact but for ~1e-16 * value / step of cancellation) and a sum of exponentials in exposure (truncation
step^2 * ln2^2 / 6 ~ 1e-11 relative).  The recovery loop's end error on the restatement is the number the GPU test's bar is ten
times of (exposure_ref.REC_CPU_ERR)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exposure_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _inputs(S=4, K=3, F=3, P=20, nc=4, seed=0):
    rng = np.random.default_rng(seed)
    N = S * K
    return dict(rgb_map=rng.uniform(0.05, 0.95, (N, 3)), target_rgb=rng.uniform(0.0, 1.0, (P, 3)), exposure=rng.uniform(-2.0, 2.0, (F, 3)),
                seg_frame=np.asarray([0, 2, -1, 2][:S], np.int32), K=K, pix=rng.integers(0, P, N), ray_weight=rng.uniform(0.25, 4.0, N),
                classes=rng.standard_normal((N, nc)), target_cls=rng.integers(0, nc, P), ce_lambda=1e-3, s_=512.0)


def test_reference_gradients_are_finite_differences():
    a = _inputs()
    r = XR.loss(**a)
    h = 1e-5
    for name, grad in (('exposure', r['grad_exposure']), ('rgb_map', r['grad_rgb_map'])):
        fd = np.zeros_like(grad)
        for idx in np.ndindex(*grad.shape):
            v = []
            for sign in (1.0, -1.0):
                b = dict(a)
                b[name] = a[name].copy()
                b[name][idx] += sign * h
                v.append(XR.loss(**b)['total'])
            fd[idx] = (v[0] - v[1]) / (2.0 * h)
        nz = grad != 0.0
        worst = float(np.abs(fd[nz] / grad[nz] - 1.0).max())
        print('d total / d %s: worst relative difference to central differences %.3e' % (name, worst))
        assert worst <= 1e-6 and np.all(fd[~nz] == 0.0)
    # frame 1 is named by no segment, the segment naming frame -1 reaches no row: its rays still have a colour gradient
    assert np.all(r['grad_exposure'][1] == 0.0) and np.all(r['grad_exposure'][[0, 2]] != 0.0)
    out = r['frame'] == -1
    assert out.sum() == a['K'] and np.all(r['grad_rgb_map'][out] != 0.0)


def test_reference_recovery_loop():
    rgb, target, seg, e_true = XR.recovery_inputs()
    e = torch.nn.Parameter(torch.zeros(XR.REC_F, 3))

    def grad_of():
        e.grad = torch.tensor(XR.loss(rgb, target, e.detach().numpy(), seg, XR.REC_K)['grad_exposure'], dtype=torch.float32)
    err = float(np.abs(XR.recover(e, grad_of) - e_true).max())
    print('recovery on the restatement: max |e - e_true| %.3e (recorded %.3e)' % (err, XR.REC_CPU_ERR))
    assert err <= 2.0 * XR.REC_CPU_ERR and XR.REC_BAR >= 1e-4


# ---- ExposureRefiner -----------------------------------------------------------------------------------------------------------
def test_exposure_refiner():
    from nerfstyle_amd.exposure import ExposureRefiner
    F = 5
    g = torch.Generator().manual_seed(2)
    ref = ExposureRefiner(F)
    assert ref.log2_gain.shape == (F, 3) and ref.log2_gain.dtype == torch.float32 and bool((ref.log2_gain == 0).all())
    assert [n for n, _ in ref.named_parameters()] == ['log2_gain'] and bool((ref() == 0).all())
    with torch.no_grad():
        ref.log2_gain.copy_(torch.randn(F, 3, generator=g))
    e = ref()
    assert e.shape == (F, 3) and float(e.detach().sum(0).abs().max()) <= 1e-6
    assert torch.allclose(e, ref.log2_gain - ref.log2_gain.mean(0, keepdim=True), atol=1e-7)
    # the gradient of log2_gain is the projection of the gradient of forward(): g - mean over the frames
    up = torch.randn(F, 3, generator=g)
    (e * up).sum().backward()
    assert torch.allclose(ref.log2_gain.grad, up - up.mean(0, keepdim=True), atol=1e-6)
    assert float(ref.log2_gain.grad.sum(0).abs().max()) <= 1e-6

    plain = ExposureRefiner(F, zero_mean=False)
    with torch.no_grad():
        plain.log2_gain.copy_(ref.log2_gain)
    assert torch.equal(plain(), plain.log2_gain)
    (plain() * up).sum().backward()
    assert torch.equal(plain.log2_gain.grad, up)

    rgb = torch.rand(7, 3, generator=g)
    assert torch.allclose(plain.apply(rgb, 3), rgb * 2.0 ** plain.log2_gain[3].detach(), rtol=1e-6)
    frames = torch.tensor([0, 4, 4, 1, 2, 3, 0])
    assert torch.allclose(ref.apply(rgb, frames), rgb * 2.0 ** ref()[frames].detach(), rtol=1e-6)
    # nn.Module.apply(fn) still reaches the module (a parent's apply() recurses into it)
    seen = []
    assert torch.nn.Sequential(ref).apply(lambda m: seen.append(type(m).__name__))[0] is ref and 'ExposureRefiner' in seen
    with pytest.raises(ValueError, match='num_frames'):
        ExposureRefiner(0)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    with open(os.path.join(ROOT, 'include', 'nsr.h')) as f:
        header = f.read()
    for name, nargs in (('nsr_recon_loss_exposure_workspace_bytes', 4), ('nsr_recon_loss_exposure', 23)):
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert name + '(' in header
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)

    def call(N=8, S=2, K=4, F=3, rgb=fake, exposure=fake, seg=fake, g_exp=fake, out=fake, ws=fake):
        return L.nsr_recon_loss_exposure(rgb, None, N, 0, fake, None, None, None, exposure, F, seg, S, K, 1e-3, 1.0, None, fake, None, g_exp,
                                         None, out, ws, None)
    # the shape checks come before any pointer is looked at: with every pointer null, and with none
    for bad in (dict(N=0, S=0), dict(N=0), dict(F=0), dict(S=0), dict(K=0), dict(N=9), dict(S=3), dict(S=1 << 20, K=1 << 20, N=0)):
        assert L.nsr_recon_loss_exposure(None, None, bad.get('N', 8), 0, None, None, None, None, None, bad.get('F', 3), None, bad.get('S', 2),
                                         bad.get('K', 4), 1e-3, 1.0, None, None, None, None, None, None, None, None) == -1, bad
        assert call(**bad) == -1
    # the null checks of the loss, and of the three new pointers; an unaligned workspace
    assert call(rgb=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(exposure=None) == -1 and call(seg=None) == -1 and call(g_exp=None) == -1
    assert call(ws=ctypes.c_void_p(4100)) == -1

    wb = L.nsr_recon_loss_exposure_workspace_bytes
    sizes = [wb(S * K, 3, S, K) for S, K in ((1, 1), (3, 1), (5, 63), (2, 64), (2, 65), (3, 257), (64, 64), (36, 21168), (1, 762048))]
    assert all(b % 8 == 0 and b > 0 for b in sizes)
    # grows with N: along N at fixed (S, K), and along K at fixed S; at least the staged terms, 12 bytes per ray
    fixed = [wb(N, 3, 4, 96) for N in (1, 2, 3, 383, 384, 385, 4096, 1 << 20)]
    assert all(b % 8 == 0 for b in fixed) and all(a <= b for a, b in zip(fixed, fixed[1:])) and fixed[0] < fixed[-1]
    along = [wb(3 * K, 3, 3, K) for K in (1, 63, 64, 65, 256, 257, 20000, 174763)]
    assert all(a < b for a, b in zip(along, along[1:]))
    assert all(wb(S * K, 3, S, K) >= 12 * S * K for S, K in ((1, 1), (64, 64), (3, 174763)))


# ---- host layer ----------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def test_recon_loss_refuses(built, monkeypatch):
    from nerfstyle_amd import _lib
    from nerfstyle_amd.recon_loss import recon_loss
    real = _lib.lib()

    class Fake:
        nsr_recon_loss_workspace_bytes = staticmethod(real.nsr_recon_loss_workspace_bytes)
        nsr_recon_loss_exposure_workspace_bytes = staticmethod(real.nsr_recon_loss_exposure_workspace_bytes)

        @staticmethod
        def nsr_recon_loss(*a):
            raise _Reached('plain')

        @staticmethod
        def nsr_recon_loss_weighted(*a):
            raise _Reached('weighted')

        @staticmethod
        def nsr_recon_loss_exposure(*a):
            raise _Reached('exposure')
    monkeypatch.setattr(_lib, 'lib', lambda: Fake)
    monkeypatch.setattr(_lib, 'p', lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, 'stream', lambda: None)
    rgb, target = torch.rand(8, 3), torch.rand(8, 3)
    e, seg = torch.zeros(3, 3), torch.zeros(2, dtype=torch.int32)
    refused = (AssertionError, ValueError, NotImplementedError)
    # exposure=None: the two existing paths, whatever the other two arguments are
    with pytest.raises(_Reached, match='plain'):
        recon_loss(rgb, None, target, exposure=None, seg_frame=seg, rays_per_segment=4)
    with pytest.raises(_Reached, match='weighted'):
        recon_loss(rgb, None, target, ray_weight=torch.ones(8))
    with pytest.raises(refused, match='seg_frame'):
        recon_loss(rgb, None, target, exposure=e, rays_per_segment=4)
    with pytest.raises(refused, match='rays_per_segment'):
        recon_loss(rgb, None, target, exposure=e, seg_frame=seg)
    for bad in (e.double(), torch.zeros(3, 4), torch.zeros(9), torch.zeros(0, 3)):
        with pytest.raises(refused, match='exposure'):
            recon_loss(rgb, None, target, exposure=bad, seg_frame=seg, rays_per_segment=4)
    for bad in (seg.long(), seg.float(), torch.zeros(2, 1, dtype=torch.int32)):
        with pytest.raises(refused, match='seg_frame'):
            recon_loss(rgb, None, target, exposure=e, seg_frame=bad, rays_per_segment=4)
    for bad_k in (3, 0, 2.5):
        with pytest.raises(refused, match='rays_per_segment'):
            recon_loss(rgb, None, target, exposure=e, seg_frame=seg, rays_per_segment=bad_k)
    # everything well-formed, but on the CPU: refused before the kernel is reached
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        recon_loss(rgb, None, target, exposure=e, seg_frame=seg, rays_per_segment=4)
