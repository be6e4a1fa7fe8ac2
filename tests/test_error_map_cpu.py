"""Host side of the error-map importance sampling: the NumPy restatement (tests/error_map_ref.py) is a probability
distribution, its weights make the weighted mean unbiased, its draws follow its pdf; the four entry points' symbols and host-side
checks; ErrorMap and recon_loss refuse or dispatch as the host layer promises.

Bars.  The pdf identities hold to 1e-6: a weight is five fp32 operations (2^-24 relative each, 3e-7 together) against an fp64
pdf.  Chi-square: the 0.999 quantile of the chi-square distribution with (bins - 1) degrees of freedom, by the Wilson-Hilferty
cube (accurate to the third digit at a thousand degrees); the draw is seeded, so the test is deterministic."""
import ctypes
import os

import numpy as np
import pytest
import torch

import error_map_ref as ER
from helpers import room_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x2545f4914f6cdd1d
W, H, CELL = 40, 27, 16                              # 3 x 2 cells, the edge cells 8 wide and 11 high


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _map(F=3, uniform_mix=0.1, seed=0, zero_frame=None):
    """masses spanning three decades: err = 10^U(-3, 0) per cell (quantised at 65536 per unit: 65 .. 65536)"""
    m = ER.Map(F, W, H, CELL, uniform_mix=uniform_mix)
    rng = np.random.default_rng(seed)
    m.err[:] = (10.0 ** rng.uniform(-3.0, 0.0, m.err.shape)).astype(np.float32)
    m.err[:, 0], m.err[:, -1] = 1.0, 1e-3            # both ends of the range in every frame
    if zero_frame is not None:
        m.err[zero_frame] = 0.0
    ER.rebuild(m)
    return m


def test_grid_is_ragged_and_quantisation_clamps():
    m = _map()
    assert (m.gw, m.gh, m.G, m.P) == (3, 2, 6, 1080)
    assert list(m.cw) == [16, 16, 8] and list(m.ch) == [16, 11]
    assert list(m.npix) == [256, 256, 128, 176, 176, 88] and int(m.npix.sum()) == m.P
    assert m.cell_of([0, 15, 16, 39, 40 * 15 + 39, 40 * 16, 40 * 26 + 39]).tolist() == [0, 0, 1, 2, 2, 3, 5]
    q = ER.quantise(np.asarray([1.0, 0.5, 3.0, 5.0, np.nan, -1.0, np.inf, 0.0, 1e-9], np.float32), 65536.0)
    assert q.tolist() == [65536, 32768, 196608, 2 ** 18, 0, 0, 2 ** 18, 0, 0]
    assert int(m.q.max()) // max(int(m.q.min()), 1) >= 900                   # three decades
    assert np.array_equal(m.prefix[:, -1], (m.npix[None, :] * m.q).sum(1)) and int(m.frame_prefix[-1]) == int(m.mass.sum())
    assert ER.threshold(0.0) == 0 and ER.threshold(1.0) == 2 ** 32 and ER.threshold(0.5) == 2 ** 31


@pytest.mark.parametrize('uniform_mix', [0.0, 0.1, 0.75, 1.0])
def test_pdf_sums_to_one_and_weights_invert_it(uniform_mix):
    m = _map(uniform_mix=uniform_mix, zero_frame=1)
    for f in range(m.F):
        p, w = ER.pdf(m, f), ER.pixel_weights(m, f)
        assert w.dtype == np.float32 and p.shape == w.shape == (m.P,)
        assert abs(p.sum() - 1.0) <= 1e-6
        assert np.all(np.abs(w.astype(np.float64) * p * m.P - 1.0) <= 1e-6)
    assert np.all(ER.pixel_weights(m, 1) == 1.0)                             # the frame without mass: uniform, weight exactly 1
    if uniform_mix == 1.0:
        assert all(np.all(ER.pixel_weights(m, f) == 1.0) for f in range(m.F))
    fp, fw = ER.frame_pdf(m), ER.frame_weights(m)
    assert abs(fp.sum() - 1.0) <= 1e-6
    if uniform_mix > 0.0:                                                    # (at 0 the empty frame is never drawn: 0 * inf)
        assert np.all(np.abs(fw.astype(np.float64) * fp * m.F - 1.0) <= 1e-6)


@pytest.mark.parametrize('frames_by_error', [False, True])
def test_weighted_expectation_is_the_uniform_mean(frames_by_error):
    m = _map(uniform_mix=0.1, seed=3, zero_frame=2 if frames_by_error else None)
    loss = np.random.default_rng(4).random((m.F, m.P))
    fp = ER.frame_pdf(m) if frames_by_error else np.full(m.F, 1.0 / m.F)
    fw = ER.frame_weights(m).astype(np.float64) if frames_by_error else np.ones(m.F)
    got = sum(fp[f] * fw[f] * (ER.pdf(m, f) * ER.pixel_weights(m, f).astype(np.float64) * loss[f]).sum() for f in range(m.F))
    assert abs(got - loss.mean()) <= 1e-6


def _chi2_quantile_999(dof):
    z = 3.090232                                                             # the standard normal's 0.999 quantile
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3


def test_reference_draws_follow_the_reference_pdf():
    """200 000 draws of one frame, one bin per pixel (expected counts from 18.6, the uniform share, up)"""
    m = _map(F=1, uniform_mix=0.1, seed=5)
    n = 200000
    seg, pix, rows, weights, by_cell, cell = ER.draw(m, 1, n, SEED, 9)
    assert seg.tolist() == [0] and pix.min() >= 0 and pix.max() < m.P and np.array_equal(rows, pix)
    assert 0.85 * n < by_cell.sum() < 0.95 * n                               # nine in ten by the map
    expected = ER.pdf(m, 0) * n
    assert expected.min() > 18.0
    chi2 = float((((np.bincount(pix, minlength=m.P) - expected) ** 2) / expected).sum())
    bound = _chi2_quantile_999(m.P - 1)
    print('chi-square %.1f over %d bins, bound (0.999 quantile) %.1f' % (chi2, m.P, bound))
    assert chi2 <= bound
    assert np.array_equal(weights, ER.pixel_weights(m, 0)[pix])
    # the frames, drawn by their totals: 20 000 segments over 3 frames, one of them without mass
    m3 = _map(uniform_mix=0.1, seed=6, zero_frame=1)
    seg3 = ER.draw(m3, 20000, 1, SEED, 9, frames_by_error=True)[0]
    e3 = ER.frame_pdf(m3) * 20000
    chi2_f = float((((np.bincount(seg3, minlength=3) - e3) ** 2) / e3).sum())
    print('frames: chi-square %.2f, bound %.2f' % (chi2_f, _chi2_quantile_999(2)))
    assert chi2_f <= _chi2_quantile_999(2)


def test_reference_fold_and_accumulate():
    m = ER.Map(2, W, H, CELL, decay=0.25)
    before = m.err.copy()
    pix = np.asarray([0, 1, 16, 40 * 26 + 39, 5, 7, 9, 2000], np.int64)
    err = np.asarray([0.5, 1.5, np.nan, 9.0, -1.0, 0.25, 0.25, 1.0], np.float32)
    ER.accumulate(m, [0, 1, 7, -1], pix, err, 2)                             # segments of two rays; frames 7 and -1 do not exist
    assert m.acc_cnt[0, 0] == 2 and m.acc_sum[0, 0] == 2 * 2 ** 20           # 0.5 + 1.5
    assert m.acc_cnt[1, 5] == 1 and m.acc_sum[1, 5] == 2 ** 22               # 9.0 clamps to 4; the NaN ray beside it is skipped
    assert int(m.acc_cnt.sum()) == 3
    ER.rebuild(m)
    assert m.err[0, 0] == np.float32(1.0) and m.err[1, 5] == np.float32(1.75)     # 1 + 0.25 * (1 - 1), 1 + 0.25 * (4 - 1)
    untouched = np.ones_like(before, bool)
    untouched[0, 0] = untouched[1, 5] = False
    assert np.array_equal(m.err[untouched], before[untouched]) and not m.acc_cnt.any() and not m.acc_sum.any()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_host_side_checks(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    want = {'nsr_error_map_accumulate': 12, 'nsr_error_map_rebuild': 12, 'nsr_draw_frame_batch_error': 21, 'nsr_recon_loss_weighted': 17}
    with open(os.path.join(ROOT, 'include', 'nsr.h')) as f:
        header = f.read()
    for name, nargs in want.items():
        assert hasattr(so, name) and len(_lib.SIGNATURES[name][1]) == nargs
        assert name + '(' in header
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION == 6
    fake = ctypes.c_void_p(4096)

    def acc(F=3, w=40, h=27, cell=16, S=2, K=4, err=fake, acc_sum=fake):
        return L.nsr_error_map_accumulate(F, w, h, cell, fake, fake, err, S, K, acc_sum, fake, None)
    assert acc(S=0) == 0                                                     # empty work is a no-op success
    assert acc(cell=0) == -1 and acc(F=0) == -1 and acc(w=0) == -1 and acc(err=None) == -1 and acc(acc_sum=None) == -1
    assert acc(acc_sum=ctypes.c_void_p(4100)) == -1 and acc(S=1 << 20, K=1 << 20) == -1
    assert acc(w=1 << 16, h=1 << 16) == -1                                   # pixel ids past 31 bits

    def reb(F=3, cell=16, decay=0.05, qs=65536.0, err=fake, prefix=fake):
        return L.nsr_error_map_rebuild(F, 40, 27, cell, decay, qs, err, fake, fake, prefix, fake, None)
    assert reb(cell=0) == -1 and reb(F=0) == -1 and reb(err=None) == -1 and reb(prefix=None) == -1
    assert reb(decay=-0.1) == -1 and reb(decay=1.5) == -1 and reb(qs=0.0) == -1 and reb(decay=float('nan')) == -1

    def drw(F=3, cell=16, mix=0.1, S=2, K=4, seqdev=None, advance=0, prefix=fake, weights=fake):
        return L.nsr_draw_frame_batch_error(F, 40, 27, cell, prefix, fake, mix, 0, S, K, 1, 0, seqdev, 0, None, advance, fake, fake, fake,
                                            weights, None)
    assert drw(S=0) == 0
    assert drw(cell=0) == -1 and drw(F=0) == -1 and drw(prefix=None) == -1 and drw(weights=None) == -1
    assert drw(mix=-0.01) == -1 and drw(mix=1.01) == -1 and drw(mix=float('nan')) == -1
    assert drw(advance=1) == -1 and drw(S=0, advance=1) == -1                # advance needs the device word

    def wl(N=8, rgb=fake, out=fake, ws=fake):
        return L.nsr_recon_loss_weighted(rgb, None, N, 0, fake, None, None, fake, 1e-3, 1.0, None, fake, None, None, out, ws, None)
    assert wl(N=0) == -1 and wl(rgb=None) == -1 and wl(out=None) == -1 and wl(ws=None) == -1


# ---- host layer --------------------------------------------------------------------------------------------------------------
def _cpu_dataset():
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    rng = np.random.default_rng(9)
    poses = np.asarray(room_cameras()['poses'], np.float32)[:3]
    return ResidentDataset(rng.random((3, 3, H, W)).astype(np.float32), poses, Intrinsics(H, W, 30.0, 30.0, 20.0, 13.5), 2.0, 'cpu')


def test_error_map_has_no_cpu_fallback(built):
    from nerfstyle_amd.dataset import ErrorMap
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ErrorMap(_cpu_dataset(), cell=CELL)
    with pytest.raises(ValueError):
        ErrorMap(_cpu_dataset(), cell=0)
    with pytest.raises(ValueError):
        ErrorMap(_cpu_dataset(), uniform_mix=1.5)


class _Reached(Exception):
    pass


def test_recon_loss_dispatch(built, monkeypatch):
    """both new arguments None: nsr_recon_loss, never the weighted entry; either one given: the weighted entry"""
    from nerfstyle_amd import _lib
    from nerfstyle_amd.recon_loss import recon_loss
    real = _lib.lib()

    class Fake:
        nsr_recon_loss_workspace_bytes = staticmethod(real.nsr_recon_loss_workspace_bytes)

        @staticmethod
        def nsr_recon_loss(*a):
            raise _Reached('plain')

        @staticmethod
        def nsr_recon_loss_weighted(*a):
            raise _Reached('weighted')
    monkeypatch.setattr(_lib, 'lib', lambda: Fake)
    monkeypatch.setattr(_lib, 'p', lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, 'stream', lambda: None)
    rgb, target = torch.rand(8, 3), torch.rand(8, 3)
    with pytest.raises(_Reached, match='plain'):
        recon_loss(rgb, None, target)
    with pytest.raises(_Reached, match='plain'):
        recon_loss(rgb, None, target, ray_weight=None, ray_err_out=None)
    with pytest.raises(_Reached, match='weighted'):
        recon_loss(rgb, None, target, ray_weight=torch.ones(8))
    with pytest.raises(_Reached, match='weighted'):
        recon_loss(rgb, None, target, ray_err_out=torch.empty(8))
