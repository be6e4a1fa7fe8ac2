"""GPU: colour transfer to a style image (nsr_color_moments, nsr_color_apply, nerfstyle_amd/color_match.py,
ResidentDataset.match_colors) against the fp64 / f32-chain restatement (color_match_ref.py) and the reference's recorded
outputs (tests/golden/color_match_reference.npz)."""
import numpy as np
import pytest
import torch

import color_match_ref as R
from test_color_match_cpu import TOL_A, TOL_B, TOL_IMAGE, load_cases

pytestmark = pytest.mark.gpu

# one row, less than a float4 group, the wave (64), the block (256), the 1024 rows a block is sized for, and several block partials
NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025, 70001)
GRID_CAP_ROWS = 2048 * 1024           # units (stride 4: rows, stride 3: groups of four rows) past which a thread takes a second trip


def _rows(n, stride, seed, dev, lo=0.0, hi=1.0):
    """(host [n, stride] f32, device copy); with stride 4 the fourth float is 1e30: reading it as colour would show"""
    rng = np.random.default_rng(seed)
    x = (lo + (hi - lo) * rng.random((n, stride))).astype(np.float32)
    if stride == 4:
        x[:, 3] = 1e30
    return x, torch.from_numpy(x).to(dev)


def _misaligned(x, dev):
    """a device copy of stride-3 rows that starts one row (12 B) past a 16-byte aligned base"""
    buf = torch.empty(x.shape[0] + 1, 3, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:]
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == 12
    return view


def _tf(seed):
    rng = np.random.default_rng(seed)
    tf = np.eye(4, dtype=np.float32)
    tf[:3, :3] = (0.8 * rng.standard_normal((3, 3))).astype(np.float32)
    tf[:3, 3] = (0.4 * rng.standard_normal(3)).astype(np.float32)
    return tf


def _check_moments(x, xd):
    from nerfstyle_amd.color_match import color_moments
    m1, m2 = color_moments(xd), color_moments(xd)
    assert m1.dtype == torch.float64 and tuple(m1.shape) == (9,) and m1.device.type == 'cuda'
    assert torch.equal(m1, m2)                                         # no atomics: the same 72 bytes
    got = m1.cpu().numpy()
    # reordered fp64 sums of n exact products: the bound n * 2^-53 of sum |terms| is far below 1e-12 for n <= 1e7
    assert (np.abs(got - R.moments(x)) <= 1e-12 * R.moment_scale(x)).all(), (got, R.moments(x))
    return m1


@pytest.mark.parametrize('stride', [3, 4])
@pytest.mark.parametrize('n', NS)
def test_moments_match_fp64_numpy(dev, n, stride):
    x, xd = _rows(n, stride, 100 + n, dev, -0.5, 1.5)
    m = _check_moments(x, xd)
    if stride == 3:
        # the order of summation does not depend on the alignment of the base, only the loads do
        assert torch.equal(_check_moments(x, _misaligned(x, dev)), m)
    else:
        # ... and the fourth float is not read: other values there, the same bits
        from nerfstyle_amd.color_match import color_moments
        y = xd.clone()
        y[:, 3] = float('nan')
        assert torch.equal(color_moments(y), m)


@pytest.mark.parametrize('stride', [3, 4])
@pytest.mark.parametrize('n', NS)
def test_apply_matches_restatement(dev, n, stride):
    """Against color_match_ref.apply, which rounds each fma's sum twice (fp64, then f32) where the kernel rounds once: per element
    2^-23 (|tf[c,3]| + sum_k |tf[c,k]| |x_k|) is allowed (apply_bound); the clamp does not widen it.  The fourth float of a
    stride-4 row is carried bit for bit."""
    from nerfstyle_amd.color_match import apply_color_transform
    x, xd = _rows(n, stride, 200 + n, dev, -0.25, 1.25)
    tf = _tf(n)
    tfd = torch.from_numpy(tf).to(dev)
    bound = R.apply_bound(x, tf)
    sources = [('aligned', lambda: xd.clone())]
    if stride == 3:
        sources.append(('misaligned', lambda: _misaligned(x, dev)))
    for clamp in (True, False):
        ref = R.apply(x, tf, clamp)
        if n >= 1025:
            assert clamp == bool(np.array_equal(ref[:, :3], np.clip(ref[:, :3], 0, 1)))       # the clamp is exercised
        for name, make in sources:
            src = make()
            out = apply_color_transform(src, tfd, clamp=clamp)                                  # out of place, dst aligned
            assert out.data_ptr() != src.data_ptr() and torch.equal(src.cpu(), torch.from_numpy(x))
            ret = apply_color_transform(src, tfd, clamp=clamp, out=src)                         # in place
            assert ret is src
            for got in (out.cpu().numpy(), src.cpu().numpy()):
                assert (np.abs(got[:, :3].astype(np.float64) - ref[:, :3]) <= bound).all(), (name, clamp)
                if stride == 4:
                    assert np.array_equal(got[:, 3].view(np.uint32), x[:, 3].view(np.uint32))
            assert torch.equal(out, src)                                                        # one arithmetic, whatever the loads
            if name == 'misaligned':
                dst = _misaligned(x, dev)                                                       # out of place, both misaligned
                apply_color_transform(make(), tfd, clamp=clamp, out=dst)
                assert torch.equal(dst, src)


@pytest.mark.parametrize('stride', [3, 4])
def test_identity_is_bit_exact_and_host_tf_is_accepted(dev, stride):
    from nerfstyle_amd.color_match import apply_color_transform
    x, xd = _rows(1025, stride, 7, dev)
    for clamp in (True, False):
        out = apply_color_transform(xd, torch.eye(4), clamp=clamp)                              # a host color_tf is copied over
        assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize('stride', [3, 4])
def test_past_the_grid_cap(dev, stride):
    """Sizes at which the grids reach their cap of 2048 blocks and a thread takes a second trip of its loop."""
    from nerfstyle_amd.color_match import apply_color_transform
    n = GRID_CAP_ROWS + 515
    x, xd = _rows(n, stride, 9, dev)
    if stride == 4:
        _check_moments(x, xd)
    tf = _tf(9)
    out = apply_color_transform(xd, torch.from_numpy(tf).to(dev))
    got = out.cpu().numpy()
    assert (np.abs(got[:, :3].astype(np.float64) - R.apply(x, tf)[:, :3]) <= R.apply_bound(x, tf)).all()
    if stride == 4:
        assert np.array_equal(got[:, 3].view(np.uint32), x[:, 3].view(np.uint32))
    else:
        del out, got
        x, xd = _rows(4 * GRID_CAP_ROWS + 1027, 3, 10, dev)                                     # moments: units are groups of four rows
        _check_moments(x, xd)


def test_refusals(dev):
    from nerfstyle_amd.color_match import apply_color_transform, color_moments
    tf = torch.eye(4, device=dev)
    for stride in (3, 4):
        buf = torch.rand(128, stride, device=dev)
        for shift in (1, 4, 63):
            with pytest.raises(RuntimeError, match='invalid argument'):                         # overlapping, not equal
                apply_color_transform(buf[:64], tf, out=buf[shift:64 + shift])
            with pytest.raises(RuntimeError, match='invalid argument'):
                apply_color_transform(buf[shift:64 + shift], tf, out=buf[:64])
    buf = torch.rand(128, 3, device=dev)
    before = buf.clone()
    apply_color_transform(buf[:64], tf, out=buf[64:])                                           # adjacent is not overlapping
    assert torch.equal(buf[64:], before[:64]) and torch.equal(buf[:64], before[:64])
    with pytest.raises(ValueError):
        color_moments(torch.rand(8, 5, device=dev))
    with pytest.raises(ValueError):
        color_moments(torch.rand(8, 3, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        apply_color_transform(buf, torch.eye(3, device=dev))
    with pytest.raises(RuntimeError, match='contiguous'):
        color_moments(torch.rand(8, 4, device=dev)[:, :3])


def test_match_colors_for_image_set_equals_reference(dev):
    from nerfstyle_amd.color_match import match_colors_for_image_set
    for name, (content, style, image, tf) in load_cases().items():
        src = torch.from_numpy(content).to(dev)
        got, got_tf = match_colors_for_image_set(src, torch.from_numpy(style).to(dev))
        assert got.shape == src.shape and got.data_ptr() != src.data_ptr() and torch.equal(src.cpu(), torch.from_numpy(content))
        assert got_tf.dtype == torch.float32 and tuple(got_tf.shape) == (4, 4) and got_tf.device.type == 'cuda'
        got, got_tf = got.cpu().numpy(), got_tf.cpu().numpy()
        dA, db = np.abs(got_tf[:3, :3] - tf[:3, :3]).max(), np.abs(got_tf[:3, 3] - tf[:3, 3]).max()
        di = np.abs(got - image).max()
        print('{:14s} device |dA| {:.3e} |db| {:.3e} |dimage| {:.3e}'.format(name, dA, db, di))
        assert dA <= TOL_A and db <= TOL_B and di <= TOL_IMAGE, name
        assert np.array_equal(got_tf[3], np.array([0, 0, 0, 1], np.float32))


@pytest.mark.parametrize('with_seg', [True, False])
def test_resident_dataset_match_colors(dev, with_seg):
    """Golden case (b) as a resident training set: the targets become the reference's recoloured frames, the segment channel and
    target_cls_rows keep their bits, and a target_rgb_rows taken before the call shows the new colours."""
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    content, style, image, tf = load_cases()['b_photo']
    N, H, W, _ = content.shape
    seg = np.random.default_rng(3).integers(0, 5, (N, H, W)).astype(np.float32) if with_seg else None
    ds = ResidentDataset(content.transpose(0, 3, 1, 2), np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)),
                         Intrinsics(H, W, 40.0, 40.0, W / 2, H / 2), 2.0, dev, seg_maps=seg, num_classes=5 if with_seg else 0)
    assert ds.color_tf is None and ds.targets.shape == (N, H * W, 4 if with_seg else 3)
    rgb_rows = ds.target_rgb_rows
    assert torch.equal(rgb_rows.cpu(), torch.from_numpy(content.reshape(-1, 3)))
    if with_seg:
        cls_rows = ds.target_cls_rows
        cls_before, seg_before = cls_rows.clone(), ds.targets[:, :, 3].clone()
    pose, picked = ds.sample(1, torch.tensor([0, 5, H * W - 1], device=dev))
    color_tf = ds.match_colors(torch.from_numpy(style.transpose(2, 0, 1)).to(dev))
    assert color_tf is ds.color_tf and color_tf.device.type == 'cuda' and color_tf.dtype == torch.float32
    got_tf = color_tf.cpu().numpy()
    assert np.abs(got_tf[:3, :3] - tf[:3, :3]).max() <= TOL_A and np.abs(got_tf[:3, 3] - tf[:3, 3]).max() <= TOL_B
    got = ds.targets[:, :, :3].cpu().numpy()
    assert np.abs(got - image.reshape(N, H * W, 3)).max() <= TOL_IMAGE
    assert float(np.abs(got - content.reshape(N, H * W, 3)).max()) > 0.05                       # the colours did move
    assert ds.target_rgb_rows is rgb_rows and torch.equal(rgb_rows, ds.targets[:, :, :3].reshape(-1, 3))
    if with_seg:
        assert torch.equal(ds.targets[:, :, 3], seg_before)
        assert ds.target_cls_rows is cls_rows and torch.equal(cls_rows, cls_before)
    assert torch.equal(ds.sample(1, torch.tensor([5], device=dev))[1][0, :3], rgb_rows[H * W + 5])
    # again: the current (matched, clamped) targets are matched to the new image; color_tf is the last transform
    again = ds.match_colors(torch.rand(3, 9, 7, generator=torch.Generator().manual_seed(1)))
    assert again is ds.color_tf and not torch.equal(again, color_tf) and bool(torch.isfinite(again).all())
    assert torch.equal(rgb_rows, ds.targets[:, :, :3].reshape(-1, 3)) and float(ds.targets[:, :, :3].min()) >= 0.0
    if with_seg:
        assert torch.equal(ds.targets[:, :, 3], seg_before)


@pytest.mark.parametrize('stride', [3, 4])
def test_unclamped_result_has_the_style_moments(dev, stride):
    """On a case whose outputs never reach the clamp, the mapped rows have the style's mean and covariance: within 1e-5
    absolute (the f32 rounding of A and of every output accounts for about 1e-6 on values of at most 1)."""
    from nerfstyle_amd.color_match import apply_color_transform, color_moments, solve_color_transform
    rng = np.random.default_rng(21)
    n, ns = 5003, 1201
    x, xd = _rows(n, stride, 22, dev)
    mix = np.array([[1.0, 0.4, 0.1], [0.0, 0.8, -0.3], [0.2, 0.0, 0.6]])
    s = (0.5 + 0.12 * (rng.random((ns, 3)) - 0.5) @ mix.T).astype(np.float32)
    sd = torch.from_numpy(s).to(dev)
    tf = solve_color_transform(color_moments(xd), n, color_moments(sd), ns)
    assert tf.device.type == 'cuda'
    out = apply_color_transform(xd, tf, clamp=False)
    assert 0.0 < float(out[:, :3].min()) and float(out[:, :3].max()) < 1.0                      # the condition of this check
    assert torch.equal(out, apply_color_transform(xd, tf, clamp=True))
    mu, cov = R.mean_cov(color_moments(out).cpu().numpy(), n)
    mu_s, cov_s = R.mean_cov(R.moments(s), ns)
    assert np.abs(mu - mu_s).max() <= 1e-5 and np.abs(cov - cov_s).max() <= 1e-5, (mu - mu_s, cov - cov_s)
