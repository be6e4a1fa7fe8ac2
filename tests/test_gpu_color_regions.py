"""GPU: region-wise colour transfer (nsr_color_region_moments, nsr_color_region_apply, nerfstyle_amd/color_match.py,
ResidentDataset.match_colors_by_region) against the fp64 / f32-chain restatement (color_regions_ref.py) and the reference's
recorded per-region outputs (tests/golden/color_regions_reference.npz).

One assignment of rows to regions is run through every layout: stride 4 with the label in the fourth float, stride 4 and
stride 3 with explicit int32 labels, stride 3 starting one row (and the labels one entry) past a 16-byte boundary."""
import numpy as np
import pytest
import torch

import color_match_ref as R
import color_regions_ref as G
from test_color_regions_cpu import KC, KS, TOL_A, TOL_B, TOL_IMAGE, load_cases

pytestmark = pytest.mark.gpu

# one row, less than a float4 group, the wave (64), the block (256), the 1024 rows a block is sized for, and several block partials
NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025, 70001)
KS_ALL = (1, 2, 5, 64)
GRID_CAP_ROWS = 2048 * 1024           # stride-4 rows past which a thread takes a second trip
PATTERNS = ('constant', 'runs', 'random', 'one_empty', 'sprinkled')


def _regions(pattern, n, K, rng):
    """[n] int64 in 0..K: the region of every row"""
    if pattern == 'constant':
        return np.full(n, K - 1, np.int64)
    if pattern == 'runs':                                              # runs of random length 1..300
        lens = rng.integers(1, 301, n // 100 + 2)
        while lens.sum() < n:
            lens = np.concatenate([lens, rng.integers(1, 301, n // 100 + 2)])
        return np.repeat(rng.integers(0, K, lens.size), lens)[:n].astype(np.int64)
    if pattern == 'random':                                            # a fresh label per row: every wave holds many regions
        return rng.integers(0, K, n).astype(np.int64)
    if pattern == 'one_empty':                                         # region K // 2 has no row (K = 1: every row is in slot K)
        reg = rng.integers(0, K, n).astype(np.int64)
        reg[reg == K // 2] = K
        return reg
    reg = rng.integers(0, K, n).astype(np.int64)                       # sprinkled: about a fifth of the rows are in no region
    reg[rng.random(n) < 0.2] = K
    return reg


def _labels(reg, K):
    """(float labels [n] f32, int labels [n] i32) that both select `reg`; slot K through -1, K, 2.5, NaN, inf / -1, K, far values"""
    wf, li = reg.astype(np.float32), reg.astype(np.int32)
    out = np.flatnonzero(reg == K)
    wf[out] = np.array([-1.0, K, 2.5 if K > 2 else 0.5, np.nan, np.inf, -0.25, K + 0.5], np.float32)[np.arange(out.size) % 7]
    li[out] = np.array([-1, K, K + 5, -2 ** 31, 2 ** 31 - 1], np.int32)[np.arange(out.size) % 5]
    first = np.flatnonzero(reg == 0)
    wf[first[::2]] = -0.0                                              # -0.0 is region 0
    assert np.array_equal(G.region_of(wf, K), reg) and np.array_equal(G.region_of(li, K), reg)
    return wf, li


def _misaligned(x, dev, dtype=torch.float32):
    """a device copy that starts one row (12 B of colour, 4 B of labels) past a 16-byte aligned base"""
    x = torch.from_numpy(x)
    buf = torch.empty((x.shape[0] + 1,) + tuple(x.shape[1:]), dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:]
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 in (4, 12)
    return view


def _layouts(x3, wf, li, dev):
    """name -> (rows, labels or None) on the device; 'explicit4' carries 1e30 where 'float4' carries the label"""
    n = x3.shape[0]
    lid = torch.from_numpy(li).to(dev)
    return {'float4': (torch.from_numpy(np.concatenate([x3, wf[:, None]], 1)).to(dev), None),
            'explicit4': (torch.from_numpy(np.concatenate([x3, np.full((n, 1), 1e30, np.float32)], 1)).to(dev), lid),
            'aligned3': (torch.from_numpy(x3).to(dev), lid),
            'aligned3_labels_off': (torch.from_numpy(x3).to(dev), _misaligned(li, dev, torch.int32)),
            'misaligned3': (_misaligned(x3, dev), _misaligned(li, dev, torch.int32))}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_moments(x3, reg, K, layouts):
    from nerfstyle_amd.color_match import region_moments
    ref, scale = G.region_moments(x3, reg, K), G.region_scale(x3, reg, K)
    got = {}
    for name, (rows, labels) in layouts.items():
        m1, m2 = region_moments(rows, K, labels), region_moments(rows, K, labels)
        assert m1.dtype == torch.float64 and tuple(m1.shape) == (K + 1, 10) and m1.device.type == 'cuda'
        assert torch.equal(_bits(m1), _bits(m2)), name                                  # no atomics: the same 80 (K + 1) bytes
        g = m1.cpu().numpy()
        assert np.array_equal(g[:, 0], ref[:, 0]), (name, g[:, 0], ref[:, 0])           # counts are exact
        # reordered fp64 sums of exact products: 1e-12 of sum |terms|, the bound of the global test
        assert (np.abs(g[:, 1:] - ref[:, 1:]) <= 1e-12 * scale[:, 1:]).all(), name
        empty = ref[:, 0] == 0
        assert np.array_equal(g[empty].view(np.uint64), np.zeros((int(empty.sum()), 10), np.uint64)), name   # ten +0.0
        got[name] = m1
    assert torch.equal(_bits(got['float4']), _bits(got['explicit4']))                   # one assignment, two ways to state it
    for name in ('aligned3_labels_off', 'misaligned3'):
        assert torch.equal(_bits(got['aligned3']), _bits(got[name])), name              # the loads differ, the order does not
    rows, labels = layouts['explicit4']
    rows = rows.clone()
    rows[:, 3] = float('nan')                                                           # ... and the fourth float is not read
    assert torch.equal(_bits(region_moments(rows, K, labels)), _bits(got['explicit4']))
    return ref


@pytest.mark.parametrize('K', KS_ALL)
@pytest.mark.parametrize('n', NS)
def test_moments_match_fp64_numpy(dev, n, K):
    rng = np.random.default_rng(1000 * K + n)
    for pattern in PATTERNS:
        x3 = (-0.5 + 2.0 * rng.random((n, 3))).astype(np.float32)
        reg = _regions(pattern, n, K, rng)
        wf, li = _labels(reg, K)
        ref = _check_moments(x3, reg, K, _layouts(x3, wf, li, dev))
        if pattern == 'one_empty' and n >= 1025:
            assert ref[K // 2, 0] == 0
        if pattern == 'random' and n >= 1025 and K == 64:
            assert len(set(reg[:64].tolist())) > 32                                     # many regions in one wave


@pytest.mark.parametrize('pattern', ['runs', 'random'])
def test_moments_past_the_grid_cap(dev, pattern):
    """2048 blocks of 1024 stride-4 rows and 515 more: the waves of the first block take a second trip"""
    n, K = GRID_CAP_ROWS + 515, 5
    rng = np.random.default_rng(77)
    x3 = rng.random((n, 3), np.float32)
    reg = _regions(pattern, n, K, rng)
    wf, li = _labels(reg, K)
    _check_moments(x3, reg, K, _layouts(x3, wf, li, dev))


def _tfs(K, seed, far):
    """[K+1,4,4] f32: random A and b per region; `far`: offsets 10 k apart, so that a wrong pick is off by about 10"""
    rng = np.random.default_rng(seed)
    tfs = np.repeat(np.eye(4, dtype=np.float32)[None], K + 1, 0)
    tfs[:, :3, :3] = (0.8 * rng.standard_normal((K + 1, 3, 3))).astype(np.float32)
    tfs[:, :3, 3] = (0.4 * rng.standard_normal((K + 1, 3))).astype(np.float32)
    if far:
        tfs[:, :3, 3] += 10.0 * np.arange(K + 1, dtype=np.float32)[:, None]
    return tfs


def _check_apply(x3, reg, K, layouts, tfs, clamp, dev):
    from nerfstyle_amd.color_match import apply_region_transforms
    ref, bound = G.apply_regions(x3, reg, tfs, clamp), G.apply_bound(x3, reg, tfs)
    tfd = torch.from_numpy(tfs).to(dev)
    rgb = {}
    for name, (rows, labels) in layouts.items():
        before = rows.clone()
        out = apply_region_transforms(rows, tfd, labels, clamp=clamp)                              # out of place, dst aligned
        assert out.data_ptr() != rows.data_ptr() and torch.equal(_bits(rows), _bits(before))
        src = rows.clone() if name != 'misaligned3' else _misaligned(x3, dev)
        assert apply_region_transforms(src, tfd, labels, clamp=clamp, out=src) is src                # in place
        assert torch.equal(_bits(out), _bits(src)), name
        got = out.cpu().numpy()
        assert (np.abs(got[:, :3].astype(np.float64) - ref) <= bound).all(), (name, clamp)
        if rows.shape[1] == 4:                                                                     # carried bit for bit, NaN included
            assert np.array_equal(got[:, 3].view(np.uint32), before.cpu().numpy()[:, 3].view(np.uint32)), name
        if name == 'misaligned3':
            dst = _misaligned(x3, dev)                                                             # out of place, both misaligned
            apply_region_transforms(rows, tfd, labels, clamp=clamp, out=dst)
            assert torch.equal(dst, src)
        rgb[name] = out[:, :3].contiguous()
    for name in ('explicit4', 'aligned3', 'aligned3_labels_off', 'misaligned3'):
        assert torch.equal(rgb[name], rgb['float4']), name                                         # one arithmetic, whatever the loads
    return ref


@pytest.mark.parametrize('K', KS_ALL)
@pytest.mark.parametrize('n', NS)
def test_apply_matches_restatement(dev, n, K):
    """Against color_match_ref.apply per region, which rounds each fma's sum twice where the kernel rounds once: apply_bound of
    the row's own transform is allowed.  With clamp off the transforms lie 10 apart, so a row mapped by another region's
    transform misses the bound (about 1e-5 at these magnitudes) by six orders."""
    from nerfstyle_amd.color_match import apply_color_transform, apply_region_transforms
    rng = np.random.default_rng(2000 * K + n)
    for pattern in PATTERNS:
        x3 = (-0.25 + 1.5 * rng.random((n, 3))).astype(np.float32)
        reg = _regions(pattern, n, K, rng)
        wf, li = _labels(reg, K)
        layouts = _layouts(x3, wf, li, dev)
        far = _tfs(K, n + K, True)
        _check_apply(x3, reg, K, layouts, far, False, dev)
        _check_apply(x3, reg, K, layouts, _tfs(K, n + K + 1, False), True, dev)
    # all K + 1 transforms equal: the global pass, bit for bit
    one = _tfs(0, n, False)[0]
    same = torch.from_numpy(np.repeat(one[None], K + 1, 0)).to(dev)
    for name, (rows, labels) in layouts.items():
        for clamp in (True, False):
            a = apply_region_transforms(rows, same, labels, clamp=clamp)
            b = apply_color_transform(rows, torch.from_numpy(one).to(dev), clamp=clamp)
            assert torch.equal(_bits(a), _bits(b)), (name, clamp)


def test_apply_past_the_grid_cap(dev):
    n, K = GRID_CAP_ROWS + 515, 5
    rng = np.random.default_rng(78)
    x3 = rng.random((n, 3), np.float32)
    reg = _regions('runs', n, K, rng)
    wf, li = _labels(reg, K)
    layouts = _layouts(x3, wf, li, dev)
    _check_apply(x3, reg, K, layouts, _tfs(K, 5, True), False, dev)


def test_refusals(dev):
    from nerfstyle_amd.color_match import apply_region_transforms, region_moments
    tfs = torch.eye(4, device=dev).repeat(3, 1, 1)
    lab = torch.zeros(128, dtype=torch.int32, device=dev)
    for stride in (3, 4):
        buf = torch.rand(128, stride, device=dev)
        for shift in (1, 4, 63):
            with pytest.raises(RuntimeError, match='invalid argument'):                         # overlapping, not equal
                apply_region_transforms(buf[:64], tfs, lab[:64], out=buf[shift:64 + shift])
    rows3, rows4 = torch.rand(8, 3, device=dev), torch.rand(8, 4, device=dev)
    with pytest.raises(ValueError, match='labels'):
        region_moments(rows3, 2)                                                                # stride 3 carries no label
    with pytest.raises(ValueError, match='labels'):
        apply_region_transforms(rows3, tfs)
    with pytest.raises(ValueError, match='labels'):
        region_moments(rows4, 2, torch.zeros(8, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match='labels'):
        region_moments(rows4, 2, lab[:7])
    with pytest.raises(ValueError, match='K must be'):
        region_moments(rows4, 0)
    with pytest.raises(ValueError, match='K must be'):
        region_moments(rows4, 65)
    with pytest.raises(ValueError, match='K must be'):
        apply_region_transforms(rows4, torch.eye(4, device=dev).repeat(66, 1, 1))
    with pytest.raises(ValueError, match='tfs'):
        apply_region_transforms(rows4, torch.eye(4, device=dev))
    assert tuple(region_moments(rows4, 64).shape) == (65, 10)


def _dataset(c, dev):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    N, H, W, _ = c['content'].shape
    return ResidentDataset(c['content'].transpose(0, 3, 1, 2), np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)),
                           Intrinsics(H, W, 40.0, 40.0, W / 2, H / 2), 2.0, dev, seg_maps=c['classes'].astype(np.float32), num_classes=KC)


@pytest.mark.parametrize('name', ['a_fallbacks', 'b_shared'])
def test_match_colors_by_region_end_to_end(dev, name):
    """The golden cases as a resident training set (a: class 2 unmatched, class 3 below min_rows, a strip labelled -1)."""
    from nerfstyle_amd.color_match import apply_region_transforms, region_moments
    c = load_cases()[name]
    N, H, W, _ = c['content'].shape
    matching, min_rows = c['matching'].tolist(), int(c['min_rows'])
    rows = c['content'].reshape(-1, 3)
    reg, sreg = G.region_of(c['classes'].reshape(-1), KC), G.region_of(c['clusters'].reshape(-1), KS)
    ds = _dataset(c, dev)
    assert ds.region_tf is None and ds.color_tf is None
    rgb_rows = ds.target_rgb_rows
    seg_before, targets_before = ds.targets[:, :, 3].clone(), ds.targets.clone()
    style, clusters = torch.from_numpy(c['style'].transpose(2, 0, 1)).to(dev), torch.from_numpy(c['clusters'])
    tfs = ds.match_colors_by_region(style, clusters, matching, min_rows=min_rows)
    assert tfs is ds.region_tf and tfs.device.type == 'cuda' and tfs.dtype == torch.float32 and tuple(tfs.shape) == (KC + 1, 4, 4)
    assert torch.equal(ds.color_tf, tfs[KC])
    got_tf, got = tfs.cpu().numpy(), ds.targets[:, :, :3].reshape(-1, 3).cpu().numpy()
    # the golden
    assert np.abs(got_tf[:, :3, :3] - c['tfs'][:, :3, :3]).max() <= TOL_A and np.abs(got_tf[:, :3, 3] - c['tfs'][:, :3, 3]).max() <= TOL_B
    assert np.abs(got - c['image'].reshape(-1, 3)).max() <= TOL_IMAGE
    # the restatement: the same transforms up to the two eigen-solvers' rounding, and the f32 chain of the device's own transforms
    r_rows, r_tfs = G.match_by_region(rows, reg, KC, c['style'].reshape(-1, 3), sreg, KS, matching, min_rows)
    assert np.abs(got_tf - r_tfs).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(r_tfs).max())
    assert (np.abs(got.astype(np.float64) - G.apply_regions(rows, reg, got_tf)) <= G.apply_bound(rows, reg, got_tf)).all()
    assert float(np.abs(got - rows).max()) > 0.05                                                # the colours did move
    assert torch.equal(_bits(ds.targets[:, :, 3]), _bits(seg_before))                            # the segment channel: its bits
    assert ds.target_rgb_rows is rgb_rows and torch.equal(rgb_rows, ds.targets[:, :, :3].reshape(-1, 3))
    # through the pieces without the clamp: every matched class has its cluster's mean and covariance
    out = apply_region_transforms(targets_before, tfs, clamp=False)
    m_out = region_moments(out, KC).cpu().numpy()
    m_style = G.region_moments(c['style'].reshape(-1, 3), sreg, KS)
    matched = [i for i in range(KC) if not np.array_equal(c['tfs'][i], c['tfs'][KC])]
    assert matched == ([0, 1] if name == 'a_fallbacks' else [0, 1, 2])
    for i in matched:
        mu, cov = R.mean_cov(m_out[i, 1:], m_out[i, 0])
        mu_s, cov_s = R.mean_cov(m_style[matching[i], 1:], m_style[matching[i], 0])
        assert np.abs(mu - mu_s).max() <= TOL_IMAGE and np.abs(cov - cov_s).max() <= TOL_IMAGE, (i, mu - mu_s, cov - cov_s)
    # identity fallback leaves the unmatched rows alone, bit for bit
    ds2 = _dataset(c, dev)
    tf2 = ds2.match_colors_by_region(style, clusters.to(dev), torch.tensor(matching), min_rows=min_rows, fallback='identity')
    assert torch.equal(tf2[KC].cpu(), torch.eye(4)) and torch.equal(tf2[:KC][torch.tensor(matched)], tfs[torch.tensor(matched)])
    keep = torch.from_numpy(~np.isin(reg, matched)).to(dev)
    assert torch.equal(ds2.targets.reshape(-1, 4)[keep], targets_before.reshape(-1, 4)[keep])


def test_global_match_colors_is_unchanged(dev):
    """match_colors on a fresh copy of the same set still gives the fallback slot's transform: all rows against all rows"""
    c = load_cases()['a_fallbacks']
    ds = _dataset(c, dev)
    tf = ds.match_colors(torch.from_numpy(c['style'].transpose(2, 0, 1)).to(dev)).cpu().numpy()
    rows, srows = c['content'].reshape(-1, 3), c['style'].reshape(-1, 3)
    ref = R.solve(R.moments(rows), rows.shape[0], R.moments(srows), srows.shape[0])
    assert np.abs(tf - ref).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max())
    assert np.abs(tf[:3, :3] - c['tfs'][KC, :3, :3]).max() <= TOL_A and np.abs(tf[:3, 3] - c['tfs'][KC, :3, 3]).max() <= TOL_B
    got = ds.targets[:, :, :3].reshape(-1, 3).cpu().numpy()
    assert (np.abs(got.astype(np.float64) - R.apply(rows, tf)) <= R.apply_bound(rows, tf)).all()
    assert ds.region_tf is None


def test_both_calls_are_capture_safe(dev):
    """moments then apply captured once as a single chain, replayed on changed rows"""
    from nerfstyle_amd import _lib as L
    n, K = 5003, 5
    rng = np.random.default_rng(31)
    tfs = _tfs(K, 3, True)
    tfd = torch.from_numpy(tfs).to(dev)
    rows = torch.zeros(n, 4, device=dev)
    out = torch.empty_like(rows)
    moments = torch.empty(K + 1, 10, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib().nsr_color_region_moments_workspace_bytes(n, K)) // 8, dtype=torch.float64, device=dev)

    def launch():
        s = L.stream()
        L.check(L.lib().nsr_color_region_moments(L.p(rows), n, 4, None, K, L.p(moments), L.p(ws), s), 'moments')
        L.check(L.lib().nsr_color_region_apply(L.p(rows), L.p(out), n, 4, None, K, L.p(tfd), 0, s), 'apply')

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for seed in (1, 2):
        x3 = rng.random((n, 3), np.float32)
        reg = _regions('sprinkled' if seed == 1 else 'runs', n, K, rng)
        wf, _ = _labels(reg, K)
        rows.copy_(torch.from_numpy(np.concatenate([x3, wf[:, None]], 1)))
        graph.replay()
        torch.cuda.synchronize()
        ref = G.region_moments(x3, reg, K)
        got = moments.cpu().numpy()
        assert np.array_equal(got[:, 0], ref[:, 0]) and (np.abs(got[:, 1:] - ref[:, 1:]) <= 1e-12 * G.region_scale(x3, reg, K)[:, 1:]).all()
        o = out.cpu().numpy()
        assert (np.abs(o[:, :3].astype(np.float64) - G.apply_regions(x3, reg, tfs, False)) <= G.apply_bound(x3, reg, tfs)).all()
        assert np.array_equal(o[:, 3].view(np.uint32), wf.view(np.uint32))
