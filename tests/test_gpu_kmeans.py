"""GPU: style-image k-means (nsr_kmeans_step, nsr_kmeans_init, nerfstyle_amd/segment.py) against the NumPy restatement
(kmeans_ref.py).  Labels, counts, the int64 sums, the changed count and the centroids are compared for equality; the inertia within
the bound of a reordered fp64 sum.

One set of rows is run through every layout: stride 3 at each of the four offsets from a 16-byte boundary (offset 0 takes the
float4 loads and int4 label stores throughout, the others a scalar head and tail and scalar label stores) and stride 4 with a
NaN in the fourth float.

Two readings of the issue, stated here because the assertions follow them.  The rows' valid range is the closed [-8, 8] of the
definition, so a row holding 8.0 is labelled and the next float above it is not.  And the full run's history is compared exactly
in its changed counts and within the inertia bound in its inertia: the restatement's NumPy sum adds in another order."""
import numpy as np
import pytest
import torch

import kmeans_ref as R
from test_kmeans_cpu import FULL, full_case

pytestmark = pytest.mark.gpu

BLOCK_ROWS = 1024                       # the rows a block is sized for
GRID_CAP_ROWS = 2048 * BLOCK_ROWS       # past it the waves take a second trip
NS = (1, 63, 64, 65, 255, 257, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1)
KS = (1, 2, 63, 64)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)


def _layouts(x3, dev, offsets=(0, 1, 2, 3)):
    """name -> rows on the device: stride 3 starting `off` floats past a 16-byte aligned base, and stride 4"""
    n = x3.shape[0]
    out = {}
    for off in offsets:
        buf = torch.zeros(n * 3 + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + n * 3].view(n, 3)
        view.copy_(torch.from_numpy(x3))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
        out['stride3+{}'.format(off)] = view
    out['stride4'] = torch.from_numpy(np.concatenate([x3, np.full((n, 1), np.nan, np.float32)], 1)).to(dev)
    return out


def _inertia_bound(n, ref):
    """The inertia is a sum of at most n non-negative fp64 terms.  Any order of adding them makes n - 1 additions, each with a
    relative error of at most 2^-53 of a partial sum that is at most the total: |error| <= (n - 1) 2^-53 total for the device's
    order and as much for the restatement's, together less than n 2^-52 total."""
    return n * 2.0 ** -52 * ref


def _check_step(x3, H, W, cent, wxy, dev, prev=None, offsets=(0, 1, 2, 3), ref=None):
    from nerfstyle_amd.segment import kmeans_step
    n, K = x3.shape[0], cent.shape[0]
    ref = R.step(x3, cent, H, W, wxy, prev) if ref is None else ref
    cd = torch.from_numpy(cent).to(dev)
    pd = None if prev is None else torch.from_numpy(prev).to(dev)
    for name, rows in _layouts(x3, dev, offsets).items():
        new = torch.full((K, 5), 123.0, dtype=torch.float64, device=dev)
        labels, counts, sums, stats = kmeans_step(rows, cd, H, W, wxy, prev_labels=pd, out_centroids=new)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int64 and sums.dtype == torch.int64 and stats.dtype == torch.float64
        assert tuple(labels.shape) == (n,) and tuple(counts.shape) == (K,) and tuple(sums.shape) == (K, 5) and tuple(stats.shape) == (2,)
        got_l, st = labels.cpu().numpy(), stats.cpu().numpy()
        print(name, 'n', n, 'K', K, 'label mismatches', int((got_l != ref['labels']).sum()), 'changed', st[0], ref['changed'],
              'inertia', st[1], ref['inertia'])
        assert np.array_equal(got_l, ref['labels']), name
        assert np.array_equal(counts.cpu().numpy(), ref['counts']), name
        assert np.array_equal(sums.cpu().numpy(), ref['sums']), name
        assert st[0] == ref['changed'], name
        assert abs(st[1] - ref['inertia']) <= _inertia_bound(n, ref['inertia']), name
        assert np.array_equal(new.cpu().numpy().view(np.uint64), ref['new'].view(np.uint64)), name
        # the same bits again, the inertia included
        again = torch.empty_like(new)
        l2, c2, s2, st2 = kmeans_step(rows, cd, H, W, wxy, prev_labels=pd, out_centroids=again)
        for a, b in ((labels, l2), (counts, c2), (sums, s2), (stats, st2), (new, again)):
            assert torch.equal(_bits(a), _bits(b)), name
    return ref


def _rows_near(cent, n, rng, pattern):
    """[n, 3] f32 around the colours of the centroids: 'runs' piecewise constant labels, 'random' a fresh label per row"""
    K = cent.shape[0]
    if pattern == 'runs':
        lens = rng.integers(1, 301, n // 100 + 2)
        while lens.sum() < n:
            lens = np.concatenate([lens, rng.integers(1, 301, n // 100 + 2)])
        lab = np.repeat(rng.integers(0, K, lens.size), lens)[:n]
    else:
        lab = rng.integers(0, K, n)
    return (cent[lab, :3] + 0.02 * rng.standard_normal((n, 3))).astype(np.float32)


def _centroids(K, rng, wxy):
    c = np.zeros((K, 5))
    c[:, :3] = rng.random((K, 3))
    if wxy:
        c[:, 3:] = wxy * rng.random((K, 2))
    return c


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('n', NS)
def test_step_at_its_edges(dev, n, K):
    rng = np.random.default_rng(1000 * K + n)
    for wxy, pattern in ((0.0, 'runs'), (1.0, 'random')):
        cent = _centroids(K, rng, wxy)
        x3 = _rows_near(cent, n, rng, pattern)
        ref = _check_step(x3, 1, n, cent, wxy, dev)
        prev = ref['labels'].copy()
        prev[::3] = -1                                                  # a third of the rows "changed"
        moved = cent + 0.05 * rng.standard_normal(cent.shape)
        r2 = _check_step(x3, 1, n, moved, wxy, dev, prev=prev, offsets=(0, 3))
        assert r2['changed'] >= (n + 2) // 3


@pytest.mark.parametrize('K,wxy', [(2, 1.0), (64, 0.0)])
def test_step_past_one_grid_of_blocks(dev, K, wxy):
    """2048 blocks of 1024 rows and 517 more: the first block's waves take a second trip.  W is no multiple of 64."""
    n = GRID_CAP_ROWS + 517
    H, W = 1, n
    if wxy:
        W = 2121
        assert n % W == 0 and W % 64
        H = n // W
    rng = np.random.default_rng(7 + K)
    cent = _centroids(K, rng, wxy)
    x3 = _rows_near(cent, n, rng, 'runs' if K == 2 else 'random')
    ref = _check_step(x3, H, W, cent, wxy, dev, offsets=(0, 1))
    assert (ref['counts'] > 0).all()


@pytest.mark.parametrize('wxy', [0.0, 1.0])
def test_two_frames_wrap_y(dev, wxy):
    """F = 2 frames of 33 x 70 (W no multiple of 64): row i of the second frame has the y of row i - H W"""
    H, W, F, K = 33, 70, 2, 6
    rng = np.random.default_rng(21)
    cent = _centroids(K, rng, wxy)
    one = _rows_near(cent, H * W, rng, 'runs')
    x3 = np.concatenate([one, one])
    ref = _check_step(x3, H, W, cent, wxy, dev)
    assert np.array_equal(ref['labels'][:H * W], ref['labels'][H * W:])     # the same pixel, the same feature
    if wxy:                                                             # ... and as one tall frame it is another problem
        assert not np.array_equal(R.step(x3, cent, 2 * H, W, wxy)['labels'], ref['labels'])


def test_ties_empty_clusters_and_unlabelled_rows(dev):
    n, K = 2 * BLOCK_ROWS + 77, 6
    rng = np.random.default_rng(33)
    cent = _centroids(K, rng, 0.0)
    cent[4] = cent[1]                                                   # two identical centroids: the tie goes to k = 1
    cent[3, :3] = [7.0, -7.0, 7.0]                                      # receives no row: keeps its centroid
    x3 = _rows_near(cent[[0, 1, 2, 5]], n, rng, 'runs')
    above = np.nextafter(np.float32(8), np.float32(9))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [above, 0, 0], [0, -above, 0], [1e30, 0, 0]], np.float32)
    where = np.array([0, 5, 63, 64, 1000, n - 1])
    x3[where] = bad
    x3[[10, 11]] = [[8.0, 0.5, 0.5], [0.5, -8.0, 0.5]]                  # the closed ends of the range are labelled
    ref = _check_step(x3, 1, n, cent, 0.0, dev)
    assert (ref['labels'][where] == -1).all() and (ref['labels'][[10, 11]] >= 0).all()
    assert ref['counts'][4] == 0 and ref['counts'][1] > 0 and ref['counts'][3] == 0 and ref['counts'].sum() == n - where.size
    assert np.array_equal(ref['new'][3], cent[3]) and np.array_equal(ref['new'][4], cent[4])
    # unlabelled rows that stay unlabelled have not changed
    r2 = _check_step(x3, 1, n, cent, 0.0, dev, prev=ref['labels'], offsets=(0, 2))
    assert r2['changed'] == 0
    # every row unlabelled
    nan = np.full((300, 3), np.nan, np.float32)
    r3 = _check_step(nan, 1, 300, cent, 0.0, dev, offsets=(0, 1))
    assert not r3['counts'].any() and r3['inertia'] == 0.0 and np.array_equal(r3['new'], cent)


@pytest.mark.parametrize('K', [1, 64])
def test_all_rows_identical_and_a_label_per_pixel(dev, K):
    n = 3 * BLOCK_ROWS + 5
    rng = np.random.default_rng(50 + K)
    cent = _centroids(K, rng, 0.0)
    same = np.tile(np.array([[0.3, 0.6, 0.9]], np.float32), (n, 1))     # every lane of every wave on one cluster
    ref = _check_step(same, 1, n, cent, 0.0, dev, offsets=(0, 1))
    assert ref['counts'].max() == n
    mixed = _rows_near(cent, n, rng, 'random')                          # many clusters in every wave
    ref = _check_step(mixed, 1, n, cent, 0.0, dev, offsets=(0, 1))
    if K == 64:
        assert len(set(ref['labels'][:64].tolist())) > 32


@pytest.mark.parametrize('n,H,W,wxy', [(5000, 50, 100, 0.0), (5000, 50, 100, 1.0), (65536 * 2 + 1, 1, 65536 * 2 + 1, 0.0),
                                       (3 * 65536, 256, 768, 2.0)])
def test_init_chooses_the_restatements_rows(dev, n, H, W, wxy):
    from nerfstyle_amd.segment import kmeans_init
    K = 9
    rng = np.random.default_rng(n + int(wxy))
    x3 = _rows_near(_centroids(5, rng, 0.0), n, rng, 'runs')
    x3[0:n:7] = np.nan                                                  # unlabelled candidates are skipped
    x3[3] = [8.0, 8.0, -8.0]                                            # a far corner (a candidate when s = 1 or 3)
    cent, chosen, nc = R.init(x3, K, H, W, wxy)
    assert (-(-n // 65536) > 1) == (n > 65536) and len(set(chosen.tolist())) == K
    for name, rows in _layouts(x3, dev, (0, 1)).items():
        got_c, got_rows = kmeans_init(rows, K, H, W, wxy, return_rows=True)
        print(name, got_rows.cpu().numpy().tolist(), chosen.tolist())
        assert got_rows.dtype == torch.int32 and np.array_equal(got_rows.cpu().numpy(), chosen), name
        assert np.array_equal(got_c.cpu().numpy().view(np.uint64), cent.view(np.uint64)), name
        assert torch.equal(_bits(kmeans_init(rows, K, H, W, wxy)), _bits(got_c))
    few = np.full((40, 3), np.nan, np.float32)
    few[:5] = x3[1:6]
    with pytest.raises(ValueError, match='labelled candidate'):
        kmeans_init(torch.from_numpy(few).to(dev), 6, 1, 40)
    assert tuple(kmeans_init(torch.from_numpy(few).to(dev), 5, 1, 40).shape) == (5, 5)


@pytest.fixture(scope='module')
def full_ref():
    return R.kmeans(full_case(), FULL['K'], FULL['H'], FULL['W'], FULL['wxy'], FULL['iters'])


def _check_full(res, ref, n):
    H, W = FULL['H'], FULL['W']
    assert tuple(res.labels.shape) == (H, W) and res.labels.dtype == torch.int32
    assert res.n_clusters.device.type == 'cuda' and int(res.n_clusters) == ref['n_clusters']
    labels = res.labels.cpu().numpy().reshape(-1)
    hist = res.history.cpu().numpy()
    print('label mismatches', int((labels != ref['labels']).sum()), 'history', hist.tolist(), ref['history'].tolist())
    assert np.array_equal(labels, ref['labels'])                        # no row is left out: the restatement has no close call
    assert np.array_equal(res.centroids.cpu().numpy().view(np.uint64), ref['centroids'].view(np.uint64))
    assert np.array_equal(res.counts.cpu().numpy(), ref['counts'])
    assert np.array_equal(hist[:, 0], ref['history'][:, 0])
    assert (np.abs(hist[:, 1] - ref['history'][:, 1]) <= _inertia_bound(n, ref['history'][:, 1])).all()
    ids = np.unique(labels[labels >= 0])
    assert np.array_equal(ids, np.arange(int(res.n_clusters)))


def test_full_kmeans(dev, full_ref):
    from nerfstyle_amd.segment import kmeans, segment_style_image
    x3 = full_case()
    n = x3.shape[0]
    img = torch.from_numpy(x3.reshape(FULL['H'], FULL['W'], 3)).to(dev)
    res = kmeans(img, FULL['K'], xy_weight=FULL['wxy'], iters=FULL['iters'])
    _check_full(res, full_ref, n)
    again = kmeans(img.reshape(-1, 3), FULL['K'], FULL['H'], FULL['W'], xy_weight=FULL['wxy'], iters=FULL['iters'])
    for a, b in zip(res, again):
        assert torch.equal(_bits(a), _bits(b))
    res4 = kmeans(torch.cat([img, torch.full_like(img[:, :, :1], float('nan'))], 2), FULL['K'], xy_weight=FULL['wxy'], iters=FULL['iters'])
    assert torch.equal(res4.labels, res.labels) and torch.equal(_bits(res4.centroids), _bits(res.centroids))
    chw = segment_style_image(img.permute(2, 0, 1).cpu(), FULL['K'], xy_weight=FULL['wxy'], iters=FULL['iters'], device=dev)
    assert torch.equal(chw.labels, res.labels)
    # a stack of two frames: labels [F, H, W]
    two = kmeans(torch.stack([img, img]), FULL['K'], xy_weight=FULL['wxy'], iters=2)
    assert tuple(two.labels.shape) == (2, FULL['H'], FULL['W']) and torch.equal(two.labels[0], two.labels[1])


def test_compaction_drops_empty_clusters(dev):
    from nerfstyle_amd.segment import kmeans
    x3 = np.zeros((6, 3), np.float32)
    x3[3:, 0] = 1.0
    x3[5] = np.inf
    cent = np.zeros((4, 5))
    cent[:, 0] = [5.0, 0.0, 7.0, 1.0]
    rows, init = torch.from_numpy(x3).to(dev), torch.from_numpy(cent).to(dev)
    for compact in (True, False):
        ref = R.kmeans(x3, 4, 1, 6, iters=2, cent=cent, compact=compact)
        res = kmeans(rows, 4, 1, 6, iters=2, init=init, compact=compact)
        assert res.labels.cpu().numpy().reshape(-1).tolist() == ref['labels'].tolist()
        assert np.array_equal(res.centroids.cpu().numpy(), ref['centroids']) and np.array_equal(res.counts.cpu().numpy(), ref['counts'])
        assert int(res.n_clusters) == 2
    assert res.labels.cpu().numpy().reshape(-1).tolist() == [1, 1, 1, 3, 3, -1]
    assert torch.equal(init.cpu(), torch.from_numpy(cent))             # init is not written


def test_kmeans_in_a_captured_graph(dev, full_ref):
    """the whole call, explicit init, captured once and replayed twice: the eager call's bits each time"""
    from nerfstyle_amd.segment import kmeans, kmeans_init
    x3 = full_case()
    img = torch.from_numpy(x3.reshape(FULL['H'], FULL['W'], 3)).to(dev)
    init = kmeans_init(img, FULL['K'], xy_weight=FULL['wxy'])

    def run():
        return kmeans(img, FULL['K'], xy_weight=FULL['wxy'], iters=FULL['iters'], init=init)

    eager = run()
    _check_full(eager, full_ref, x3.shape[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run()
    for _ in range(2):
        for t in res:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(res, eager):
            assert torch.equal(_bits(a), _bits(b))


def test_integrations(dev, tmp_path):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    from nerfstyle_amd.losses import SemanticStyleLoss
    from nerfstyle_amd.segment import save_seg_map, segment_style_image
    from test_color_regions_cpu import KC, load_cases
    c = load_cases()['b_shared']
    style = torch.from_numpy(c['style'].transpose(2, 0, 1)).to(dev)                   # [3, H, W], as the style images are kept
    res = segment_style_image(style, 4)
    assert tuple(res.labels.shape) == tuple(style.shape[1:]) and 1 <= int(res.n_clusters) <= 4
    sem = SemanticStyleLoss(['relu3'], clusters=res.labels)                            # asserts ids 0..n-1
    assert sem.n_clusters == int(res.n_clusters)
    path = str(tmp_path / 'style_seg.npz')
    save_seg_map(path, res.labels)
    back = np.load(path)['seg_map']
    assert back.dtype == np.int32 and np.array_equal(back, res.labels.cpu().numpy())
    SemanticStyleLoss(['relu3'], clusters=back)

    def dataset():
        N, H, W, _ = c['content'].shape
        return ResidentDataset(c['content'].transpose(0, 3, 1, 2), np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)),
                               Intrinsics(H, W, 40.0, 40.0, W / 2, H / 2), 2.0, dev, seg_maps=c['classes'].astype(np.float32), num_classes=KC)
    matching = [m if m < int(res.n_clusters) else -1 for m in c['matching'].tolist()]
    a, b = dataset(), dataset()
    before = a.targets.clone()
    tf_a = a.match_colors_by_region(style, 4, matching, min_rows=int(c['min_rows']))
    tf_b = b.match_colors_by_region(style, res.labels, matching, min_rows=int(c['min_rows']))
    assert torch.equal(_bits(tf_a), _bits(tf_b)) and torch.equal(_bits(a.targets), _bits(b.targets))
    assert not torch.equal(a.targets, before)
