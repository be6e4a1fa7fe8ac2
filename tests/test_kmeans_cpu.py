"""CPU: the NumPy restatement of the style-image k-means (kmeans_ref.py) against SciPy and scikit-learn, the per-row core compiled by
the host compiler (csrc/km_core.h through tests/kmeans_host.cpp) against the restatement, the maximin init on a hand-made case,
and what nerfstyle_amd/segment.py refuses on the host."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the full-k-means case of test_gpu_kmeans.py: 96 x 80, blobs plus noise, six steps
FULL = dict(H=96, W=80, K=5, seed=11, noise=0.04, wxy=0.5, iters=6)


def full_case():
    img, _ = R.blobs(FULL['H'], FULL['W'], FULL['K'], FULL['seed'], FULL['noise'])
    return img.reshape(-1, 3)


@pytest.fixture(scope='module')
def blob_step():
    """one step on 64 x 120 blobs from centroids near the palette: the features, the centroids and the restatement's step"""
    H, W, K = 64, 120, 5
    img, lab = R.blobs(H, W, K, 3)
    rows = img.reshape(-1, 3)
    f = R.features(rows, H, W, 0.5)
    rng = np.random.default_rng(4)
    cent = np.stack([f[lab.reshape(-1) == k].mean(0) for k in range(K)]) + 0.01 * rng.standard_normal((K, 5))
    return H, W, rows, f, cent, lab.reshape(-1), R.step(rows, cent, H, W, 0.5)


def _centroid_tol(n, f):
    """Quantisation: each of the n_k terms of a mean is off by at most 2^-33, so is the mean.  The libraries' fp64 means: n_k
    additions, each with relative error 2^-53 of a partial sum of at most n_k max|f|, divided by n_k: n 2^-53 max|f|; four more
    roundings at that magnitude for scikit-learn's centring of the data and back."""
    return 2.0 ** -33 + (n + 4) * 2.0 ** -53 * np.abs(f).max()


def test_restatement_against_scipy(blob_step):
    from scipy.cluster.vq import kmeans2
    H, W, rows, f, cent, lab, r = blob_step
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        c, l = kmeans2(f, cent.copy(), iter=1, minit='matrix')
    assert np.array_equal(l, r['labels']) and np.array_equal(l, lab)
    assert np.abs(c - r['new']).max() <= _centroid_tol(f.shape[0], f)


def test_restatement_against_sklearn(blob_step):
    from sklearn.cluster import KMeans
    H, W, rows, f, cent, lab, r = blob_step
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        km = KMeans(n_clusters=cent.shape[0], init=cent.copy(), n_init=1, max_iter=1, algorithm='lloyd', tol=0.0).fit(f)
    assert np.array_equal(km.labels_, r['labels'])
    assert np.abs(km.cluster_centers_ - r['new']).max() <= _centroid_tol(f.shape[0], f)
    assert abs(km.inertia_ - R.step(rows, r['new'], H, W, 0.5)['inertia']) <= 1e-9 * km.inertia_   # its labels are those of the new centres


def test_restatement_sums_are_the_quantised_features(blob_step):
    H, W, rows, f, cent, lab, r = blob_step
    assert r['counts'].sum() == rows.shape[0] and r['changed'] == rows.shape[0]
    for k in range(cent.shape[0]):
        want = sum(int(round(float(v) * 2 ** 32)) for v in f[r['labels'] == k][:, 3])     # Python integers: exact
        assert int(r['sums'][k, 3]) == want


@pytest.mark.parametrize('stride', [3, 4])
def test_core_header_on_the_host_matches_the_restatement(stride, tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'kmeans_host')
    subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', os.path.join(ROOT, 'tests', 'kmeans_host.cpp'), '-o', exe], check=True)
    H, W, K, F = 37, 53, 7, 2                                          # two frames: y wraps
    rng = np.random.default_rng(5)
    img, _ = R.blobs(H, W, K - 1, 6, noise=0.2)                        # noise as wide as the blobs are apart: close calls
    rows = np.concatenate([img.reshape(-1, 3), rng.random((H * W, 3), np.float32)])
    rows[[3, 500, 501, 2000]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, np.nextafter(np.float32(8), np.float32(9))], [-8.5, 0, 0]]
    rows[[7, 8]] = [[8.0, -8.0, 8.0], [1e-20, -1e-11, 3e-10]]          # the closed end of the range; values that round in 2^-32
    if stride == 4:
        rows = np.concatenate([rows, np.full((rows.shape[0], 1), np.nan, np.float32)], 1)
    cent = np.concatenate([R.features(rows[[20, 300, 900, 1500, 1800, 2500]], H, W, 1.0, [20, 300, 900, 1500, 1800, 2500]), np.zeros((1, 5))])
    cent[K - 1] = cent[2]                                              # two equal centroids: the lower k takes the rows
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    n = rows.shape[0]
    with open(src, 'wb') as fh:
        fh.write(np.asarray([n, stride, H, W, K], np.uint32).tobytes() + np.asarray([1.0], np.float64).tobytes() +
                 cent.tobytes() + np.ascontiguousarray(rows).tobytes())
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    raw = open(dst, 'rb').read()
    labels = np.frombuffer(raw, np.int32, n)
    counts = np.frombuffer(raw, np.int64, K, offset=4 * n)
    sums = np.frombuffer(raw, np.int64, K * 5, offset=4 * n + 8 * K).reshape(K, 5)
    want = R.step(rows, cent, H, W, 1.0)
    assert (want['labels'][[3, 500, 501, 2000]] == -1).all() and want['labels'][7] >= 0 and want['counts'][K - 1] == 0
    assert np.array_equal(labels, want['labels'])
    assert np.array_equal(counts, want['counts']) and np.array_equal(sums, want['sums'])


def test_maximin_on_a_hand_made_case():
    """Red values on a line.  Mean 0.4375: the nearest is 0.5.  From 0.5 the ends 0 and 1 are both 0.25 away: the lower row, 0.
    Then 1.0 (0.25 from 0.5), then 0.125 (0.015625 from 0) before 0.5625 (0.00390625 from 0.5).  A NaN row in front moves every
    index up by one and is never chosen."""
    red = np.array([0.0, 0.125, 0.5, 0.5625, 1.0], np.float32)
    rows = np.zeros((5, 3), np.float32)
    rows[:, 0] = red
    cent, chosen, nc = R.init(rows, 4, 1, 5)
    assert chosen.tolist() == [2, 0, 4, 1] and nc == 5
    assert np.array_equal(cent[:, 0], red[[2, 0, 4, 1]].astype(np.float64)) and not cent[:, 1:].any()
    rows2 = np.concatenate([np.full((1, 3), np.nan, np.float32), rows])
    cent2, chosen2, nc2 = R.init(rows2, 4, 1, 6)
    assert chosen2.tolist() == [3, 1, 5, 2] and nc2 == 5 and np.array_equal(cent2, cent)
    assert R.init(rows2, 5, 1, 6)[1].tolist() == [3, 1, 5, 2, 4]
    with pytest.raises(ValueError):
        R.init(rows2, 6, 1, 6)
    # with the position weighed in, x tells the duplicates of one colour apart
    same = np.zeros((4, 3), np.float32)
    assert R.init(same, 2, 1, 4)[1].tolist() == [0, 1]                 # all distances 0: the lowest rows
    assert R.init(same, 2, 1, 4, 1.0)[1].tolist() == [1, 3]            # mean x = 1.5: row 1 before row 2; then the far end


def test_subsample_step():
    rows = np.zeros((65536 * 2 + 1, 3), np.float32)
    rows[::3, 0] = 1.0
    rows[6] = [2.0, 0, 0]                                              # row 6 = candidate 2 with s = 3
    rows[7] = [5.0, 0, 0]                                              # not a candidate
    _, chosen, nc = R.init(rows, 2, 1, rows.shape[0])
    assert nc == -(-rows.shape[0] // 3) and (chosen % 3 == 0).all() and chosen[1] == 6


def test_full_case_has_no_close_call():
    """The seed of the GPU suite's full run: in the restatement no row's two nearest centroids come within 1e-12 relative in any of
    the six steps, so the device's labels have no excuse to differ."""
    r = R.kmeans(full_case(), FULL['K'], FULL['H'], FULL['W'], FULL['wxy'], FULL['iters'])
    assert r['min_margin'] >= 1e-12, r['min_margin']
    assert r['n_clusters'] == FULL['K'] and r['history'][0, 0] == FULL['H'] * FULL['W']
    assert (np.diff(r['history'][:, 1]) <= 0).all() and r['history'][1:, 0].max() > 0        # Lloyd descends; labels did move


def test_compaction_in_the_restatement():
    rows = np.zeros((6, 3), np.float32)
    rows[3:, 0] = 1.0
    rows[5] = np.inf
    cent = np.zeros((4, 5))
    cent[:, 0] = [5.0, 0.0, 7.0, 1.0]                                  # clusters 0 and 2 get nothing
    r = R.kmeans(rows, 4, 1, 6, iters=2, cent=cent)
    assert r['labels'].tolist() == [0, 0, 0, 1, 1, -1] and r['n_clusters'] == 2
    assert r['centroids'][:, 0].tolist() == [0.0, 1.0, 5.0, 7.0] and r['counts'].tolist() == [3, 2, 0, 0]
    r = R.kmeans(rows, 4, 1, 6, iters=2, cent=cent, compact=False)
    assert r['labels'].tolist() == [1, 1, 1, 3, 3, -1] and r['centroids'][:, 0].tolist() == [5.0, 0.0, 7.0, 1.0]


# ---- what segment.py decides on the host ----------------------------------------------------------------------------------------
def test_argument_checks_need_no_device():
    from nerfstyle_amd import segment as S
    img = torch.zeros(8, 8, 3)
    cent = torch.zeros(2, 5, dtype=torch.float64)
    for K in (0, 65):
        with pytest.raises(ValueError, match='K must be'):
            S.kmeans(img, K)
        with pytest.raises(ValueError, match='K must be'):
            S.kmeans_init(img, K)
        with pytest.raises(ValueError, match='K must be'):
            S.kmeans_step(img, torch.zeros(K, 5, dtype=torch.float64))
    big = torch.zeros(1, 3).expand(2 ** 27 + 1, 3)                     # no memory behind it: shape arithmetic only
    for call in (lambda: S.kmeans(big, 2, 1, 2 ** 27 + 1), lambda: S.kmeans_init(big, 2, 1, 2 ** 27 + 1),
                 lambda: S.kmeans_step(big, cent, 1, 2 ** 27 + 1)):
        with pytest.raises(ValueError, match=r'2\^27'):
            call()
    with pytest.raises(ValueError, match='rows must be'):
        S.kmeans(torch.zeros(3, 8, 8), 2)                              # [3,H,W]
    with pytest.raises(ValueError, match='rows must be'):
        S.kmeans_step(torch.zeros(3, 8, 8), cent)
    for w in (-0.5, 8.5, float('nan')):
        with pytest.raises(ValueError, match='xy_weight'):
            S.kmeans(img, 2, xy_weight=w)
        with pytest.raises(ValueError, match='xy_weight'):
            S.kmeans_step(img, cent, xy_weight=w)
    with pytest.raises(ValueError, match='frames'):
        S.kmeans(torch.zeros(10, 3), 2, 3, 4)
    with pytest.raises(ValueError, match='H and W'):
        S.kmeans(torch.zeros(10, 3), 2)
    with pytest.raises(ValueError, match='iters'):
        S.kmeans(img, 2, iters=0)
    with pytest.raises(ValueError, match='centroids'):
        S.kmeans_step(img, torch.zeros(2, 5))                          # float32 centroids
    for call in (lambda: S.kmeans(img, 2), lambda: S.kmeans_init(img, 2), lambda: S.kmeans_step(img, cent)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):     # CPU tensors
            call()


def test_c_abi_refuses_before_any_launch():
    from nerfstyle_amd import _lib
    L = _lib.lib()
    assert L.nsr_kmeans_step_workspace_bytes(0, 4) == 0 and L.nsr_kmeans_step_workspace_bytes(100, 65) == 0
    assert L.nsr_kmeans_step_workspace_bytes(2 ** 27 + 1, 4) == 0 and L.nsr_kmeans_init_workspace_bytes(2 ** 27 + 1) == 0
    assert L.nsr_kmeans_step_workspace_bytes(1025, 4) == 2 * (4 * 6 + 2) * 8
    assert L.nsr_kmeans_step_workspace_bytes(2 ** 27, 64) == 2048 * (64 * 6 + 2) * 8
    assert L.nsr_kmeans_init_workspace_bytes(65536) == 65536 * 8 and L.nsr_kmeans_init_workspace_bytes(65537) == 32769 * 8
    a = 4096                                                           # never dereferenced: every call below is refused first
    ok = dict(rows=a, n=64, stride=3, H=8, W=8, w=0.0, cent=a, K=4, prev=None, labels=a, counts=a, sums=a, out=None, stats=a, ws=a)

    def step(**kw):
        v = dict(ok, **kw)
        return L.nsr_kmeans_step(v['rows'], v['n'], v['stride'], v['H'], v['W'], v['w'], v['cent'], v['K'], v['prev'], v['labels'],
                                 v['counts'], v['sums'], v['out'], v['stats'], v['ws'], None)
    for bad in (dict(n=0), dict(n=2 ** 27 + 64), dict(stride=5), dict(K=0), dict(K=65), dict(H=0), dict(W=7), dict(w=-1.0), dict(w=8.5),
                dict(w=float('nan')), dict(rows=None), dict(cent=None), dict(labels=None), dict(counts=None), dict(sums=None),
                dict(stats=None), dict(ws=None), dict(rows=a + 2), dict(stride=4, rows=a + 4), dict(cent=a + 4), dict(labels=a + 2),
                dict(prev=a + 1), dict(out=a + 4)):
        assert step(**bad) == -1, bad
    assert L.nsr_kmeans_init(a, 64, 3, 8, 8, 0.0, a, 0, a, a, a, a, None) == -1
    assert L.nsr_kmeans_init(a, 64, 3, 8, 8, 9.0, a, 4, a, a, a, a, None) == -1
    assert L.nsr_kmeans_init(a, 64, 3, 8, 8, 0.0, None, 4, a, a, a, a, None) == -1
    assert L.nsr_kmeans_init(a, 64, 3, 8, 8, 0.0, a, 4, a, a + 2, a, a, None) == -1
