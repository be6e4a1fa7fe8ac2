"""NumPy restatement of the style-image k-means (include/nsr.h, "Style image clustering"): every fp64 operation of the definition
as one NumPy operation, in the written order, so each is rounded on its own as the kernels round it.  The per-cluster sums are
int64 and therefore exact whatever their order; only the inertia depends on an order of additions."""
import numpy as np

FEATS = 5
ONE = 4294967296.0
MAX_CANDIDATES = 65536


def valid(rows):
    """[n] bool: every colour component in [-8, 8] (NaN and the infinities fail)"""
    with np.errstate(invalid='ignore'):
        return (np.abs(rows[:, :3]) <= np.float32(8.0)).all(1)


def features(rows, H, W, wxy=0.0, index=None):
    """rows [n, 3|4] f32 -> f [n, 5] fp64; `index`: the rows' indices in the full layout (default 0..n-1)"""
    n = rows.shape[0]
    i = np.arange(n, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    f = np.zeros((n, FEATS), np.float64)
    f[:, :3] = rows[:, :3].astype(np.float64)
    if wxy != 0.0:
        m = np.float64(max(H, W))
        f[:, 3] = (np.float64(wxy) * (i % W).astype(np.float64)) / m
        f[:, 4] = (np.float64(wxy) * ((i // W) % H).astype(np.float64)) / m
    return f


def dist(f, c):
    """d [n] of features f [n, 5] to one centroid c [5]: ((((t0 t0 + t1 t1) + t2 t2) + t3 t3) + t4 t4)"""
    with np.errstate(invalid='ignore', over='ignore'):
        t = f - c[None, :]
        d = t[:, 0] * t[:, 0]
        for j in range(1, FEATS):
            d = d + t[:, j] * t[:, j]
    return d


def assign(f, cent):
    """-> (label [n] int32, d_label [n], second-smallest d [n]); the lowest k among equal distances"""
    best = dist(f, cent[0])
    label = np.zeros(f.shape[0], np.int32)
    second = np.full(f.shape[0], np.inf)
    for k in range(1, cent.shape[0]):
        d = dist(f, cent[k])
        with np.errstate(invalid='ignore'):
            lt = d < best
        second = np.where(lt, best, np.minimum(second, d))
        label = np.where(lt, np.int32(k), label)
        best = np.where(lt, d, best)
    return label, best, second


def quant(f):
    return np.rint(f * ONE).astype(np.int64)               # exact product; rint rounds to nearest even, as llrint


def step(rows, cent, H, W, wxy=0.0, prev=None):
    """One Lloyd step -> dict(labels [n] i32, counts [K] i64, sums [K, 5] i64, changed, inertia, new [K, 5], d [labelled rows],
    margin [n])"""
    n, K = rows.shape[0], cent.shape[0]
    ok = valid(rows)
    f = features(rows, H, W, wxy)
    lab, d, second = assign(f[ok], cent)
    labels = np.full(n, -1, np.int32)
    labels[ok] = lab
    q = quant(f[ok])
    counts = np.zeros(K, np.int64)
    sums = np.zeros((K, FEATS), np.int64)
    for k in np.unique(lab):
        sel = lab == k
        counts[k] = sel.sum()
        sums[k] = q[sel].sum(0, dtype=np.int64)
    new = cent.copy()
    has = counts > 0
    new[has] = sums[has].astype(np.float64) / ONE / counts[has].astype(np.float64)[:, None]
    changed = n if prev is None else int((labels != prev).sum())
    margin = np.full(n, np.inf)                              # relative gap of the two smallest distances
    with np.errstate(invalid='ignore', divide='ignore'):
        margin[ok] = np.where(np.isfinite(second), np.where(second > 0, (second - d) / np.where(second > 0, second, 1.0), 0.0), np.inf)
    return dict(labels=labels, counts=counts, sums=sums, changed=changed, inertia=float(np.sum(d)), new=new, d=d, margin=margin)


def init(rows, K, H, W, wxy=0.0):
    """Maximin -> (centroids [K, 5], chosen rows [K] int64, number of labelled candidates)"""
    n = rows.shape[0]
    s = -(-n // MAX_CANDIDATES)
    cand = np.arange(0, n, s, dtype=np.int64)
    cand = cand[valid(rows[cand])]
    if cand.size < K:
        raise ValueError('fewer labelled candidates than K')
    mean = step(rows, np.zeros((1, FEATS)), H, W, wxy)['new'][0]
    f = features(rows[cand], H, W, wxy, cand)
    first = int(np.argmin(dist(f, mean)))                  # argmin / argmax take the first of equals: the lowest row
    chosen = [first]
    md = np.full(cand.size, np.inf)
    for _ in range(1, K):
        md = np.minimum(md, dist(f, f[chosen[-1]]))
        md[chosen[-1]] = -1.0
        chosen.append(int(np.argmax(md)))
    return f[chosen].copy(), cand[chosen], cand.size


def kmeans(rows, K, H, W, wxy=0.0, iters=10, cent=None, compact=True):
    """-> dict(labels [n], centroids [K, 5], counts [K], n_clusters, history [iters, 2], min_margin: the smallest relative gap of
    the two nearest centroids over all rows and steps)"""
    cent = init(rows, K, H, W, wxy)[0] if cent is None else np.array(cent, np.float64)
    history = np.zeros((iters, 2))
    prev, rel = None, np.inf
    for it in range(iters):
        r = step(rows, cent, H, W, wxy, prev)
        history[it] = (r['changed'], r['inertia'])
        rel = min(rel, float(r['margin'].min()))
        prev, cent, counts = r['labels'], r['new'], r['counts']
    labels = prev
    keep = counts > 0
    if compact:
        new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        labels = np.where(labels >= 0, new_id[np.maximum(labels, 0)], -1).astype(np.int32)
        order = np.argsort(~keep, kind='stable')
        cent, counts = cent[order], counts[order]
    return dict(labels=labels, centroids=cent, counts=counts, n_clusters=int(keep.sum()), history=history, min_margin=rel)


def blobs(H, W, K, seed, noise=0.02):
    """[H, W, 3] f32: K well-separated colour blobs (vertical bands of random widths, a square patch) plus noise"""
    rng = np.random.default_rng(seed)
    palette = np.array([[(k * 37 % 5) / 4.0, (k * 11 % 4) / 3.0, (k % 3) / 2.0] for k in range(K)])
    edges = np.sort(rng.choice(np.arange(1, W), K - 1, replace=False)) if K > 1 else np.zeros(0, int)
    band = np.searchsorted(edges, np.arange(W), side='right')
    lab = np.tile(band, (H, 1))
    lab[H // 4:H // 2, W // 5:W // 2] = K - 1
    img = palette[lab] + noise * rng.standard_normal((H, W, 3))
    return img.astype(np.float32), lab
