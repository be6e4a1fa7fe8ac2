"""Style image clustering: the cluster map of a style image, made on the device.

`SemanticStyleLoss(clusters=...)` and `ResidentDataset.match_colors_by_region` tie each scene class to one cluster of the style
image; the reference only ever loads such a map (`style_seg_path`, an .npz['seg_map'] written elsewhere).  This module makes one:
Lloyd k-means over the pixels in (r, g, b, w x / m, w y / m), m = max(H, W), as fused HIP (csrc/kmeans.hip; the definition is
include/nsr.h, "Style image clustering").

The per-cluster sums are int64 fixed point (2^-32), so they have no order of addition: labels, counts, sums and centroids are the
same bits on every call, and tests/kmeans_ref.py reproduces them exactly in NumPy.  A fixed number of iterations, nothing read
back: `kmeans(..., init=centroids)` is legal inside a captured graph (the default init reads one integer, see kmeans_init)."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from .color_match import _check_k

MAX_ROWS = 1 << 27              # KM_MAX_ROWS
MAX_CANDIDATES = 65536
FEATS = 5

KMeansResult = namedtuple('KMeansResult', ['labels', 'centroids', 'counts', 'n_clusters', 'history'])


def _layout(rows, H, W, what):
    """(n, stride, F, H, W) of rows [H,W,C], [F,H,W,C] or [...,C] with H and W given, C in (3, 4): shape arithmetic only"""
    if not torch.is_tensor(rows) or rows.dim() < 2 or rows.shape[-1] not in (3, 4):
        raise ValueError('{}: rows must be a tensor [H,W,3|4], [F,H,W,3|4] or [n,3|4] with H and W; got {}'.format(
            what, tuple(rows.shape) if torch.is_tensor(rows) else type(rows)))
    stride = int(rows.shape[-1])
    n = 1
    for s in rows.shape[:-1]:
        n *= int(s)
    if (H is None) != (W is None):
        raise ValueError('{}: pass both H and W or neither'.format(what))
    if H is None:
        if rows.dim() not in (3, 4):
            raise ValueError('{}: rows {} need H and W'.format(what, tuple(rows.shape)))
        H, W = int(rows.shape[-3]), int(rows.shape[-2])
    H, W = int(H), int(W)
    if n == 0 or H < 1 or W < 1 or n % (H * W):
        raise ValueError('{}: {} rows are not a stack of {} x {} frames'.format(what, n, H, W))
    if n > MAX_ROWS:
        raise ValueError('{}: {} rows; at most 2^27 (the int64 sums hold 2^27 rows of |f| <= 8)'.format(what, n))
    return n, stride, n // (H * W), H, W


def _device_rows(rows, what):
    ptr = L.p(rows)                                         # refuses CPU and non-contiguous tensors
    if rows.dtype != torch.float32:
        raise ValueError('{}: rows must be float32; got {}'.format(what, rows.dtype))
    return ptr


def _check_w(xy_weight, what):
    w = float(xy_weight)
    if not 0.0 <= w <= 8.0:
        raise ValueError('{}: xy_weight must be in [0, 8]; got {}'.format(what, xy_weight))
    return w


def _centroids(centroids, dev, what):
    if not torch.is_tensor(centroids) or centroids.dim() != 2 or centroids.shape[1] != FEATS or centroids.dtype != torch.float64:
        raise ValueError('{}: centroids must be a float64 tensor [K, 5]; got {}'.format(
            what, (centroids.dtype, tuple(centroids.shape)) if torch.is_tensor(centroids) else type(centroids)))
    K = _check_k(centroids.shape[0], what)
    if centroids.device != dev:
        raise ValueError('{}: centroids must be on {}; got {}'.format(what, dev, centroids.device))
    return K


def _step(rows, ptr, n, stride, H, W, w, centroids, K, prev, labels, out_centroids, stats):
    dev = rows.device
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    sums = torch.empty(K, FEATS, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.lib().nsr_kmeans_step_workspace_bytes(n, K)) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().nsr_kmeans_step(ptr, n, stride, H, W, w, L.p(centroids), K, L.p(prev), L.p(labels), L.p(counts), L.p(sums),
                                    L.p(out_centroids), L.p(stats), L.p(ws), L.stream()), 'kmeans_step')
    return counts, sums


def kmeans_step(rows: torch.Tensor, centroids: torch.Tensor, H: int = None, W: int = None, xy_weight: float = 0.,
                prev_labels: torch.Tensor = None, out_centroids: torch.Tensor = None):
    """One fused Lloyd step.  rows as in kmeans; centroids [K,5] float64 on the rows' device ->
    labels int32 [n] (-1: unlabelled), counts int64 [K], sums int64 [K,5] (sum of llrint(f 2^32) per cluster), stats float64 [2]
    (the number of rows whose label differs from prev_labels, all n of them without prev_labels; the inertia).
    out_centroids ([K,5] float64, may be `centroids`) receives sums / 2^32 / counts, an empty cluster keeping its centroid."""
    n, stride, _, H, W = _layout(rows, H, W, 'kmeans_step')
    w = _check_w(xy_weight, 'kmeans_step')
    K = _centroids(centroids, rows.device, 'kmeans_step')
    ptr = _device_rows(rows, 'kmeans_step')
    if out_centroids is not None and (_centroids(out_centroids, rows.device, 'kmeans_step') != K):
        raise ValueError('kmeans_step: out_centroids must have the shape of centroids')
    if prev_labels is not None and (prev_labels.dtype != torch.int32 or prev_labels.numel() != n or prev_labels.device != rows.device):
        raise ValueError('kmeans_step: prev_labels must be int32 with one entry per row ({}) on {}'.format(n, rows.device))
    labels = torch.empty(n, dtype=torch.int32, device=rows.device)
    stats = torch.empty(2, dtype=torch.float64, device=rows.device)
    counts, sums = _step(rows, ptr, n, stride, H, W, w, centroids, K, prev_labels, labels, out_centroids, stats)
    return labels, counts, sums, stats


def _init(rows, ptr, n, stride, H, W, w, K):
    dev = rows.device
    # the mean of all labelled rows: the centroid that one step with K = 1 gives
    mean = torch.zeros(1, FEATS, dtype=torch.float64, device=dev)
    _step(rows, ptr, n, stride, H, W, w, mean, 1, None, torch.empty(n, dtype=torch.int32, device=dev), mean,
          torch.empty(2, dtype=torch.float64, device=dev))
    centroids = torch.empty(K, FEATS, dtype=torch.float64, device=dev)
    chosen = torch.empty(K, dtype=torch.int32, device=dev)
    n_labelled = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.lib().nsr_kmeans_init_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().nsr_kmeans_init(ptr, n, stride, H, W, w, L.p(mean), K, L.p(centroids), L.p(chosen), L.p(n_labelled), L.p(ws),
                                    L.stream()), 'kmeans_init')
    if not torch.cuda.is_current_stream_capturing() and int(n_labelled) < K:
        raise ValueError('kmeans_init: {} labelled candidate rows for K = {}'.format(int(n_labelled), K))
    return centroids, chosen


def kmeans_init(rows: torch.Tensor, K: int, H: int = None, W: int = None, xy_weight: float = 0., return_rows: bool = False):
    """Deterministic maximin over the candidate rows j * ceil(n / 65536): the candidate nearest to the mean of all labelled rows,
    then K - 1 times the candidate farthest from its nearest chosen centre (equal distances: the lowest row) -> centroids [K,5]
    float64 (with return_rows also the chosen row indices, int32 [K]).
    Fewer labelled candidates than K is a ValueError: THE ONE HOST READ of this module, one integer.  It is skipped while the
    stream is being captured, where the remaining centres repeat the last one chosen."""
    n, stride, _, H, W = _layout(rows, H, W, 'kmeans_init')
    K = _check_k(K, 'kmeans_init')
    w = _check_w(xy_weight, 'kmeans_init')
    ptr = _device_rows(rows, 'kmeans_init')
    centroids, chosen = _init(rows, ptr, n, stride, H, W, w, K)
    return (centroids, chosen) if return_rows else centroids


def kmeans(rows_or_image: torch.Tensor, K: int, H: int = None, W: int = None, xy_weight: float = 0., iters: int = 10,
           init: torch.Tensor = None, compact: bool = True) -> KMeansResult:
    """Lloyd k-means of pixel rows.  rows_or_image: float32 on the HIP device, contiguous, [H,W,3|4], [F,H,W,3|4], or any [...,3|4]
    with H and W given (rows [n,3|4], a resident set's targets [N,H*W,4]); a fourth float is never read.  [3,H,W] and CPU
    tensors are refused.  xy_weight in [0, 8] weighs the pixel position (0: colour alone); `iters` fixed Lloyd steps, no
    convergence test; init: explicit centroids [K,5] float64 instead of kmeans_init.

    -> KMeansResult: labels int32 [H,W] ([F,H,W] for a stack; -1: a pixel with a NaN, infinite or |c| > 8 colour), the assignment
    of the last step; centroids float64 [K,5], the means of those labels' rows (an empty cluster keeps its last centroid);
    counts int64 [K]; n_clusters, a 0-dim int64 DEVICE tensor; history float64 [iters,2]: per step the number of labels that
    changed (n in the first) and the inertia.
    compact=True drops the clusters that end empty and renumbers the rest in ascending order of their old id, so the ids are
    0..n_clusters-1: the format SemanticStyleLoss asserts and the reference's seg_map has.  centroids and counts keep K rows, the
    first n_clusters of them are the kept clusters in their new order.  With compact=False n_clusters still counts the non-empty."""
    n, stride, F, H, W = _layout(rows_or_image, H, W, 'kmeans')
    K = _check_k(K, 'kmeans')
    w = _check_w(xy_weight, 'kmeans')
    iters = int(iters)
    if iters < 1:
        raise ValueError('kmeans: iters must be at least 1; got {}'.format(iters))
    rows = rows_or_image
    ptr = _device_rows(rows, 'kmeans')
    dev = rows.device
    if init is None:
        centroids, _ = _init(rows, ptr, n, stride, H, W, w, K)
    else:
        if _centroids(init, dev, 'kmeans') != K:
            raise ValueError('kmeans: init must be [{}, 5]; got {}'.format(K, tuple(init.shape)))
        centroids = init.detach().clone().contiguous()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    history = torch.empty(iters, 2, dtype=torch.float64, device=dev)
    for it in range(iters):
        counts, _ = _step(rows, ptr, n, stride, H, W, w, centroids, K, labels if it else None, labels, centroids, history[it])
    keep = counts > 0
    n_clusters = keep.sum()
    if compact:
        new_id = torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full_like(counts, -1)).to(torch.int32)
        labels = torch.where(labels >= 0, new_id[labels.clamp(min=0).long()], labels)
        # the kept clusters first, in their new order, then the empty ones in theirs
        slot = torch.where(keep, torch.cumsum(keep, 0) - 1, n_clusters + torch.cumsum(~keep, 0) - 1)
        centroids = torch.empty_like(centroids).index_copy_(0, slot, centroids)
        counts = torch.empty_like(counts).index_copy_(0, slot, counts)
    return KMeansResult(labels.reshape((H, W) if F == 1 else (F, H, W)), centroids, counts, n_clusters, history)


def segment_style_image(style_image: torch.Tensor, K: int, xy_weight: float = 0., iters: int = 10, device=None) -> KMeansResult:
    """The common case: a style image [H,W,3] or, as the style images are kept elsewhere in this package, [3,H,W], float32 in
    [0,1], on any device -> kmeans of its pixels on `device` (default: the image's own if that is a HIP device, else the current
    one).  result.labels is the map SemanticStyleLoss(clusters=...) and match_colors_by_region(style_clusters=...) take."""
    if not torch.is_tensor(style_image) or style_image.dim() != 3 or 3 not in (style_image.shape[0], style_image.shape[-1]):
        raise ValueError('segment_style_image: style_image must be [H,W,3] or [3,H,W]; got {}'.format(
            tuple(style_image.shape) if torch.is_tensor(style_image) else type(style_image)))
    if device is None:
        device = style_image.device if style_image.is_cuda else torch.device('cuda', torch.cuda.current_device())
    img = style_image.detach().to(device, torch.float32)
    if img.shape[-1] != 3:
        img = img.permute(1, 2, 0)
    return kmeans(img.contiguous(), K, xy_weight=xy_weight, iters=iters)


def save_seg_map(path, labels) -> None:
    """labels [H,W] -> np.savez(path, seg_map=labels): the file the reference's `style_seg_path` / `clusters_path` reads"""
    np.savez(path, seg_map=(labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)))
