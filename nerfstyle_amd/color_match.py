"""Colour transfer of pixel rows to a style image: ARF's colour matching, the reference's `utils.match_colors_for_image_set`
(utils/__init__.py:262-295), which `DatasetConfig.ct_image` applies to the training images before the stylisation stage
(data/base_dataset.py:97-105).

With mu, C the mean and 3x3 covariance of every content pixel and mu_s, C_s those of the style image, the map is
x -> A x + b, A = C_s^(1/2) C^(-1/2), b = mu_s - A mu, clamped to [0, 1]: the content's colours get the style's mean and
covariance.  The reference does this in fp32 torch on [N*H*W, 3] rows; here the rows stay where they are in HBM and two HIP
passes stream over them (csrc/color_match.hip): nsr_color_moments sums x and x x^T in fp64 in a fixed order (bit-identical from
run to run and across data-parallel ranks), nsr_color_apply maps the rows in place as an f32 fma chain.  The eigen-solve of the
two 3x3 covariances between them is host code."""
import torch

from . import _lib as L


def _rows(rows: torch.Tensor, what: str):
    """(device pointer, n, stride) of a contiguous f32 device tensor [..., 3] or [..., 4]"""
    ptr = L.p(rows)
    if rows.dtype != torch.float32 or rows.dim() < 1 or rows.shape[-1] not in (3, 4) or rows.numel() == 0:
        raise ValueError('{}: rows must be a non-empty float32 tensor [..., 3] or [..., 4]; got {} {}'.format(
            what, rows.dtype, tuple(rows.shape)))
    stride = int(rows.shape[-1])
    return ptr, rows.numel() // stride, stride


def color_moments(rows: torch.Tensor) -> torch.Tensor:
    """rows [..., 3] or [..., 4] f32 contiguous on the HIP device (a fourth float is never read) -> [9] float64 device tensor
    sum r, g, b, rr, rg, rb, gg, gb, bb over all rows, every product and sum in fp64, in an order that depends on the row count
    and the layout only (include/nsr.h): two calls, and two ranks holding the same rows, get the same bits."""
    ptr, n, stride = _rows(rows, 'color_moments')
    moments = torch.empty(9, dtype=torch.float64, device=rows.device)
    ws = torch.empty(int(L.lib().nsr_color_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device=rows.device)
    L.check(L.lib().nsr_color_moments(ptr, n, stride, L.p(moments), L.p(ws), L.stream()), 'color_moments')
    return moments


def _mean_cov(moments, n):
    m = torch.as_tensor(moments).detach().to('cpu', torch.float64)
    if m.shape != (9,) or n < 1:
        raise ValueError('solve_color_transform: moments must be [9] and the row counts positive')
    mu = m[:3] / n
    s = m[3:]
    second = torch.stack([torch.stack([s[0], s[1], s[2]]), torch.stack([s[1], s[3], s[4]]), torch.stack([s[2], s[4], s[5]])])
    return mu, second / n - torch.outer(mu, mu)


def solve_color_transform(content_moments, n_c: int, style_moments, n_s: int) -> torch.Tensor:
    """The reference's `color_tf` from the moments of n_c content rows and n_s style rows (color_moments, or host tensors of
    the same nine sums): [4,4] float32 with A in [:3,:3], b in [:3,3] and the last row 0 0 0 1, on the device of
    `content_moments` when that is a tensor.

    Host code in fp64: mu = sum x / n, C = sum x x^T / n - mu mu^T; both covariances are decomposed with torch.linalg.eigh on
    the CPU, their eigenvalues clamped to [1e-8, 1e8] as the reference clamps its singular values;
    A = U_s S_s^(1/2) U_s^T U_c S_c^(-1/2) U_c^T, b = mu_s - A mu_c, rounded to float32 once.
    THE ONE HOST READ of the colour transfer happens here: 18 doubles, which waits for the moment kernels.  This is set-up,
    not a training step; do not call it inside a captured graph."""
    mu_c, cov_c = _mean_cov(content_moments, int(n_c))
    mu_s, cov_s = _mean_cov(style_moments, int(n_s))
    e_c, u_c = torch.linalg.eigh(cov_c)
    e_s, u_s = torch.linalg.eigh(cov_s)
    inv_sqrt_c = (u_c * (1.0 / torch.sqrt(e_c.clamp(1e-8, 1e8)))) @ u_c.T
    sqrt_s = (u_s * torch.sqrt(e_s.clamp(1e-8, 1e8))) @ u_s.T
    A = sqrt_s @ inv_sqrt_c
    tf = torch.eye(4, dtype=torch.float64)
    tf[:3, :3] = A
    tf[:3, 3] = mu_s - A @ mu_c
    tf = tf.to(torch.float32)
    return tf.to(content_moments.device) if isinstance(content_moments, torch.Tensor) else tf


def apply_color_transform(rows: torch.Tensor, color_tf: torch.Tensor, clamp: bool = True, out: torch.Tensor = None) -> torch.Tensor:
    """rows [..., 3] or [..., 4] f32 contiguous on the HIP device -> the rows with (r, g, b) <- A (r, g, b) + b of `color_tf`
    [4,4] (solve_color_transform; a host tensor is copied to the device), as an f32 fma chain (include/nsr.h), clamped to
    [0, 1] unless clamp=False; a fourth float is carried over bit for bit.  out=rows works in place; out=None allocates; any
    other `out` must have the rows' shape and not overlap them.  The same call maps rendered `rgb_map` rows."""
    ptr, n, stride = _rows(rows, 'apply_color_transform')
    if tuple(color_tf.shape) != (4, 4):
        raise ValueError('apply_color_transform: color_tf must be [4,4]; got {}'.format(tuple(color_tf.shape)))
    tf = color_tf.detach().to(rows.device, torch.float32).contiguous()
    if out is None:
        out = torch.empty_like(rows)
    elif out.shape != rows.shape or out.dtype != torch.float32:
        raise ValueError('apply_color_transform: out must be float32 of shape {}'.format(tuple(rows.shape)))
    L.check(L.lib().nsr_color_apply(ptr, L.p(out), n, stride, L.p(tf), int(bool(clamp)), L.stream()), 'color_apply')
    return out


def match_colors_for_image_set(image_set: torch.Tensor, style_img: torch.Tensor):
    """The reference's function of this name on the HIP device: image_set [N,H,W,3], style_img [H,W,3], both f32 ->
    (the recoloured image set, a new tensor clamped to [0, 1]; color_tf [4,4] f32 on the device)."""
    if image_set.dim() != 4 or image_set.shape[-1] != 3 or style_img.dim() != 3 or style_img.shape[-1] != 3:
        raise ValueError('match_colors_for_image_set: image_set [N,H,W,3] and style_img [H,W,3]; got {} and {}'.format(
            tuple(image_set.shape), tuple(style_img.shape)))
    style = style_img.to(image_set.device).contiguous()
    color_tf = solve_color_transform(color_moments(image_set), image_set.numel() // 3, color_moments(style), style.numel() // 3)
    return apply_color_transform(image_set, color_tf), color_tf


# ---- region-wise transfer: one transform per scene class, matched to a style cluster (csrc/color_regions.hip) ----------------------
MAX_REGIONS = 64                # NSR_COLOR_MAX_REGIONS


def _labels(labels, rows, n, stride, what):
    """device pointer of explicit labels (int32 [n] on the rows' device), or None for the fourth float of stride-4 rows"""
    if labels is None:
        if stride != 4:
            raise ValueError('{}: rows [..., 3] carry no label; pass labels'.format(what))
        return None
    ptr = L.p(labels)
    if labels.dtype != torch.int32 or labels.numel() != n or labels.device != rows.device:
        raise ValueError('{}: labels must be int32 with one entry per row ({}) on {}; got {} {} on {}'.format(
            what, n, rows.device, labels.dtype, tuple(labels.shape), labels.device))
    return ptr


def _check_k(K, what):
    K = int(K)
    if not 1 <= K <= MAX_REGIONS:
        raise ValueError('{}: K must be in 1..{}; got {}'.format(what, MAX_REGIONS, K))
    return K


def region_moments(rows: torch.Tensor, K: int, labels: torch.Tensor = None) -> torch.Tensor:
    """rows [..., 3] or [..., 4] f32 contiguous on the HIP device -> [K+1, 10] float64 device tensor: per region count, sum r, g,
    b, rr, rg, rb, gg, gb, bb.  A row's region is labels[i] (int32, one per row) or, with labels=None and rows [..., 4], its
    fourth float when that is exactly an integer in 0..K-1; every other row is counted in slot K.  fp64 throughout, the count
    exact, no atomics: the order of additions depends on the row count, the layout, K and the labels only (include/nsr.h)."""
    ptr, n, stride = _rows(rows, 'region_moments')
    K = _check_k(K, 'region_moments')
    lp = _labels(labels, rows, n, stride, 'region_moments')
    moments = torch.empty(K + 1, 10, dtype=torch.float64, device=rows.device)
    ws = torch.empty(int(L.lib().nsr_color_region_moments_workspace_bytes(n, K)) // 8, dtype=torch.float64, device=rows.device)
    L.check(L.lib().nsr_color_region_moments(ptr, n, stride, lp, K, L.p(moments), L.p(ws), L.stream()), 'color_region_moments')
    return moments


def solve_region_transforms(content_moments, style_moments, matching, min_rows: int = 256, fallback: str = 'global') -> torch.Tensor:
    """content_moments [Kc+1, 10], style_moments [Ks+1, 10] (region_moments, or host tensors / arrays of the same sums) and
    matching [Kc] (class i -> style cluster matching[i]) -> [Kc+1, 4, 4] float32, on the device of `content_moments` when that
    is a tensor.

    Class i gets solve_color_transform(content region i, style region matching[i]) when 0 <= matching[i] < Ks and both regions
    hold at least `min_rows` rows (the eigenvalue clamp already keeps a thin covariance finite; min_rows keeps a handful of
    mislabelled pixels from getting a palette of their own).  Every other class, and slot Kc, gets the fallback: 'global' is all
    content rows against all style rows (the sums over every slot, slot K included), 'identity' the identity.  Two classes may
    share a cluster.  Host code in fp64; THE ONE HOST READ of the region transfer: 10 (Kc + Ks + 2) doubles.  Set-up, not for a
    captured graph."""
    if fallback not in ('global', 'identity'):
        raise ValueError("solve_region_transforms: fallback must be 'global' or 'identity'; got {!r}".format(fallback))
    mc = torch.as_tensor(content_moments).detach().to('cpu', torch.float64)
    ms = torch.as_tensor(style_moments).detach().to('cpu', torch.float64)
    if mc.dim() != 2 or ms.dim() != 2 or mc.shape[1] != 10 or ms.shape[1] != 10 or mc.shape[0] < 2 or ms.shape[0] < 2:
        raise ValueError('solve_region_transforms: moments must be [K+1, 10]; got {} and {}'.format(tuple(mc.shape), tuple(ms.shape)))
    Kc, Ks = mc.shape[0] - 1, ms.shape[0] - 1
    matching = [int(m) for m in (matching.tolist() if isinstance(matching, torch.Tensor) else matching)]
    if len(matching) != Kc:
        raise ValueError('solve_region_transforms: matching has {} entries for {} classes'.format(len(matching), Kc))
    base = torch.eye(4, dtype=torch.float32)
    if fallback == 'global':
        tc, ts = mc.sum(0), ms.sum(0)
        if tc[0] < 1 or ts[0] < 1:
            raise ValueError('solve_region_transforms: no rows')
        base = solve_color_transform(tc[1:], int(tc[0]), ts[1:], int(ts[0]))
    tfs = base.repeat(Kc + 1, 1, 1)
    for i, j in enumerate(matching):
        if 0 <= j < Ks and mc[i, 0] >= max(1, min_rows) and ms[j, 0] >= max(1, min_rows):
            tfs[i] = solve_color_transform(mc[i, 1:], int(mc[i, 0]), ms[j, 1:], int(ms[j, 0]))
    return tfs.to(content_moments.device) if isinstance(content_moments, torch.Tensor) else tfs


def apply_region_transforms(rows: torch.Tensor, tfs: torch.Tensor, labels: torch.Tensor = None, clamp: bool = True,
                            out: torch.Tensor = None) -> torch.Tensor:
    """rows [..., 3] or [..., 4] f32 contiguous on the HIP device -> every row mapped by tfs[region] of `tfs` [K+1, 4, 4]
    (solve_region_transforms; a host tensor is copied to the device), region as in region_moments, with the f32 fma chain and
    clamp of apply_color_transform; a fourth float is carried over bit for bit.  out as in apply_color_transform.  The same call
    maps rendered `rgb_map` rows with labels = preds.to(torch.int32)."""
    ptr, n, stride = _rows(rows, 'apply_region_transforms')
    if tfs.dim() != 3 or tuple(tfs.shape[1:]) != (4, 4) or tfs.shape[0] < 2:
        raise ValueError('apply_region_transforms: tfs must be [K+1,4,4]; got {}'.format(tuple(tfs.shape)))
    K = _check_k(tfs.shape[0] - 1, 'apply_region_transforms')
    lp = _labels(labels, rows, n, stride, 'apply_region_transforms')
    t = tfs.detach().to(rows.device, torch.float32).contiguous()
    if out is None:
        out = torch.empty_like(rows)
    elif out.shape != rows.shape or out.dtype != torch.float32:
        raise ValueError('apply_region_transforms: out must be float32 of shape {}'.format(tuple(rows.shape)))
    L.check(L.lib().nsr_color_region_apply(ptr, L.p(out), n, stride, lp, K, L.p(t), int(bool(clamp)), L.stream()), 'color_region_apply')
    return out
