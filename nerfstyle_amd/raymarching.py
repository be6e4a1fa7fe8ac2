"""Host-side mirror of the reference's `raymarching` package (raymarching/raymarching.py): same
function names, argument meaning and return values, backed by libnsr_hip.so through the C ABI.

Reference aliases mirrored: near_far_from_aabb (:52), morton3D (:113), morton3D_invert (:136),
packbits (:167), march_rays_train (:288), composite_rays_train (:350), march_rays (:427),
composite_rays (:462).  Like the reference wrappers, inputs are cast to float32 and made
contiguous; unlike them, nothing is silently moved to the GPU: a CPU tensor raises.

Extra entry points with no reference counterpart (used by the renderer's fast path):
march_rays_train_nosync (capacity-bounded, no `.item()`), compact_alive, ray_geometry (differentiable depth and
distortion on the training composite's weights).
"""
import torch
from torch.autograd import Function

from . import _lib as L
from . import profiling


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class _near_far_from_aabb(Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, aabb, min_near=0.2):
        """raymarching.py:19-49"""
        rays_o = _f32(rays_o).view(-1, 3)
        rays_d = _f32(rays_d).view(-1, 3)
        aabb = _f32(aabb)
        N = rays_o.shape[0]
        nears = torch.empty(N, dtype=torch.float32, device=rays_o.device)
        fars = torch.empty(N, dtype=torch.float32, device=rays_o.device)
        L.check(L.lib().nsr_near_far_from_aabb(L.p(rays_o), L.p(rays_d), L.p(aabb), N, float(min_near), L.p(nears),
                                               L.p(fars), L.stream()), 'near_far_from_aabb')
        ctx.mark_non_differentiable(nears, fars)
        return nears, fars


near_far_from_aabb = _near_far_from_aabb.apply


def near_far_from_aabb_into(rays_o, rays_d, aabb, min_near, nears, fars):
    """near_far_from_aabb writing into caller-owned [N] float32 buffers (static buffers of a captured step)"""
    rays_o = _f32(rays_o).view(-1, 3)
    rays_d = _f32(rays_d).view(-1, 3)
    N = rays_o.shape[0]
    assert nears.numel() == N and fars.numel() == N and nears.dtype == fars.dtype == torch.float32
    L.check(L.lib().nsr_near_far_from_aabb(L.p(rays_o), L.p(rays_d), L.p(_f32(aabb)), N, float(min_near), L.p(nears),
                                           L.p(fars), L.stream()), 'near_far_from_aabb')
    return nears, fars


def morton3D(coords):
    """raymarching.py:89-113: coords [N,3] int -> indices [N] int32"""
    coords = coords.int().contiguous()
    N = coords.shape[0]
    indices = torch.empty(N, dtype=torch.int32, device=coords.device)
    L.check(L.lib().nsr_morton3d(L.p(coords), N, L.p(indices), L.stream()), 'morton3D')
    return indices


def morton3D_invert(indices):
    """raymarching.py:116-136"""
    indices = indices.int().contiguous()
    N = indices.shape[0]
    coords = torch.empty(N, 3, dtype=torch.int32, device=indices.device)
    L.check(L.lib().nsr_morton3d_invert(L.p(indices), N, L.p(coords), L.stream()), 'morton3D_invert')
    return coords


def packbits(grid, thresh, bitfield=None):
    """raymarching.py:139-167: grid [C, H^3] float -> bitfield uint8 [C*H^3/8]"""
    grid = _f32(grid)
    C, H3 = grid.shape[0], grid.shape[1]
    N = C * H3 // 8
    if bitfield is None:
        bitfield = torch.empty(N, dtype=torch.uint8, device=grid.device)
    L.check(L.lib().nsr_packbits(L.p(grid), N, float(thresh), L.p(bitfield), L.stream()), 'packbits')
    return bitfield


def mark_untrained_grid(density_grid, bitfield, poses, frustum, camera_flip, bound, cascade, grid_size, margin_cells, min_views,
                        counts=None):
    """nsr_occ_mark_untrained (no reference counterpart; torch-ngp's mark_untrained_grid): cells that fewer than `min_views` of
    the cameras see get density_grid = -1 and a cleared bit, in place; cells seen again that held a negative value get 0.
    density_grid [C, H^3] float32 and bitfield uint8 [C*H^3/8] (or None) are written in place and must be contiguous device
    tensors; poses [F,3,4] float32 on the device; frustum = (x_lo, x_hi, y_lo, y_hi) host floats, the pinhole coordinates of the
    frame's outer edges; counts (optional int32 [C*H^3]) receives the number of frames that see each cell.
    Returns n_untrained, int32 [C] on the device: the cells per cascade left at -1.  No host read."""
    if density_grid.dtype != torch.float32 or (bitfield is not None and bitfield.dtype != torch.uint8):
        raise ValueError('mark_untrained_grid: density_grid float32, bitfield uint8')
    L.p(density_grid)            # a CPU tensor raises before anything is allocated
    if int(min_views) < 1:
        raise ValueError('mark_untrained_grid: min_views >= 1')
    C, H = int(cascade), int(grid_size)
    cells = C * H ** 3
    poses = poses.detach().to(torch.float32)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError('mark_untrained_grid: poses [F,3,4]')
    poses = poses.contiguous()
    if density_grid.numel() != cells or (bitfield is not None and bitfield.numel() != cells // 8) or \
            (counts is not None and (counts.numel() != cells or counts.dtype != torch.int32)):
        raise ValueError('mark_untrained_grid: density_grid [C, H^3], bitfield [C*H^3/8], counts int32 [C*H^3]')
    n_untrained = torch.empty(C, dtype=torch.int32, device=density_grid.device)
    x_lo, x_hi, y_lo, y_hi = (float(v) for v in frustum)
    with profiling.timed('mark_untrained'):
        L.check(L.lib().nsr_occ_mark_untrained(
            L.p(density_grid), L.p(bitfield), C, H, float(bound), L.p(poses), poses.shape[0], x_lo, x_hi, y_lo, y_hi,
            int(camera_flip), float(margin_cells), int(min_views), L.p(counts), L.p(n_untrained), L.stream()), 'occ_mark_untrained')
    return n_untrained


# ---- occupancy components and the floater cull (csrc/occ_components.hip; include/nsr.h, "Occupancy components") ----------------
def _occ_cells(who, cascade, grid_size):
    C, H = int(cascade), int(grid_size)
    if not (1 <= C <= 8 and 8 <= H <= 512 and H & (H - 1) == 0 and C * H ** 3 < 2 ** 31):
        raise ValueError('{}: cascade in 1..8 and grid_size a power of two in 8..512 with cascade * grid_size^3 < 2^31; got {} and '
                         '{}'.format(who, cascade, grid_size))
    return C, H, C * H ** 3


def _occ_tensor(who, name, t, dtype, shape):
    """a tensor of that dtype and number of elements"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != int(torch.Size(shape).numel()):
        raise ValueError('{}: {} must be a {} tensor of shape {}; got {} {}'.format(
            who, name, str(dtype).replace('torch.', ''), list(shape), getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
    return t


def _occ_on_device(*tensors):
    """a CPU (or non-contiguous) tensor raises before anything is allocated ("no CPU fallback")"""
    for t in tensors:
        L.p(t)


def check_cull_rule(min_cells, min_diagonal, keep_largest, who):
    """the keep rule's arguments, in the words of mesh._check_keep_rule"""
    if int(min_cells) != min_cells or not 0 <= min_cells < 2 ** 31:
        raise ValueError('{}: min_cells must be an integer in 0 .. 2^31 - 1; got {}'.format(who, min_cells))
    if not float(min_diagonal) >= 0.0:
        raise ValueError('{}: min_diagonal must be >= 0; got {}'.format(who, min_diagonal))
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
        raise ValueError('{}: keep_largest must be None or an integer >= 1; got {}'.format(who, keep_largest))


def occupancy_components(bitfield, cascade, grid_size):
    """nsr_occ_components: labels int32 [C*H^3] of the occupancy bitfield (uint8 [C*H^3/8] on the device).  labels[u] is the
    smallest cell id of the component of cell u = c * H^3 + morton(ix, iy, iz), or -1 where the cell is not occupied; occupied
    cells of one cascade that share a face are joined, nothing wraps and nothing joins two cascades.  No host read."""
    C, H, cells = _occ_cells('occupancy_components', cascade, grid_size)
    _occ_on_device(_occ_tensor('occupancy_components', 'bitfield', bitfield, torch.uint8, (cells // 8,)))
    labels = torch.empty(cells, dtype=torch.int32, device=bitfield.device)
    with profiling.timed('occ_components'):
        L.check(L.lib().nsr_occ_components(L.p(bitfield), C, H, L.p(labels), L.stream()), 'occ_components')
    return labels


def occupancy_component_stats(labels, cascade, grid_size):
    """nsr_occ_component_stats -> (n_cells int32 [C*H^3], lo, hi int32 [C*H^3,3]), indexed by cell id and meaningful at the roots
    (labels[u] == u): the component's number of cells and its inclusive box in cell coordinates.  Every other cell holds 0,
    lo = H, hi = -1.  `labels` as occupancy_components returns them.  No host read."""
    C, H, cells = _occ_cells('occupancy_component_stats', cascade, grid_size)
    _occ_on_device(_occ_tensor('occupancy_component_stats', 'labels', labels, torch.int32, (cells,)))
    dev = labels.device
    n_cells = torch.empty(cells, dtype=torch.int32, device=dev)
    lo = torch.empty(cells, 3, dtype=torch.int32, device=dev)
    hi = torch.empty(cells, 3, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_occ_component_stats(L.p(labels), C, H, L.p(n_cells), L.p(lo), L.p(hi), L.stream()), 'occ_component_stats')
    return n_cells, lo, hi


def keep_occupancy_components(n_cells, lo, hi, cascade, grid_size, bound, min_cells=0, min_diagonal=0.0, keep_largest=None):
    """The keep rule on occupancy_component_stats' arrays -> keep uint8 [C*H^3], set at the roots of the kept components.  A
    component of cascade c is kept iff n_cells >= min_cells, (2 b_c / H)^2 * (ex^2 + ey^2 + ez^2) >= min_diagonal^2 (e = hi - lo
    + 1 in cells, b_c = min(2^c, bound): the box's diagonal in the grid's units; fp64, in this written order) and, with
    keep_largest = k, it is among the k components of the most cells of its own cascade among those that passed (ties to the
    smaller label).  The defaults keep everything.  Elementwise torch over all cells and a fixed-k topk a cascade: no host read."""
    check_cull_rule(min_cells, min_diagonal, keep_largest, 'keep_occupancy_components')
    C, H, cells = _occ_cells('keep_occupancy_components', cascade, grid_size)
    _occ_tensor('keep_occupancy_components', 'n_cells', n_cells, torch.int32, (cells,))
    _occ_tensor('keep_occupancy_components', 'lo', lo, torch.int32, (cells, 3))
    _occ_tensor('keep_occupancy_components', 'hi', hi, torch.int32, (cells, 3))
    _occ_on_device(n_cells, lo, hi)
    dev = n_cells.device
    n = n_cells.view(C, H ** 3).to(torch.int64)
    e = (hi.view(C, H ** 3, 3) - lo.view(C, H ** 3, 3) + 1).to(torch.float64)
    b = torch.tensor([min(float(2 ** c), float(bound)) for c in range(C)], dtype=torch.float64, device=dev)
    unit = 2.0 * b / float(H)
    diag2 = (unit * unit).view(C, 1) * ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    ok = (n > 0) & (n >= int(min_cells)) & (diag2 >= float(min_diagonal) * float(min_diagonal))      # n > 0: a root
    if keep_largest is not None:
        k = min(int(keep_largest), H ** 3)
        never = torch.iinfo(torch.int64).max
        ids = torch.arange(cells, dtype=torch.int64, device=dev).view(C, H ** 3)
        key = torch.where(ok, (0x7fffffff - n) * (1 << 32) + ids, never)                   # most cells first, then the label
        best, at = torch.topk(key, k, dim=1, largest=False)
        return torch.zeros(C, H ** 3, dtype=torch.uint8, device=dev).scatter_(1, at, (best != never).to(torch.uint8)).view(cells)
    return ok.to(torch.uint8).view(cells)


def cull_occupancy(density_grid, bitfield, labels, keep, cascade, grid_size):
    """nsr_occ_cull, in place: every occupied cell whose component's root has keep == 0 loses its bit in `bitfield` and, with a
    density_grid (float32 [C, H^3]; None: bits only), gets density_grid = -1, the untrained state that update_state never
    changes.  Every other bit and grid word stays as it is.  -> n_culled int32 [C] on the device.  No host read."""
    C, H, cells = _occ_cells('cull_occupancy', cascade, grid_size)
    if density_grid is not None:
        _occ_tensor('cull_occupancy', 'density_grid', density_grid, torch.float32, (C, H ** 3))
    _occ_tensor('cull_occupancy', 'bitfield', bitfield, torch.uint8, (cells // 8,))
    _occ_tensor('cull_occupancy', 'labels', labels, torch.int32, (cells,))
    _occ_tensor('cull_occupancy', 'keep', keep, torch.uint8, (cells,))
    _occ_on_device(density_grid, bitfield, labels, keep)
    n_culled = torch.empty(C, dtype=torch.int32, device=bitfield.device)
    with profiling.timed('occ_cull'):
        L.check(L.lib().nsr_occ_cull(L.p(density_grid), L.p(bitfield), L.p(labels), L.p(keep), C, H, L.p(n_culled), L.stream()),
                'occ_cull')
    return n_culled


def _march_workspace(N, device, bound, max_steps):
    nbytes = int(L.lib().nsr_march_rays_train_workspace_bytes(N, float(bound), int(max_steps)))
    return torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)


def march_rays_train_nosync(rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, M, step_counter,
                            dt_gamma=0., max_steps=1024, want_dirs=False, out=None):
    """Capacity-bounded march: emits into [M, .] buffers and never reads the sample count on the
    host (the count stays in step_counter[0] on the device).  Samples past the count are NOT
    zero-filled (the reference memsets 40 B x N x max_steps per call, raymarching.py:238-240):
    consumers bound themselves by the device count / by `rays`.
    Returns xyzs [M,3], dirs [M,3] | None, deltas [M,4], rays [N,3]."""
    rays_o = _f32(rays_o).view(-1, 3)
    rays_d = _f32(rays_d).view(-1, 3)
    N = rays_o.shape[0]
    dev = rays_o.device
    if out is not None:
        # caller-owned sample buffers (xyzs [M,3], deltas [M,4] f32, rays [N,3] i32, and with want_dirs a fourth, dirs [M,3]
        # f32), e.g. the static buffers of a captured step
        if want_dirs:
            xyzs, deltas, rays, dirs = out
            assert dirs.shape == (M, 3) and dirs.dtype == torch.float32 and dirs.is_contiguous()
        else:
            xyzs, deltas, rays = out
            dirs = None
        assert xyzs.shape == (M, 3) and deltas.shape == (M, 4) and rays.shape == (N, 3)
    else:
        xyzs = torch.empty(M, 3, dtype=torch.float32, device=dev)
        dirs = torch.empty(M, 3, dtype=torch.float32, device=dev) if want_dirs else None
        deltas = torch.empty(M, 4, dtype=torch.float32, device=dev)
        rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    ws = _march_workspace(N, dev, bound, max_steps)
    with profiling.timed('march_train'):
        L.check(L.lib().nsr_march_rays_train(
            L.p(rays_o), L.p(rays_d), None, L.p(density_bitfield), float(bound), float(dt_gamma), int(max_steps), 0,
            N, int(C), int(H), int(M), L.p(nears), L.p(fars), L.p(xyzs), L.p(dirs), L.p(deltas), L.p(rays),
            L.p(step_counter), None, L.p(ws), L.stream()), 'march_rays_train')
    return xyzs, dirs, deltas, rays


def march_rays_train(rays_o, rays_d, z_hats, bound, density_bitfield, C, H, nears, fars,
                     step_counter=None, mean_count=-1, perturb=False, align=-1,
                     force_all_rays=False, dt_gamma=0, max_steps=1024, is_ndc=False):
    """raymarching.py:174-288, same arguments and return values (xyzs, dirs, deltas, rays), same
    host synchronisation on the emitted count (`step_counter[0].item()`, :276) and the same
    align-to-`align` padding with zeroed samples (:238-240,277-281).  perturb is ignored like
    the reference does (:247)."""
    rays_o = _f32(rays_o).view(-1, 3)
    rays_d = _f32(rays_d).view(-1, 3)
    density_bitfield = density_bitfield.contiguous()
    N = rays_o.shape[0]
    dev = rays_o.device
    M = N * max_steps
    if not force_all_rays and mean_count > 0:
        if align > 0:
            mean_count += align - mean_count % align
        M = mean_count
    if is_ndc:
        z_hats = _f32(z_hats).view(-1)
    xyzs = torch.empty(M, 3, dtype=torch.float32, device=dev)
    dirs = torch.empty(M, 3, dtype=torch.float32, device=dev)
    deltas = torch.empty(M, 4, dtype=torch.float32, device=dev)
    rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    if step_counter is None:
        step_counter = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = _march_workspace(N, dev, bound, max_steps)
    L.check(L.lib().nsr_march_rays_train(
        L.p(rays_o), L.p(rays_d), L.p(z_hats) if is_ndc else None, L.p(density_bitfield), float(bound),
        float(dt_gamma), int(max_steps), int(bool(is_ndc)), N, int(C), int(H), int(M), L.p(nears), L.p(fars),
        L.p(xyzs), L.p(dirs), L.p(deltas), L.p(rays), L.p(step_counter), None, L.p(ws), L.stream()),
        'march_rays_train')
    m_emitted = int(step_counter[0].item())   # D2H sync, as in the reference
    m = m_emitted
    if force_all_rays or mean_count <= 0:
        if align > 0:
            m += align - m % align
        m = min(m, M)
    else:
        m = M
    # the reference hands back zero-initialised tails (torch.zeros allocation); only the tail needs it
    lo = min(m_emitted, m)
    xyzs, dirs, deltas = xyzs[:m], dirs[:m], deltas[:m]
    xyzs[lo:].zero_()
    dirs[lo:].zero_()
    deltas[lo:].zero_()
    if not is_ndc:
        deltas[:, 2:].zero_()
    return xyzs, dirs, deltas, rays


class _composite_rays_train(Function):
    @staticmethod
    def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh=1e-4, is_ndc=False):
        """raymarching.py:291-325"""
        sigmas = sigmas.to(torch.float32).contiguous().view(-1)
        rgbs = rgbs.to(torch.float32).contiguous()
        deltas = deltas.contiguous()
        M, N, C = sigmas.shape[0], rays.shape[0], rgbs.shape[1]
        dev = sigmas.device
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty(N, C, dtype=torch.float32, device=dev)
        L.check(L.lib().nsr_composite_rays_train_forward(
            L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rays), M, N, C, float(T_thresh), int(bool(is_ndc)),
            L.p(weights_sum), L.p(depth), L.p(image), L.stream()), 'composite_rays_train_forward')
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, image)
        ctx.dims = [M, N, C, T_thresh]
        ctx.is_ndc = is_ndc
        ctx.mark_non_differentiable(depth)
        return weights_sum, depth, image

    @staticmethod
    def backward(ctx, grad_weights_sum, grad_depth, grad_image):
        """raymarching.py:327-347 (grad_depth is ignored there too, :331)"""
        sigmas, rgbs, deltas, rays, weights_sum, image = ctx.saved_tensors
        M, N, C, T_thresh = ctx.dims
        grad_weights_sum = grad_weights_sum.to(torch.float32).contiguous()
        grad_image = grad_image.to(torch.float32).contiguous()
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        L.check(L.lib().nsr_composite_rays_train_backward(
            L.p(grad_weights_sum), L.p(grad_image), L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rays),
            int(bool(ctx.is_ndc)), L.p(weights_sum), L.p(image), M, N, C, float(T_thresh), L.p(grad_sigmas),
            L.p(grad_rgbs), L.stream()), 'composite_rays_train_backward')
        return grad_sigmas, grad_rgbs, None, None, None, None


composite_rays_train = _composite_rays_train.apply


class _ray_geometry(Function):
    """nsr_ray_geometry_forward / _backward (no reference counterpart): depth and distortion of every ray from the weights of
    the training composite, with a gradient for sigmas alone."""

    @staticmethod
    def forward(ctx, sigmas, deltas, rays, nears, fars, T_thresh=1e-4, is_ndc=False, zero_unowned=True):
        ctx.set_materialize_grads(False)     # an output the loss does not use arrives as None: NULL for the kernel
        ctx.sigmas_shape = sigmas.shape
        sigmas = sigmas.to(torch.float32).contiguous().view(-1)
        deltas = deltas.contiguous()
        nears, fars = _f32(nears).view(-1), _f32(fars).view(-1)
        M, N = sigmas.shape[0], rays.shape[0]
        dev = sigmas.device
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        distortion = torch.empty(N, dtype=torch.float32, device=dev)
        totals = torch.empty(N, 4, dtype=torch.float32, device=dev)
        with profiling.timed('geometry_fwd'):
            L.check(L.lib().nsr_ray_geometry_forward(
                L.p(sigmas), L.p(deltas), L.p(rays), L.p(nears), L.p(fars), M, N, float(T_thresh), int(bool(is_ndc)),
                L.p(depth), L.p(distortion), L.p(totals), L.stream()), 'ray_geometry_forward')
        ctx.save_for_backward(sigmas, deltas, rays, nears, fars, totals)
        ctx.args = (M, N, float(T_thresh), int(bool(is_ndc)), bool(zero_unowned))
        return depth, distortion

    @staticmethod
    def backward(ctx, grad_depth, grad_distortion):
        if grad_depth is None and grad_distortion is None:
            return (None,) * 8
        sigmas, deltas, rays, nears, fars, totals = ctx.saved_tensors
        M, N, T_thresh, is_ndc, zero_unowned = ctx.args

        def prep(g):
            return None if g is None else g.to(torch.float32).contiguous()
        grad_depth, grad_distortion = prep(grad_depth), prep(grad_distortion)
        # the kernel writes every sample that belongs to a ray; slots no ray owns keep what the buffer held
        grad_sigmas = torch.zeros_like(sigmas) if zero_unowned else torch.empty_like(sigmas)
        with profiling.timed('geometry_bwd'):
            L.check(L.lib().nsr_ray_geometry_backward(
                L.p(grad_depth), L.p(grad_distortion), L.p(sigmas), L.p(deltas), L.p(rays), L.p(nears), L.p(fars), L.p(totals),
                M, N, T_thresh, is_ndc, L.p(grad_sigmas), L.stream()), 'ray_geometry_backward')
        return (grad_sigmas.view(ctx.sigmas_shape),) + (None,) * 7


def ray_geometry(sigmas, deltas, rays, nears, fars, T_thresh=1e-4, is_ndc=False, zero_unowned=True):
    """Differentiable per-ray geometry terms on the weights w_i of composite_rays_train (same samples, delta columns and
    stop rule) -> (depth [N], distortion [N]), R = fars - nears:
      depth      = clamp(sum_i w_i t_i - nears, 0) / R: render_train's depth, but with a gradient;
      distortion = (sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 delta_i) / R, the mip-NeRF 360 regulariser.
    Both are 0 (and pass no gradient) for dropped and empty rays and where R is not a positive finite number, e.g. rays that
    miss the box.  The gradient reaches `sigmas` only and is exact on every live sample, the one a ray stops on included.
    zero_unowned=False hands the gradient's slots that no ray owns back uninitialised (capacity-sized buffers whose consumer
    bounds itself by the rays, as the renderer's does)."""
    return _ray_geometry.apply(sigmas, deltas, rays, nears, fars, T_thresh, is_ndc, zero_unowned)


def rays_position_backward(grad_xyzs, deltas, rays, M, nears=None, is_ndc=False):
    """nsr_rays_position_backward: the samples' position gradients [M,3] summed back to their rays for xyz_i = o + t_i d
    -> (grad_rays_o [N,3], grad_rays_d [N,3]).  M: the capacity the march used for its drop test.  nears [N]: the rays' first
    parameters, so that t_i is the sample's own parameter (without, the composite's running sum of deltas[:, 1])."""
    grad_xyzs = grad_xyzs.to(torch.float32).contiguous()
    N, dev = rays.shape[0], grad_xyzs.device
    g_o = torch.empty(N, 3, dtype=torch.float32, device=dev)
    g_d = torch.empty(N, 3, dtype=torch.float32, device=dev)
    with profiling.timed('rays_position_bwd'):
        L.check(L.lib().nsr_rays_position_backward(L.p(grad_xyzs), L.p(deltas), L.p(rays), L.p(nears), int(M), N, int(bool(is_ndc)),
                                                   L.p(g_o), L.p(g_d), L.stream()), 'rays_position_backward')
    return g_o, g_d


class _sample_positions(Function):
    """The marched positions as a function of their rays (xyz_i = o + t_i d, the t_i and the set of samples constant): returns
    the marched buffer itself, the backward is rays_position_backward."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, xyzs, deltas, rays, nears, M):
        ctx.save_for_backward(deltas, rays, nears)
        ctx.M = M
        return xyzs

    @staticmethod
    def backward(ctx, grad_xyzs):
        deltas, rays, nears = ctx.saved_tensors
        g_o, g_d = rays_position_backward(grad_xyzs, deltas, rays, ctx.M, nears)
        return g_o, g_d, None, None, None, None, None


def sample_positions(rays_o, rays_d, xyzs, deltas, rays, nears, M):
    return _sample_positions.apply(rays_o, rays_d, xyzs, deltas, rays, nears, M)


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, z_hats, bound, density_bitfield,
               C, H, near, far, align=-1, perturb=False, dt_gamma=0, max_steps=1024, is_ndc=False):
    """raymarching.py:357-424"""
    rays_o = _f32(rays_o).view(-1, 3)
    rays_d = _f32(rays_d).view(-1, 3)
    dev = rays_o.device
    M = n_alive * n_step
    if align > 0:
        M += align - (M % align)
    xyzs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    dirs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    deltas = torch.zeros(M, 4, dtype=torch.float32, device=dev)
    noises = torch.rand(n_alive, dtype=torch.float32, device=dev) if perturb else None
    L.check(L.lib().nsr_march_rays(
        int(n_alive), int(n_step), L.p(rays_alive), L.p(rays_t), L.p(rays_o), L.p(rays_d),
        L.p(_f32(z_hats).view(-1)) if is_ndc else None, float(bound), float(dt_gamma), int(max_steps),
        int(bool(is_ndc)), int(C), int(H), L.p(density_bitfield), L.p(near), L.p(far), L.p(xyzs), L.p(dirs),
        L.p(deltas), L.p(noises), L.stream()), 'march_rays')
    return xyzs, dirs, deltas


def composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, is_ndc, weights_sum, depth, image,
                   T_thresh=1e-2):
    """raymarching.py:430-459 (in place on rays_alive, rays_t, weights_sum, depth, image)"""
    t_size = 2 if is_ndc else 1
    assert rays_t.shape[-1] == t_size
    sigmas = sigmas.to(torch.float32).contiguous().view(-1)
    rgbs = rgbs.to(torch.float32).contiguous()
    C = rgbs.shape[-1]
    L.check(L.lib().nsr_composite_rays(
        int(n_alive), int(n_step), float(T_thresh), L.p(rays_alive), L.p(rays_t), L.p(sigmas), L.p(rgbs),
        L.p(deltas), C, int(bool(is_ndc)), L.p(weights_sum), L.p(depth), L.p(image), L.stream()), 'composite_rays')
    return tuple()


def compact_alive(rays_alive, n_alive, out=None, n_out=None):
    """Stable device-side compaction of `rays_alive[:n_alive] >= 0` (replaces the boolean-mask
    indexing of renderer.py:284).  Returns (out, n_out) with n_out a 1-element device tensor."""
    dev = rays_alive.device
    if out is None:
        out = torch.empty(max(n_alive, 1), dtype=torch.int32, device=dev)
    if n_out is None:
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(L.lib().nsr_compact_alive_workspace_bytes(n_alive))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_compact_alive(L.p(rays_alive), int(n_alive), L.p(out), L.p(n_out), L.p(ws), L.stream()),
            'compact_alive')
    return out, n_out
