"""Host orchestration of the hot path: the counterpart of the reference's renderer.py
(`Renderer`: update_state :139-194, render_train :196-235, render_test :237-293, render :295-313,
state_dict / load_state_dict :78-107).  Same public methods, same state keys, same outputs.

What is different underneath (MI355X-first):
  * render_train never reads the sample count on the host: the march emits into a
    capacity-bounded buffer, the count stays on the device and the fused field kernels bound
    themselves by it (the reference does `step_counter[0].item()` + `empty_cache()` per call and
    memsets 40 B x N x max_steps first, raymarching.py:238-283);
  * the model is two fused launches (forward / backward), not 2 encoders + 4 MLPs + exp + cat;
  * the white-background / depth epilogue stays in torch (a few [N]-sized ops).
"""
from contextlib import contextmanager
from math import ceil, log2
from typing import Dict, Optional

import torch

from . import raymarching
from .common import Box2D, Intrinsics, RayBatch
from .config import RendererConfig
from .rays import generate_rays, generate_rays_frames, pixel_window, tile_order
from .style_nerf import StyleTCNerf

STEP_CTR_SIZE = 16


class Renderer(torch.nn.Module):
    def __init__(self, model: StyleTCNerf, cfg: RendererConfig, intr: Intrinsics, bound: float, name: str = 'Renderer',
                 precrop_frac: float = 1., raymarch_channels: int = 3, samples_per_ray_cap: Optional[int] = None):
        """samples_per_ray_cap: capacity of the sample buffers in samples per ray (None = max_steps,
        i.e. the reference's force_all_rays allocation N * max_steps; smaller values trade memory for
        the reference's mean_count-style "drop rays that do not fit" behaviour, raymarching.py:230-236)."""
        super().__init__()
        self.model = model
        self.cfg = cfg
        self.intr = intr
        self._use_precrop = False
        self.precrop_frac = precrop_frac
        self.raymarch_channels = raymarch_channels
        self.update_occ = True
        self.bound = bound
        self.samples_per_ray_cap = samples_per_ray_cap
        # Spatially ordered table scatter in the backward (nsr_sample_order + the two-kernel nsr_field_backward).  'auto': for
        # dense batches only -- on a full 1008x756 frame the backward drops from 49 to 29 ms (+ 1.8 ms sort); on sparse random
        # batches the blocks hold too few samples (65 536 random rays: 6.2 vs 4.5 ms).  True / False force it.
        self.sort_samples = 'auto'
        self.sort_min_rays = 90000       # any batch of at least this many rays ...
        self.sort_min_dense_rays = 16384  # ... or a DENSE pixel set (full frame / patch / crop: neighbouring pixels) of this many
        self._pinned_bitfield = None
        # Inference through the streaming kernel (render_test_fused: march, field and composite in one launch, no sample
        # buffer).  Opt-in; `reference_inference_loop` still wins.
        self.fused_inference = False
        # The no-grad training render through the same kernel with the TRAINING composite (render_train_fused): what pass 1
        # of the deferred stylisation iteration and validation renders ask for.  Opt-in; unmeasured on the GPU so far.
        self.fused_nograd_train = False
        # Per-ray geometry terms of the training render (raymarching.ray_geometry on the shaded samples): a differentiable depth and
        # the mip-NeRF 360 distortion, for depth supervision and a floater regulariser.  Opt-in: shade_train fills a `geometry` dict,
        # render(training=True) / finish_train add 'depth' and 'distortion' to their output; render_test never does.
        self.geometry_terms = False
        # Camera pose gradients through the training render (pose refinement, nerfstyle_amd/pose.py).  Opt-in: with the switch on
        # AND a pose tensor that requires grad, the rays stay attached to the pose (rays.generate_rays), the marched positions to
        # their rays (xyz_i = o + t_i d; the t_i, the set of samples, nears / fars and the depth normalisation are constants, as in
        # instant-ngp) and the field returns d loss / d position.  The call then always takes the spatially ordered backward,
        # whose encoder-gradient buffer the position gradient is built from.  Off, or with a pose that does not require grad,
        # none of that is in the graph.
        self.pose_gradients = False
        self.reference_inference_loop = False     # render_test through render_test_loop (the reference's iteration structure)
        self.last_test_overflow = False            # the last bounded-capacity render_test overflowed and fell back to the loop
        self._infer_stats = None
        self._last_counter = self._last_capacity = None    # _set_last: what last_call_overflowed() answers from
        self._tile_orders = {}
        self.aabb = torch.tensor([-bound, -bound, -bound, bound, bound, bound], dtype=torch.float32)
        self.cascade = 1 + ceil(log2(bound))
        grid_size = self.cfg.grid_size
        bitfield_size = self.cascade * (grid_size ** 3) // 8
        self.density_grid = torch.zeros((self.cascade, grid_size ** 3))
        self.density_bitfield = torch.zeros((bitfield_size, ), dtype=torch.uint8)
        self.step_counter = torch.zeros((STEP_CTR_SIZE, 2), dtype=torch.int32)
        self.local_step = 0
        self._mean_density_dev, self._mean_density_host = None, 0.0
        self._mean_count_host, self._mean_count_stale = 0, False
        self._occ_state = None
        self._occ_key = self._occ_ws = self._occ_xyzs = self._occ_idx = None
        self.occ_seed = 0
        self.device = torch.device('cpu')

    # TensorModule behaviour of the reference (common.py:207-240): plain tensor attributes move too
    def _apply(self, fn, *args, **kwargs):
        for k in ('aabb', 'density_grid', 'density_bitfield', 'step_counter'):
            setattr(self, k, fn(getattr(self, k)))
        super()._apply(fn, *args, **kwargs)
        self.device = self.aabb.device
        if self._mean_density_dev is not None and self._mean_density_dev.device != self.device:
            self.mean_density = float(self._mean_density_dev.item())
        return self

    def state_dict(self):
        """renderer.py:78-91"""
        sd = {'model': self.model.state_dict()}
        for k in ['intr', 'precrop_frac', 'raymarch_channels', 'bound', 'density_grid', 'density_bitfield',
                  'step_counter', 'local_step', 'mean_count', 'mean_density']:
            v = getattr(self, k)
            if torch.is_tensor(v):
                v = v.detach()
            sd[k] = v
        return sd

    def load_state_dict(self, state_dict):
        """renderer.py:93-107"""
        for k in ['intr', 'precrop_frac', 'raymarch_channels', 'bound']:
            if getattr(self, k) != state_dict[k]:
                raise RuntimeError('Values do not match when loading key "{}"'.format(k))
        self.model.load_state_dict(state_dict['model'])
        for k in ['density_grid', 'density_bitfield', 'step_counter', 'local_step', 'mean_count', 'mean_density']:
            v = state_dict[k]
            if torch.is_tensor(v):
                v = v.to(self.device)
            setattr(self, k, v)

    @property
    def use_precrop(self):
        return self._use_precrop

    @use_precrop.setter
    def use_precrop(self, value: bool):
        self._use_precrop = value

    # ---- occupancy grid ------------------------------------------------------------------------
    @property
    def mean_density(self) -> float:
        """renderer.py:186 keeps a host float; here the value lives on the device and is read only when asked for."""
        if self._mean_density_dev is not None:
            return float(self._mean_density_dev.item())
        return self._mean_density_host

    @mean_density.setter
    def mean_density(self, v):
        self._mean_density_host = float(v)
        self._mean_density_dev = None

    @property
    def mean_count(self) -> int:
        """renderer.py:192-194 (mean emitted samples of the last min(16, update_iter) steps).  The reference marches
        with force_all_rays=True (:219-221), so the value is checkpoint state only: computed when read."""
        if self._mean_count_stale and self.step_counter.is_cuda:
            total_step = min(STEP_CTR_SIZE, self.cfg.update_iter)
            self._mean_count_host = int(self.step_counter[:total_step, 0].sum().item() / total_step)
            self._mean_count_stale = False
        return self._mean_count_host

    @mean_count.setter
    def mean_count(self, v):
        self._mean_count_host = int(v)
        self._mean_count_stale = False

    def manual_seed(self, seed: int):
        """Seed of the occupancy jitter / cell draws (counter-based: every rank that uses the same seed draws
        the same points, so data-parallel replicas keep identical grids without a collective)."""
        self.occ_seed = int(seed)
        return self

    def _occ_buffers(self, P):
        """Scratch of one update; allocated once per shape (no allocation in the steady state)."""
        key = (P, str(self.device))
        if self._occ_key != key:
            from . import _lib as L
            dev = self.device
            nbytes = int(L.lib().nsr_occ_workspace_bytes(self.cascade, self.cfg.grid_size))
            if nbytes == 0:
                raise RuntimeError('occupancy grid of size {} x {}^3 is not supported (H a power of two, 8..512)'.format(
                    self.cascade, self.cfg.grid_size))
            self._occ_ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
            self._occ_xyzs = torch.empty(P, 3, dtype=torch.float32, device=dev)
            self._occ_idx = torch.empty(P, dtype=torch.int32, device=dev)
            self._occ_key = key
        return self._occ_ws, self._occ_xyzs, self._occ_idx

    @torch.no_grad()
    def update_state(self, noise: Optional[torch.Tensor] = None) -> None:
        """renderer.py:139-194 on the device: cell choice + jitter (nsr_occ_sample_points), the sigma-only fused
        field on those points, then scatter / max-decay / mean / packbits (nsr_occ_update).  No host read, no
        allocation after the first call, legal under hipGraph capture.  `noise` [P,3] in [0,1) pins the jitter."""
        from . import _lib as L
        C, H = self.cascade, self.cfg.grid_size
        full = 1 if self.local_step < self.cfg.update_thres else 0
        P = int(L.lib().nsr_occ_num_points(C, H, full))
        ws, xyzs, idx = self._occ_buffers(P)
        if self._occ_state is None or self._occ_state.device != self.device:
            self._occ_state = torch.zeros(4, dtype=torch.int32, device=self.device)    # [0]: update sequence
        if self._mean_density_dev is None:
            self._mean_density_dev = torch.full((1,), self._mean_density_host, dtype=torch.float32, device=self.device)
        if not self.density_grid.is_contiguous():
            self.density_grid = self.density_grid.contiguous()
        L.check(L.lib().nsr_occ_sample_points(L.p(self.density_grid), C, H, float(self.bound), full, self.occ_seed, 0,
                                              L.p(self._occ_state), L.p(noise), L.p(xyzs), L.p(idx), L.p(ws), L.stream()),
                'occ_sample_points')
        sigmas = self.model.field(xyzs, sigma_only=True, density_scale=self.cfg.density_scale)
        L.check(L.lib().nsr_occ_update(L.p(self.density_grid), L.p(sigmas), L.p(idx), P, C, H, full,
                                       float(self.cfg.density_decay), float(self.cfg.density_thresh),
                                       L.p(self.density_bitfield), L.p(self._mean_density_dev), L.p(self._occ_state),
                                       L.p(ws), L.stream()), 'occ_update')
        self._mean_count_stale = True

    @torch.no_grad()
    def mark_untrained_grid(self, poses, lens=None, margin_cells: float = 1.5, min_views: int = 1, return_counts: bool = False):
        """Marks the occupancy cells that fewer than `min_views` of the training cameras see as untrained: density_grid = -1,
        which update_state never changes and never lists as occupied, and a cleared bit in density_bitfield (torch-ngp's
        mark_untrained_grid; raymarching.mark_untrained_grid states the test).  Opt-in: a trainer calls it once after loading
        the dataset; nothing calls it otherwise.  The marks are part of density_grid and so of state_dict().
        poses: [F,3,4] or [F,4,4], a tensor or NumPy, the poses generate_rays takes (all training frames, one set of intrinsics).
        The frustum is the outer pixel edges of `self.intr`, computed on the host in fp64; with lens ([6], LensRefiner.forward())
        that lens instead, read back ONCE here -- a setup call that synchronises, not for use inside a captured step -- and with
        k1, k2 the bounding rectangle of the distorted border (rays.frustum_bounds).
        margin_cells: a cell counts as seen when the sphere of margin_cells half-diagonals around its centre reaches into the
        frustum.  1 is already conservative for exact positions; the default of 1.5 also covers the fp32 rounding of the march's
        own cell index and small pose corrections.  With a PoseRefiner raise it, or call again with the refined poses: a call
        re-opens (sets to 0) marked cells that are now seen and leaves learnt densities alone.
        It works on density_grid / density_bitfield, never on a pinned bitfield, and is deterministic: ranks that call it with the
        same poses hold the same grid.  Returns n_untrained (int32 [cascade] on the device), with return_counts also the number
        of frames that see each cell (int32 [cascade, H^3])."""
        if self.cfg.use_ndc:
            raise NotImplementedError('mark_untrained_grid: use_ndc: the frustum test is in world space, NDC rays are warped')
        from .rays import _check_lens, frustum_bounds
        _check_lens(lens)
        poses = torch.as_tensor(poses, dtype=torch.float32, device=self.device)
        if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
            raise ValueError('mark_untrained_grid: poses [F,3,4] or [F,4,4]')
        w, h = self.intr.size()
        cam = (self.intr.fx, self.intr.fy, self.intr.cx, self.intr.cy)
        if lens is not None:
            cam = tuple(lens.detach().cpu().tolist())        # the one host read
        C, H = self.cascade, self.cfg.grid_size
        if not self.density_grid.is_contiguous():
            self.density_grid = self.density_grid.contiguous()
        counts = torch.empty(C, H ** 3, dtype=torch.int32, device=self.device) if return_counts else None
        n_untrained = raymarching.mark_untrained_grid(self.density_grid, self.density_bitfield, poses[:, :3, :], frustum_bounds(w, h, *cam),
                                                      self.cfg.flip_camera, self.bound, C, H, margin_cells, min_views, counts=counts)
        return (n_untrained, counts) if return_counts else n_untrained

    @torch.no_grad()
    def cull_floaters(self, min_cells: int = 0, min_diagonal: float = 0.0, keep_largest: Optional[int] = None, permanent: bool = True,
                      return_labels: bool = False):
        """Closes the small islands of occupied cells in the occupancy grid -- the floaters every march walks through: the
        volume-level counterpart of Mesh.clean.  The occupied cells of density_bitfield are split into connected components
        (cells of one cascade that share a face; raymarching.occupancy_components), each cascade on its own, and a component is
        kept iff it has at least `min_cells` cells, the diagonal of its box of cells is at least `min_diagonal` (in the grid's
        units, the world's -- with use_ndc the warped space the grid lives in) and, with keep_largest = k, it is among the k
        components of the most cells of its cascade among those (ties to the smaller label).  The defaults keep everything.
        Every cell of a component that is not kept loses its bit.
        permanent=True also writes density_grid = -1 there, the untrained state: update_state never changes such a cell and never
        lists it as occupied, and the marks are part of state_dict(), like those of mark_untrained_grid.  A later
        mark_untrained_grid re-opens (sets to 0) the marked cells that enough cameras see, so call it before, not after.
        permanent=False clears bits only, for inference until the next update_state rebuilds them.
        It works on density_grid / density_bitfield, never on a pinned bitfield, reads nothing on the host and is deterministic:
        data-parallel ranks that call it with the same arguments hold the same grid.  Opt-in; nothing calls it otherwise.
        Returns n_culled (int32 [cascade] on the device: the cells closed per cascade), with return_labels also the labels the
        cull was decided on (int32 [cascade * H^3]: the smallest cell id of the cell's component, -1 where it was not occupied)."""
        raymarching.check_cull_rule(min_cells, min_diagonal, keep_largest, 'cull_floaters')
        C, H = self.cascade, self.cfg.grid_size
        if not self.density_grid.is_contiguous():
            self.density_grid = self.density_grid.contiguous()
        labels = raymarching.occupancy_components(self.density_bitfield, C, H)
        n_cells, lo, hi = raymarching.occupancy_component_stats(labels, C, H)
        keep = raymarching.keep_occupancy_components(n_cells, lo, hi, C, H, self.bound, min_cells, min_diagonal, keep_largest)
        n_culled = raymarching.cull_occupancy(self.density_grid if permanent else None, self.density_bitfield, labels, keep, C, H)
        return (n_culled, labels) if return_labels else n_culled

    def pin_march_bitfield(self, bitfield: Optional[torch.Tensor]):
        """Benchmark / debugging hook: march through THIS bitfield while update_state keeps maintaining density_grid,
        mean_density and density_bitfield from the model as usual (None: back to density_bitfield).  Synthetic
        throughput runs use it: a random-initialised model has no scene, so the seeded synthetic occupancy stands in for
        the converged one while the periodic update still runs at full cost inside the step."""
        self._pinned_bitfield = bitfield
        return self

    @property
    def march_bitfield(self):
        return self.density_bitfield if self._pinned_bitfield is None else self._pinned_bitfield

    # ---- training render -----------------------------------------------------------------------
    def sample_capacity(self, n_rays: int) -> int:
        per_ray = self.cfg.max_steps if self.samples_per_ray_cap is None else min(self.samples_per_ray_cap,
                                                                               self.cfg.max_steps)
        return n_rays * per_ray

    def render_train(self, rays: RayBatch, **kwargs):
        """renderer.py:196-235 -> (image [N,3], depth [N], classes [N,nc]).  Three stages that graph.GraphedPatchBackward
        also drives one by one: march (sync-free), optional spatial order of the samples, shade (field + composite).
        With `fused_nograd_train` set and autograd off the call is render_train_fused instead (non-NDC, all model channels, and no
        `geometry_terms`: the streaming kernel has no such outputs).  geometry=dict: see shade_train."""
        pose_grad = self._pose_grad_wanted(rays.origins, rays.dirs)
        if self.fused_nograd_train and self.model.use_dir:
            raise NotImplementedError('fused_nograd_train: the streaming kernel has no direction input (view_dependent model)')
        if (self.fused_nograd_train and not torch.is_grad_enabled() and not self.cfg.use_ndc and not self.geometry_terms
                and self.raymarch_channels == self.model.out_channels):
            return self.render_train_fused(rays, dense_shape=kwargs.get('dense_shape'))
        if self.occupancy_update_due():
            self.update_state()
        mt = self.march_train(rays)
        perm = None
        if torch.is_grad_enabled() and (pose_grad or self._use_spatial_order(mt['N'], bool(kwargs.get('dense', False)))):
            perm = self.model.sample_order(mt['xyzs'], mt['counter'])
        return self.shade_train(mt, perm, geometry=kwargs.get('geometry'))

    def _pose_grad_wanted(self, *tensors) -> bool:
        """True when this training call differentiates with respect to the camera: the switch is on, autograd is recording and one
        of `tensors` (the pose, or the rays made from it) requires grad.  Raises NotImplementedError, naming the reason, for the
        configurations that cannot serve it -- before anything is launched."""
        if not (self.pose_gradients and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)):
            return False
        why = self.model.position_gradient_refusal()
        if why is None and self.cfg.use_ndc:
            why = 'use_ndc: an NDC sample is not o + t d of the rays the march is given'
        if why is None and (self.fused_nograd_train or self.fused_inference):
            why = 'the streaming fused_* paths keep no samples to differentiate through; switch fused_nograd_train / fused_inference off'
        if why is not None:
            raise NotImplementedError('pose_gradients: ' + why)
        return True

    @contextmanager
    def occupancy_frozen(self):
        """March and render without an occupancy update and without step bookkeeping (local_step and the count ring stay as
        they are, every march counts into a counter of its own): inside a captured graph, for a render beside the training
        schedule.  update_occ is restored on exit, also when the body raises."""
        keep = self.update_occ
        self.update_occ = False
        try:
            yield self
        finally:
            self.update_occ = keep

    def _call_counter(self, static: Optional[torch.Tensor] = None):
        """-> (counter, slot): the zeroed device-side (samples, rays) counter of this call, and the step bookkeeping in one place.
        With update_occ the call is a training step: ring slot local_step % STEP_CTR_SIZE (what mean_count averages) IS the
        counter and local_step advances.  Without (occupancy_frozen()): a fresh counter; the ring and local_step stay.
        static: the counter of an `into=` march, whose address a captured graph holds.  The march counts into IT and the caller
        copies it into the step's slot afterwards, the one difference: `slot` is that slot, None in every other case."""
        slot = None
        if self.update_occ:
            slot = self.step_counter[self.local_step % STEP_CTR_SIZE]
            self.local_step += 1
        if static is None and slot is None:
            return torch.zeros(2, dtype=torch.int32, device=self.device), None
        counter = slot if static is None else static
        counter.zero_()
        return counter, (None if static is None else slot)

    def _set_last(self, counter, capacity=None):
        """(device-side counter, sample capacity) of the last training render; a graph replay hands in its captured counter alone"""
        self._last_counter = counter
        self._last_capacity = self._last_capacity if capacity is None else capacity

    def _march(self, rays: RayBatch, into: Optional[dict] = None, step: bool = True) -> dict:
        """march_train; step=False (render_test): a counter of the call's own, no bookkeeping, nothing for last_call_overflowed()"""
        cfg = self.cfg
        if into is None:
            nears, fars = raymarching.near_far_from_aabb(rays.origins, rays.dirs, self.aabb, cfg.min_near)
            N = rays.origins.shape[0]
            M = self.sample_capacity(N)
            want_dirs, out = self.model.use_dir, None
        else:
            N, M = into['N'], into['M']
            assert rays.origins.shape[0] == N
            nears, fars = raymarching.near_far_from_aabb_into(rays.origins, rays.dirs, self.aabb, cfg.min_near,
                                                              into['nears'], into['fars'])
            want_dirs = into.get('dirs') is not None          # a view-dependent model: the samples' directions, a static buffer too
            out = (into['xyzs'], into['deltas'], into['rays_info']) + ((into['dirs'],) if want_dirs else ())
        if step:
            counter, slot = self._call_counter(None if into is None else into['counter'])
            self._set_last(counter, M)
        else:
            counter, slot = torch.zeros(2, dtype=torch.int32, device=self.device), None
        xyzs, dirs, deltas, rays_info = raymarching.march_rays_train_nosync(
            rays.origins, rays.dirs, self.bound, self.march_bitfield, self.cascade, cfg.grid_size, nears, fars,
            M, counter, 0., cfg.max_steps, want_dirs=want_dirs, out=out)
        if slot is not None:
            slot.copy_(counter)          # the static counter of an `into=` march, published to the count ring (_call_counter)
        if into is not None:
            return into
        return {'N': N, 'M': M, 'nears': nears, 'fars': fars, 'counter': counter, 'xyzs': xyzs, 'deltas': deltas,
                'rays_info': rays_info, 'dirs': dirs}

    def march_train(self, rays: RayBatch, into: Optional[dict] = None) -> dict:
        """near/far + occupancy-grid march + compaction: capacity-sized sample buffers, device-side counts.
        into: the dict a previous call returned -- its tensors are written in place (static buffers of a captured step).
        With `pose_gradients` and rays that require grad, 'xyzs' is the marched buffer attached to (origins, dirs)."""
        if not self._pose_grad_wanted(rays.origins, rays.dirs):
            return self._march(rays, into)
        if into is not None:
            raise NotImplementedError('pose_gradients: a march into static buffers (into=) keeps no graph from the samples to the rays')
        mt = self._march(rays)
        mt['xyzs'] = raymarching.sample_positions(rays.origins, rays.dirs, mt['xyzs'], mt['deltas'], mt['rays_info'], mt['nears'], mt['M'])
        return mt

    def shade_train(self, mt: dict, perm=None, geometry: Optional[dict] = None):
        """fused field on the marched samples + train composite with the epilogue of renderer.py:225-233 folded in
        (nsr_render_train_forward / _backward): two autograd nodes, no torch glue between them.
        geometry: with `geometry_terms` set, a dict that receives 'depth' [N] (the depth returned here, but differentiable) and
        'distortion' [N] from a third node on the same sigmas (raymarching.ray_geometry); autograd adds its d/d sigmas to the
        composite's.  Left alone with the switch off."""
        extra = {'pos_grad': True} if self._pose_grad_wanted(mt['xyzs']) else {}
        sigmas, rgbs = self.model.field(mt['xyzs'], sigma_only=False, m_dev=mt['counter'], density_scale=self.cfg.density_scale,
                                        perm=perm, dirs=mt.get('dirs'), **extra)
        image, depth, classes, _ = _render_train(sigmas, rgbs, mt['deltas'], mt['rays_info'], mt['nears'], mt['fars'],
                                                 self.cfg.t_thresh)
        if geometry is not None and self.geometry_terms:
            geometry['depth'], geometry['distortion'] = raymarching.ray_geometry(
                sigmas, mt['deltas'], mt['rays_info'], mt['nears'], mt['fars'], self.cfg.t_thresh, False, zero_unowned=False)
        return image, depth, classes

    @torch.no_grad()
    def render_normals(self, rays: RayBatch) -> Dict[str, torch.Tensor]:
        """Geometry of the reconstruction: {'normal_map' [N,3], 'weights_sum' [N], 'depth' [N]}.  The buffered march of
        render_train (so NDC scenes are allowed), the analytic unit normal -grad sigma / |grad sigma| of every sample
        (StyleTCNerf.density_gradient) and the training composite with the normals as a 3-channel colour.
        normal_map = sum_i w_i n_i is NOT renormalised: its length is at most weights_sum, and shorter where the normals
        along a ray disagree; rays that miss the box get zeros.  depth is render_train's.  No occupancy bookkeeping: no
        update_state, and local_step and the step-counter ring stay as they are."""
        keep = (self._last_counter, self._last_capacity)
        with self.occupancy_frozen():                # march_train then counts into a counter of its own
            mt = self.march_train(rays)
        self._set_last(*keep)
        sigmas, normals = self.model.density_gradient(mt['xyzs'], m_dev=mt['counter'], density_scale=self.cfg.density_scale,
                                                      normalize=True)
        # the normals as a 3-channel colour; the composite's white-background image is unused
        weights_sum, _, normal_map, _, depth, _ = _render_train_forward(sigmas, normals, mt['deltas'], mt['rays_info'], mt['nears'],
                                                                        mt['fars'], self.cfg.t_thresh)
        return {'normal_map': normal_map, 'weights_sum': weights_sum, 'depth': depth}

    def extract_mesh(self, resolution=256, iso: float = 10.0, aabb=None, colors: bool = True, normals: bool = True,
                     labels: bool = True, min_faces: int = 0, min_diagonal: float = 0.0, keep_largest=None):
        """The scene's geometry as a triangle mesh (nerfstyle_amd.mesh.Mesh; `.save_ply(path)` writes it): the iso-surface
        sigma = iso of the density on a lattice of `resolution` points an axis (an int or a triple, at most 1024) over `aabb`
        ([x0,y0,z0,x1,y1,z1]; default: the model's box), by surface nets on the device.  sigma includes cfg.density_scale, as
        every render sees it; iso = 10 is torch-ngp's default.  Per vertex, each from one fused launch over the vertices:
          normals  the unit normal of model.density_gradient(verts, normalize=True), pointing out of the dense side like the
                   faces' right-hand normals
          colors   uint8, round to nearest of the sigmoid RGB of model.field(verts)
          labels   int32, the argmax of the same call's class channels -- the region a stylisation would paint the vertex with
                   (None for a model without class channels)
        A switch that is off returns None there and launches nothing for it.  A view_dependent model has no colour without a
        direction: its vertices are shaded with dirs = -normal, the surface seen head-on from outside.
        min_faces, min_diagonal, keep_largest: mesh cleaning (mesh.filter_components).  A connected component of the mesh stays
        iff it has at least min_faces triangles, its box's diagonal is at least min_diagonal (world units) and, with
        keep_largest = k, it is among the k components of the most triangles that passed; the floaters of a density trained on
        few views go this way.  The filter runs on the device between the extractor and the per-vertex launches, so dropped
        vertices are never shaded.  With the defaults none of it is called.
        No occupancy bookkeeping, no gradients.  Reads its counts on the host: not legal while a graph is captured."""
        from .mesh import extract_mesh
        return extract_mesh(self, resolution=resolution, iso=iso, aabb=aabb, colors=colors, normals=normals, labels=labels,
                            min_faces=min_faces, min_diagonal=min_diagonal, keep_largest=keep_largest)

    def _use_spatial_order(self, n_rays: int, dense: bool) -> bool:
        if self.model._spatial_scatter_unsupported:
            return False                 # learnt from a backward that fell back (style_nerf._field.backward)
        if self.sort_samples != 'auto':
            return bool(self.sort_samples)
        return n_rays >= self.sort_min_rays or (dense and n_rays >= self.sort_min_dense_rays)

    def last_call_overflowed(self) -> torch.Tensor:
        """Device-side flag (0-dim bool tensor, no host sync) of the last render_train call: the march emitted
        at least `capacity` samples, so the rays at the end of the batch were dropped exactly like the reference's
        mean_count path does (raymarching.cu:517).  Their in-buffer samples are zero-filled and carry zero gradient."""
        return self._last_counter[0] >= self._last_capacity

    # ---- inference render ----------------------------------------------------------------------
    @torch.no_grad()
    def render_test(self, rays: RayBatch, **kwargs):
        """renderer.py:237-293.  By default ONE march + ONE fused field launch + ONE composite with the
        inference kernel's arithmetic (nsr_composite_rays_infer) instead of up to max_steps host
        iterations; `self.reference_inference_loop = True` selects the reference's loop structure
        (render_test_loop), which the tests hold equal to this path."""
        if self.reference_inference_loop:
            return self.render_test_loop(rays, **kwargs)
        if self.fused_inference:
            return self.render_test_fused(rays, **kwargs)
        return self._infer_epilogue(*self._render_test_buffered(rays))

    def _render_test_buffered(self, rays: RayBatch):
        """render_test's buffered path up to its epilogue -> (image [N,C], weights_sum [N], depth [N], nears, fars) as composited"""
        from . import _lib as L
        mt = self._march(rays, step=False)
        N, M, counter, nears = mt['N'], mt['M'], mt['counter'], mt['nears']
        if self.samples_per_ray_cap is not None and self.samples_per_ray_cap < self.cfg.max_steps:
            # a bounded buffer can overflow, and the march then DROPS the rays that do not fit (raymarching.cu:517);
            # the reference's inference loop never drops a ray, so fall back to its iteration structure.  One host read
            # per frame (the reference reads the alive count every iteration); never taken with the default capacity.
            self.last_test_overflow = int(counter[0].item()) >= M
            if self.last_test_overflow:
                return self._render_test_loop(rays)
        sigmas, rgbs = self.model.field(mt['xyzs'], sigma_only=False, m_dev=counter, density_scale=self.cfg.density_scale,
                                        dirs=mt['dirs'])
        C = self.raymarch_channels
        weights_sum = torch.empty(N, dtype=torch.float32, device=self.device)
        depth = torch.empty(N, dtype=torch.float32, device=self.device)
        image = torch.empty(N, C, dtype=torch.float32, device=self.device)
        L.check(L.lib().nsr_composite_rays_infer(L.p(sigmas), L.p(rgbs), L.p(mt['deltas']), L.p(mt['rays_info']), L.p(nears), M, N,
                                                 C, float(self.cfg.t_thresh), L.p(weights_sum), L.p(depth), L.p(image),
                                                 L.stream()), 'composite_rays_infer')
        return image, weights_sum, depth, nears, mt['fars']

    @staticmethod
    def _infer_epilogue(image, weights_sum, depth, nears, fars):
        """renderer.py:287-293 for the three inference paths: class slice, white background, depth normalisation"""
        classes = image[:, 3:]
        image = image[:, :3] + (1 - weights_sum).unsqueeze(-1)
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return image, depth, classes

    def _render_stream(self, rays: RayBatch, dense_shape, train: bool):
        """What render_test_fused and render_train_fused share: near/far, tile order, outputs and the one launch.  train: the training
        composite, its epilogue outputs, the counts go to this step's counter; else the launch is nsr_render_rays_infer's.
        -> ((image, weights_sum, depth, nears, fars) as composited, (rgb_map, depth, classes) of the epilogue | Nones, stats)"""
        import ctypes
        from . import _lib as L
        nears, fars = raymarching.near_far_from_aabb(rays.origins, rays.dirs, self.aabb, self.cfg.min_near)
        N, dev, C = rays.origins.shape[0], rays.origins.device, self.raymarch_channels
        assert C == self.model.out_channels, 'the fused kernel composites the 3 + num_classes channels of the model'
        order = self._tile_order(dense_shape, N, dev)

        def empty(*shape):
            return torch.empty(*shape, dtype=torch.float32, device=dev)
        stats = self._call_counter()[0] if train else None
        weights_sum, depth, image = empty(N), empty(N), empty(N, C)
        if train:
            epilogue = (empty(N, 3), empty(N), empty(N, C - 3))
        else:
            epilogue, stats = (None, None, None), torch.zeros(2, dtype=torch.int32, device=dev)
        desc = self.model._desc(self.cfg.density_scale)
        L.check(L.lib().nsr_render_rays_stream(
            ctypes.byref(desc), L.p(self.model._gather_tables()), L.p(self.model._mlp_flat()), L.p(rays.origins), L.p(rays.dirs),
            L.p(order), N, L.p(nears), L.p(fars), L.p(self.march_bitfield), float(self.bound), 0., self.cfg.max_steps, self.cascade,
            self.cfg.grid_size, float(self.cfg.t_thresh), L.NSR_STREAM_TRAIN if train else L.NSR_STREAM_INFER, L.p(weights_sum),
            L.p(depth), L.p(image), L.p(epilogue[0]), L.p(epilogue[1]), L.p(epilogue[2]) if C > 3 else None, None, L.p(stats),
            L.stream()), 'render_rays_stream')
        self._infer_stats = stats
        return (image, weights_sum, depth, nears, fars), epilogue, stats

    @torch.no_grad()
    def render_test_fused(self, rays: RayBatch, dense_shape=None, **kwargs):
        """renderer.py:237-293 as ONE launch (nsr_render_rays_infer): the march, the fused field and render_test's composite
        in one kernel that keeps the ray state in registers.  Same samples, same order and same arithmetic as render_test,
        but nothing here is sized by samples -- no capacity, so no dropped ray and no overflow fallback, no host read -- and
        a ray that stopped early costs nothing further.  dense_shape = (w, h): the rays are the row-major pixels of a
        w x h window, walked in 8 x 8 tiles so that the 16 rays a wave holds are neighbours; anything else in batch order."""
        if self.model.use_dir:
            raise NotImplementedError('fused_inference: the streaming kernel has no direction input (view_dependent model)')
        if self.cfg.use_ndc:
            raise NotImplementedError('render_test_fused: NDC scenes march through render_test / render_test_loop')
        return self._infer_epilogue(*self._render_stream(rays, dense_shape, train=False)[0])

    def _tile_order(self, dense_shape, N, dev):
        """The cached 8 x 8-tile work list of a w x h window (None when the rays are not such a window)."""
        if dense_shape is None or dense_shape[0] * dense_shape[1] != N:
            return None
        key = (int(dense_shape[0]), int(dense_shape[1]), str(dev))
        order = self._tile_orders.get(key)
        if order is None:
            order = self._tile_orders[key] = tile_order(key[0], key[1]).to(torch.int32).to(dev)
        return order

    @torch.no_grad()
    def render_train_fused(self, rays: RayBatch, dense_shape=None):
        """render_train without autograd as ONE launch (nsr_render_rays_stream, NSR_STREAM_TRAIN): the march, the fused field,
        the TRAINING composite (running product, stop test after the sample, depth parameter from 0) and the epilogue of
        renderer.py:229-233 in the streaming kernel -> (image [N,3], depth [N], classes [N,nc]) as the kernel wrote them.
        Memory is proportional to the rays: no sample buffer, no capacity, and therefore the one difference from render_train:
        that path zeroes the rays whose samples do not fit its buffer (last_call_overflowed), this one never drops a ray.
        The occupancy bookkeeping is render_train's (update_state when due, local_step, the step-counter ring), except that
        the ring slot receives (samples SHADED, N): what lies behind the point where a ray stopped is not counted, where the
        march of render_train counts every emitted sample.  dense_shape: as for render_test_fused."""
        if self.model.use_dir:
            raise NotImplementedError('fused_nograd_train: the streaming kernel has no direction input (view_dependent model)')
        if self.cfg.use_ndc:
            raise NotImplementedError('render_train_fused: NDC scenes render through the buffered render_train')
        if self.occupancy_update_due():
            self.update_state()
        _, out, stats = self._render_stream(rays, dense_shape, train=True)
        self._set_last(stats, rays.origins.shape[0] * self.cfg.max_steps + 1)   # nothing is ever dropped: last_call_overflowed() answers False
        return out

    def last_infer_stats(self) -> Optional[torch.Tensor]:
        """Device tensor int32 [2] of the last render_test_fused / render_train_fused call -- (samples shaded, rays finished)
        -- without a synchronisation; None before the first call."""
        return self._infer_stats

    @torch.no_grad()
    def render_test_loop(self, rays: RayBatch, **kwargs):
        """renderer.py:237-293.  Same iteration structure (n_step = max(min(N // n_alive, 8), 1));
        alive-ray compaction is a device scan instead of boolean-mask indexing."""
        return self._infer_epilogue(*self._render_test_loop(rays))

    def _render_test_loop(self, rays: RayBatch):
        """render_test_loop up to its epilogue -> what _render_test_buffered returns"""
        nears, fars = raymarching.near_far_from_aabb(rays.origins, rays.dirs, self.aabb, self.cfg.min_near)
        N = len(rays)
        dev = self.device
        weights_sum = torch.zeros(N, dtype=torch.float32, device=dev)
        depth = torch.zeros(N, dtype=torch.float32, device=dev)
        image = torch.zeros(N, self.raymarch_channels, dtype=torch.float32, device=dev)
        n_alive = N
        rays_alive = torch.arange(n_alive, dtype=torch.int32, device=dev)
        rays_alive_next = torch.empty_like(rays_alive)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        rays_t = nears.clone()[:, None].contiguous()
        step = 0
        while step < self.cfg.max_steps:
            if n_alive <= 0:
                break
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = raymarching.march_rays(
                n_alive, n_step, rays_alive, rays_t, rays.origins, rays.dirs, None, self.bound, self.march_bitfield,
                self.cascade, self.cfg.grid_size, nears, fars, 128, False, 0., self.cfg.max_steps, self.cfg.use_ndc)
            sigmas, rgbs = self.model.field(xyzs, sigma_only=False, density_scale=self.cfg.density_scale,
                                            dirs=dirs if self.model.use_dir else None)
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, self.cfg.use_ndc,
                                       weights_sum, depth, image, self.cfg.t_thresh)
            raymarching.compact_alive(rays_alive, n_alive, rays_alive_next, n_out)
            rays_alive, rays_alive_next = rays_alive_next, rays_alive
            n_alive = int(n_out.item())
            step += n_step
        return image, weights_sum, depth, nears, fars

    # ---- a training render in two halves (data-parallel overlap, parallel.py) ---------------------------------------
    def occupancy_update_due(self) -> bool:
        """The next training render starts with update_state (renderer.py:206-207): it reads the parameters."""
        return bool(self.update_occ and (self.local_step % self.cfg.update_iter == 0))

    def begin_train(self, pose, pix_subset, dense: bool = False, into: Optional[dict] = None) -> dict:
        """First half of render(pose, training=True, pix_subset=...): ray generation, [occupancy update when due,] occupancy
        march + compaction and the spatial order of the samples.  Apart from the occupancy update none of it reads the
        PARAMETERS (the march reads the bitfield only), so a data-parallel step may issue it for step i+1 while the gradient
        all-reduce of step i is in flight and the optimiser has not stepped yet -- as long as occupancy_update_due() is
        False.  finish_train(ctx) does the rest."""
        pose_grad = self._pose_grad_wanted(pose)
        rays, _ = generate_rays(pose, self.intr, None, camera_flip=self.cfg.flip_camera, pix_subset=pix_subset, device=self.device,
                                pose_grad=pose_grad)
        if self.occupancy_update_due():
            self.update_state()
        # into: the ctx a previous call returned; every tensor of it is rewritten in place (graph.GraphedRenderStep(prefetch=True))
        mt = self.march_train(rays, into=into['mt'] if into is not None else None)
        perm = None
        if torch.is_grad_enabled() and (pose_grad or self._use_spatial_order(mt['N'], dense)):
            perm = self.model.sample_order(mt['xyzs'], mt['counter'], out=into['perm'] if into is not None else None)
        if into is not None:
            assert (perm is None) == (into['perm'] is None)
            return into
        return {'mt': mt, 'perm': perm}

    def begin_train_on(self, stream, pose, pix_subset, dense: bool = False, after=None, into: Optional[dict] = None) -> dict:
        """begin_train issued on `stream` (a side stream) so that it runs BESIDE whatever the current stream is doing -- the
        previous step's backward: its table scatter waits on the memory-side atomic unit with most of its issue slots idle, and
        the march / sort kernels fit next to it.  finish_train(ctx) makes the current stream wait for it.  Only legal when no
        occupancy update is due (occupancy_update_due(): that one reads the parameters).  after: an event the side stream waits
        for first (the producer of `pose` / `pix_subset`, the last occupancy update, the last reader of `into`).
        into: the ctx of an earlier call whose tensors are rewritten in place -- a training loop alternates between two of them
        and allocates nothing per step.  Without it the tensors are allocated by the side stream and consumed -- and released
        -- by the current one: they are marked for the caching allocator accordingly (which then keeps two pools of
        capacity-sized buffers busy; prefer `into`)."""
        assert not self.occupancy_update_due(), 'an occupancy update reads the parameters: march on the training stream'
        cur = torch.cuda.current_stream(self.device)
        if after is not None:
            stream.wait_event(after)
        with torch.cuda.stream(stream):
            ctx = self.begin_train(pose, pix_subset, dense, into=into)
        if into is None:
            for t in list(ctx['mt'].values()) + [ctx['perm']]:
                if torch.is_tensor(t):
                    t.record_stream(cur)
        ctx['stream'] = stream
        return ctx

    def finish_train(self, ctx: dict) -> Dict[str, torch.Tensor]:
        """Second half: fused field + composite + epilogue on the samples begin_train marched (reads the parameters)."""
        if ctx.get('stream') is not None:
            torch.cuda.current_stream(self.device).wait_stream(ctx['stream'])
        out = {'target': None}
        geometry = {} if self.geometry_terms else None
        out['rgb_map'], out['trans_map'], out['classes'] = self.shade_train(ctx['mt'], ctx['perm'], geometry=geometry)
        out.update(geometry or {})
        self._set_last(ctx['mt']['counter'], ctx['mt']['M'])
        return out

    def render(self, pose, image=None, patch: Optional[Box2D] = None, num_rays: Optional[int] = None,
               training: bool = False, pix_subset=None, dense: Optional[bool] = None, lens=None) -> Dict[str, torch.Tensor]:
        """renderer.py:295-313.  `dense` overrides the guess below for callers that pass a patch as `pix_subset`.
        lens ([6], LensRefiner.forward()): the rays go through that lens instead of the fixed intrinsics; in a training render it
        is a camera tensor like the pose (`pose_gradients`, the same refusals), a test render uses it without a gradient."""
        output = {}
        precrop_frac = self.precrop_frac if self._use_precrop else 1.
        self._refuse_lens(lens)
        rays, output['target'] = generate_rays(pose, self.intr, image, patch=patch, precrop=precrop_frac, bsize=num_rays,
                                               camera_flip=self.cfg.flip_camera, pix_subset=pix_subset, device=self.device,
                                               pose_grad=training and self._pose_grad_wanted(pose, lens), lens=lens)
        render_fn = self.render_train if training else self.render_test
        # a full frame, a patch or a centre crop is a dense pixel set: neighbouring rays share hash-table rows
        if dense is None:
            dense = pix_subset is None and num_rays is None
        extra = {}
        fused = (self.fused_nograd_train and not torch.is_grad_enabled() and not self.geometry_terms) if training else self.fused_inference
        if fused and dense and pix_subset is None and num_rays is None:
            extra['dense_shape'] = pixel_window(self.intr, patch, precrop_frac)[:2]
        geometry = {} if training and self.geometry_terms else None
        if geometry is not None:
            extra['geometry'] = geometry
        output['rgb_map'], output['trans_map'], output['classes'] = render_fn(rays, dense=dense, **extra)
        output.update(geometry or {})
        return output

    # ---- metric depth and view consistency (nerfstyle_amd/consistency.py) ---------------------------------------------
    @torch.no_grad()
    def render_rgbd(self, pose, min_opacity: float = 0.5) -> Dict[str, torch.Tensor]:
        """A no-grad inference render of the whole frame that also hands out the metric depth, which render() normalises away.
        -> 'rgb_map', 'trans_map', 'classes': those of render(pose), bit for bit (the same launches on render_test's buffered path,
        or on the reference loop with `reference_inference_loop`); 'weights_sum' [N]; 'distance' [N]: the composite's raw depth
        divided by weights_sum where weights_sum >= min_opacity, else 0, the "no surface" value of reproject_frames; 'nears',
        'fars' [N].
        What the raw depth is (csrc/raymarch_infer.hip, k_composite_infer and the loop's composite): sum_i w_i t_i over the ray's
        shaded samples, where t_i starts at the ray's near and advances by the march's second delta column, t_next - last_t, so
        t_i is the ray parameter at the FAR end of sample i's step (one step past the position the field was asked at, and for
        the last sample before `far` possibly a step beyond it).  The rays are unit vectors (ray generation normalises them), so a
        parameter is a distance from the camera origin, and depth / weights_sum is the weight-averaged distance of the ray's
        surface: the `dist` of include/nsr.h, "View reprojection".
        Refuses use_ndc (an NDC depth is not a distance) and fused_inference (the streaming kernel is not what this method
        launches; switch it off for the call).  No lens argument: the reprojection is a pinhole's."""
        if self.cfg.use_ndc:
            raise NotImplementedError('render_rgbd: use_ndc: the depth of an NDC march is not a distance along the ray')
        if self.fused_inference and not self.reference_inference_loop:
            raise NotImplementedError('render_rgbd: fused_inference: the metric depth comes from the buffered render_test path; switch '
                                      'fused_inference off for this call')
        precrop_frac = self.precrop_frac if self._use_precrop else 1.
        rays, _ = generate_rays(pose, self.intr, None, precrop=precrop_frac, camera_flip=self.cfg.flip_camera, device=self.device)
        raw = self._render_test_loop(rays) if self.reference_inference_loop else self._render_test_buffered(rays)
        _, weights_sum, depth, nears, fars = raw
        out = {'target': None}
        out['rgb_map'], out['trans_map'], out['classes'] = self._infer_epilogue(*raw)
        out['weights_sum'] = weights_sum
        out['distance'] = torch.where(weights_sum >= min_opacity, depth / weights_sum, torch.zeros_like(depth))
        out['nears'], out['fars'] = nears, fars
        return out

    @torch.no_grad()
    def view_consistency(self, poses, gaps=(1, 7), depth_tol: float = 0.01, min_opacity: float = 0.5, frames=None):
        """The warped error between views of this field: every pose of `poses` ([F,3,4] or [F,4,4]) is rendered with render_rgbd, the frames
        and their distance maps stay on the device, and for every gap g each frame i + g is reprojected into frame i
        (consistency.reproject_frames over sequence_pairs(F, g): one call per gap, metric only, neither warped frames nor masks
        written) -> {g: [F - g, 2] float64 (rmse, coverage)} on the device (consistency.warp_error), no host read.  gap 1 is the
        short-range protocol, a larger gap the long-range one; a gap >= F yields an empty tensor.
        frames = (rgb [F,H*W,3] or [F,H,W,3], dist [F,H*W] or [F,H,W]): score images stylised elsewhere against this field's
        geometry (dist None: the distance maps are rendered here, the images are the caller's); nothing is rendered when both
        are given."""
        from . import consistency
        poses = torch.as_tensor(poses, dtype=torch.float32, device=self.device)
        if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError('view_consistency: poses must be [F, 3, 4] or [F, 4, 4]; got {}'.format(tuple(poses.shape)))
        poses = poses[:, :3].contiguous()                  # the cameras of scene.py are homogeneous 4 x 4
        F = int(poses.shape[0])
        rgb, dist = frames if frames is not None else (None, None)
        if rgb is None or dist is None:
            if self._use_precrop and self.precrop_frac < 1.:
                raise NotImplementedError('view_consistency: the centre crop (use_precrop) renders only part of the frame')
            outs = [self.render_rgbd(poses[i], min_opacity=min_opacity) for i in range(F)]
            if dist is None:
                dist = torch.stack([o['distance'] for o in outs])
            if rgb is None:
                rgb = torch.stack([o['rgb_map'] for o in outs])
        result = {}
        for gap in gaps:
            pairs = consistency.sequence_pairs(F, gap)
            _, _, stats = consistency.reproject_frames(rgb, dist, poses, self.intr, pairs, camera_flip=self.cfg.flip_camera,
                                                       depth_tol=depth_tol, want_warped=False, want_mask=False)
            result[int(gap)] = consistency.warp_error(stats, self.intr.h, self.intr.w)
        return result

    def _refuse_lens(self, lens):
        if lens is not None and self.cfg.use_ndc:
            raise NotImplementedError('lens: use_ndc: the NDC warp reads the focal length of the fixed intrinsics, not the lens')

    def render_frames(self, poses, batch, training: bool = True, lens=None) -> Dict[str, torch.Tensor]:
        """A training render of a mixed-frame batch: poses [F,3,4] (PoseRefiner.forward_all(), or the dataset's), batch =
        ResidentDataset.draw(...) (seg_frame, pix, rows, S, K): ray n is pixel pix[n] of frame seg_frame[n // K].  The output
        dict of render(); 'target' is None -- the caller has batch.rows for recon_loss(..., pix=batch.rows).  From the rays on
        it IS render_train: occupancy updates, geometry_terms, the sample order and, with `pose_gradients` and poses that
        require grad, the camera gradient (one row of poses.grad per frame, zeros for frames outside the batch) with every
        refusal of the single-pose path.  Training only; begin_train / GraphedRenderStep have no mixed-frame form.
        lens ([6], LensRefiner.forward()): one lens for all frames, a camera tensor like the poses; lens.grad arrives with
        poses.grad from one backward launch sequence."""
        if not training:
            raise NotImplementedError('render_frames is a training render: an image has one pose, use render(pose)')
        self._refuse_lens(lens)
        rays = generate_rays_frames(poses, batch.seg_frame, batch.pix, batch.K, self.intr, camera_flip=self.cfg.flip_camera,
                                    pose_grad=self._pose_grad_wanted(poses, lens), lens=lens)
        output = {'target': None}
        geometry = {} if self.geometry_terms else None
        extra = {} if geometry is None else {'geometry': geometry}
        output['rgb_map'], output['trans_map'], output['classes'] = self.render_train(rays, dense=False, **extra)
        output.update(geometry or {})
        return output


def _render_train_forward(sigmas, rgbs, deltas, rays, nears, fars, T_thresh):
    """nsr_render_train_forward and its six outputs -> (weights_sum [N], depth_raw [N], image [N,C], rgb_map [N,3], depth [N],
    classes [N,C-3]): the training composite of C colour channels with the epilogue of renderer.py:229-233 folded in."""
    from . import _lib as L
    M, N, C = sigmas.shape[0], rays.shape[0], rgbs.shape[1]
    dev = sigmas.device
    weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
    depth_raw = torch.empty(N, dtype=torch.float32, device=dev)
    image = torch.empty(N, C, dtype=torch.float32, device=dev)
    rgb_map = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    classes = torch.empty(N, C - 3, dtype=torch.float32, device=dev)
    L.check(L.lib().nsr_render_train_forward(
        L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rays), L.p(nears), L.p(fars), M, N, C, float(T_thresh), L.p(weights_sum),
        L.p(depth_raw), L.p(image), L.p(rgb_map), L.p(depth), L.p(classes) if C > 3 else None, L.stream()), 'render_train_forward')
    return weights_sum, depth_raw, image, rgb_map, depth, classes


class _render_train_fn(torch.autograd.Function):
    """composite_rays_train (raymarching.cu:806-997) + `image[:, :3] + (1 - weights_sum)`, the class slice and the depth
    normalisation (renderer.py:229-233) as ONE kernel each way, over capacity-sized sample buffers.  Outputs
    (rgb_map [N,3], depth [N], classes [N,nc], weights_sum [N]); gradients are produced with torch.empty (the backward kernel
    writes every sample that belongs to a ray, zeros included)."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, deltas, rays, nears, fars, T_thresh):
        ctx.set_materialize_grads(False)     # outputs the loss does not use arrive as None, not as zero tensors (two fills a step)
        from . import profiling
        with profiling.timed('composite_fwd'):
            weights_sum, _, image, rgb_map, depth, classes = _render_train_forward(sigmas, rgbs, deltas, rays, nears, fars, T_thresh)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, image)
        ctx.T_thresh = T_thresh
        ctx.mark_non_differentiable(depth)
        return rgb_map, depth, classes, weights_sum

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_classes, g_ws):
        from . import _lib as L
        from . import profiling
        sigmas, rgbs, deltas, rays, weights_sum, image = ctx.saved_tensors
        M, N, C = sigmas.shape[0], rays.shape[0], rgbs.shape[1]

        def prep(g):
            return None if g is None else g.to(torch.float32).contiguous()
        g_rgb, g_classes, g_ws = prep(g_rgb), prep(g_classes), prep(g_ws)
        if C == 3:
            g_classes = None
        grad_sigmas = torch.empty_like(sigmas)
        grad_rgbs = torch.empty_like(rgbs)
        with profiling.timed('composite_bwd'):
            L.check(L.lib().nsr_render_train_backward(
                L.p(g_rgb), L.p(g_classes), L.p(g_ws), L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rays), L.p(weights_sum), L.p(image),
                M, N, C, float(ctx.T_thresh), L.p(grad_sigmas), L.p(grad_rgbs), L.stream()), 'render_train_backward')
        return grad_sigmas, grad_rgbs, None, None, None, None, None


_render_train = _render_train_fn.apply
