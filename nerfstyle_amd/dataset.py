"""HBM-resident training targets.

The reference's `generate_rays` slices a host NumPy image per step and copies the picked pixels to the
device (`nerf_lib.py:126-141`).  Here every frame's per-pixel target row -- RGB plus the segment id, the
4-channel layout `generate_rays` hands to `calc_loss` (`trainers/base.py:266-269`) -- and every pose live in
HBM for the whole run (35 frames at 1008x756 are 427 MB of the 288 GB), so a step gathers its targets with
one device index op.

File parsing (transforms JSON, PNG decode, segment .npz) is the caller's: `data/` is outside the hot path
 and is not rebuilt here.  `ResidentDataset` takes the decoded arrays."""
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from .common import BBox, Intrinsics


# a drawn mixed-frame batch: seg_frame [S] int32, pix [S*K] int32, rows [S*K] int64 (rows of target_rgb_rows / target_cls_rows)
FrameBatch = namedtuple('FrameBatch', ('seg_frame', 'pix', 'rows', 'S', 'K'))


class ResidentDataset:
    """targets [N, H*W, C] (C = 3, or 4 with the segment id as float like the reference's 4th plane,
    base_dataset.py:140-148) and poses [N,4,4], both on `device`."""

    def __init__(self, images: np.ndarray, poses: np.ndarray, intr: Intrinsics, bound: float, device,
                 seg_maps: Optional[np.ndarray] = None, num_classes: int = 0):
        images = np.asarray(images, np.float32)
        poses = np.asarray(poses, np.float32)
        n, c, h, w = images.shape
        if c != 3:
            raise ValueError('images must be [N,3,H,W] (alpha already composited)')
        if (h, w) != (intr.h, intr.w):
            raise ValueError('images are {}x{}, intrinsics say {}x{}'.format(w, h, intr.w, intr.h))
        if poses.shape != (n, 4, 4):
            raise ValueError('poses must be [N,4,4]')
        planes = [torch.from_numpy(images).reshape(n, 3, h * w)]
        if seg_maps is not None:
            seg = np.asarray(seg_maps, np.float32)
            if seg.shape != (n, h, w):
                raise ValueError('seg_maps must be [N,H,W]')
            planes.append(torch.from_numpy(seg).reshape(n, 1, h * w))
        # pixel-major rows: one index_select row per ray
        self.targets = torch.cat(planes, dim=1).transpose(1, 2).contiguous().to(device)
        self.poses = torch.from_numpy(poses).to(device)
        self.intr, self.num_classes, self.bound = intr, int(num_classes), bound
        self.bbox = BBox.from_radius(bound)
        self._rgb_rows = self._cls_rows = None
        self.color_tf = None            # [4,4] f32 on the device once match_colors() has run
        self.region_tf = None           # [num_classes+1,4,4] f32 on the device once match_colors_by_region() has run

    def __len__(self):
        return self.poses.shape[0]

    def sample(self, frame: int, pix: torch.Tensor):
        """(pose [4,4], target [len(pix), C]) for pixel ids `pix` (row-major y * w + x) of frame `frame`"""
        return self.poses[frame], self.targets[frame].index_select(0, pix)

    # ---- mixed-frame batches: rays of many frames in one step ------------------------------------------------------------------
    @property
    def target_rgb_rows(self):
        """[F*HW, 3] f32 contiguous: row f * HW + p is pixel p of frame f.  Built once, on first use; with `rows` of a drawn
        batch it is what recon_loss(target_rgb=..., pix=rows) takes."""
        if self._rgb_rows is None:
            self._rgb_rows = self.targets[:, :, :3].reshape(-1, 3).contiguous()
        return self._rgb_rows

    def match_colors(self, style_image: torch.Tensor) -> torch.Tensor:
        """Matches the colours of every frame's targets to `style_image` [3,H,W] f32 in [0,1] (what StyleCriterion.init_style takes;
        any size): the reference's `ct_image` step (data/base_dataset.py:97-105, color_match.py), to be called after the dataset
        is built and before the stylisation stage.  One mean and covariance over all frames' pixels, read from `targets` where it
        lies ([F, H*W, C] rows, no RGB copy); the affine map is applied to `targets` IN PLACE and clamped to [0, 1]; the segment
        channel is not touched, bit for bit.  -> color_tf [4,4] f32 on the device, kept as `self.color_tf`: apply it to rendered
        rgb rows with color_match.apply_color_transform.  The solve reads 18 doubles on the host: set-up, not a training step.

        A `target_rgb_rows` handed out before the call is UPDATED IN PLACE (copied anew from the targets), so whoever holds it
        sees the new colours; target_cls_rows, draw, ErrorMap and sample read what they read before.
        Calling it again matches the current, already matched and clamped, targets to the new image: transforms do not compose
        into `color_tf`, which holds the last one only."""
        from . import color_match as CM
        if style_image.dim() != 3 or style_image.shape[0] != 3:
            raise ValueError('match_colors: style_image must be [3,H,W]; got {}'.format(tuple(style_image.shape)))
        dev = self.targets.device
        style = style_image.detach().to(dev, torch.float32).permute(1, 2, 0).contiguous()
        n = self.targets.shape[0] * self.targets.shape[1]
        self.color_tf = CM.solve_color_transform(CM.color_moments(self.targets), n, CM.color_moments(style), style.numel() // 3)
        CM.apply_color_transform(self.targets, self.color_tf, clamp=True, out=self.targets)
        if self._rgb_rows is not None and self._rgb_rows.data_ptr() != self.targets.data_ptr():       # C == 3: one storage
            self._rgb_rows.copy_(self.targets[:, :, :3].reshape(-1, 3))
        return self.color_tf

    def match_colors_by_region(self, style_image: torch.Tensor, style_clusters, matching, min_rows: int = 256,
                               fallback: str = 'global') -> torch.Tensor:
        """match_colors per scene class: the pixels of class i get the mean and covariance of cluster matching[i] of the style
        image, not the image's average palette.  style_image [3,H,W] f32 in [0,1]; style_clusters [H,W] integer, the cluster of
        each style pixel (-1 = unlabelled), or an int K: the image is clustered first (segment.segment_style_image(style_image, K):
        colour alone, 10 steps), with the same result as passing that map; matching [num_classes] is the caller's (SemanticStyleLoss.matching, or a fixed list;
        -1 = unmatched), it is not computed here.

        The class ids are read from the targets where they lie (the fourth float of every row, no label copy); the style side
        passes its cluster map as explicit labels.  Classes that are unmatched or hold fewer than `min_rows` pixels on either
        side, and pixels of no class, get the fallback ('global': all pixels against the whole style image, what match_colors
        computes; 'identity').  The maps are applied to `targets` IN PLACE and clamped to [0, 1]; the segment channel keeps its
        bits; a `target_rgb_rows` handed out before is refreshed as match_colors does.
        -> region_tf [num_classes+1, 4, 4] f32 on the device, kept as `self.region_tf` (apply it to rendered rows with
        color_match.apply_region_transforms and labels = preds.to(torch.int32)); `self.color_tf` is set to the fallback slot.
        One host read of 10 (num_classes + clusters + 2) doubles: set-up, not a training step."""
        from . import color_match as CM
        if self.targets.shape[2] < 4:
            raise ValueError('match_colors_by_region: the dataset was built without segment maps')
        if style_image.dim() != 3 or style_image.shape[0] != 3:
            raise ValueError('match_colors_by_region: style_image must be [3,H,W]; got {}'.format(tuple(style_image.shape)))
        if isinstance(style_clusters, int) and not isinstance(style_clusters, bool):
            from .segment import segment_style_image
            CM._rows(self.targets, 'match_colors_by_region')
            style_clusters = segment_style_image(style_image, style_clusters, device=self.targets.device).labels
        if tuple(style_clusters.shape) != tuple(style_image.shape[1:]) or style_clusters.is_floating_point():
            raise ValueError('match_colors_by_region: style_clusters must be integer [H,W] of the style image {}; got {} {}'.format(
                tuple(style_image.shape[1:]), style_clusters.dtype, tuple(style_clusters.shape)))
        if not 1 <= self.num_classes <= CM.MAX_REGIONS:
            raise ValueError('match_colors_by_region: num_classes must be in 1..{}; got {}'.format(CM.MAX_REGIONS, self.num_classes))
        matching = [int(m) for m in (matching.tolist() if isinstance(matching, torch.Tensor) else matching)]
        if len(matching) != self.num_classes:
            raise ValueError('match_colors_by_region: matching has {} entries for {} classes'.format(len(matching), self.num_classes))
        dev = self.targets.device
        ks = max(int(style_clusters.max()) + 1, max(matching) + 1, 1)
        if ks > CM.MAX_REGIONS:
            raise ValueError('match_colors_by_region: {} style clusters; at most {}'.format(ks, CM.MAX_REGIONS))
        CM._rows(self.targets, 'match_colors_by_region')                  # a CPU dataset is refused before anything is moved
        style = style_image.detach().to(dev, torch.float32).permute(1, 2, 0).contiguous()
        clusters = style_clusters.detach().to(dev, torch.int32).contiguous().reshape(-1)
        content_m = CM.region_moments(self.targets, self.num_classes)
        style_m = CM.region_moments(style, ks, clusters)
        self.region_tf = CM.solve_region_transforms(content_m, style_m, matching, min_rows=min_rows, fallback=fallback)
        self.color_tf = self.region_tf[self.num_classes]
        CM.apply_region_transforms(self.targets, self.region_tf, clamp=True, out=self.targets)
        if self._rgb_rows is not None:
            self._rgb_rows.copy_(self.targets[:, :, :3].reshape(-1, 3))
        return self.region_tf

    @property
    def target_cls_rows(self):
        """[F*HW] int64 segment ids, row order of target_rgb_rows; only when segment maps were given"""
        if self.targets.shape[2] < 4:
            raise AttributeError('target_cls_rows: the dataset was built without segment maps')
        if self._cls_rows is None:
            self._cls_rows = self.targets[:, :, 3].reshape(-1).to(torch.int64).contiguous()
        return self._cls_rows

    def draw(self, S: int, K: int, seed: int, sequence: int = 0, sequence_dev: Optional[torch.Tensor] = None, stream_id: int = 0,
             frames: Optional[torch.Tensor] = None, advance: bool = False, out: Optional[FrameBatch] = None) -> FrameBatch:
        """A batch of S segments of K rays drawn on the device (nsr_draw_frame_batch): per segment a frame, per ray a pixel of
        it, UNIFORM WITH REPLACEMENT -> FrameBatch(seg_frame, pix, rows, S, K).  Counter-based: (seed, sequence
        [+ sequence_dev[0], a uint32-valued int32 device word], stream_id = the data-parallel rank) name the batch.
        frames [S] int32 on the device: the segments' frames, only the pixels are drawn.  advance: sequence_dev is incremented
        after the draw, so a captured graph draws a fresh batch on every replay.  out: a previous batch of the same S and K,
        rewritten in place (nothing is allocated)."""
        from . import _lib as L
        from . import profiling
        dev = self.targets.device
        n_frames, P = self.targets.shape[0], self.targets.shape[1]
        if out is not None:
            assert (out.S, out.K) == (S, K), 'out: a batch of the same S and K'
            seg_frame, pix, rows = out.seg_frame, out.pix, out.rows
        else:
            seg_frame = torch.empty(S, dtype=torch.int32, device=dev)
            pix = torch.empty(S * K, dtype=torch.int32, device=dev)
            rows = torch.empty(S * K, dtype=torch.int64, device=dev)
        if frames is not None:
            assert frames.dtype == torch.int32 and frames.numel() == S, 'frames [S] int32'
        if sequence_dev is not None:
            assert sequence_dev.dtype == torch.int32 and sequence_dev.numel() >= 1, 'sequence_dev: an int32 device word'
        with profiling.timed('draw_frame_batch'):
            L.check(L.lib().nsr_draw_frame_batch(n_frames, P, S, K, int(seed) & (2 ** 64 - 1), int(sequence) & 0xffffffff,
                                                 L.p(sequence_dev), int(stream_id), L.p(frames), int(bool(advance)), L.p(seg_frame),
                                                 L.p(pix), L.p(rows), L.stream()), 'draw_frame_batch')
        return out if out is not None else FrameBatch(seg_frame, pix, rows, S, K)


class ErrorMap:
    """Error-map importance sampling of training rays (instant-ngp's error map) on top of ResidentDataset.draw.

    Every frame is cut into cell x cell pixel cells (gw = ceil(w / cell), gh = ceil(h / cell), G = gw * gh; the edge cells are
    ragged).  `err` [F,G] f32 is the running mean squared RGB error (summed over the channels) of the rays drawn in a cell,
    `init` at the start.  draw() picks pixels in proportion to it, mixed with `uniform_mix` of the uniform draw so that no pixel
    starves, and returns per ray the weight (uniform pdf) / (pdf of the draw): mean(weight * loss) still estimates the uniform
    mean loss, recon_loss(..., ray_weight=weights) is that mean.  update() folds the step's per-ray errors into the map:
    err += decay * (mean error of the step's rays in the cell - err).

    Determinism: everything that decides a draw is integer arithmetic.  The per-ray errors are accumulated as fixed-point
    integers (`acc_sum` [F,G], `acc_cnt` [F,G], zero between steps), err is quantised to q = min(floor(err * quant_scale), 2^18)
    and the sampling CDF is the 64-bit prefix sum of the masses npix * q (`prefix` [F,G], `frame_prefix` [F]); integer sums do
    not depend on the order atomics arrive in, so runs and ranks agree bit for bit and include/nsr.h states the arithmetic
    precisely enough to restate it.  The 64-bit unsigned state lives in int64 tensors, the 32-bit in int32.
    Data-parallel: torch.distributed.all_reduce(SUM) of acc_sum and acc_cnt between the loss and update() gives every rank the
    map of all ranks' rays, bit-identical on every rank.

    Nothing is read on the host and nothing is allocated with out=: a captured graph replays the loop

        batch, wts = emap.draw(S, K, seed, sequence_dev=seq, advance=True)
        out = renderer.render_frames(poses, batch)
        loss = recon_loss(out['rgb_map'], out['classes'], ds.target_rgb_rows, ds.target_cls_rows, batch.rows,
                          ray_weight=wts, ray_err_out=err_buf)
        loss.backward(); emap.update(batch, err_buf)
    """

    def __init__(self, dataset: ResidentDataset, cell: int = 16, decay: float = 0.05, uniform_mix: float = 0.1, init: float = 1.0,
                 quant_scale: float = 65536.0):
        if cell < 1 or not 0.0 <= decay <= 1.0 or not 0.0 <= uniform_mix <= 1.0 or not quant_scale > 0.0:
            raise ValueError('ErrorMap: cell >= 1, decay and uniform_mix in [0, 1], quant_scale > 0')
        self.cell, self.decay, self.uniform_mix, self.init, self.quant_scale = int(cell), float(decay), float(uniform_mix), float(init), float(quant_scale)
        self.F, self.w, self.h = len(dataset), dataset.intr.w, dataset.intr.h
        self.gw, self.gh = -(-self.w // self.cell), -(-self.h // self.cell)
        self.G, self.P = self.gw * self.gh, self.w * self.h
        dev = dataset.targets.device
        self.err = torch.full((self.F, self.G), self.init, dtype=torch.float32, device=dev)
        self.acc_sum = torch.zeros(self.F, self.G, dtype=torch.int64, device=dev)
        self.acc_cnt = torch.zeros(self.F, self.G, dtype=torch.int32, device=dev)
        self.prefix = torch.zeros(self.F, self.G, dtype=torch.int64, device=dev)
        self.frame_prefix = torch.zeros(self.F, dtype=torch.int64, device=dev)
        self.rebuild()

    def _grid(self):
        return self.F, self.w, self.h, self.cell

    def rebuild(self):
        """Folds the accumulators into err (cells that got rays) and rebuilds prefix and frame_prefix from err: two launches.
        Call it after writing err by hand."""
        from . import _lib as L
        from . import profiling
        with profiling.timed('error_map_rebuild'):
            L.check(L.lib().nsr_error_map_rebuild(*self._grid(), self.decay, self.quant_scale, L.p(self.err), L.p(self.acc_sum),
                                                  L.p(self.acc_cnt), L.p(self.prefix), L.p(self.frame_prefix), L.stream()), 'error_map_rebuild')

    def draw(self, S: int, K: int, seed: int, sequence: int = 0, sequence_dev: Optional[torch.Tensor] = None, stream_id: int = 0,
             frames: Optional[torch.Tensor] = None, frames_by_error: bool = False, advance: bool = False, out=None):
        """ResidentDataset.draw with the pixels drawn from the map -> (FrameBatch, weights [S*K] f32); the arguments of
        ResidentDataset.draw mean what they mean there (nsr_draw_frame_batch_error makes the same Philox calls: uniform_mix = 1
        draws the very batch of ResidentDataset.draw, with weights 1).  frames_by_error: the segments' frames too are drawn in
        proportion to their total error (mixed with the uniform draw likewise), and the weights carry that factor.
        out: a previous (FrameBatch, weights) pair of the same S and K, rewritten in place."""
        from . import _lib as L
        from . import profiling
        dev = self.err.device
        if out is not None:
            batch, weights = out
            assert (batch.S, batch.K) == (S, K), 'out: a batch of the same S and K'
        else:
            batch = FrameBatch(torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S * K, dtype=torch.int32, device=dev),
                               torch.empty(S * K, dtype=torch.int64, device=dev), S, K)
            weights = torch.empty(S * K, dtype=torch.float32, device=dev)
        if frames is not None:
            assert frames.dtype == torch.int32 and frames.numel() == S, 'frames [S] int32'
        if sequence_dev is not None:
            assert sequence_dev.dtype == torch.int32 and sequence_dev.numel() >= 1, 'sequence_dev: an int32 device word'
        assert weights.dtype == torch.float32 and weights.numel() == S * K, 'weights [S*K] float32'
        with profiling.timed('draw_frame_batch_error'):
            L.check(L.lib().nsr_draw_frame_batch_error(*self._grid(), L.p(self.prefix), L.p(self.frame_prefix), self.uniform_mix,
                                                       int(bool(frames_by_error)), S, K, int(seed) & (2 ** 64 - 1),
                                                       int(sequence) & 0xffffffff, L.p(sequence_dev), int(stream_id), L.p(frames),
                                                       int(bool(advance)), L.p(batch.seg_frame), L.p(batch.pix), L.p(batch.rows),
                                                       L.p(weights), L.stream()), 'draw_frame_batch_error')
        return out if out is not None else (batch, weights)

    def accumulate(self, batch: FrameBatch, ray_err: torch.Tensor):
        """Adds the batch's per-ray errors (recon_loss's ray_err_out) to acc_sum / acc_cnt: one launch.  update() without the
        rebuild, for a data-parallel all-reduce of the two tensors in between."""
        from . import _lib as L
        from . import profiling
        assert ray_err.dtype == torch.float32 and ray_err.numel() == batch.S * batch.K, 'ray_err [S*K] float32'
        with profiling.timed('error_map_accumulate'):
            L.check(L.lib().nsr_error_map_accumulate(*self._grid(), L.p(batch.seg_frame), L.p(batch.pix), L.p(ray_err), batch.S, batch.K,
                                                     L.p(self.acc_sum), L.p(self.acc_cnt), L.stream()), 'error_map_accumulate')

    def update(self, batch: FrameBatch, ray_err: torch.Tensor):
        """accumulate() + rebuild(): three launches, no host read."""
        self.accumulate(batch, ray_err)
        self.rebuild()

    def pdf(self, frame: int) -> torch.Tensor:
        """[h, w] float64 on the host: the probability with which draw() picks each pixel of `frame`, given the frame (for
        inspection and tests; it reads the device)."""
        prefix = self.prefix[frame].cpu().numpy().astype(np.uint64)
        mass = np.diff(prefix, prepend=np.uint64(0)).astype(np.float64).reshape(self.gh, self.gw)
        total = float(prefix[-1])
        cw = np.minimum(self.cell, self.w - np.arange(self.gw) * self.cell)
        ch = np.minimum(self.cell, self.h - np.arange(self.gh) * self.cell)
        uniform = np.full((self.h, self.w), 1.0 / self.P)
        if total == 0.0:
            return torch.from_numpy(uniform)
        u = float(np.float32(self.uniform_mix))
        per_pixel = mass / total / (ch[:, None] * cw[None, :])
        ys, xs = np.arange(self.h) // self.cell, np.arange(self.w) // self.cell
        return torch.from_numpy(u * uniform + (1.0 - u) * per_pixel[ys[:, None], xs[None, :]])

    def state_dict(self):
        return {'err': self.err.detach().cpu().clone(), 'cell': self.cell, 'decay': self.decay, 'uniform_mix': self.uniform_mix,
                'init': self.init, 'quant_scale': self.quant_scale}

    def load_state_dict(self, state):
        if int(state['cell']) != self.cell or tuple(state['err'].shape) != (self.F, self.G):
            raise ValueError('ErrorMap.load_state_dict: the map was saved for another grid')
        self.decay, self.uniform_mix = float(state['decay']), float(state['uniform_mix'])
        self.init, self.quant_scale = float(state['init']), float(state['quant_scale'])
        self.err.copy_(state['err'])
        self.acc_sum.zero_()
        self.acc_cnt.zero_()
        self.rebuild()
