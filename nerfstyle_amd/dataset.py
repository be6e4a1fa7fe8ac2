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
