"""Total-variation regulariser on the hash-grid tables: torch-ngp's `GridEncoder.grad_total_variation`, which the reference
predates.  The gradient of a squared-difference smoothness term between neighbouring lattice vertices is added straight into the
table gradient, after the backward and before the optimiser step (csrc/grid_tv.hip; include/nsr.h, "Total variation", states the
definition).  It acts on the tables themselves, where every other regulariser here acts through the rays: against floaters and
fine-level noise of few-view reconstruction (the density table) and against hash-collision speckle of stylisation (the colour
table).

    tv = TVRegulariser(model, lambda_density=1e-6)            # once: owns the sequence counter and the workspace
    loss.backward(); tv.add_grad(scaler.scale_tensor(dev)); scaler.step(opt)

Inside a GraphedRenderStep the call sits in the user's loss_fn, behind the backward.  Opt-in: not called, nothing changes."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .gridencoder import GridEncoder, _offsets_host

DEFAULT_SAMPLES = 1 << 18
ALL_LEVELS = 0xffffffff


def _level_mask(levels, n_levels):
    if levels is None:
        return ALL_LEVELS
    mask = 0
    for l in levels:
        if not 0 <= int(l) < n_levels:
            raise ValueError('level {} outside [0, {})'.format(l, n_levels))
        mask |= 1 << int(l)
    return mask


def grid_tv(tables, grad, lambdas, offsets, S, H, *, gridtype=0, level_mask=ALL_LEVELS, n_samples, seed, sequence=0, sequence_dev=None,
            stream_id=0, advance=False, scale=1.0, scale_dev=None, want_value=False, workspace=None):
    """nsr_grid_tv on device tensors.  tables: contiguous f32 whose leading offsets[-1] * len(lambdas) floats are the rows
    (a [rows, C] table, or the fused model's arena); grad: the same layout, accumulated into (None with want_value: the value
    only); lambdas: one host float per lane (0: the lane is neither read for the gradient nor written); offsets [L+1] (host or
    device: read on the host); S = log2(per_level_scale) as a float, H the base resolution.  sequence_dev: uint32 word on the
    device as an int32 tensor [1] (advance=True increments it after the draws); scale_dev: 0-dim or [1] f32 device tensor.
    -> [L, lanes] float64 device tensor with want_value, else None.  CPU tensors are refused."""
    ptr = L.p(tables)
    lam = np.ascontiguousarray(np.asarray(lambdas, np.float32).reshape(-1))
    rf = int(lam.size)
    off_np, off_p = _offsets_host(offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets)))
    n_levels = int(off_np.size) - 1
    need = int(off_np[-1]) * rf
    if tables.dtype != torch.float32 or tables.numel() < need:
        raise ValueError('grid_tv: tables must be float32 with at least {} elements; got {} {}'.format(need, tables.dtype, tables.numel()))
    if grad is not None and (grad.dtype != torch.float32 or grad.numel() < need or grad.device != tables.device):
        raise ValueError('grid_tv: grad must be float32 on the tables\' device with at least {} elements'.format(need))
    if grad is None and not want_value:
        raise ValueError('grid_tv: nothing to do (grad is None and want_value is False)')
    if sequence_dev is not None and (sequence_dev.dtype != torch.int32 or sequence_dev.numel() != 1):
        raise ValueError('grid_tv: sequence_dev must be an int32 tensor of one element')
    if scale_dev is not None and (scale_dev.dtype != torch.float32 or scale_dev.numel() != 1):
        raise ValueError('grid_tv: scale_dev must be a float32 tensor of one element')
    value = ws = None
    if want_value:
        value = torch.empty(n_levels, rf, dtype=torch.float64, device=tables.device)
        nbytes = int(L.lib().nsr_grid_tv_workspace_bytes(n_levels, int(n_samples), rf))
        ws = workspace if workspace is not None else torch.empty(nbytes // 8, dtype=torch.float64, device=tables.device)
        if ws.dtype != torch.float64 or ws.numel() * 8 < nbytes:
            raise ValueError('grid_tv: workspace must be float64 with at least {} elements'.format(nbytes // 8))
    L.check(L.lib().nsr_grid_tv(
        ptr, L.p(grad), rf, lam.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), off_p, n_levels, float(S), int(H), int(gridtype),
        int(level_mask) & ALL_LEVELS, int(n_samples), int(seed) & 0xffffffffffffffff, int(sequence) & 0xffffffff, L.p(sequence_dev),
        int(stream_id), int(bool(advance)), float(scale), L.p(scale_dev), L.p(value), L.p(ws), L.stream()), 'grid_tv')
    return value


class TVRegulariser:
    """The regulariser of one model or encoder.  target: a StyleTCNerf -- lanes (lambda_density, lambda_density, lambda_color,
    lambda_color) on model.arena / model._ensure_grad(); the MLP part of the arena is never touched -- or a GridEncoder with a
    single weight= for all its lanes.  levels: the levels to regularise (None: all).  rank: the data-parallel rank, passed as
    stream_id so that the averaged gradient uses distinct draws.  The device sequence counter and the workspace are allocated
    here, so nothing is allocated while a step is captured."""

    def __init__(self, target, lambda_density=0.0, lambda_color=0.0, n_samples=DEFAULT_SAMPLES, seed=0, levels=None, rank=0, weight=None):
        self.target = target
        self.is_encoder = isinstance(target, GridEncoder)
        if self.is_encoder:
            if weight is None or lambda_density or lambda_color:
                raise ValueError('TVRegulariser: a GridEncoder takes a single weight=')
            if target.input_dim != 3:
                raise ValueError('TVRegulariser: only input_dim == 3 is built')
            self.lambdas = [float(weight)] * int(target.level_dim)
            self.S = float(np.float32(np.log2(target.per_level_scale)))
            self.H, self.gridtype = int(target.base_resolution), int(target.gridtype_id)
            self.offsets = target.offsets.detach().to('cpu', torch.int32)
            device = target.embeddings.device
        else:
            if weight is not None:
                raise ValueError('TVRegulariser: weight= is for a GridEncoder; a model takes lambda_density and lambda_color')
            for lam, flag, what in ((lambda_density, 'train_density_table', 'density'), (lambda_color, 'train_color_table', 'colour')):
                if lam and not getattr(target, flag):
                    raise ValueError('TVRegulariser: lambda_{0} = {1} addresses the {0} table, which the model does not train '
                                     '({2} is False)'.format(what, lam, flag))
            self.lambdas = [float(lambda_density)] * 2 + [float(lambda_color)] * 2
            self.S, self.H, self.gridtype = float(target.S), int(target.cfg.pos_enc.min_res), 0
            self.offsets = torch.from_numpy(target._offsets_np.copy())
            device = target.arena.device
        if device.type != 'cuda':
            raise RuntimeError('TVRegulariser needs its target on a HIP device; got {} (there is no CPU fallback)'.format(device))
        self.n_levels = int(self.offsets.numel()) - 1
        self.level_mask = _level_mask(levels, self.n_levels)
        self.n_samples, self.seed, self.rank = int(n_samples), int(seed), int(rank)
        self.sequence_dev = torch.zeros(1, dtype=torch.int32, device=device)
        nbytes = int(L.lib().nsr_grid_tv_workspace_bytes(self.n_levels, self.n_samples, len(self.lambdas)))
        self.workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=device)

    def _tables(self):
        return self.target.embeddings.detach() if self.is_encoder else self.target.arena.detach()

    def _grad(self):
        if not self.is_encoder:
            return self.target._ensure_grad()
        emb = self.target.embeddings
        if emb.dtype != torch.float32:
            raise RuntimeError('TVRegulariser: the encoder\'s embeddings must be float32')
        if emb.grad is None:
            emb.grad = torch.zeros_like(emb)
        return emb.grad

    def _call(self, grad, advance, scale, scale_dev, want_value):
        return grid_tv(self._tables(), grad, self.lambdas, self.offsets, self.S, self.H, gridtype=self.gridtype,
                       level_mask=self.level_mask, n_samples=self.n_samples, seed=self.seed, sequence_dev=self.sequence_dev,
                       stream_id=self.rank, advance=advance, scale=scale, scale_dev=scale_dev, want_value=want_value,
                       workspace=self.workspace)

    def add_grad(self, loss_scale=1.0):
        """Accumulates the gradient of the term, times loss_scale (a float, or the 0-dim device tensor of
        LossScaler.scale_tensor), into the target's gradient and advances the sequence counter.  After the backward, before
        the optimiser step; no host read, legal while a graph is captured."""
        if isinstance(loss_scale, torch.Tensor):
            self._call(self._grad(), True, 1.0, loss_scale.detach(), False)
        else:
            self._call(self._grad(), True, float(loss_scale), None, False)

    def value(self):
        """[L, lanes] float64 on the device: the estimator's value per level and lane at the current sequence (which it does not
        advance); lanes with a zero weight and levels left out report 0.  For logging: the loss is sum(lambda_k * value[:, k])."""
        return self._call(None, False, 1.0, None, True)
