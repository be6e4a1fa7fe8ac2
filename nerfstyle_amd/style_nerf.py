"""Model wiring of the hot path: the counterpart of the reference's networks/style_nerf.py
(`StyleTCNerf`) and networks/tcnn_nerf.py (`get_grid_encoder`, `trunc_exp`).

`StyleTCNerf(cfg, bbox, class_dim, enc_dtype, use_dir=False)` keeps the reference constructor and
`forward(pts, dirs=None)` contract (sigma [M,1] when dirs is None, else (rgbs|classes [M,3+nc],
sigma [M,1]); style_nerf.py:120-159) and the reference's state_dict keys
(`x_density_embedder.{embeddings,offsets}`, `x_color_embedder.{...}`, `{density,color1,color2,
class}_net.params`), but the storage is MI355X-first:

  * ONE flat fp32 parameter arena [rows*4 + 15360] = the two hash tables INTERLEAVED as
    tables[row][enc][feat] followed by the four MLP parameter vectors, and one gradient arena of
    the same shape.  One 16-byte gather / one atomic request serves both encoders; the optimiser
    is one streaming pass; the multi-GPU gradient all-reduce is one flat bucket.
  * the whole field is evaluated by two fused launches (nsr_field_forward / nsr_field_backward);
    the backward recomputes the forward instead of saving [M,.] activations and accumulates
    straight into the gradient arena.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L
from . import profiling
from .common import BBox
from .config import NetworkConfig
from .gridencoder import GridEncoder
from .network import init_mlp_params

MLP_PARAMS = 15360
# view-dependent models: color2's first layer is [64, 32] = [color1 | SH]; its SH columns are a row-major [64, 16] block
# appended to the MLP block, so that every offset below holds for both kinds of model
MLP_PARAMS_DIRS = 16384
SH_OFF, SH_LEN = 15360, 1024
COLOR2_OFF, COLOR2_LEN, COLOR2_LEN_DIRS = 6144, 6144, 7168
# (name, offset in the MLP block, length); order fixed by include/nsr.h
MLP_LAYOUT = (('density_net', 0, 3072), ('color1_net', 3072, 3072), ('color2_net', 6144, 6144),
              ('class_net', 12288, 3072))


class _trunc_exp(Function):
    """tcnn_nerf.py:55-69"""
    @staticmethod
    def forward(ctx, x):
        x = x.to(torch.float32)
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        x = ctx.saved_tensors[0]
        return g * torch.exp(x.clamp(-15, 15))


trunc_exp = _trunc_exp.apply


def per_level_scale_from_cfg(cfg: NetworkConfig, max_bound: float) -> float:
    """tcnn_nerf.py:20-22"""
    pe = cfg.pos_enc
    max_res = pe.max_res_coeff * max_bound
    return float(np.exp2(np.log2(max_res / pe.min_res) / (pe.n_lvls - 1)))


def get_grid_encoder(cfg: NetworkConfig, max_bound: float, enc_dtype=None, use_custom_impl=True):
    """tcnn_nerf.py:14-52 (only the custom torch-ngp-style encoder exists here)."""
    pe = cfg.pos_enc
    return GridEncoder(input_dim=3, num_levels=pe.n_lvls, level_dim=pe.n_feats_per_lvl,
                       per_level_scale=per_level_scale_from_cfg(cfg, max_bound), base_resolution=pe.min_res,
                       log2_hashmap_size=pe.hashmap_size, gridtype='hash', align_corners=True)


def _field_call(entry, dirs, *args):
    """nsr_<entry>(*args, stream) -> status; with the samples' directions nsr_<entry>_dirs(*args, dirs, stream) (view-dependent models)"""
    if dirs is None:
        return getattr(L.lib(), 'nsr_' + entry)(*args, L.stream())
    return getattr(L.lib(), 'nsr_' + entry + '_dirs')(*args, L.p(dirs), L.stream())


class _field(Function):
    """Fused field: xyzs -> (sigmas [M], rgbs [M, 3+nc] | None).  `arena` is an input only so that
    autograd routes gradients here; the backward accumulates in place into model.grad_arena (which
    is arena.grad) and returns None for it."""

    @staticmethod
    def forward(ctx, xyzs, arena, model, sigma_only, m_dev, density_scale, want_feats=False, perm=None, dirs=None, pos_grad=False):
        # pos_grad (Renderer.pose_gradients): the backward also returns d loss / d xyzs; off, positions are constants as ever
        ctx.pos_grad = bool(pos_grad)
        xyzs = xyzs.detach().to(torch.float32).contiguous()
        if dirs is not None:
            dirs = dirs.detach().to(torch.float32).reshape(-1, 3).contiguous()
            assert dirs.shape[0] == xyzs.shape[0], 'one direction per sample'
        if model.use_dir and not sigma_only and dirs is None:
            raise ValueError('a view_dependent StyleTCNerf needs the samples\' directions: field(pts, dirs=...)')
        M = xyzs.shape[0]
        dev = xyzs.device
        sigmas = torch.empty(M, dtype=torch.float32, device=dev)
        rgbs = None if sigma_only else torch.empty(M, model.out_channels, dtype=torch.float32, device=dev)
        desc = model._desc(density_scale)
        tables = model._gather_tables()
        # the one thing a training forward saves: the encoded features as MFMA fragments (128 B/sample)
        feats = None
        # (decided by the caller: grad mode is always off inside Function.forward)
        if (not sigma_only) and want_feats:
            feats = torch.empty(((M + 15) // 16) * 512, dtype=torch.int32, device=dev)
        if sigma_only or not model.use_dir:
            dirs = None
        with profiling.timed('field_fwd_sigma' if sigma_only else 'field_fwd'):
            L.check(_field_call('field_forward', dirs, ctypes.byref(desc), L.p(tables), L.p(model._mlp_flat()), L.p(xyzs), M,
                                L.p(m_dev), L.p(sigmas), L.p(rgbs), L.p(feats), L.p(perm) if feats is not None else None),
                    'field_forward' if dirs is None else 'field_forward_dirs')
        ctx.model = model
        ctx.m_dev = m_dev
        ctx.density_scale = density_scale
        ctx.sigma_only = sigma_only
        # feats (15.6 GB at a full-frame capacity) and perm go through save_for_backward, NOT ctx attributes: autograd
        # drops saved tensors when backward() has run, attributes live as long as anything still holds the loss
        ctx.save_for_backward(xyzs, feats, perm, dirs)
        if sigma_only:
            return sigmas
        return sigmas, rgbs

    @staticmethod
    def backward(ctx, grad_sigmas, grad_rgbs=None):
        model = ctx.model
        xyzs, feats, perm, dirs = ctx.saved_tensors
        M = xyzs.shape[0]
        dev = xyzs.device
        if grad_sigmas is None:
            grad_sigmas = torch.zeros(M, dtype=torch.float32, device=dev)
        if grad_rgbs is None:
            grad_rgbs = torch.zeros(M, model.out_channels, dtype=torch.float32, device=dev)
        grad_sigmas = grad_sigmas.to(torch.float32).contiguous()
        grad_rgbs = grad_rgbs.to(torch.float32).contiguous()
        model._ensure_grad()
        desc = model._desc(ctx.density_scale)
        ga = model.grad_arena
        tables = model._gather_tables()
        ws = None
        if perm is not None:
            # [M][16] float4 of per-level encoder gradients for the spatially ordered table scatter (second kernel): 256 B
            # per sample SLOT (31 GB for a 122 M-slot capacity buffer), kept on the model and only ever grown -- the
            # caching allocator would otherwise be asked for the largest block of the step every step
            need = int(L.lib().nsr_field_backward_workspace_bytes(M, 1)) // 4
            if torch.cuda.is_current_stream_capturing():
                ws = torch.empty(need, dtype=torch.float32, device=dev)      # graph-owned: a captured pointer must never dangle
            else:
                ws = model._bwd_ws
                if ws is None or ws.device != dev or ws.numel() < need:
                    model._bwd_ws = None
                    ws = model._bwd_ws = torch.empty(need, dtype=torch.float32, device=dev)
        with profiling.timed('field_bwd'):
            def call(perm, wsp):
                return _field_call(
                    'field_backward', dirs, ctypes.byref(desc), L.p(tables), L.p(model._mlp_flat()), L.p(xyzs), M, L.p(ctx.m_dev),
                    L.p(grad_sigmas), L.p(grad_rgbs), L.p(ga), (ga.data_ptr() + model.table_elems * 4) if model.train_mlps else None,
                    int(model.train_density_table), int(model.train_color_table), L.p(feats), L.p(perm), L.p(wsp))
            st = call(perm, ws)
            want_pos = ctx.pos_grad and ctx.needs_input_grad[0]
            if want_pos and (perm is None or st == -2 or dirs is not None):
                raise NotImplementedError('position gradients need the encoder-gradient buffer of the spatially ordered backward '
                                          '(a perm, a grid the spatial scatter supports, no view-dependent colour)')
            if st == -2 and perm is not None:
                feats = None             # saved in the permutation's order: useless to a kernel that walks the buffers
                # NSR_ERR_UNSUPPORTED: a grid finer than the spatial scatter's LDS lattices hold (finest resolution above
                # ~5 cells per 1/1024 block) -- nothing was launched; the fused run-tracker backward takes over
                model._spatial_scatter_unsupported = True
                st = call(None, None)
            L.check(st, 'field_backward')
        grad_xyzs = None
        if want_pos:
            # the workspace just filled IS the input: d loss / d (encoder output) of every sample, contracted with the
            # interpolation's spatial partials (nsr_field_position_gradient)
            grad_xyzs = torch.empty(M, 3, dtype=torch.float32, device=dev)
            with profiling.timed('field_pos_grad'):
                L.check(L.lib().nsr_field_position_gradient(ctypes.byref(desc), L.p(tables), L.p(xyzs), M, L.p(ctx.m_dev), L.p(ws),
                                                            L.p(perm), L.p(grad_xyzs), L.stream()), 'field_position_gradient')
        return grad_xyzs, None, None, None, None, None, None, None, None, None


class _EncoderView(nn.Module):
    """Reference-shaped handle on one of the two interleaved tables (names used by checkpoints
    and by the trainers' keyword filters, e.g. OPTIM_KEYS = ['x_color_embedder'], style.py:25)."""

    def __init__(self, owner, enc_index, template: GridEncoder):
        super().__init__()
        self.__dict__['_owner'] = owner
        self.enc_index = enc_index
        for k in ('input_dim', 'num_levels', 'level_dim', 'per_level_scale', 'log2_hashmap_size', 'base_resolution',
                  'output_dim', 'gridtype', 'gridtype_id', 'align_corners', 'n_output_dims'):
            setattr(self, k, getattr(template, k))
        self.register_buffer('offsets', template.offsets.clone())

    @property
    def embeddings(self):
        """[rows, 2] strided view into the arena (not a copy)."""
        return self._owner.tables_view()[:, self.enc_index, :]


class _NetView(nn.Module):
    def __init__(self, owner, name, off, n, n_in, n_out):
        super().__init__()
        self.__dict__['_owner'] = owner
        self.n_input_dims, self.n_output_dims = n_in, n_out
        self._off, self._n = off, n

    @property
    def params(self):
        o = self._owner
        return o.arena.detach()[o.table_elems + self._off: o.table_elems + self._off + self._n]


class _Color2DirsView(_NetView):
    """color2_net of a view-dependent model: `params` is the reference-shaped (7168,) vector, ASSEMBLED from the arena's two
    blocks (a copy, not a view; write through load_state_dict)."""

    @property
    def params(self):
        return self._owner.views_of(self._owner.arena.detach())['color2_net.params']


def color2_assemble(block, sh):
    """arena blocks -> reference-shaped color2 vector: first layer row-major [64, 32] = [color1 columns | SH columns]."""
    first = torch.cat((block[:1024].view(64, 16), sh.view(64, 16)), dim=1).reshape(-1)
    return torch.cat((first, block[1024:]))


def color2_split(vec):
    """reference-shaped (7168,) color2 vector -> (arena block (6144,), SH columns (1024,))"""
    first = vec[:2048].view(64, 32)
    return torch.cat((first[:, :16].reshape(-1), vec[2048:])), first[:, 16:].reshape(-1)


class SHEncoder(nn.Module):
    """The tcnn.Encoding({'otype': 'SphericalHarmonics', 'degree': 4}) stand-in: [M,3] inputs u = (d + 1) / 2 in [0,1] (what the
    reference feeds it) -> [M,16] fp32 coefficients (nsr_sh_encode).  Forward only: no direction gradient exists on this path."""

    def __init__(self, degree=4):
        super().__init__()
        if degree != 4:
            raise NotImplementedError('SHEncoder: only degree 4 (16 coefficients) is built, got {}'.format(degree))
        self.n_input_dims, self.n_output_dims = 3, 16

    @torch.no_grad()
    def forward(self, u):
        return self.encode_dirs(u.detach().to(torch.float32) * 2 - 1)

    @staticmethod
    @torch.no_grad()
    def encode_dirs(dirs):
        """The same, from the directions themselves (the kernels' input)."""
        dirs = dirs.detach().to(torch.float32).reshape(-1, 3).contiguous()
        out = torch.empty(dirs.shape[0], 16, dtype=torch.float32, device=dirs.device)
        L.check(L.lib().nsr_sh_encode(L.p(dirs), dirs.shape[0], L.p(out), L.stream()), 'sh_encode')
        return out


class StyleTCNerf(nn.Module):
    def __init__(self, cfg: NetworkConfig, bbox: BBox, class_dim: int, enc_dtype=None, use_dir: bool = False,
                 compute_dtype=torch.float16, device=None, view_dependent: bool = False):
        """enc_dtype: None -> half gather tables (the reference's AMP behaviour, trainers/base.py:148
        + grid.py:42-43); torch.float32 -> fp32 tables.
        view_dependent=True: the reference's use_dir=True model -- colour depends on the viewing direction through a
        degree-4 SH encoding concatenated to color1_net's output (color2_net is 32 -> 64 -> 64 -> 3)."""
        super().__init__()
        if use_dir and not view_dependent:
            raise NotImplementedError('use_dir=True alone is not accepted: pass view_dependent=True for the SH direction '
                                      'encoding (both reference entry points pass use_dir=False, trainers/base.py:149-151, '
                                      'render.py:68-69)')
        if view_dependent and int(getattr(cfg, 'dir_enc_sh_deg', 4)) != 4:
            raise NotImplementedError('view_dependent: only cfg.dir_enc_sh_deg == 4 is built, got {}'.format(cfg.dir_enc_sh_deg))
        assert cfg.density_hidden_dims == 64 and cfg.rgb_hidden_dims == 64
        assert cfg.density_hidden_layers == 1 and cfg.rgb_hidden_layers == 2
        assert cfg.pos_enc.n_lvls == 16 and cfg.pos_enc.n_feats_per_lvl == 2
        self.cfg = cfg
        self.bounds_bbox = bbox
        self.use_dir = bool(view_dependent)
        self.mlp_params = MLP_PARAMS_DIRS if self.use_dir else MLP_PARAMS
        self.class_dim = class_dim
        self.out_channels = 3 + class_dim
        self.compute_dtype = compute_dtype
        self.table_dtype = torch.float16 if enc_dtype in (None, torch.float16) else torch.float32
        self.train_density_table = True
        self.train_color_table = True
        self.train_mlps = True                   # False (set by an optimiser that trains no net): the backward skips the weight gradients
        self.save_features = True     # forward keeps 128 B/sample of encoded features for the backward

        max_bound = torch.max(bbox.size).item()
        template = get_grid_encoder(cfg, max_bound)
        self.per_level_scale = template.per_level_scale
        self.S = float(np.float32(np.log2(self.per_level_scale)))
        self._offsets_np = template.offsets.numpy().astype(np.int32).copy()
        self.rows = int(self._offsets_np[-1])
        self.table_elems = self.rows * 4

        # ---- the arena -------------------------------------------------------------------------
        flat = torch.empty(self.table_elems + self.mlp_params, dtype=torch.float32)
        g = torch.Generator().manual_seed(int(cfg.network_seed or 0))
        flat[:self.table_elems].uniform_(-1e-4, 1e-4, generator=g)   # grid.py:150-152
        seed = int(cfg.network_seed or 0)
        if self.use_dir:
            c2, sh = color2_split(init_mlp_params(32, 3, 64, 2, seed + 2))
        else:
            c2, sh = init_mlp_params(16, 3, 64, 2, seed + 2), torch.empty(0)
        mlp = torch.cat([
            init_mlp_params(32, 1, 64, 1, seed), init_mlp_params(32, 16, 64, 1, seed + 1),
            c2, init_mlp_params(32, class_dim, 64, 1, seed + 3), sh])
        flat[self.table_elems:] = mlp
        self.arena = nn.Parameter(flat)
        self.grad_arena = None
        self._half_tables = None
        self._half_version = -1
        self._bbox_host = None                   # _bbox()
        self._bwd_ws = None                      # the ordered backward's encoder-gradient buffer (_field.backward), only ever grown
        self._spatial_scatter_unsupported = False    # set by a backward that had to fall back from the spatial table scatter

        self.x_density_embedder = _EncoderView(self, 0, template)
        self.x_color_embedder = _EncoderView(self, 1, template)
        self.density_net = _NetView(self, 'density_net', 0, 3072, 32, 1)
        self.color1_net = _NetView(self, 'color1_net', 3072, 3072, 32, 16)
        if self.use_dir:
            self.color2_net = _Color2DirsView(self, 'color2_net', 6144, 6144, 32, 3)
            self.dir_encoder = SHEncoder(4)
        else:
            self.color2_net = _NetView(self, 'color2_net', 6144, 6144, 16, 3)
        self.class_net = _NetView(self, 'class_net', 12288, 3072, 32, class_dim)
        if device is not None:
            self.to(device)

    # ---- storage helpers -----------------------------------------------------------------------
    @property
    def device(self):
        return self.arena.device

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.bounds_bbox.to(self.arena.device)
        self.grad_arena = None
        self._half_tables = None
        self._half_version = -1
        return self

    def tables_view(self):
        return self.arena.detach()[:self.table_elems].view(self.rows, 2, 2)

    def _mlp_flat(self):
        return self.arena.detach()[self.table_elems:]

    def _ensure_grad(self):
        if self.grad_arena is None or self.grad_arena.device != self.arena.device:
            self.grad_arena = torch.zeros_like(self.arena.detach())
        if self.arena.grad is None:
            self.grad_arena.zero_()
            self.arena.grad = self.grad_arena
        elif self.arena.grad.data_ptr() != self.grad_arena.data_ptr():
            self.grad_arena = self.arena.grad
        return self.grad_arena

    def half_tables(self):
        """f16 gather copy of the tables; storage is stable so fused optimisers can write into it."""
        if self._half_tables is None or self._half_tables.device != self.arena.device:
            self._half_tables = torch.empty(self.table_elems, dtype=torch.float16, device=self.arena.device)
            self._half_version = -1
        return self._half_tables

    def mark_half_synced(self):
        self._half_version = self.arena._version

    def sync_gather_tables(self):
        """Make the gather tables current if the arena changed: the f16 copy is cast again after anything but a fused optimiser
        (which refreshes it in its own pass) wrote the parameters.  Nothing to do for fp32 tables, which are the arena."""
        if self.table_dtype == torch.float32:
            return
        h = self.half_tables()
        if self._half_version != self.arena._version:
            L.check(L.lib().nsr_cast_f32_to_f16(L.p(self.arena.detach()), L.p(h), self.table_elems, L.stream()),
                    'cast_f32_to_f16')
            self._half_version = self.arena._version

    def _gather_tables(self):
        self.sync_gather_tables()
        return self.arena.detach() if self.table_dtype == torch.float32 else self.half_tables()

    def _bbox(self):
        """Host copy (min, size) of the constant bounding box, read back once: a per-call .cpu() would be a device
        synchronisation in the middle of an otherwise sync-free step"""
        if self._bbox_host is None:
            self._bbox_host = (self.bounds_bbox.min_pt.detach().cpu().tolist(), self.bounds_bbox.size.detach().cpu().tolist())
        return self._bbox_host

    def _desc(self, density_scale=1.0):
        d = L.FieldDesc()
        d.L, d.H, d.S = 16, int(self.cfg.pos_enc.min_res), self.S
        d.num_classes = self.class_dim
        d.table_dtype = L.dt(self.table_dtype)
        d.compute_dtype = L.dt(self.compute_dtype)
        mn, sz = self._bbox()
        for i in range(3):
            d.bbox_min[i] = mn[i]
            d.bbox_size[i] = sz[i]
        d.density_scale = float(density_scale)
        d.offsets = self._offsets_np.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        return d

    # ---- reference-shaped checkpoints ----------------------------------------------------------
    def views_of(self, flat):
        """name -> view of an arena-shaped flat tensor (the parameter arena, a moment or an EMA arena of an optimiser), in the
        reference's named_parameters() order.  The one place that writes the arena layout out."""
        t = flat[:self.table_elems].view(self.rows, 2, 2)
        out = {'x_density_embedder.embeddings': t[:, 0, :], 'x_color_embedder.embeddings': t[:, 1, :]}
        for name, off, n in MLP_LAYOUT:
            out[name + '.params'] = flat[self.table_elems + off: self.table_elems + off + n]
        if self.use_dir:
            # the one entry that is a COPY: the reference-shaped vector interleaves two arena blocks
            out['color2_net.params'] = color2_assemble(out['color2_net.params'],
                                                       flat[self.table_elems + SH_OFF: self.table_elems + SH_OFF + SH_LEN])
        return out

    def state_dict(self, *args, **kwargs):
        sd = {name: v.clone() for name, v in self.views_of(self.arena.detach()).items()}
        sd['x_density_embedder.offsets'] = self.x_density_embedder.offsets.clone()
        sd['x_color_embedder.offsets'] = self.x_color_embedder.offsets.clone()
        return sd

    def load_state_dict(self, sd, strict=True):
        n2 = sd['color2_net.params'].numel()
        if n2 != (COLOR2_LEN_DIRS if self.use_dir else COLOR2_LEN):
            raise ValueError('color2_net.params has {} entries, this model (view_dependent={}) holds {}: a checkpoint of a '
                             'view_dependent={} model loads only into a model built with that switch'.format(
                                 n2, self.use_dir, COLOR2_LEN_DIRS if self.use_dir else COLOR2_LEN, n2 == COLOR2_LEN_DIRS))
        with torch.no_grad():
            flat = self.arena.detach()
            for name, v in self.views_of(flat).items():
                if self.use_dir and name == 'color2_net.params':
                    block, sh = color2_split(sd[name].reshape(-1).to(flat))
                    flat[self.table_elems + COLOR2_OFF: self.table_elems + COLOR2_OFF + COLOR2_LEN].copy_(block)
                    flat[self.table_elems + SH_OFF: self.table_elems + SH_OFF + SH_LEN].copy_(sh)
                    continue
                v.copy_(sd[name].reshape(v.shape))
            self.arena.add_(0)   # bump the version counter: the half copy is stale
        return self

    def named_views(self):
        """(name, arena slice or strided view) pairs in the reference's named_parameters() order."""
        return list(self.views_of(self.arena.detach()).items())

    # ---- forward -------------------------------------------------------------------------------
    def position_gradient_refusal(self):
        """Why this model cannot give d loss / d position through `field(..., pos_grad=True)` (None: it can).  The gradient is
        built from the encoder-gradient buffer of the spatially ordered backward, which must hold both encoders' halves."""
        if self.use_dir:
            return 'view_dependent=True: no gradient with respect to the samples\' directions exists'
        if self._spatial_scatter_unsupported:
            return 'the spatial table scatter is unsupported for this grid, so its encoder-gradient buffer does not exist'
        if not self.train_density_table or not self.train_mlps:
            return ('train_density_table = False or train_mlps = False selects the colour-only backward (the stylisation stage), '
                    'which leaves the density half of the encoder-gradient buffer zero')
        return None

    def field(self, pts, sigma_only=False, m_dev=None, density_scale=1.0, perm=None, dirs=None, pos_grad=False):
        """Fast path: flat sigmas [M] (and rgbs [M,3+nc]); m_dev = device int32 sample count; perm = spatial order from
        `sample_order` (int32 [M] device tensor): a training forward then walks the samples in that order (its saved features
        are tile-major in it) and the backward follows -- MLP chain first, then the table gradient with the stand-alone
        lattice scatter kernel (same result per sample, table gradient up to fp32 summation order; pays on dense batches).
        pos_grad=True (needs perm): `pts` that require grad receive d loss / d position from the backward
        (nsr_field_position_gradient on the encoder gradients the ordered backward has just written); otherwise positions are
        constants of the loss and the backward returns None for them."""
        want_feats = bool(self.save_features and torch.is_grad_enabled() and self.arena.requires_grad and not sigma_only)
        if not pos_grad:
            return _field.apply(pts, self.arena, self, sigma_only, m_dev, density_scale, want_feats, perm, dirs)
        why = self.position_gradient_refusal() or (None if perm is not None else 'pos_grad needs perm (the spatially ordered backward)')
        if why is not None:
            raise NotImplementedError('position gradients: ' + why)
        return _field.apply(pts, self.arena, self, sigma_only, m_dev, density_scale, want_feats, perm, dirs, True)

    @torch.no_grad()
    def density_gradient(self, pts, m_dev=None, density_scale=1.0, normalize=False):
        """(sigmas [M], grads [M,3]): the density and its gradient with respect to the world position, one fused launch in
        forward mode (nsr_field_density_gradient).  normalize: the unit normal -grad / |grad| instead (zero where the
        gradient is zero).  Positions outside the box or NaN, and slots at or past m_dev, get a zero gradient (the latter keep
        an unwritten sigma, as in `field`).  NO-GRAD ONLY: neither output is attached to the autograd graph -- a loss on
        them (Eikonal, normal consistency) would need a second-order backward through the fused kernels, which does not exist."""
        pts = pts.detach().reshape(-1, 3).to(torch.float32).contiguous()
        M = pts.shape[0]
        sigmas = torch.empty(M, dtype=torch.float32, device=pts.device)
        grads = torch.empty(M, 3, dtype=torch.float32, device=pts.device)
        desc = self._desc(density_scale)
        tables = self._gather_tables()
        with profiling.timed('field_density_grad'):
            L.check(L.lib().nsr_field_density_gradient(ctypes.byref(desc), L.p(tables), L.p(self._mlp_flat()), L.p(pts), M,
                                                       L.p(m_dev), L.p(sigmas), L.p(grads), int(bool(normalize)), L.stream()),
                    'field_density_gradient')
        return sigmas, grads

    def sample_order(self, xyzs, m_dev=None, sort_prefix=None, out=None):
        """nsr_sample_order: Morton-order permutation of the samples [M,3] (int32 tensor [M], a uint32 bit pattern;
        written into `out` when given)."""
        M = xyzs.shape[0]
        dev = xyzs.device
        need = (int(L.lib().nsr_sample_order_workspace_bytes(M)) + 3) // 4 + 64
        # a temporary of torch's stream-ordered caching allocator: no hipMalloc in the steady state, correct on any stream,
        # and under capture it belongs to the graph's own pool (a captured launch bakes its pointers in)
        ws = torch.empty(need, dtype=torch.int32, device=dev)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        perm = torch.empty(M, dtype=torch.int32, device=dev) if out is None else out
        assert perm.dtype == torch.int32 and perm.numel() == M and perm.is_contiguous() and perm.device == dev
        mn, sz = self._bbox()
        c3 = ctypes.c_float * 3
        L.check(L.lib().nsr_sample_order(L.p(xyzs), M, L.p(m_dev), M if sort_prefix is None else int(min(sort_prefix, M)),
                                         c3(*mn), c3(*sz), L.p(perm), ws_ptr, L.stream()), 'sample_order')
        return perm

    def forward(self, pts, dirs=None, bsize=1000000):
        """style_nerf.py:144-159.  The >1M-point chunking of the reference (utils.batch_exec) is
        unnecessary here: the fused kernel keeps no per-sample intermediates in HBM."""
        pts = pts.reshape(-1, 3)
        if dirs is None:
            return self.field(pts, sigma_only=True).unsqueeze(-1)
        sigmas, rgbs = self.field(pts, sigma_only=False, dirs=dirs.reshape(-1, 3) if self.use_dir else None)
        return rgbs, sigmas.unsqueeze(-1)
