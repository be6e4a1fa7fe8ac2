"""Data-parallel optimiser step sharded across ranks (SURVEY.md sections 5 and 8e: reduce-scatter + all-gather).

`ShardedFusedAdam` is a sibling of `optim.FusedAdam` under `optim.AdamBase`, which gives both the same constructor
bookkeeping, step scalars, scaler adoption, counters and state dicts.  It takes FusedAdam's constructor arguments and
`step(grad_scale=..., scaler=..., lr_decay_steps=...)` semantics, but every rank checks, steps and keeps Adam / EMA state for
1/N of the trained elements only:

    1. reduce-scatter of the gradient (the whole arena in place, or the packed lanes of one table: nsr_lanes_pack)
    2. scaler path: nsr_grad_check on the rank's reduced shard, MAX of found_inf over the ranks, nsr_scaler_update
       (every rank takes the same skip / scale / lr / bias-correction decision)
    3. Adam + EMA on the shard (nsr_adam_step* with offset pointers, or nsr_lanes_adam*)
    4. all-gather of the updated fp32 parameters in place; the f16 gather copy of the other ranks' shards is refreshed
       locally (nsr_cast_f32_to_f16, or nsr_lanes_unpack)

It does the gradient reduction itself: callers must not also call `parallel.sync_gradients*` (stylize.py skips its own
all-reduce for an optimiser whose `reduces_gradients` is true).  At world size 1 it issues no collective and equals
FusedAdam bit for bit.  A ring all-reduce is itself a reduce-scatter followed by an all-gather: the bytes on the links are
the same as with the all-reduce path; what shrinks is the optimiser work and state per rank (1/N).

Two trained sets are supported, those of the reference's trainers: everything (keywords=None, trainers/base.py:185-221)
and one hash table without nets (keywords=['x_color_embedder'], trainers/style.py:25; the density table alone comes with
the same code).  Anything else raises NotImplementedError.

Under gloo (one-card rehearsals, CPU tests) the collectives are staged through host buffers; under RCCL they run on the
device buffers directly and the compute stream waits for them without a host block."""
import types

import torch
import torch.distributed as dist

from . import _lib as L
from .optim import AdamBase, select_regions, single_trained_table
from .style_nerf import MLP_LAYOUT, MLP_PARAMS, StyleTCNerf

SHARD_ALIGN = 16          # floats: 64 B, and a multiple of 4 keeps the element-mask phase of the interleaved rows


def trained_lane_mask(model: StyleTCNerf, keywords=None) -> int:
    """0xF: everything is trained (reconstruction); 0x3 / 0xC: one hash table and no net (stylisation).  Other selections
    raise NotImplementedError."""
    if model.use_dir:
        raise NotImplementedError('ShardedFusedAdam does not handle a view_dependent=True model (the appended SH-column block '
                                  'of color2_net is not in its lane layout): use optim.FusedAdam with parallel.sync_gradients')
    mask, nets = select_regions(model, keywords)
    if mask == 0xF and len(nets) == len(MLP_LAYOUT):
        return 0xF
    if single_trained_table(mask, nets) is not None:
        return mask
    raise NotImplementedError(
        'ShardedFusedAdam supports keywords=None (everything) and one hash table without nets (e.g. keywords='
        "['x_color_embedder']); keywords={} select table mask {:#x} and {} of {} nets: use optim.FusedAdam with "
        'parallel.sync_gradients'.format(keywords, mask, len(nets), len(MLP_LAYOUT)))


def shard_chunk(total: int, world: int) -> int:
    """Elements per rank: ceil(total / world) rounded up to a multiple of SHARD_ALIGN."""
    c = -(-total // world)
    return -(-c // SHARD_ALIGN) * SHARD_ALIGN


class ShardGeometry:
    """Host-only shard layout.  The trained elements form one flat space of `total` elements: the whole arena
    (lane_mask 0xF) or the packed lanes of one table (0x3 / 0xC: element j is lane j & 1 of that table in row j // 2).
    Rank k owns [k c, (k + 1) c) & [0, total); collective buffers hold world * c elements, the rest is padding."""

    def __init__(self, rows: int, mlp_elems: int, lane_mask: int, world: int, rank: int):
        assert lane_mask in (0x3, 0xC, 0xF) and 0 <= rank < world
        self.rows, self.table_elems = int(rows), 4 * int(rows)
        self.arena_elems = self.table_elems + int(mlp_elems)
        self.lane_mask, self.world, self.rank = lane_mask, int(world), int(rank)
        self.packed = lane_mask != 0xF
        self.lane0 = 2 if lane_mask == 0xC else 0
        self.total = 2 * self.rows if self.packed else self.arena_elems
        self.chunk = shard_chunk(self.total, self.world)
        self.padded = self.world * self.chunk
        self.slot = self.rank * self.chunk                   # start of the rank's slot in a collective buffer
        self.lo = min(self.slot, self.total)
        self.hi = min(self.slot + self.chunk, self.total)
        self.n = self.hi - self.lo

    @classmethod
    def of(cls, model: StyleTCNerf, keywords, world: int, rank: int):
        return cls(model.rows, model.arena.numel() - model.table_elems, trained_lane_mask(model, keywords), world, rank)

    def bounds(self, rank):
        lo = min(rank * self.chunk, self.total)
        return lo, min(lo + self.chunk, self.total)

    # ---- packed lanes (lane_mask 0x3 / 0xC) ----
    @property
    def row_lo(self):
        return self.lo // 2

    @property
    def row_hi(self):
        return self.hi // 2

    def lane_to_arena(self, j):
        """packed index -> arena index (int or integer tensor)"""
        return (j // 2) * 4 + self.lane0 + (j % 2)

    def arena_to_lane(self, i):
        """arena index of a trained table lane -> packed index"""
        return (i // 4) * 2 + (i % 4) - self.lane0

    # ---- the f16 gather copy (whole arena, lane_mask 0xF) ----
    def half_own(self):
        """(offset, n) of the table elements this rank's Adam writes into the f16 copy"""
        return self.lo, max(0, min(self.hi, self.table_elems) - self.lo)

    def half_refresh(self):
        """[(offset, n)] of the table elements outside the rank's shard: cast from the gathered fp32 parameters"""
        out = [(0, min(self.lo, self.table_elems)), (self.hi, self.table_elems - self.hi)]
        return [(o, n) for (o, n) in out if n > 0]


class _Reduction:
    """Handle of the gradient reduce-scatter in flight (reduce_gradients_async).  wait() makes the CURRENT stream wait for
    it (RCCL: a stream dependency, no host block) and then zeroes the gradient outside the rank's shard.  Idempotent; the
    next step() consumes the reduction."""

    def __init__(self, opt, work, after):
        self.opt, self.work, self.after = opt, work, after

    def wait(self):
        if self.work is not None:
            self.work.wait()
        if self.after is not None:
            self.after()
        self.work = self.after = None


class ShardedFusedAdam(AdamBase):
    """FusedAdam with the optimiser step sharded across the data-parallel ranks (module docstring).  Construct it after the
    model has been moved to its device: the whole-arena set re-homes `model.arena` (the same nn.Parameter) and its gradient
    arena in padded storage, so that the collectives work in place."""

    reduces_gradients = True

    def __init__(self, model: StyleTCNerf, lr=1e-2, betas=(0.9, 0.999), eps=1e-15, keywords=None, ema_decay=None,
                 process_group=None):
        self.group = process_group
        if dist.is_initialized():
            world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
            self._staged = dist.get_backend(process_group) == 'gloo'
        else:
            world, rank, self._staged = 1, 0, False
        self.geo = geo = ShardGeometry.of(model, keywords, world, rank)
        super().__init__(model, lr, betas, eps, keywords, ema_decay)
        self._pending = None
        self._frozen = None               # packed set: full-layout moments of the untrained elements, as last loaded
        a = model.arena.detach()
        dev = a.device
        self.exp_avg = torch.zeros(geo.chunk, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(geo.chunk, dtype=torch.float32, device=dev)
        if geo.packed:
            # gradient in (reduce-scatter), updated parameters out (all-gather): one buffer
            self._packed = torch.zeros(geo.padded, dtype=torch.float32, device=dev)
            # EMA of all four lanes of the rank's rows (FusedAdam's EMA moves every element of the rows it steps); the
            # MLP block's EMA is not stepped by this set and is kept whole on every rank
            self.ema = None if ema_decay is None else torch.zeros(2 * geo.chunk, dtype=torch.float32, device=dev)
            self.ema_rest = None if ema_decay is None else a[model.table_elems:].clone()
            if self.ema is not None:
                self.ema[:4 * (geo.row_hi - geo.row_lo)].copy_(a[4 * geo.row_lo:4 * geo.row_hi])
        else:
            self._home()
            self.ema = None
            if ema_decay is not None:
                self.ema = torch.zeros(geo.chunk, dtype=torch.float32, device=dev)
                self.ema[:geo.n].copy_(a[geo.lo:geo.hi])

    # ---- storage -------------------------------------------------------------------------------------------------------
    def _home(self):
        """Whole-arena set: model.arena (the same Parameter) and its gradient arena live in the first T elements of padded
        buffers of world * chunk elements.  Done at construction; again only if the model was moved or its gradient replaced."""
        m, geo = self.model, self.geo
        p = m.arena
        store = getattr(self, '_arena_store', None)
        gstore = getattr(self, '_grad_store', None)
        if (store is not None and p.device == store.device and p.data_ptr() == store.data_ptr()
                and m._ensure_grad().data_ptr() == gstore.data_ptr()):
            return
        T = geo.total
        with torch.no_grad():
            store = torch.zeros(geo.padded, dtype=torch.float32, device=p.device)
            store[:T].copy_(p.detach())
            g = m._ensure_grad()
            gstore = torch.zeros(geo.padded, dtype=torch.float32, device=p.device)
            gstore[:T].copy_(g)
            p.data = store[:T]
            m.grad_arena = gstore[:T]
            p.grad = m.grad_arena
        m._half_version = -1
        self._arena_store, self._grad_store = store, gstore

    # ---- collectives (gloo: staged through host buffers) ----------------------------------------------------------------
    def _reduce_scatter(self, out, inp):
        if self._staged:
            o = torch.empty(out.numel(), dtype=out.dtype)
            dist.reduce_scatter_tensor(o, inp.cpu(), op=dist.ReduceOp.SUM, group=self.group)
            out.copy_(o)
            return None
        return dist.reduce_scatter_tensor(out, inp, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def _all_gather(self, out, inp):
        if self._staged:
            o = torch.empty(out.numel(), dtype=out.dtype)
            dist.all_gather_into_tensor(o, inp.cpu(), group=self.group)
            out.copy_(o)
        else:
            dist.all_gather_into_tensor(out, inp, group=self.group, async_op=True).wait()

    def _all_reduce_max(self, t):
        if self._staged:
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.MAX, group=self.group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)

    def _gather(self, shard):
        """collective: the world's shards of a per-rank buffer, concatenated (world * shard.numel() elements)"""
        if self.geo.world == 1:
            return shard.clone()
        out = torch.empty(self.geo.world * shard.numel(), dtype=shard.dtype, device=shard.device)
        self._all_gather(out, shard.contiguous())
        return out

    # ---- step --------------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        if self._pending is not None:
            self._pending.wait()
            self._pending = None
        self.model._ensure_grad().zero_()

    @torch.no_grad()
    def reduce_gradients_async(self) -> _Reduction:
        """Starts the gradient reduce-scatter and returns its handle (wait()); step() completes a pending one itself.  The
        caller may enqueue parameter-independent work (Renderer.begin_train of the next step) before waiting.  Until step()
        has run, further calls return the same handle."""
        if self._pending is not None:
            return self._pending
        m, geo = self.model, self.geo
        if geo.packed:
            g = m._ensure_grad()
            L.check(L.lib().nsr_lanes_pack(L.p(g), geo.rows, geo.lane_mask, L.p(self._packed), L.stream()), 'lanes_pack')
            g[m.table_elems:].zero_()                    # the MLP gradient: not trained, zeroed as FusedAdam does
            work = None
            if geo.world > 1:
                work = self._reduce_scatter(self._packed[geo.slot:geo.slot + geo.chunk], self._packed)
            self._pending = _Reduction(self, work, None)
            return self._pending
        self._home()
        if geo.world == 1:
            self._pending = _Reduction(self, None, None)
            return self._pending
        full = self._grad_store
        work = self._reduce_scatter(full[geo.slot:geo.slot + geo.chunk], full)

        def zero_foreign():
            full[:geo.slot].zero_()
            full[geo.slot + geo.chunk:].zero_()
        self._pending = _Reduction(self, work, zero_foreign)
        return self._pending

    @torch.no_grad()
    def step(self, grad_scale=1.0, scaler=None, lr_decay_steps=0.0):
        """FusedAdam's step on this rank's shard, between a gradient reduce-scatter and a parameter all-gather."""
        (self._pending or self.reduce_gradients_async()).wait()
        self._pending = None
        m, geo = self.model, self.geo
        a = m.arena.detach()
        half = m.half_tables() if m.table_dtype == torch.float16 else None
        lib = L.lib()
        ptr = lambda t, off: t.data_ptr() + off * 4
        hptr = lambda off: half.data_ptr() + off * 2
        if geo.packed:
            grad = self._packed[geo.slot:geo.slot + geo.chunk]
        else:
            grad = self._grad_store[geo.slot:geo.slot + geo.chunk]
        st = None
        if scaler is None:
            lr, decay, step = self._host_scalars()
        else:
            st = self.attach_scaler(scaler, a.device)
            L.check(lib.nsr_grad_check(L.p(grad), geo.n, 0xF, L.p(st), L.stream()), 'grad_check')
            if geo.world > 1:
                self._all_reduce_max(st[2:3])             # found_inf: every rank takes the same decision
            self._scaler_update(scaler, st, lr_decay_steps)
        b1, b2, eps = float(self.betas[0]), float(self.betas[1]), float(self.eps)
        if geo.packed:
            args = (a.data_ptr(), half.data_ptr() if half is not None else None, L.p(grad), L.p(self.exp_avg),
                    L.p(self.exp_avg_sq), L.p(self.ema), L.p(grad), geo.row_lo, geo.row_hi, geo.lane_mask)
            if st is None:
                L.check(lib.nsr_lanes_adam(*args, float(lr), b1, b2, eps, float(1.0 / grad_scale), float(decay), step,
                                           L.stream()), 'lanes_adam')
            else:
                L.check(lib.nsr_lanes_adam_scaled(*args, b1, b2, eps, L.p(st), L.stream()), 'lanes_adam_scaled')
            if geo.world > 1:
                self._all_gather(self._packed, self._packed[geo.slot:geo.slot + geo.chunk])
                for (r0, r1) in ((0, geo.row_lo), (geo.row_hi, geo.rows)):
                    L.check(lib.nsr_lanes_unpack(L.p(self._packed), r0, r1, geo.lane_mask, a.data_ptr(),
                                                 half.data_ptr() if half is not None else None, L.stream()), 'lanes_unpack')
        else:
            g = self._grad_store
            te = m.table_elems
            ema = lambda o: ptr(self.ema, o - geo.lo) if self.ema is not None else None
            if st is None:
                # as FusedAdam: the host-scalar entry point has no half_n, the shard is split at the table end
                cut = min(max(te, geo.lo), geo.hi) if half is not None else geo.hi
                for (o, k) in ((geo.lo, cut - geo.lo), (cut, geo.hi - cut)):
                    if k > 0:
                        L.check(lib.nsr_adam_step(
                            ptr(a, o), ptr(g, o), ptr(self.exp_avg, o - geo.lo), ptr(self.exp_avg_sq, o - geo.lo), ema(o),
                            hptr(o) if (half is not None and o < te) else None, k, float(lr), b1, b2, eps,
                            float(1.0 / grad_scale), float(decay), step, 0xF, L.stream()), 'adam_step')
            else:
                ho, hn = geo.half_own()
                L.check(lib.nsr_adam_step_scaled(
                    ptr(a, geo.lo), ptr(g, geo.lo), L.p(self.exp_avg), L.p(self.exp_avg_sq), ema(geo.lo),
                    hptr(ho) if (half is not None and hn > 0) else None, geo.n, hn if half is not None else 0,
                    b1, b2, eps, 0xF, L.p(st), L.stream()), 'adam_step_scaled')
            if geo.world > 1:
                self._all_gather(self._arena_store, self._arena_store[geo.slot:geo.slot + geo.chunk])
                if half is not None:
                    for (o, k) in geo.half_refresh():
                        L.check(lib.nsr_cast_f32_to_f16(ptr(a, o), hptr(o), k, L.stream()), 'cast_f32_to_f16')
        if half is not None and self.table_mask:
            m.mark_half_synced()

    # ---- state: full layout in, full layout out ---------------------------------------------------------------------------
    def _full(self, shard, base):
        """collective: full-layout (arena-sized) tensor of a per-rank moment shard; base = values of the untrained elements"""
        m, geo = self.model, self.geo
        flat = self._gather(shard)
        if not geo.packed:
            return flat[:geo.total].clone()
        out = torch.zeros(geo.arena_elems, dtype=torch.float32, device=shard.device) if base is None else \
            base.to(shard.device, copy=True)
        t = out[:m.table_elems].view(geo.rows, 2, 2)
        t[:, geo.lane0 // 2, :].copy_(flat[:geo.total].view(geo.rows, 2))
        return out

    def _full_ema(self):
        if self.ema is None:
            return None
        geo = self.geo
        flat = self._gather(self.ema)
        if not geo.packed:
            return flat[:geo.total].clone()
        return torch.cat([flat[:geo.table_elems], self.ema_rest])

    def _full_state(self):
        """Collective: state_dict() then has the layout of FusedAdam's, bit for bit."""
        fr = self._frozen or {}
        return self._full(self.exp_avg, fr.get('exp_avg')), self._full(self.exp_avg_sq, fr.get('exp_avg_sq')), self._full_ema()

    def gathered(self):
        """Collective.  An object with FusedAdam's state_dict(), ema and ema_updates: what checkpoint.save_checkpoint reads
        (`save_checkpoint(path, renderer, optim=opt.gathered(), ...)` on rank 0)."""
        sd = self.state_dict()
        return types.SimpleNamespace(state_dict=lambda: sd, ema=sd['ema'], ema_updates=self.ema_updates)

    def _load_full(self, exp_avg, exp_avg_sq, ema):
        """keeps this rank's shard of full-layout tensors (a state_dict() of either optimiser, or the reference's state)"""
        m, geo = self.model, self.geo
        with torch.no_grad():
            if geo.packed:
                def lanes(full):
                    return full[:m.table_elems].view(geo.rows, 2, 2)[geo.row_lo:geo.row_hi, geo.lane0 // 2, :].reshape(-1)
                self.exp_avg[:geo.n].copy_(lanes(exp_avg))
                self.exp_avg_sq[:geo.n].copy_(lanes(exp_avg_sq))
                self._frozen = {'exp_avg': exp_avg.detach().cpu().clone(), 'exp_avg_sq': exp_avg_sq.detach().cpu().clone()}
                if self.ema is not None and ema is not None:
                    self.ema[:4 * (geo.row_hi - geo.row_lo)].copy_(ema[4 * geo.row_lo:4 * geo.row_hi])
                    self.ema_rest.copy_(ema[m.table_elems:])
            else:
                self.exp_avg[:geo.n].copy_(exp_avg[geo.lo:geo.hi])
                self.exp_avg_sq[:geo.n].copy_(exp_avg_sq[geo.lo:geo.hi])
                if self.ema is not None and ema is not None:
                    self.ema[:geo.n].copy_(ema[geo.lo:geo.hi])
