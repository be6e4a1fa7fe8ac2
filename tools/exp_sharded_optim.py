"""Rank 0's device work of one ShardedFusedAdam step, on ONE GPU, with the collectives left out: at world sizes N = 1, 2,
4, 8, for the reconstruction set (whole arena) and the stylisation set (colour lanes), against FusedAdam.step on the same
arena (grad check + Adam over every trained element).  HIP-event times (median of --reps), bytes from the shapes, share of
the 8.0 TB/s HBM peak.  The link-side time of the reduce-scatter / all-gather is not measured (no multi-GPU node).

    python tools/exp_sharded_optim.py [--reps 50] [--json out.json]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/exp_sharded_optim.py` (a separate run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerfstyle_amd import _lib as L
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig
from nerfstyle_amd.optim import LossScaler
from nerfstyle_amd.sharded_optim import ShardGeometry
from nerfstyle_amd.style_nerf import MLP_PARAMS, StyleTCNerf

HBM_PEAK = 8.0e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False).to(dev)
    rows, te = model.rows, model.table_elems
    T = model.arena.numel()
    lib, s = L.lib(), L.stream
    sc = LossScaler(init_scale=1.0, enabled=False)
    st = sc.state_on(dev)
    b1, b2, eps = 0.9, 0.999, 1e-15
    half = model.half_tables()
    ptr = lambda t, off, es=4: t.data_ptr() + off * es
    L.check(lib.nsr_scaler_update(L.p(st), 1e-2, 0.0, b1, b2, 2.0, 0.5, 2000, 0, 0.95, s()), 'scaler_update')
    rows_out = []

    def row(set_name, N, part, us, nbytes):
        rows_out.append({'set': set_name, 'N': N, 'part': part, 'us': round(us, 2), 'MB': round(nbytes / 1e6, 2),
                         'hbm_pct': round(100.0 * nbytes / (us * 1e-6) / HBM_PEAK, 1) if us > 0 else None})

    # ---- FusedAdam.step on the same arena (what every rank runs today) ----
    a = model.arena.detach()
    g = torch.zeros(T, device=dev)
    m, v, e = torch.zeros(T, device=dev), torch.zeros(T, device=dev), a.clone()
    for set_name, n, mask in (('recon', T, 0xF), ('style', te, 0xC)):
        us_c = timed(lambda: L.check(lib.nsr_grad_check(L.p(g), n, mask, L.p(st), s()), 'grad_check'), args.reps)
        us_a = timed(lambda: L.check(lib.nsr_adam_step_scaled(L.p(a), L.p(g), L.p(m), L.p(v), L.p(e), L.p(half), n, te, b1, b2, eps,
                                                              mask, L.p(st), s()), 'adam'), args.reps)
        row(set_name, 'FusedAdam', 'check', us_c, 4 * n)
        row(set_name, 'FusedAdam', 'adam', us_a, 40 * n + 2 * te)
    del g, m, v, e

    for N in (1, 2, 4, 8):
        # ---- reconstruction: whole arena, shard [0, c) ----
        geo = ShardGeometry(rows, MLP_PARAMS, 0xF, N, 0)
        c, n = geo.chunk, geo.n
        gs = torch.zeros(geo.padded, device=dev)
        ps = torch.zeros(geo.padded, device=dev)
        ps[:T].copy_(a)
        m, v, e = torch.zeros(c, device=dev), torch.zeros(c, device=dev), ps[:c].clone()
        us_z = timed(lambda: gs[c:].zero_(), args.reps) if N > 1 else 0.0
        us_c = timed(lambda: L.check(lib.nsr_grad_check(L.p(gs), n, 0xF, L.p(st), s()), 'grad_check'), args.reps)
        ho, hn = geo.half_own()
        us_a = timed(lambda: L.check(lib.nsr_adam_step_scaled(L.p(ps), L.p(gs), L.p(m), L.p(v), L.p(e), ptr(half, ho, 2), n, hn,
                                                              b1, b2, eps, 0xF, L.p(st), s()), 'adam'), args.reps)
        refresh = geo.half_refresh()

        def cast():
            for (o, k) in refresh:
                L.check(lib.nsr_cast_f32_to_f16(ptr(ps, o), ptr(half, o, 2), k, s()), 'cast')
        us_u = timed(cast, args.reps) if refresh else 0.0
        row('recon', N, 'zero', us_z, 4 * (geo.padded - c))
        row('recon', N, 'check', us_c, 4 * n)
        row('recon', N, 'adam', us_a, 40 * n + 2 * hn)
        row('recon', N, 'cast', us_u, 6 * sum(k for (_, k) in refresh))
        del gs, ps, m, v, e

        # ---- stylisation: colour lanes, rows [row_lo, row_hi) ----
        geo = ShardGeometry(rows, MLP_PARAMS, 0xC, N, 0)
        c, n = geo.chunk, geo.n
        ga = torch.zeros(T, device=dev)
        packed = torch.zeros(geo.padded, device=dev)
        m, v = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
        e = torch.zeros(2 * c, device=dev)
        nr = geo.row_hi - geo.row_lo

        def pack():
            L.check(lib.nsr_lanes_pack(L.p(ga), rows, 0xC, L.p(packed), s()), 'lanes_pack')
            ga[te:].zero_()
        us_p = timed(pack, args.reps)
        us_c = timed(lambda: L.check(lib.nsr_grad_check(L.p(packed), n, 0xF, L.p(st), s()), 'grad_check'), args.reps)
        us_a = timed(lambda: L.check(lib.nsr_lanes_adam_scaled(L.p(a), L.p(half), L.p(packed), L.p(m), L.p(v), L.p(e), L.p(packed),
                                                               geo.row_lo, geo.row_hi, 0xC, b1, b2, eps, L.p(st), s()),
                                     'lanes_adam'), args.reps)
        us_u = timed(lambda: L.check(lib.nsr_lanes_unpack(L.p(packed), geo.row_hi, rows, 0xC, L.p(a), L.p(half), s()),
                                     'lanes_unpack'), args.reps) if N > 1 else 0.0
        row('style', N, 'pack', us_p, 40 * rows + 4 * MLP_PARAMS)
        row('style', N, 'check', us_c, 4 * n)
        row('style', N, 'adam', us_a, 120 * nr)
        row('style', N, 'unpack', us_u, 48 * (rows - geo.row_hi))
        del ga, packed, m, v, e

    print('{:6s} {:>9s} {:7s} {:>9s} {:>9s} {:>7s}'.format('set', 'N', 'part', 'us', 'MB', 'HBM %'))
    for r in rows_out:
        print('{:6s} {:>9s} {:7s} {:9.2f} {:9.2f} {:>7s}'.format(r['set'], str(r['N']), r['part'], r['us'], r['MB'],
                                                              '-' if r['hbm_pct'] is None else '{:.1f}'.format(r['hbm_pct'])))
    totals = {}
    for r in rows_out:
        totals.setdefault((r['set'], str(r['N'])), 0.0)
        totals[(r['set'], str(r['N']))] += r['us']
    for (k, n), t in totals.items():
        print('total {:6s} N={:9s} {:9.2f} us  (+ reduce-scatter / all-gather on the links: not measured, no multi-GPU node)'.format(
            k, n, t))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'rows': rows_out, 'hbm_peak_Bps': HBM_PEAK}, f, indent=1)


if __name__ == '__main__':
    main()
