"""Cost of the style-image k-means (nsr_kmeans_step; nerfstyle_amd/segment.py): one fused Lloyd step and the whole default call
(maximin init, 10 steps, compaction) on
  style     a 512 x 512 style image, [H,W,3], K = 8
  resident  a resident set's targets, 35 frames of 1008 x 756, [F,H*W,4], K = 8 and K = 64
each on two kinds of image:
  blocky   rectangles of 64 x 48 pixels around one of K colours each: what a painting looks like to a wave
  random   one of the K colours per pixel: every wave holds many clusters in every slot
against, in the same process with alternating windows,
  moments  nsr_color_moments on the same rows: the global colour pass, one read of the rows and no per-row search
  torch    the same step composed from torch: fp64 cdist, argmin, index_add_ (colour alone, no validity test, no fixed point)

  python tools/bench_kmeans.py
  python tools/bench_kmeans.py --repeats 20 --inner 5

Every figure is a median over `repeats` windows of `inner` back-to-back calls timed by device events, after a warm-up, with the
min / max of the windows beside it.  Bytes are counted from the shapes: a step reads the rows and writes 4 bytes a row.  Prints
one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_color_match import alternate  # noqa: E402


def image(kind, F, H, W, C, K, dev, g):
    palette = torch.rand(K, 3, device=dev, generator=g)
    if kind == 'random':
        lab = torch.randint(0, K, (F, H, W), device=dev, generator=g)
    else:
        by, bx = (H + 47) // 48, (W + 63) // 64
        lab = torch.randint(0, K, (F, by, bx), device=dev, generator=g).repeat_interleave(48, 1).repeat_interleave(64, 2)[:, :H, :W]
    rgb = palette[lab] + 0.03 * torch.randn(F, H, W, 3, device=dev, generator=g)
    if C == 4:
        rgb = torch.cat([rgb, torch.zeros(F, H, W, 1, device=dev)], 3)
    return rgb.reshape(F * H * W, C).contiguous()


def run(dev, kind, F, H, W, C, K, args, whole):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import segment as S
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rows = image(kind, F, H, W, C, K, dev, g)
    n = rows.shape[0]
    cent = S.kmeans_init(rows, K, H, W)
    lib, stream = L.lib(), L.stream()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    sums = torch.empty(K, 5, dtype=torch.int64, device=dev)
    new = torch.empty_like(cent)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.nsr_kmeans_step_workspace_bytes(n, K)) // 8, dtype=torch.float64, device=dev)
    gm = torch.empty(9, dtype=torch.float64, device=dev)
    gws = torch.empty(int(lib.nsr_color_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    pr, pc, pl, pn, ps, pnew, pst, pw, pg, pgw = (L.p(t) for t in (rows, cent, labels, counts, sums, new, stats, ws, gm, gws))

    def step():
        lib.nsr_kmeans_step(pr, n, C, H, W, 0.0, pc, K, pl, pl, pn, ps, pnew, pst, pw, stream)

    def moments():
        lib.nsr_color_moments(pr, n, C, pg, pgw, stream)

    def torch_step():
        x = rows[:, :3].double()
        lab = torch.cdist(x, cent[:, :3]).argmin(1)
        s = torch.zeros(K, 3, dtype=torch.float64, device=dev).index_add_(0, lab, x)
        c = torch.zeros(K, dtype=torch.float64, device=dev).index_add_(0, lab, torch.ones(n, dtype=torch.float64, device=dev))
        return s / c.clamp(min=1).unsqueeze(1)

    L.check(lib.nsr_kmeans_step(pr, n, C, H, W, 0.0, pc, K, None, pl, pn, ps, pnew, pst, pw, stream), 'kmeans_step')
    torch.cuda.synchronize()
    med, span = alternate({'step': step, 'moments': moments}, args.warmup, args.repeats, args.inner)
    med_t, span_t = alternate({'torch': torch_step}, 1, args.torch_repeats, 1)
    traffic = n * (C * 4 + 4)

    def entry(ms, sp, nbytes):
        return {'ms': round(ms, 4), 'ms_min_max': [round(sp[0], 4), round(sp[1], 4)], 'TBps': round(nbytes / (ms * 1e-3) / 1e12, 3)}

    out = {'step': entry(med['step'], span['step'], traffic), 'moments': entry(med['moments'], span['moments'], n * C * 4),
           'torch_step': entry(med_t['torch'], span_t['torch'], traffic),
           'step_over_moments': round(med['step'] / med['moments'], 2), 'torch_over_step': round(med_t['torch'] / med['step'], 1),
           'ns_per_row': round(med['step'] * 1e6 / n, 4)}
    if whole:
        view = rows.view(F, H, W, C)
        med_w, span_w = alternate({'whole': lambda: S.kmeans(view, K)}, 1, args.whole_repeats, 1)
        out['whole_call_ms'] = round(med_w['whole'], 3)
        out['whole_call_ms_min_max'] = [round(span_w['whole'][0], 3), round(span_w['whole'][1], 3)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=35)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=11, help='timed windows per candidate, alternating')
    ap.add_argument('--inner', type=int, default=3, help='back-to-back calls per window')
    ap.add_argument('--torch-repeats', type=int, default=3, help='timed single calls of the torch composition')
    ap.add_argument('--whole-repeats', type=int, default=3, help='timed whole default calls')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    for name, F, H, W, C, K in (('style_512_K8', 1, 512, 512, 3, 8), ('resident_K8', args.frames, 756, 1008, 4, 8),
                                ('resident_K64', args.frames, 756, 1008, 4, 64)):
        out[name] = {'rows': F * H * W, 'K': K}
        for kind in ('blocky', 'random'):
            out[name][kind] = run(dev, kind, F, H, W, C, K, args, whole=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
