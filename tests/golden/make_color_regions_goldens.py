"""Generates tests/golden/color_regions_reference.npz: the reference's utils.match_colors_for_image_set
(utils/__init__.py:262-295) evaluated on the CPU once per matched (class, cluster) pair of a labelled content set and a
clustered style image, on that region's rows alone (reshaped to [1,1,n,3] and [1,n_s,3]), and once on all rows for the fallback
(run in the authoring container only; the reference does not travel).  The reference `utils` module is imported exactly as
make_color_match_goldens.py imports it.  The outputs are data only.

Two seeded cases, both F=3 frames of 33x47 photo-like content with 4 blocky classes and a 21x19 style image with 3 clusters,
min_rows = 64 (a cluster of the small style image holds 105..147 pixels):
  a_fallbacks   matching [1, 0, -1, 2]: class 2 is unmatched, class 3 holds 36 pixels (below min_rows), a strip is labelled -1
  b_shared      matching [2, 2, 0, 1]: classes 0 and 1 share cluster 2; class 3 again holds 36 pixels; some style pixels are
                unlabelled (-1)
Per case <name>: <name>_content [F,H,W,3] f32, <name>_classes [F,H,W] i32, <name>_style [h,w,3] f32, <name>_clusters [h,w] i32,
<name>_matching [4] i32, <name>_min_rows i32, <name>_tfs [5,4,4] f32 (the reference's color_tf per class; the all-rows one for
fallback classes and slot 4), <name>_image [F,H,W,3] f32 (every pixel from the reference's output for its region).

Also prints, per case, the distance of the test-side restatement (tests/color_regions_ref.py) from the reference's outputs: max
abs over A, over b and over the image.  The tolerances of tests/test_color_regions_cpu.py are four times the largest of each.

Usage: python tests/golden/make_color_regions_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import import_reference  # noqa: E402
from make_color_match_goldens import photo_like  # noqa: E402
import color_regions_ref as G  # noqa: E402

F, H, W, KC, KS, MIN_ROWS = 3, 33, 47, 4, 3, 64
PALETTE = np.array([[0.10, 0.00, -0.08], [-0.06, 0.08, 0.02], [0.00, -0.05, 0.12], [0.15, 0.10, 0.00]])
STYLE = np.array([[0.85, 0.35, 0.20], [0.15, 0.45, 0.80], [0.40, 0.75, 0.30]])


def class_maps(rng, with_unlabelled):
    """blocky maps: 11x12 blocks of classes 0..2 that shift from frame to frame, a 4x3 rectangle of class 3 per frame"""
    maps = np.empty((F, H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):
        table = rng.integers(0, 3, (3, 4))
        maps[f] = table[yy // 11, np.minimum((xx + 3 * f) // 12, 3)]
        y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 3))
        maps[f, y0:y0 + 4, x0:x0 + 3] = 3
        if with_unlabelled:
            maps[f, H - 1, : 10 + f] = -1
    return maps


def cases():
    rng = np.random.default_rng(2026)
    out = []
    for name, matching in (('a_fallbacks', [1, 0, -1, 2]), ('b_shared', [2, 2, 0, 1])):
        classes = class_maps(rng, name == 'a_fallbacks')
        content = photo_like(rng, F, H, W) + PALETTE[np.maximum(classes, 0)].astype(np.float32)
        content = np.clip(content, 0.0, 1.0).astype(np.float32)
        clusters = np.broadcast_to(np.minimum(np.arange(19) // 7, 2)[None, :], (21, 19)).astype(np.int32).copy()
        style = STYLE[clusters] * (0.5 + 0.5 * rng.random((21, 19, 1))) + 0.06 * rng.random((21, 19, 3))
        if name == 'b_shared':
            clusters[rng.random((21, 19)) < 0.05] = -1
        out.append((name, content, classes, np.clip(style, 0.0, 1.0).astype(np.float32), clusters, matching))
    return out


def main():
    _, _, utils, _ = import_reference()
    out = {}
    for name, content, classes, style, clusters, matching in cases():
        rows, srows = content.reshape(-1, 3), style.reshape(-1, 3)
        reg, sreg = G.region_of(classes.reshape(-1), KC), G.region_of(clusters.reshape(-1), KS)
        image, tf = utils.match_colors_for_image_set(torch.tensor(rows).view(1, 1, -1, 3), torch.tensor(srows).view(1, -1, 3))
        image, tfs = image.numpy().reshape(-1, 3).copy(), np.repeat(tf.numpy()[None], KC + 1, 0)
        matched = []
        for i, j in enumerate(matching):
            sel, ssel = reg == i, sreg == j
            if 0 <= j < KS and sel.sum() >= MIN_ROWS and ssel.sum() >= MIN_ROWS:
                im, tf = utils.match_colors_for_image_set(torch.tensor(rows[sel]).view(1, 1, -1, 3),
                                                          torch.tensor(srows[ssel]).view(1, -1, 3))
                image[sel], tfs[i] = im.numpy().reshape(-1, 3), tf.numpy()
                matched.append(i)
        assert image.dtype == np.float32 and tfs.dtype == np.float32
        out[name + '_content'], out[name + '_classes'] = content, classes
        out[name + '_style'], out[name + '_clusters'] = style, clusters
        out[name + '_matching'], out[name + '_min_rows'] = np.array(matching, np.int32), np.int32(MIN_ROWS)
        out[name + '_tfs'], out[name + '_image'] = tfs, image.reshape(content.shape)
        r_rows, r_tfs = G.match_by_region(rows, reg, KC, srows, sreg, KS, matching, MIN_ROWS, 'global')
        print('{:12s} matched {}  counts {} / {}  |dA| {:.3e}  |db| {:.3e}  |dimage| {:.3e}  clamped {:.2%}'.format(
            name, matched, np.bincount(reg, minlength=KC + 1).tolist(), np.bincount(sreg, minlength=KS + 1).tolist(),
            np.abs(r_tfs[:, :3, :3] - tfs[:, :3, :3]).max(), np.abs(r_tfs[:, :3, 3] - tfs[:, :3, 3]).max(),
            np.abs(r_rows - image).max(), float(np.mean((image == 0.0) | (image == 1.0)))))
    path = os.path.join(HERE, 'color_regions_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
