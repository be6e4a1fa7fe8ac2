"""Generates tests/golden/color_match_reference.npz: the reference's utils.match_colors_for_image_set
(utils/__init__.py:262-295) evaluated on the CPU on seeded inputs (run in the authoring container only; the reference does not
travel).  The reference `utils` module is imported exactly as make_goldens.py imports it.  The outputs are data only.

Per case <name>: <name>_content [N,H,W,3] f32, <name>_style [h,w,3] f32 (case c reuses case b's content), <name>_image
[N,H,W,3] f32 the returned image set, <name>_tf [4,4] f32 the returned color_tf.

Also prints, per case, the distance of the test-side restatement (tests/color_match_ref.py: fp64 moments and solve, f32 fma
chain) from the reference's outputs: max abs over A, over b and over the image, and the share of outputs at the clamp.  The
tolerances of tests/test_color_match_cpu.py are four times the largest of each.

Usage: python tests/golden/make_color_match_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import import_reference  # noqa: E402
import color_match_ref as R  # noqa: E402


def photo_like(rng, n, h, w):
    """a grey ramp plus channel noise plus offsets: one large and two small eigenvalues of the covariance"""
    ramp = np.linspace(0.1, 0.8, h * w).reshape(1, h, w, 1) * (0.7 + 0.3 * rng.random((n, 1, 1, 1)))
    img = ramp + 0.03 * rng.standard_normal((n, h, w, 3)) + np.array([0.05, 0.0, -0.04])
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def cases():
    rng = np.random.default_rng(2025)
    out = []
    out.append(('a_uniform', rng.random((3, 5, 7, 3)).astype(np.float32), rng.random((6, 9, 3)).astype(np.float32)))
    content_b = photo_like(rng, 4, 33, 47)
    warm = rng.random((21, 19, 1)) * np.array([0.9, 0.6, 0.3]) + 0.08 * rng.random((21, 19, 3))
    out.append(('b_photo', content_b, warm.astype(np.float32)))
    grey = np.repeat(rng.random((8, 8, 1)), 3, axis=2).astype(np.float32)
    out.append(('c_grey_style', content_b, grey))
    # a narrow, bell-shaped content palette stretched onto a style that fills the unit cube: the tails leave [0, 1]
    narrow = np.clip(0.5 + 0.08 * rng.standard_normal((2, 16, 20, 3)), 0.0, 1.0).astype(np.float32)
    out.append(('d_clamped', narrow, rng.random((12, 10, 3)).astype(np.float32)))
    return out


def main():
    _, _, utils, _ = import_reference()
    out = {}
    for name, content, style in cases():
        image, tf = utils.match_colors_for_image_set(torch.tensor(content), torch.tensor(style))
        image, tf = image.numpy(), tf.numpy()
        assert image.dtype == np.float32 and tf.dtype == np.float32 and image.shape == content.shape and tf.shape == (4, 4)
        if name != 'c_grey_style':
            out[name + '_content'] = content
        out[name + '_style'] = style
        out[name + '_image'] = image
        out[name + '_tf'] = tf
        r_image, r_tf = R.match(content, style)
        clamped = float(np.mean((image == 0.0) | (image == 1.0)))
        print('{:14s} |dA| {:.3e}  |db| {:.3e}  |dimage| {:.3e}  clamped {:.2%}'.format(
            name, np.abs(r_tf[:3, :3] - tf[:3, :3]).max(), np.abs(r_tf[:3, 3] - tf[:3, 3]).max(), np.abs(r_image - image).max(), clamped))
    path = os.path.join(HERE, 'color_match_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
