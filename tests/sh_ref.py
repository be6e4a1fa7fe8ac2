"""Test-side reference of the view-dependent colour path: the degree-4 spherical-harmonics table in fp64 numpy and the
view-dependent model wiring, composed from the rounding-emulating MLP pieces of oracle/oracle.py and the fp32 autograd modules
of oracle/torch_port.py (neither is changed).  tiny-cuda-nn's convention: order and signs as in its SphericalHarmonics
encoding; written from general knowledge of it, parity with a tiny-cuda-nn build is unpinned."""
import math

import numpy as np
import torch

from oracle import torch_port as TP


def sh_ref(d):
    """[M,3] directions -> [M,16] fp64 coefficients."""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
        0.94617469575755997 * zz - 0.31539156525251999,
        -1.0925484305920792 * x * z, 0.54627421529603959 * (xx - yy),
        0.59004358992664352 * y * (-3 * xx + yy), 2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1 - 5 * zz), 0.3731763325901154 * z * (5 * zz - 3),
        0.45704579946446572 * x * (1 - 5 * zz), 1.4453057213202769 * z * (xx - yy),
        0.59004358992664352 * x * (-xx + 3 * yy)], axis=1)


def sh_torch(dirs):
    """fp32 torch tensor of the coefficients (no gradient: the path has no direction gradient)."""
    return torch.tensor(sh_ref(dirs.detach().cpu().numpy()), dtype=torch.float32)


def color2_vector(block, sh):
    """arena blocks ([6144] with a [64,16] first layer, [64,16] SH columns) -> the reference-shaped (7168,) vector whose first
    layer is row-major [64,32] = [color1 columns | SH columns]."""
    block, sh = np.asarray(block, np.float32), np.asarray(sh, np.float32)
    first = np.concatenate([block[:1024].reshape(64, 16), sh.reshape(64, 16)], axis=1).reshape(-1)
    return np.concatenate([first, block[1024:]])


def mlp_block(ref):
    """The 16384-float MLP block of the *_dirs entry points from a FieldDirs."""
    return np.concatenate([ref.p_density.detach().numpy(), ref.p_color1.detach().numpy(), ref.p_color2.detach().numpy(),
                           ref.p_class.detach().numpy(), ref.p_sh.detach().numpy()]).astype(np.float32)


class FieldDirs(TP.Field):
    """torch_port.Field with use_dir=True: color2 = mlp(cat(color1 output, SH(dirs)), 32 -> 64 -> 64 -> 3)."""

    def __init__(self, num_classes=5, seed=80000, table_scale=0.5):
        super().__init__(num_classes=num_classes, seed=seed, table_scale=table_scale)
        g = torch.Generator().manual_seed(seed + 17)
        self.p_sh = torch.nn.Parameter((torch.rand(64, 16, generator=g) * 2 - 1).reshape(-1) * math.sqrt(6.0 / (64 + 32)))

    def color2_params(self):
        first = torch.cat((self.p_color2[:1024].view(64, 16), self.p_sh.view(64, 16)), dim=1).reshape(-1)
        return torch.cat((first, self.p_color2[1024:]))

    def forward(self, pts, dirs, half=None, table_half=False):
        x = self.encoder_input(pts)
        ed = TP.quant(self.emb_density, 'f16') if table_half else self.emb_density
        xd = TP.grid_encode(x, ed, self.offsets, self.pls, base_resolution=self.min_res)
        sigmas = TP.TruncExp.apply(TP.mlp(xd, self.p_density, 32, 1, half=half))
        ec = TP.quant(self.emb_color, 'f16') if table_half else self.emb_color
        xc = TP.grid_encode(x, ec, self.offsets, self.pls, base_resolution=self.min_res)
        classes = TP.mlp(xc, self.p_class, 32, self.nc, half=half)
        c1 = TP.mlp(xc, self.p_color1, 32, 16, half=half)
        rgb = TP.mlp(torch.cat((c1, sh_torch(dirs)), dim=1), self.color2_params(), 32, 3, n_hidden_layers=2, out_act='sigmoid',
                     half=half)
        return torch.cat((rgb, classes), dim=1), sigmas


def field_forward_dirs(O, ref, pts, dirs, half=None, table_half=False):
    """oracle.field_forward's wiring with the direction input, numpy, roundings emulated by oracle.mlp_forward.
    Returns (rgbs|classes [M,3+nc], sigmas [M])."""
    fp = O.FieldParams(ref.emb_density.detach().numpy(), ref.emb_color.detach().numpy(), ref.p_density.detach().numpy(),
                       ref.p_color1.detach().numpy(), ref.p_color2.detach().numpy(), ref.p_class.detach().numpy(),
                       ref.offsets, ref.pls, num_classes=ref.nc)
    x = O.encoder_inputs(pts, fp.bound)
    ed = O.round_f16(fp.emb_density) if table_half else fp.emb_density
    xd = O.grid_encode_forward(x, ed, fp.offsets, fp.per_level_scale, fp.base_resolution, 0, True, 0)
    sigmas = np.exp(O.mlp_forward(xd, fp.p_density, 32, 1, 64, 1, 'none', half)[:, 0].astype(np.float32))
    ec = O.round_f16(fp.emb_color) if table_half else fp.emb_color
    xc = O.grid_encode_forward(x, ec, fp.offsets, fp.per_level_scale, fp.base_resolution, 0, True, 0)
    classes = O.mlp_forward(xc, fp.p_class, 32, fp.num_classes, 64, 1, 'none', half)
    c1 = O.mlp_forward(xc, fp.p_color1, 32, 16, 64, 1, 'none', half)
    x2 = np.concatenate([c1, sh_ref(dirs).astype(np.float32)], axis=1)
    rgb = O.mlp_forward(x2, color2_vector(fp.p_color2, ref.p_sh.detach().numpy()), 32, 3, 64, 2, 'sigmoid', half)
    return np.concatenate([rgb, classes], axis=1).astype(np.float32), sigmas
