"""View-dependent colour, host side: the SH table's constants, the new C-ABI symbols, the larger arena and its checkpoints."""
import os
import re

import numpy as np
import pytest
import torch

from sh_ref import sh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(view_dependent, **kw):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    return StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, None, view_dependent=view_dependent, **kw)


def test_sh_table_is_orthonormal():
    """Gauss-Legendre in cos(theta) with 8 nodes x 16 uniform phi integrates these degree <= 6 products exactly."""
    mu, w = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5) * (2 * np.pi / 16)
    st = np.sqrt(1 - mu ** 2)
    d = np.stack([(st[:, None] * np.cos(phi)[None]).ravel(), (st[:, None] * np.sin(phi)[None]).ravel(),
                  np.repeat(mu, 16)], axis=1)
    wt = np.repeat(w, 16) * (2 * np.pi / 16)
    Y = sh_ref(d)
    gram = (Y * wt[:, None]).T @ Y
    assert np.abs(gram - np.eye(16)).max() <= 1e-9


def _header_params(src, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', re.sub(r'/\*.*?\*/', '', src, flags=re.S), re.S)
    assert m, name
    return [p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']


def test_new_symbols_header_and_ctypes_agree():
    from nerfstyle_amd import _lib, build
    build.build()
    src = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    for name, n in (('nsr_field_mlp_param_count', 1), ('nsr_field_forward_uses_lattice', 3), ('nsr_sh_encode', 4), ('nsr_field_forward_dirs', 12),
                    ('nsr_field_backward_dirs', 17)):
        assert len(_header_params(src, name)) == len(_lib.SIGNATURES[name][1]) == n, name
    # the plain entry points keep their signatures
    assert len(_header_params(src, 'nsr_field_forward')) == len(_lib.SIGNATURES['nsr_field_forward'][1]) == 11
    assert len(_header_params(src, 'nsr_field_backward')) == len(_lib.SIGNATURES['nsr_field_backward'][1]) == 16
    L = _lib.lib()
    assert L.nsr_field_mlp_param_count(0) == 15360 and L.nsr_field_mlp_param_count(1) == 16384
    assert L.nsr_sh_encode(None, 0, None, None) == 0 and L.nsr_sh_encode(None, 4, None, None) != 0


def test_arena_and_checkpoint_round_trip():
    m = _model(True)
    assert m.use_dir is True
    assert m.arena.numel() == m.rows * 4 + 16384
    assert _model(False).arena.numel() == m.rows * 4 + 15360
    sd = m.state_dict()
    assert sd['color2_net.params'].shape == (7168,) and m.color2_net.params.shape == (7168,)
    # the reference-shaped first layer is [64, 32]: columns 0..15 the arena's [64,16] block, 16..31 the appended SH block
    mlp = m.arena.detach()[m.table_elems:]
    first = sd['color2_net.params'][:2048].view(64, 32)
    assert torch.equal(first[:, :16].reshape(-1), mlp[6144:7168]) and torch.equal(first[:, 16:].reshape(-1), mlp[15360:])
    assert torch.equal(sd['color2_net.params'][2048:], mlp[7168:12288])
    # initialised from init_mlp_params(32, 3, 64, 2, seed + 2)
    from nerfstyle_amd.network import init_mlp_params
    assert torch.equal(sd['color2_net.params'], init_mlp_params(32, 3, 64, 2, int(m.cfg.network_seed or 0) + 2))
    g = torch.Generator().manual_seed(3)
    new = {k: (torch.rand(v.shape, generator=g) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    m2 = _model(True)
    m2.load_state_dict(new)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, new[k]), k
    # every other offset of the MLP block is where a direction-less model has it
    assert torch.equal(m2.arena.detach()[m2.table_elems + 12288: m2.table_elems + 15360], new['class_net.params'])


def test_checkpoint_mismatch_names_the_switch():
    plain, vd = _model(False), _model(True)
    with pytest.raises(ValueError, match='view_dependent'):
        vd.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match='view_dependent'):
        plain.load_state_dict(vd.state_dict())


def test_use_dir_alone_still_raises_and_names_the_keyword():
    with pytest.raises(NotImplementedError, match='view_dependent'):
        _model(False, use_dir=True)
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.style_nerf import SHEncoder, StyleTCNerf
    with pytest.raises(NotImplementedError):
        StyleTCNerf(NetworkConfig(dir_enc_sh_deg=3), BBox.from_radius(2.0), 5, view_dependent=True)
    with pytest.raises(NotImplementedError):
        SHEncoder(3)


def test_optimiser_regions_cover_the_sh_block():
    from nerfstyle_amd.optim import select_regions
    from nerfstyle_amd.sharded_optim import trained_lane_mask
    vd = _model(True)
    assert (15360, 1024) in select_regions(vd, None)[1] and (15360, 1024) in select_regions(vd, ['color2_net'])[1]
    assert (15360, 1024) not in select_regions(vd, ['color1_net'])[1]
    assert len(select_regions(_model(False), None)[1]) == 4
    # the sharded optimiser does not know the fifth block: a refusal that names the switch
    with pytest.raises(NotImplementedError, match='view_dependent'):
        trained_lane_mask(vd, None)


def test_lattice_forward_is_chosen_with_directions():
    """The direction-taking lattice kernel fits four workgroups per CU on the default grid, like the direction-less one."""
    import ctypes
    from nerfstyle_amd import _lib, build
    build.build()
    L = _lib.lib()
    for vd in (False, True):
        m = _model(vd)
        d = m._desc(1.0)
        assert L.nsr_field_forward_uses_lattice(ctypes.byref(d), 1, int(vd)) == 1
        assert L.nsr_field_forward_uses_lattice(ctypes.byref(d), 0, int(vd)) == 0
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m32 = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, torch.float32, view_dependent=True)
    d = m32._desc(1.0)
    assert L.nsr_field_forward_uses_lattice(ctypes.byref(d), 1, 1) == 0            # fp32 tables: the gather kernel
