"""Shard geometry of the sharded optimiser step (nerfstyle_amd/sharded_optim.py), host only: the shards partition the
trained elements, chunks are multiples of 16 floats, padding stays below world * 16, the packed-lane index maps round-trip,
and selections other than the reference trainers' two raise."""
import pytest
import torch

from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig
from nerfstyle_amd.sharded_optim import SHARD_ALIGN, ShardGeometry, ShardedFusedAdam, shard_chunk, trained_lane_mask
from nerfstyle_amd.style_nerf import StyleTCNerf


@pytest.fixture(scope='module', params=[None, torch.float32], ids=['f16_tables', 'f32_tables'])
def model(request):
    return StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=request.param, use_dir=False)


SETS = [(None, 0xF), (['x_color_embedder'], 0xC), (['x_density_embedder'], 0x3)]


@pytest.mark.parametrize('keywords,mask', SETS)
def test_shards_partition_the_trained_elements(model, keywords, mask):
    assert trained_lane_mask(model, keywords) == mask
    total = model.arena.numel() if mask == 0xF else 2 * model.rows
    for world in range(1, 9):
        geos = [ShardGeometry.of(model, keywords, world, k) for k in range(world)]
        c = geos[0].chunk
        assert c % SHARD_ALIGN == 0 and c == shard_chunk(total, world)
        assert geos[0].total == total and geos[0].padded == world * c
        assert 0 <= world * c - total < world * SHARD_ALIGN
        covered = 0
        for k, g in enumerate(geos):
            assert g.chunk == c and g.slot == k * c
            assert g.lo == covered and g.hi - g.lo == g.n <= c
            assert (g.lo, g.hi) == geos[0].bounds(k)
            covered = g.hi
            if mask != 0xF:
                assert g.lo % 2 == 0 and g.hi % 2 == 0 and 0 <= g.row_lo <= g.row_hi <= model.rows
        assert covered == total


@pytest.mark.parametrize('keywords,mask', SETS[1:])
def test_lane_index_maps_round_trip(model, keywords, mask):
    g = ShardGeometry.of(model, keywords, 3, 1)
    j = torch.arange(g.total, dtype=torch.int64)
    i = g.lane_to_arena(j)
    assert torch.equal(g.arena_to_lane(i), j)
    assert int(i.max()) < model.table_elems
    lanes = i % 4
    assert bool(((1 << lanes) & mask).bool().all())                # only trained lanes
    assert torch.equal(i.view(-1, 2) // 4, torch.arange(model.rows)[:, None].expand(-1, 2))
    # the rank's rows hold exactly its packed elements
    assert g.row_lo * 2 == g.lo and g.row_hi * 2 == g.hi


def test_half_copy_ranges_cover_the_tables(model):
    te = model.table_elems
    for world in range(1, 9):
        for k in range(world):
            g = ShardGeometry.of(model, None, world, k)
            seen = torch.zeros(te, dtype=torch.int32)
            for (o, n) in [g.half_own()] + g.half_refresh():
                assert o % 4 == 0 and n % 4 == 0          # 16-byte aligned fp32 / 8-byte aligned f16 pointers, whole rows
                seen[o:o + n] += 1
            assert bool((seen == 1).all()), (world, k)


@pytest.mark.parametrize('keywords', [['x_color_embedder', 'color2_net'], ['_net'], ['embedder'], ['density']])
def test_other_selections_raise(model, keywords):
    with pytest.raises(NotImplementedError, match='ShardedFusedAdam supports'):
        ShardedFusedAdam(model, keywords=keywords)


def test_unknown_keywords_still_raise_value_error(model):
    with pytest.raises(ValueError):
        ShardedFusedAdam(model, keywords=['no_such_parameter'])
