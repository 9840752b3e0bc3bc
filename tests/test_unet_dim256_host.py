"""Host-side contract of DenoisingVDMUNet(dim=256) (no GPU): the state dicts of the three fixture models equal the reference's key
lists and shapes (tests/golden/w_unet_dim256_*.npz), the weight recipes reproduce the stored fingerprints and load strictly, the
engine configuration carries the width, downsampling_attention=True is accepted at 256 and refused at 64 and 96, a Lightning
checkpoint of the per-block-attention model round-trips, and the workspace sizes are answered without a device."""
import ctypes as C

import pytest
import torch

from tests.unet_attn_weights import FF, SKETCH
from tests.unet_dim256_cases import DIM, FORWARD, HIST, SKETCH_BUCKETS, TRAIN, WEIGHTS, checked_weights
from tests.util import golden


def build(tag, heads=4, dim=DIM, attention=None):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    shape, levels, _, block_attn = WEIGHTS[tag]
    return DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=heads, dropout=0.1,
                            downsampling_attention=block_attn if attention is None else attention,
                            fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_state_dict_equals_reference_and_recipe_loads(tag):
    w = golden("w_unet_dim256_" + tag)
    keys = bytes(w["keys"].numpy()).decode().split("\n")
    shapes = [tuple(int(s) for s in row[:int(n)]) for row, n in zip(w["shapes"].tolist(), w["ndim"].tolist())]
    for heads in (1, 2, 4, 8, 16, 3):  # the state dict does not depend on the head count
        sd = build(tag, heads).state_dict()
        assert list(sd) == keys, heads
        assert [tuple(v.shape) for v in sd.values()] == shapes, heads
    W = checked_weights(tag, w)
    m = build(tag, 8)
    m.load_state_dict(W, strict=True)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in W.items())


def test_config_carries_dim_and_block_heads():
    for heads in (2, 4, 8, 16):
        cfg = build("d256l1", heads)._config()
        assert cfg.dim == 256 and cfg.heads == heads and cfg.block_heads == 0 and cfg.levels == 1
    cfg = build("d256attn", 8)._config()
    assert cfg.dim == 256 and cfg.heads == 8 and cfg.block_heads == 4
    cfg = build("d256l2", 8)._config()
    assert cfg.dim == 256 and cfg.levels == 2 and (cfg.H, cfg.W) == (16, 16)


def test_downsampling_attention_accepted_at_256_refused_at_64_and_96():
    m = build("d256attn")
    assert m._blocks()[0].res_attention.fn[1].heads == 4  # head dim 64
    build("d256attn", dim=128)
    with pytest.raises(NotImplementedError, match="head dim 16"):
        build("d256attn", dim=64)
    with pytest.raises(NotImplementedError, match="head dim 24"):
        build("d256attn", dim=96)
    build("d256l1", dim=64)   # without per-block attention every width still builds, as in the reference
    build("d256l1", dim=96, heads=3)


def test_lightning_checkpoint_round_trip_with_block_attention():
    from bsi_amd import drivers
    tag = "d256attn"
    W = checked_weights(tag, golden("w_unet_dim256_" + tag))
    src, ema = build(tag, 8), build(tag, 8)
    src.load_state_dict(W)
    ema.load_state_dict({k: v * 0.5 for k, v in W.items()})
    ck = {"state_dict": drivers.to_lightning_state_dict(src, ema, ema_step=3)}
    a, b = build(tag, 8), build(tag, 8)
    drivers.load_lightning_checkpoint(ck, a, b)
    for k, v in W.items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v * 0.5), k


def test_fixtures_name_their_cases():
    """Every forward fixture records its head count and has fp64 outputs; every train fixture has a norm and a gradient or a sketch
    for every parameter of its model, and nothing else."""
    for name, (tag, heads, _, B, _, t0_zero) in FORWARD.items():
        g = golden(name)
        assert int(g["heads"]) == heads and tuple(g["mu"].shape) == (B, *WEIGHTS[tag][0]) and g["out64"].dtype == torch.float64
        assert (float(g["t"][0]) == 0.0) == t0_zero
    name, tag, heads, n, k, _ = HIST
    g = golden(name)
    assert int(g["heads"]) == heads and int(g["k"]) == k and tuple(g["x_hats"].shape) == (k + 1, n, *WEIGHTS[tag][0])
    for name, (tag, heads, _, B, _) in TRAIN.items():
        g = golden(name)
        params = [k for k, _ in build(tag, heads).named_parameters()]
        assert sorted(k[2:] for k in g if k.startswith("N.")) == sorted(params)
        assert sorted(k[2:] for k in g if k[:2] in ("G.", "K.")) == sorted(params)
        assert int(g["heads"]) == heads and tuple(g["loss"].shape) == (B,)
        assert {v.numel() for k, v in g.items() if k.startswith("K.")} == {SKETCH_BUCKETS.get(name, SKETCH)}


def _sizes(tag, dim, B):
    from bsi_amd import _native as N
    lib = N.lib()
    cfg = build(tag, 4, dim=dim)._config()
    return (lib.bsi_unet_workspace_bytes(C.byref(cfg), B), lib.bsi_unet_tape_bytes(C.byref(cfg), B),
            lib.bsi_unet_backward_workspace_bytes(C.byref(cfg), B))


@pytest.mark.parametrize("tag", ["d256l1", "d256l2"])
def test_workspace_sizes_need_no_device_and_grow_with_dim(tag):
    """The three sizes are positive at dim 256 and larger than at dim 128 (same B and image); the call needs no device."""
    for B in (1, 4):
        big, small = _sizes(tag, 256, B), _sizes(tag, 128, B)
        assert all(b > s > 0 for b, s in zip(big, small)), (big, small)


def test_workspace_bytes_at_least_twice_dim128():
    """bsi_unet_workspace_bytes at dim 256 is at least twice the dim-128 value at the same B and image (the engine reserves the two
    width-independent regions, the bf16 input and the zero bytes, in proportion to the width above dim 128), and the dim-128 and
    dim-64 sizes are what the layout gives without that."""
    for tag in ("d256l1", "d256l2"):
        for B in (1, 4):
            big, small = _sizes(tag, 256, B)[0], _sizes(tag, 128, B)[0]
            assert big > 0
            assert big >= 2 * small, (tag, B, big, small, big / small)
            assert big <= 2 * small + 4096, (tag, B, big, small)  # and no more than the alignment of a few buffers above it
