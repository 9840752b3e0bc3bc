"""Host-side contract of DenoisingVDMUNet(n_attention_heads=N) (no GPU): the state dict does not depend on the head count and
equals the reference's key list and shapes (tests/golden/w_unet_heads_*.npz), the weight recipe reproduces the stored fingerprints,
and the engine configuration carries the argument."""
import pytest
import torch

from tests.unet_attn_weights import FF
from tests.unet_heads_cases import FORWARD, HIST, TRAIN, WEIGHTS, checked_weights
from tests.util import golden


def build(tag, heads):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    shape, dim, levels, _, block_attn = WEIGHTS[tag]
    return DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=heads, dropout=0.1,
                            downsampling_attention=block_attn, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_state_dict_independent_of_heads_and_equal_to_reference(tag):
    w = golden("w_unet_heads_" + tag)
    keys = bytes(w["keys"].numpy()).decode().split("\n")
    shapes = [tuple(int(s) for s in row[:int(n)]) for row, n in zip(w["shapes"].tolist(), w["ndim"].tolist())]
    dim = WEIGHTS[tag][1]
    for heads in (1, 2, 4, 8, 16, 3):
        if dim % heads == 0 or heads == 3:
            sd = build(tag, heads).state_dict()
            assert list(sd) == keys, heads
            assert [tuple(v.shape) for v in sd.values()] == shapes, heads


@pytest.mark.parametrize("tag", list(WEIGHTS))
def test_weight_recipe_reproduces_fingerprint_and_loads(tag):
    W = checked_weights(tag, golden("w_unet_heads_" + tag))
    m = build(tag, 8)
    m.load_state_dict(W, strict=True)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in W.items())


@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_config_carries_heads(heads):
    cfg = build("d128l1", heads)._config()
    assert cfg.heads == heads and cfg.dim == 128 and cfg.block_heads == 0
    m = build("d128l1", heads)
    assert m.u_net.center_block[1].fn[1].heads == heads
    cfg = build("blockattn", heads)._config()
    assert cfg.heads == heads and cfg.block_heads == 4


def test_fixtures_name_their_cases():
    """Every fixture records the head count of its case; the train fixture has a norm and a gradient or sketch for every parameter
    of the model, and nothing else."""
    for name, (tag, heads, B, _) in FORWARD.items():
        g = golden(name)
        assert int(g["heads"]) == heads and tuple(g["mu"].shape) == (B, *WEIGHTS[tag][0]) and g["out64"].dtype == torch.float64
        if name != "g18_unet_heads_fwd2":
            assert float(g["t"][0]) == 0.0
    name, tag, heads, n, k, _ = HIST
    g = golden(name)
    assert int(g["heads"]) == heads and int(g["k"]) == k and tuple(g["x_hats"].shape) == (k + 1, n, *WEIGHTS[tag][0])
    name, tag, heads, B, _ = TRAIN
    g = golden(name)
    params = [k for k, _ in build(tag, heads).named_parameters()]
    assert sorted(k[2:] for k in g if k.startswith("N.")) == sorted(params)
    assert sorted(k[2:] for k in g if k[:2] in ("G.", "K.")) == sorted(params)
    assert int(g["heads"]) == heads and tuple(g["loss"].shape) == (B,)
