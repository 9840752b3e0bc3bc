"""Host-side contract of DenoisingVDMUNet(downsampling_attention=True) (no GPU): the state dict equals the reference's key
list and shapes (tests/golden/w_unet_attn_l*.npz), dim 64 is refused, and the appended C-ABI fields are declared and mirrored."""
import os
import re

import pytest
import torch

from tests.unet_attn_weights import FF, fingerprint_matches, unet_attn_weights
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(shape, levels, dim=128, attention=True):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    return DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=1, dropout=0.1,
                            downsampling_attention=attention, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))


@pytest.mark.parametrize("levels,shape", [(1, (3, 8, 8)), (2, (3, 16, 16))])
def test_state_dict_matches_reference_keys_and_shapes(levels, shape):
    w = golden(f"w_unet_attn_l{levels}")
    keys = bytes(w["keys"].numpy()).decode().split("\n")
    shapes = [tuple(int(s) for s in row[:int(n)]) for row, n in zip(w["shapes"].tolist(), w["ndim"].tolist())]
    sd = build(shape, levels).state_dict()
    assert list(sd) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    for pfx in ([f"u_net.downsampling_blocks.{i}.0" for i in range(levels)] + ["u_net.center_block.0", "u_net.center_block.2"] +
                [f"u_net.upsampling_blocks.{i}.0" for i in range(levels)]):
        for k in ("fn.0.weight", "fn.0.bias", "fn.1.to_qkv.weight", "fn.1.to_qkv.bias", "fn.1.to_out.weight", "fn.1.to_out.bias"):
            assert f"{pfx}.res_attention.{k}" in sd
    # the recipe that stands in for stored weights reproduces what the reference ran with, and loads strictly
    W = unet_attn_weights(shape, levels, int(w["seed"]))
    assert fingerprint_matches(W, w["fingerprint"])
    build(shape, levels).load_state_dict(W, strict=True)


def test_lightning_checkpoint_with_ema_loads():
    from bsi_amd import drivers
    src = build((3, 8, 8), 1)
    W = unet_attn_weights((3, 8, 8), 1, 160)
    src.load_state_dict(W)
    ema = build((3, 8, 8), 1)
    ema.load_state_dict({k: v * 0.5 for k, v in W.items()})
    ck = {"state_dict": drivers.to_lightning_state_dict(src, ema, ema_step=3)}
    a, b = build((3, 8, 8), 1), build((3, 8, 8), 1)
    drivers.load_lightning_checkpoint(ck, a, b)
    for k, v in W.items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v * 0.5), k


def test_dim_64_refused():
    with pytest.raises(NotImplementedError, match="head dim 16"):
        build((3, 8, 8), 1, dim=64)
    build((3, 8, 8), 1, dim=64, attention=False)  # the default stays available


def test_header_and_ctypes_fields():
    from bsi_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "bsi_hip.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"\**\s*(\w+)\s*[,;]", body)

    assert fields("bsi_unet_config")[-1] == "block_heads"
    assert fields("bsi_unet_resblock_weights")[-6:] == ["agn_w", "agn_b", "aqkv_w", "aqkv_b", "aout_w", "aout_b"]
    assert fields("bsi_unet_resblock_weights_t")[-2:] == ["aqkv_wT", "aout_wT"]
    assert fields("bsi_unet_resblock_grads")[-6:] == ["agn_w", "agn_b", "aqkv_w", "aqkv_b", "aout_w", "aout_b"]
    for cls, struct in ((N.UNetConfig, "bsi_unet_config"), (N.UNetResBlockWeights, "bsi_unet_resblock_weights"),
                        (N.UNetResBlockWeightsT, "bsi_unet_resblock_weights_t"), (N.UNetResBlockGrads, "bsi_unet_resblock_grads")):
        assert [f[0] for f in cls._fields_] == fields(struct), struct
    cfg = build((3, 8, 8), 1)._config()
    assert cfg.block_heads == 4 and build((3, 8, 8), 1, attention=False)._config().block_heads == 0
