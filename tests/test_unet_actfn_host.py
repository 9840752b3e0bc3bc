"""Host-side contract of DenoisingVDMUNet(actfn=...) (no GPU): the reference's five activation names construct with the silu model's
state dict (ActFn modules have no parameters), unknown names raise KeyError as actfn_from_str does, padding_mode stays refused, and
the activation codes and the appended C-ABI fields are declared in include/bsi_hip.h and mirrored in bsi_amd._native."""
import os
import re

import pytest
import torch

from tests.util import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ("silu", "gelu", "relu", "softplus", "tanh")


def build(actfn, padding_mode="zeros"):
    """The model of tests/golden/w_unet_ff.npz (dim 64, levels 1, 3x8x8, Fourier features 6..8, dropout slot)."""
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    return DenoisingVDMUNet((3, 8, 8), NyquistPositionalEmbedding(32, 100), actfn, 64, 1, 4, n_attention_heads=1, dropout=0.1,
                            fourier_features=FourierFeatures(n_min=6, n_max=8), padding_mode=padding_mode)


@pytest.mark.parametrize("actfn", ACTS)
def test_every_reference_actfn_constructs_with_the_same_state_dict(actfn):
    from bsi_amd import _native as N
    ref = build("silu").state_dict()
    m = build(actfn)
    sd = m.state_dict()
    assert list(sd) == list(ref)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ref.values()]
    m.load_state_dict(weights("unet_ff"), strict=True)  # the reference's checkpoint keys load unchanged
    assert m._act_code == N.ACT_CODES[actfn]
    acts = [type(mod).__name__ for mod in m.modules() if isinstance(mod, (torch.nn.SiLU, torch.nn.GELU, torch.nn.ReLU, torch.nn.Softplus,
                                                                            torch.nn.Tanh))]
    assert acts and len(set(acts)) == 1  # the same ActFn at every site (pos_map and residual blocks)


def test_unknown_actfn_raises_keyerror_and_padding_mode_stays_refused():
    with pytest.raises(KeyError):
        build("mish")
    with pytest.raises(NotImplementedError, match="padding_mode"):
        build("gelu", padding_mode="reflect")


def test_header_activation_codes_equal_python_constants():
    from bsi_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "bsi_hip.h")).read()
    codes = dict((k, int(v)) for k, v in re.findall(r"BSI_ACT_(\w+)\s*=\s*(\d+)", hdr))
    assert codes == {"NONE": N.ACT_NONE, "SILU": N.ACT_SILU, "GELU": N.ACT_GELU, "RELU": N.ACT_RELU, "SOFTPLUS": N.ACT_SOFTPLUS,
                     "TANH": N.ACT_TANH}
    assert {k: v for k, v in N.ACT_CODES.items()} == {"silu": 1, "gelu": 2, "relu": 3, "softplus": 4, "tanh": 5}
    for name in ("bsi_act_bf16", "bsi_act_bwd_bf16", "bsi_film_act", "bsi_film_act_bwd"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in N.EXPORTS


def test_header_and_ctypes_fields():
    from bsi_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "bsi_hip.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"\**\s*(\w+)\s*[,;]", body)

    assert fields("bsi_unet_weights")[-1] == "actfn"
    assert fields("bsi_conv_args")[-1] == "act"
    assert fields("bsi_unet_config")[-1] == "block_heads"  # not appended to: the per-block attention test pins it
    for cls, struct in ((N.UNetWeights, "bsi_unet_weights"), (N.ConvArgs, "bsi_conv_args")):
        assert [f[0] for f in cls._fields_] == fields(struct), struct
    assert N.UNetWeights().actfn == 0 and N.ConvArgs().act == 0  # zero-initialised callers: SiLU


@pytest.mark.parametrize("actfn", ("gelu", "softplus"))
def test_lightning_checkpoint_of_non_silu_model_round_trips(actfn):
    from bsi_amd import drivers
    W = weights("unet_ff")
    src, ema = build(actfn), build(actfn)
    src.load_state_dict(W)
    ema.load_state_dict({k: v * 0.5 for k, v in W.items()})
    ck = {"state_dict": drivers.to_lightning_state_dict(src, ema, ema_step=3)}
    a, b = build(actfn), build(actfn)
    drivers.load_lightning_checkpoint(ck, a, b)
    for k, v in W.items():
        assert torch.equal(a.state_dict()[k], v) and torch.equal(b.state_dict()[k], v * 0.5), k
    assert a.actfn == actfn and b._act_code == src._act_code
