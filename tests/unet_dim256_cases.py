"""Cases of the dim-256 fixtures (tests/golden/g19_unet_dim256_*, written by tools/gen_golden_unet_dim256.py) and the deterministic
weights they were computed with.

w_unet_dim256_<tag>.npz stores the seed, the reference's state-dict key list, the shapes and a per-tensor fingerprint instead of the
parameters (18 to 46 MB at this width); `dim256_weights` rebuilds the tensors bit for bit.  Base keys come from
`oracle.unet_oracle.unet_random_weights`; the per-block attention case adds the `res_attention` keys by the recipe of
tests/unet_attn_weights.py (which is written for dim 128) at dim 256."""
import math

import torch

from tests.unet_attn_weights import FF, block_prefixes, fingerprint_matches

DIM = 256
# weight tag -> (data shape, levels, seed, downsampling_attention)
WEIGHTS = {
    "d256l1": ((3, 8, 8), 1, 200, False),      # HW 64: ring convolution, row-FiLM epilogue, unfused GroupNorm
    "d256l2": ((3, 16, 16), 2, 201, False),    # HW 256: slab convolutions, fused FiLM epilogue, fused GroupNorm statistics (512-channel merge)
    "d256attn": ((3, 8, 8), 1, 202, True),     # per-block Attention2D at head dim 64
}
# forward fixture -> (weight tag, centre heads, actfn, batch, seed of the inputs, t[0] = 0)
FORWARD = {
    "g19_unet_dim256_fwd_h2": ("d256l1", 2, "silu", 4, 203, True),
    "g19_unet_dim256_fwd_h4": ("d256l1", 4, "silu", 4, 204, True),
    "g19_unet_dim256_fwd_h16": ("d256l1", 16, "silu", 4, 205, True),
    "g19_unet_dim256_fwd2": ("d256l2", 8, "silu", 4, 206, False),
    "g19_unet_dim256_attn": ("d256attn", 8, "silu", 4, 207, True),
    "g19_unet_dim256_fwd_gelu": ("d256l1", 4, "gelu", 4, 208, True),
}
# train fixture -> (weight tag, centre heads, actfn, batch, seed)
TRAIN = {
    "g19_unet_dim256_train": ("d256l1", 4, "silu", 4, 209),
    "g19_unet_dim256_train2": ("d256l2", 8, "silu", 4, 211),
    "g19_unet_dim256_train_gelu": ("d256l1", 4, "gelu", 4, 213),
}
# buckets of a fixture's gradient sketches (tests.unet_attn_weights.count_sketch; default SKETCH = 2048).  The levels-2 model has 36
# sketched tensors: 1536 buckets keep its file under 400 KB; the estimate of a gradient's relative error then has a relative
# standard deviation of sqrt(2 / 1536) = 3.6 % instead of 3.1 %, far inside the distance of the achieved errors from their bound.
SKETCH_BUCKETS = {"g19_unet_dim256_train2": 1536}
HIST = ("g19_unet_dim256_hist", "d256l1", 4, 2, 16, 215)  # name, weights, heads, n, k, seed


def dim256_weights(tag):
    from oracle import unet_oracle as uo
    shape, levels, seed, block_attn = WEIGHTS[tag]
    W = uo.unet_random_weights(shape, DIM, levels, seed=seed, ff=FF)
    if block_attn:
        g = torch.Generator().manual_seed(seed + 1000)
        for pfx in block_prefixes(levels):
            a = pfx + "res_attention.fn."
            W[a + "0.weight"] = 1 + 0.05 * torch.randn(DIM, generator=g)
            W[a + "0.bias"] = 0.05 * torch.randn(DIM, generator=g)
            for name, cout in (("1.to_qkv", 3 * DIM), ("1.to_out", DIM)):
                bound = 1 / math.sqrt(DIM * 9)
                W[a + name + ".weight"] = (torch.rand((cout, DIM, 3, 3), generator=g) * 2 - 1) * bound
                W[a + name + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound
    return W


_CHECKED = {}


def checked_weights(tag, stored):
    """The weights of `tag`, checked against the stored fixture (tests.util.golden('w_unet_dim256_' + tag)); built once per process."""
    if tag not in _CHECKED:
        assert int(stored["seed"]) == WEIGHTS[tag][2]
        W = dim256_weights(tag)
        assert fingerprint_matches(W, stored["fingerprint"]), "the weight recipe no longer reproduces the fixture's weights"
        _CHECKED[tag] = W
    return _CHECKED[tag]
