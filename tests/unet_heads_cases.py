"""Cases of the n_attention_heads fixtures (tests/golden/g18_unet_heads_*, written by tools/gen_golden_unet_heads.py) and the
deterministic weights they were computed with.

Weights do not depend on the head count (the centre Attention2D splits the same to_qkv channels into more heads), so one weight
file per (dim, levels) serves every head count: w_unet_heads_<tag>.npz stores the seed, the reference's state-dict key list, the
shapes and a per-tensor fingerprint; `heads_weights` rebuilds the tensors bit for bit."""
from tests.unet_attn_weights import FF, fingerprint_matches, unet_attn_weights

# weight tag -> (data shape, dim, levels, seed, downsampling_attention)
WEIGHTS = {
    "d128l1": ((3, 8, 8), 128, 1, 180, False),
    "d64l1": ((3, 8, 8), 64, 1, 181, False),
    "d128l2": ((3, 16, 16), 128, 2, 182, False),
    "blockattn": ((3, 8, 8), 128, 1, 183, True),
}
# forward fixture -> (weight tag, centre heads, batch, seed of the inputs)
FORWARD = {
    "g18_unet_heads_fwd_d128h8": ("d128l1", 8, 4, 184),
    "g18_unet_heads_fwd_d128h4": ("d128l1", 4, 4, 185),
    "g18_unet_heads_fwd_d64h4": ("d64l1", 4, 4, 186),
    "g18_unet_heads_fwd2": ("d128l2", 8, 4, 187),
    "g18_unet_heads_blockattn": ("blockattn", 8, 4, 188),
}
TRAIN = ("g18_unet_heads_train", "d128l1", 8, 4, 189)
HIST = ("g18_unet_heads_hist", "d128l1", 8, 2, 16, 191)  # name, weights, heads, n, k, seed


def heads_weights(tag):
    shape, dim, levels, seed, block_attn = WEIGHTS[tag]
    if block_attn:
        return unet_attn_weights(shape, levels, seed)
    from oracle import unet_oracle as uo
    return uo.unet_random_weights(shape, dim, levels, seed=seed, ff=FF)


def checked_weights(tag, stored):
    """The weights of `tag`, checked against the stored fixture (tests.util.golden('w_unet_heads_' + tag))."""
    assert int(stored["seed"]) == WEIGHTS[tag][3]
    W = heads_weights(tag)
    assert fingerprint_matches(W, stored["fingerprint"]), "the weight recipe no longer reproduces the fixture's weights"
    return W
