"""Cases of the DenoisingDiT at decoder widths P = patch^2 * C in (64, 256]: the g21 fixtures of the patch-8 model
(tests/golden/g21_dit_patch8_*, written by tools/gen_golden_dit_patch.py) with the deterministic weights they were computed with,
and the geometries without a reference fixture, which the tests compare with the fp64 CPU oracle.

w_dit_patch8.npz stores the seed and a per-tensor fingerprint instead of the parameters (the patch encoder alone is 128 x 1344);
`patch8_weights` rebuilds the tensors bit for bit from `oracle.dit_oracle.dit_random_weights`."""
import functools

import torch

from tests.unet_attn_weights import fingerprint_matches
from tests.util import golden

# the fixture model: 3x64x64 at patch 8 = 64 tokens of P = 192 decoder columns; with Fourier features 6..8 the encoder reads
# kin = 64 * 21 = 1344 columns per token (a multiple of 64: no padding)
SHAPE, PATCH, DIM, DEPTH, FF, SEED = (3, 64, 64), 8, 128, 2, (6, 8), 2108
TRAIN_B, TRAIN_SEED, TRAIN_HEADS = 2, 2110, 1
FWD = {"g21_dit_patch8_fwd": (1, 2111), "g21_dit_patch8_fwd_h2": (2, 2112)}  # fixture -> (heads, seed of the inputs)
HIST_N, HIST_K, HIST_SEED, HIST_HEADS = 1, 4, 2113, 1
WHOLE = ("dit.patch_decoder.", "dit.patch_encoder.")  # gradients stored whole: the tensors whose kernels depend on P and kin
ENC_W = "dit.patch_encoder.weight"                    # 688 KB: a file of its own


def patch8_weights():
    from oracle import dit_oracle as do
    return do.dit_random_weights(SHAPE, PATCH, DIM, DEPTH, ff=FF, seed=SEED)


@functools.lru_cache(maxsize=None)
def checked_weights():
    """The fixture model's weights, checked against the stored fingerprint (built once per process, never written to)."""
    stored = golden("w_dit_patch8")
    assert int(stored["seed"]) == SEED
    W = patch8_weights()
    assert fingerprint_matches(W, stored["fingerprint"]), "the weight recipe no longer reproduces the fixture's weights"
    return W


@functools.lru_cache(maxsize=None)
def train_fixture():
    """g21_dit_patch8_train with the encoder weight gradient and the sketches of its side files merged in."""
    g = dict(golden("g21_dit_patch8_train"))
    for side in ("g21_dit_patch8_train_encw", "g21_dit_patch8_train_k"):
        part = golden(side)
        assert not set(part) & set(g)
        g.update(part)
    return g


@functools.lru_cache(maxsize=None)
def hist_fixture():
    g = dict(golden("g21_dit_patch8_hist"))
    g.update(golden("g21_dit_patch8_hist_out"))
    return g


# Geometries without a reference fixture.  tag: (shape, patch, Fourier features, dim, heads, seed); depth 1, batch 2.
#   c8p3    P = 72: the first width past 64 (two columns per lane, the second one nearly empty); kin 72 padded to 128
#   p7      P = 147: odd, padded to Pp = 152 in the weight-gradient operand, bias gradient through the P % 4 != 0 copy; kin 147 -> 192
#   c4p8    P = 256: the upper edge, four columns per lane; the decoder weights (128 KB) no longer fit the backward's LDS stage
#   d64     P = 192 > dim = 64: dYb wider than a row of the residual stream; the d <= 256 instances at another width
#   wide    3x32x128, non-square token grid, at kin 1344 with Fourier features
GEOMETRIES = {
    "c8p3": ((8, 24, 24), 3, None, 128, 1, 41),
    "p7": ((3, 56, 56), 7, None, 128, 1, 42),
    "c4p8": ((4, 64, 64), 8, None, 128, 1, 43),
    "d64": ((3, 64, 64), 8, None, 64, 1, 44),
    "wide": ((3, 32, 128), 8, (6, 8), 128, 1, 45),
}
GEO_B, GEO_DEPTH = 2, 1
# the fp32 oracle's own distance from the fp64 one has to stay this factor below every bound the GPU results are held to
ORACLE_MARGIN = 10.0
X_HAT, LOSS_MEAN, LOSS_SAMPLE, GRAD = 1e-2, 1e-4, 1e-3, 1e-2


def geometry_inputs(tag):
    """(W, mu, t, x, offset, perm, eps) of a geometry: seeded CPU draws."""
    from oracle import dit_oracle as do
    shape, patch, ff, dim, _, seed = GEOMETRIES[tag]
    W = do.dit_random_weights(shape, patch, dim, GEO_DEPTH, ff=ff, seed=seed)
    g = torch.Generator().manual_seed(seed + 500)
    mu = torch.randn((GEO_B, *shape), generator=g) * 2
    t = torch.rand(GEO_B, generator=g)
    x = (torch.round(255 * torch.rand((GEO_B, *shape), generator=g)) / 255) * 2 - 1
    off = torch.rand((), generator=g)
    perm = torch.randperm(GEO_B, generator=g)
    eps = torch.randn((GEO_B, *shape), generator=g)
    return W, mu, t, x, off, perm, eps


@functools.lru_cache(maxsize=None)
def geometry_oracle(tag, double):
    """Forward, per-sample train loss and every parameter gradient of the CPU oracle at fp64 (`double`) or fp32.
    Returns (y, loss, {name: grad}); computed once per process and shared."""
    from oracle import bsi_oracle as bo
    from oracle import dit_oracle as do
    shape, patch, ff, dim, heads, _ = GEOMETRIES[tag]
    W, mu, t, x, off, perm, eps = geometry_inputs(tag)
    dt = torch.float64 if double else torch.float32
    Wr = {k: v.to(dt).requires_grad_(True) for k, v in W.items()}
    f = lambda a, b: do.dit_forward(Wr, a, b, patch_size=patch, dim=dim, depth=GEO_DEPTH, heads=heads, ff=ff)  # noqa: E731
    with torch.no_grad():
        y = f(mu.to(dt), t.to(dt))
    loss = bo.BSIOracle(f, data_shape=shape, k=16, dtype=dt).train_loss(x.to(dt), off.to(dt), perm.to(dt), eps.to(dt))
    loss.mean().backward()
    return y, loss.detach(), {k: v.grad for k, v in Wr.items()}
