"""Deterministic weights of a DenoisingVDMUNet with downsampling_attention=True (dim 128, Fourier features 6..8).

The fixtures tests/golden/g16_unet_attn*.npz were computed by the reference with exactly these weights loaded; the weight
files w_unet_attn*.npz store the reference's state-dict key list, the shapes and a per-tensor fingerprint instead of ~20 MB
of parameters, and `unet_attn_weights` rebuilds the tensors bit for bit (seeded CPU generators).  Base keys come from
`oracle.unet_oracle.unet_random_weights`; every block's `res_attention` gets GroupNorm affine 1 + 0.05 N(0, 1) / 0.05 N(0, 1)
(as the reference-side fixtures perturb them) and convolutions U(-1/sqrt(fan_in), 1/sqrt(fan_in)), like nn.Conv2d's init."""
import math

import torch

DIM = 128
FF = (6, 8)


def block_prefixes(levels):
    return ([f"u_net.downsampling_blocks.{i}.0." for i in range(levels)] + ["u_net.center_block.0.", "u_net.center_block.2."] +
            [f"u_net.upsampling_blocks.{i}.0." for i in range(levels)])


def unet_attn_weights(data_shape, levels, seed):
    from oracle import unet_oracle as uo
    W = uo.unet_random_weights(data_shape, DIM, levels, seed=seed, ff=FF)
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


def fingerprint(W):
    """[n_keys, 4] fp64 (sum, sum |.|, first, last) in sorted key order."""
    return torch.stack([torch.stack((v.double().sum(), v.double().abs().sum(), v.flatten()[0].double(), v.flatten()[-1].double()))
                        for _, v in sorted(W.items())])


def fingerprint_matches(W, stored):
    """First and last elements exactly; the fp64 sums to 1e-12 (their summation order depends on the machine)."""
    fp = fingerprint(W)
    return fp.shape == stored.shape and torch.equal(fp[:, 2:], stored[:, 2:]) and torch.allclose(fp[:, :2], stored[:, :2], rtol=1e-12, atol=0)


SKETCH = 2048  # buckets of the gradient sketch; tensors up to this size are stored whole


def count_sketch(t, k=SKETCH):
    """Count sketch of a tensor (fp64 [k]): element i goes, with a sign, into one of k buckets, both from an integer hash of i (the
    same on every machine).  For any x, E ||sketch(x)||^2 = ||x||^2 with a relative standard deviation <= sqrt(2 / k) (3 % at
    k = 2048, 1.6 % on the norm), and sketch(a) - sketch(b) = sketch(a - b): the relative error of a gradient against a
    reference is estimated from the sketches alone."""
    x = t.detach().reshape(-1).double().cpu()
    i = torch.arange(x.numel(), dtype=torch.int64)
    h = (i * 2654435761 + 0x5BD1E995) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    h = ((h ^ (h >> 12)) * 0x297A2D39) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    sign = 1.0 - 2.0 * ((h >> 31) & 1).double()
    return torch.zeros(k, dtype=torch.float64).index_add_(0, h % k, sign * x)
