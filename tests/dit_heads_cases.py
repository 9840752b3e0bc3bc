"""The g20 fixtures of the DenoisingDiT with one head of 128 channels (tools/gen_golden_dit_heads.py): the calibration weights
w_dit_ff (dim 128, depth 2, patch 2, 3x16x16, Fourier features 6..8) run with heads=1."""
import functools

from tests.util import golden

SHAPE, PATCH, DIM, DEPTH, HEADS, FF = (3, 16, 16), 2, 128, 2, 1, (6, 8)


@functools.lru_cache(maxsize=None)
def train_fixture():
    """g20_dit_dh128_train with the gradients G.<key> of its train_g<i> files merged in (read once, shared, never written to)."""
    g = dict(golden("g20_dit_dh128_train"))
    for i in range(int(g["n_grad_files"])):
        part = golden(f"g20_dit_dh128_train_g{i}")
        assert not set(part) & set(g)
        g.update(part)
    return g
