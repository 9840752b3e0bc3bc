"""Pin the CPU oracle at patch 8 (decoder width 192, encoder width 1344) against the reference's g21 fixtures
(tools/gen_golden_dit_patch.py) with the bounds tests/test_dit_heads_host.py uses, check the weight recipe and the fixture sizes,
and measure the fp32 oracle against the fp64 one on the geometries the GPU tests compare with the fp64 oracle alone.  CPU only."""
import math
import os

import pytest
import torch

from oracle import bsi_oracle as bo
from oracle import dit_oracle as do
from tests import dit_patch_cases as pc
from tests.unet_attn_weights import count_sketch
from tests.util import GOLDEN, golden, max_rel, rel_l2, rel_linf

FIXTURES = ["w_dit_patch8", *pc.FWD, "g21_dit_patch8_train", "g21_dit_patch8_train_encw", "g21_dit_patch8_train_k",
            "g21_dit_patch8_hist", "g21_dit_patch8_hist_out"]


def dit_f(W, heads):
    return lambda mu, t: do.dit_forward(W, mu, t, patch_size=pc.PATCH, dim=pc.DIM, depth=pc.DEPTH, heads=heads, ff=pc.FF)


def test_weight_recipe_reproduces_the_fingerprint():
    W = pc.checked_weights()
    assert int(golden("w_dit_patch8")["n_keys"]) == len(W)
    assert W["dit.patch_encoder.weight"].shape == (pc.DIM, 1344) and W["dit.patch_decoder.1.weight"].shape == (192, pc.DIM)


@pytest.mark.parametrize("name", FIXTURES)
def test_every_fixture_file_is_below_one_mib(name):
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20


@pytest.mark.parametrize("name", list(pc.FWD))
def test_forward_patch8(name):
    heads, _ = pc.FWD[name]
    g = golden(name)
    assert int(g["heads"]) == heads and g["mu"].shape == (2, *pc.SHAPE)
    W = pc.checked_weights()
    with torch.no_grad():
        y = dit_f(W, heads)(g["mu"], g["t"])
        y64 = dit_f({k: v.double() for k, v in W.items()}, heads)(g["mu"].double(), g["t"].double())
    assert rel_linf(y, g["out"]) < 2e-5, rel_linf(y, g["out"])
    assert rel_linf(y64, g["out64"]) < 1e-10, rel_linf(y64, g["out64"])


def test_the_two_head_counts_differ():
    a, b = golden("g21_dit_patch8_fwd"), golden("g21_dit_patch8_fwd_h2")
    with torch.no_grad():
        y1 = dit_f(pc.checked_weights(), 1)(b["mu"], b["t"])
    assert not torch.equal(a["mu"], b["mu"]) and rel_linf(y1, b["out"]) > 1e-3


def test_train_loss_and_gradients_patch8():
    g = pc.train_fixture()
    B = pc.TRAIN_B
    W = {k: v.clone().requires_grad_(True) for k, v in pc.checked_weights().items()}
    o = bo.BSIOracle(dit_f(W, pc.TRAIN_HEADS), data_shape=pc.SHAPE, k=16, discretization=bo.Disc.image_8bit())
    loss = o.train_loss(g["x"], g["offset"], g["perm"], g["eps"])
    assert max_rel(loss, g["loss"]) < 2e-5, max_rel(loss, g["loss"])
    assert abs(float(loss.mean()) / float(g["loss_mean"]) - 1) < 1e-5
    loss.mean().backward()
    sq = 0.0
    for k, v in W.items():
        sq += float((v.grad.double() ** 2).sum())
        if "G." + k in g:
            assert rel_linf(v.grad, g["G." + k]) < 2e-3, (k, rel_linf(v.grad, g["G." + k]))
        else:
            ref = g["K." + k]
            err = float((count_sketch(v.grad, ref.numel()) - ref).norm()) / float(g["N." + k])
            assert err < 2e-3, (k, err)
        assert abs(float(v.grad.double().norm()) / float(g["N." + k]) - 1) < 2e-3, k
    assert set(W) == {k[2:] for k in g if k.startswith("N.")}
    assert {k[2:] for k in g if k.startswith("G.")} >= {k for k in W if k.startswith(pc.WHOLE)}
    assert abs(math.sqrt(sq) / float(g["grad_norm"]) - 1) < 1e-4
    W64 = {k: v.double() for k, v in pc.checked_weights().items()}
    o64 = bo.BSIOracle(dit_f(W64, pc.TRAIN_HEADS), data_shape=pc.SHAPE, k=16, dtype=torch.float64, discretization=bo.Disc.image_8bit())
    lam = o64.p_lambda.icdf(torch.remainder(g["perm"].double() / (1 + B) + g["offset"].double(), 1))
    mu = o64.q_mu_lambda(g["x"].double(), lam, g["eps"].double())
    with torch.no_grad():
        xh = o64.predict_x(mu, o64.p_lambda.cdf(lam))
    loss64 = o64.p_lambda.reciprocal_pdf(lam) * (g["x"].double() - xh).square().flatten(1).mean(1)
    assert max_rel(loss64, g["loss_fp64"]) < 1e-9


def test_sample_history_patch8():
    """Teacher-forced, as tests/test_dit_heads_host.py does with Fourier features."""
    g = pc.hist_fixture()
    assert int(g["heads"]) == pc.HIST_HEADS and int(g["k"]) == pc.HIST_K
    o = bo.BSIOracle(dit_f(pc.checked_weights(), pc.HIST_HEADS), data_shape=pc.SHAPE, k=pc.HIST_K, discretization=bo.Disc.image_8bit())
    with torch.no_grad():
        mus, xh, ys = o.sample_history(g["eps0"], g["eps"], teacher_mus=g["mus"])
    assert mus.shape == g["mus"].shape and xh.shape == g["x_hats"].shape and ys.shape == g["ys"].shape
    for a, b, n in [(mus, g["mus"], "mu"), (xh, g["x_hats"], "x_hat"), (ys, g["ys"], "y")]:
        for i in range(a.shape[0]):
            assert rel_linf(a[i], b[i]) < 1e-4, (n, i, rel_linf(a[i], b[i]))


def test_backward_workspace_grows_with_the_decoder_width():
    """bsi_dit_backward_workspace_bytes accounts for everything that scales with P: the decoder weight gradient [Pp, dim] fp32, the
    bf16 operand dYb [M, Pp] and the per-workgroup bias sums.  Two models that differ in the channel count only (P 64 and 192, no
    Fourier features, so that the encoder's 64 / 192 columns stay below 4 dim and the weight-gradient slabs are the same)."""
    import ctypes as C
    from bsi_amd import _native as N
    lib = N.lib()
    B, dim, tokens = 2, 128, 64
    size = {c: lib.bsi_dit_backward_workspace_bytes(C.byref(N.DitConfig(c, 64, 64, 8, dim, 1, 1, 1, 0)), B) for c in (1, 3)}
    M, dP = B * tokens, 192 - 64
    assert size[3] - size[1] >= dP * dim * 4 + M * dP * 2 + 2 * dP * 4, size
    # patch 8 with Fourier features on a narrow model: the encoder's weight gradient [dim, 1344] is the widest one, its split slabs
    # (bsi_gemm_tn_workspace_bytes) must fit
    cfg = N.DitConfig(3, 64, 64, 8, dim, 1, 1, 6, 8)
    assert lib.bsi_dit_kpad(C.byref(cfg)) == 1344
    assert lib.bsi_dit_backward_workspace_bytes(C.byref(cfg), B) >= lib.bsi_gemm_tn_workspace_bytes(M, dim, 1344)


def test_geometries_cover_the_widths_the_kernels_branch_on():
    P = {t: s[0] * p * p for t, (s, p, *_) in pc.GEOMETRIES.items()}
    assert P == {"c8p3": 72, "p7": 147, "c4p8": 256, "d64": 192, "wide": 192}
    assert {(p + 63) // 64 for p in P.values()} == {2, 3, 4}            # every per-lane count past one
    assert any(p % 4 for p in P.values()) and any(p % 8 for p in P.values())  # the odd bias path, a padded Pp
    assert any(p > pc.GEOMETRIES[t][3] for t, p in P.items())            # wider than the residual stream
    for t, (shape, patch, ff, dim, heads, _) in pc.GEOMETRIES.items():
        assert (shape[1] // patch) * (shape[2] // patch) == 64 and dim // heads in (64, 128), t


@pytest.mark.parametrize("tag", list(pc.GEOMETRIES))
def test_fp32_oracle_error_is_a_factor_below_the_bounds(tag):
    """The GPU tests hold these geometries to the fp64 oracle; the bounds mean something only where fp32 arithmetic itself stays far
    inside them.  Checked here: the fp32 oracle against the fp64 one, ORACLE_MARGIN below every bound."""
    y64, l64, G64 = pc.geometry_oracle(tag, True)
    y32, l32, G32 = pc.geometry_oracle(tag, False)
    m = pc.ORACLE_MARGIN
    assert rel_linf(y32, y64) < pc.X_HAT / m, rel_linf(y32, y64)
    assert abs(float(l32.mean()) / float(l64.mean()) - 1) < pc.LOSS_MEAN / m
    assert max_rel(l32, l64) < pc.LOSS_SAMPLE / m
    for k in G64:
        assert rel_l2(G32[k], G64[k]) < pc.GRAD / m, (k, rel_l2(G32[k], G64[k]))
