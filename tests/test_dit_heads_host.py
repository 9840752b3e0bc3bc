"""Pin the CPU oracle at ONE head of 128 channels against the reference's g20 fixtures (tools/gen_golden_dit_heads.py), with the
bounds tests/test_oracle_golden.py uses for g7_dit_fwd, g4_train_dit and g5_hist_dit_ff -- before anything on the GPU is compared
with the oracle at this head count.  CPU only."""
import math

import torch

from oracle import bsi_oracle as bo
from oracle import dit_oracle as do
from tests.dit_heads_cases import DEPTH, DIM, FF, HEADS, PATCH, SHAPE, train_fixture
from tests.util import golden, max_rel, rel_linf, sub, weights


def dit_f(W):
    return lambda mu, t: do.dit_forward(W, mu, t, patch_size=PATCH, dim=DIM, depth=DEPTH, heads=HEADS, ff=FF)


def make(f, k=16, dtype=torch.float32):
    return bo.BSIOracle(f, data_shape=SHAPE, k=k, dtype=dtype, discretization=bo.Disc.image_8bit())


def test_forward_one_head():
    g = golden("g20_dit_dh128_fwd")
    assert int(g["heads"]) == HEADS and g["mu"].shape[0] == 4
    W = weights("dit_ff")
    with torch.no_grad():
        y = dit_f(W)(g["mu"], g["t"])
        y64 = dit_f({k: v.double() for k, v in W.items()})(g["mu"].double(), g["t"].double())
    assert rel_linf(y, g["out"]) < 2e-5, rel_linf(y, g["out"])
    assert rel_linf(y64, g["out64"]) < 1e-10, rel_linf(y64, g["out64"])
    # one head is not two: the fixture differs from what the same weights give with two heads of 64
    with torch.no_grad():
        y2 = do.dit_forward(W, g["mu"], g["t"], patch_size=PATCH, dim=DIM, depth=DEPTH, heads=2, ff=FF)
    assert rel_linf(y2, g["out"]) > 1e-3


def test_train_loss_and_gradients_one_head():
    g = train_fixture()
    src = golden("g4_train_dit")
    for k in ("x", "offset", "perm", "eps"):
        assert torch.equal(g[k], src[k]), k
    W = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in weights("dit_ff").items()}
    o = make(dit_f(W))
    loss = o.train_loss(g["x"], g["offset"], g["perm"], g["eps"])
    assert max_rel(loss, g["loss"]) < 2e-5, max_rel(loss, g["loss"])
    assert abs(float(loss.mean()) / float(g["loss_mean"]) - 1) < 1e-5
    loss.mean().backward()
    G = sub(g, "G.")
    assert set(G) == {k for k, v in W.items() if v.requires_grad}
    sq = 0.0
    for k, ref in G.items():
        got = W[k].grad
        sq += float((got.double() ** 2).sum())
        assert rel_linf(got, ref) < 2e-3, (k, rel_linf(got, ref))
    assert abs(math.sqrt(sq) / float(g["grad_norm"]) - 1) < 1e-4
    # the fp64 oracle against the fp64 reference run on the same draws
    W64 = {k: v.double() for k, v in weights("dit_ff").items()}
    o64 = make(dit_f(W64), dtype=torch.float64)
    lam = o64.p_lambda.icdf(torch.remainder(g["perm"].double() / (1 + 4) + g["offset"].double(), 1))
    mu = o64.q_mu_lambda(g["x"].double(), lam, g["eps"].double())
    with torch.no_grad():
        xh = o64.predict_x(mu, o64.p_lambda.cdf(lam))
    loss64 = o64.p_lambda.reciprocal_pdf(lam) * (g["x"].double() - xh).square().flatten(1).mean(1)
    assert max_rel(loss64, g["loss_fp64"]) < 1e-9


def test_sample_history_one_head():
    """Teacher-forced as g5_hist_dit_ff (Fourier features amplify a last-bit difference of mu along a free-running trajectory)."""
    g = golden("g20_dit_dh128_hist")
    assert int(g["heads"]) == HEADS
    o = make(dit_f(weights("dit_ff")), k=int(g["k"]))
    with torch.no_grad():
        mus, xh, ys = o.sample_history(g["eps0"], g["eps"], teacher_mus=g["mus"])
    assert mus.shape == g["mus"].shape and xh.shape == g["x_hats"].shape and ys.shape == g["ys"].shape
    for a, b, n in [(mus, g["mus"], "mu"), (xh, g["x_hats"], "x_hat"), (ys, g["ys"], "y")]:
        for i in range(a.shape[0]):
            assert rel_linf(a[i], b[i]) < 1e-4, (n, i, rel_linf(a[i], b[i]))
