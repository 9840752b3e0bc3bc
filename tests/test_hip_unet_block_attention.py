"""DenoisingVDMUNet(downsampling_attention=True): Residual(GroupNorm -> Attention2D) after every residual block
(bsi/nn/residual_block.py:50-64 of the reference), 4 heads of 32 channels at dim 128, on the HIP engines.

Kernels at head dim 32 against fp64 softmax attention; the model against the reference's fixtures (tools/gen_golden_unet_attn.py,
tests/golden/g16_*); the CIFAR-10 geometry against an fp64 restatement; reproducibility, a DPTrainer step, and the default
(no per-block attention) UNet's bits against a fresh process that runs the same thing."""
import contextlib
import math
import os
import subprocess
import sys
from unittest import mock

import pytest
import torch

from tests.unet_attn_weights import FF, count_sketch, unet_attn_weights
from tests.util import bound, golden, rel_linf, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BF16 = 0x7FC1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nan_filled(rows, cols):
    return torch.full((rows, cols), NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def attn_ref(qkv, dh):
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    B, T, _, H, _ = qkv.shape
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, T, H * dh), torch.logsumexp(sc, -1)


# ----------------------------------------------------------------------------------------------
# kernels at head dim 32
# ----------------------------------------------------------------------------------------------
FWD = [(t, h) for t in (64, 128, 192, 256, 320, 1024) for h in (1, 4)]


@pytest.mark.parametrize("tokens,heads", FWD, ids=[f"t{t}_h{h}" for t, h in FWD])
def test_attention_dh32_forward(N, tokens, heads):
    """Resident path (<= 256 tokens), 128-key chunks (tokens % 128 == 0) and 64-key chunks (320); bounds of
    test_attention_forward_sequence_lengths."""
    B, dh = 2, 32
    d = heads * dh
    gen = torch.Generator().manual_seed(tokens * 7 + heads)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.5)
    ref, ref_lse = attn_ref(qkv, dh)
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    out = nan_filled(B * tokens, d)
    N.check(N.lib().bsi_attention_fwd(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.stream()))
    o = out.cpu().double().reshape(B, tokens, d)
    err, mean = rel_linf(o, ref), float((o - ref).abs().mean() / ref.abs().mean())
    assert err < 1e-2 and mean < 4e-3, (err, mean)
    out2, lse = nan_filled(B * tokens, d), torch.full((B, heads, tokens), float("nan"), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out2), d, N.ptr(lse), N.stream()))
    assert torch.equal(out2.view(torch.int16).cpu(), out.view(torch.int16).cpu()), "the log-sum-exp variant changed the output"
    lse_err = float((lse.cpu().double() - ref_lse).abs().max())
    assert lse_err < 2e-3, lse_err
    report("attention_dh32_fwd", tokens=tokens, heads=heads, rel_linf=err, rel_mean=mean, lse_abs=lse_err)


@pytest.mark.parametrize("tokens", [192, 320, 1024])
def test_attention_dh32_padded_rows(N, tokens):
    """ld_qkv = 3*d + 64, ld_out = d + 64: NaN in the input's padding does not leak in, the output's padding keeps its bits."""
    B, heads, dh = 2, 4, 32
    d = heads * dh
    ldq, ldo = 3 * d + 64, d + 64
    gen = torch.Generator().manual_seed(tokens + 11)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.5)
    ref, _ = attn_ref(qkv, dh)
    buf = torch.full((B * tokens, ldq), float("nan"), dtype=torch.bfloat16)
    buf[:, :3 * d] = qkv.reshape(B * tokens, 3 * d).to(torch.bfloat16)
    dq = buf.to(DEV)
    for with_lse in (False, True):
        out = nan_filled(B * tokens, ldo)
        if with_lse:
            lse = torch.empty((B, heads, tokens), device=DEV)
            N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), ldq, B, tokens, heads, dh, N.ptr(out), ldo, N.ptr(lse), N.stream()))
        else:
            N.check(N.lib().bsi_attention_fwd(N.ptr(dq), ldq, B, tokens, heads, dh, N.ptr(out), ldo, N.stream()))
        o = out[:, :d].cpu().double().reshape(B, tokens, d)
        assert rel_linf(o, ref) < 1e-2
        assert bool((out[:, d:].cpu().view(torch.int16) == NAN_BF16).all()), "columns past heads*dh were written"


@pytest.mark.parametrize("tokens,heads", [(64, 4), (192, 1), (256, 4), (320, 4), (1024, 4)])
def test_attention_dh32_backward_long(N, tokens, heads):
    """bsi_attention_bwd_long at head dim 32 against fp64 autograd (bounds of test_attention_backward_sequence_lengths)."""
    B, dh = 2, 32
    d = heads * dh
    gen = torch.Generator().manual_seed(tokens * 5 + heads)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.2)
    dout = bf16r(torch.randn((B, tokens, d), generator=gen))
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    out = torch.empty((B, tokens, d), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, heads, tokens), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.ptr(lse), N.stream()))
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, tokens, d).backward(dout.double())
    dqkv = torch.full((B, tokens, 3 * d), float("nan"), dtype=torch.bfloat16, device=DEV)
    dd = dout.to(torch.bfloat16).to(DEV)
    N.check(N.lib().bsi_attention_bwd_long(N.ptr(dq), 3 * d, N.ptr(out), N.ptr(dd), d, N.ptr(lse), B, tokens, heads, dh, N.ptr(dqkv),
                                           3 * d, N.stream()))
    got = dqkv.cpu().float().reshape(B, tokens, 3, heads, dh)
    errs = {}
    for i, nm in enumerate("qkv"):
        errs[nm] = rel_linf(got[:, :, i], x.grad[:, :, i])
        errs[nm + "_mean"] = float((got[:, :, i].double() - x.grad[:, :, i]).abs().mean() / x.grad[:, :, i].abs().mean())
        assert errs[nm] < 1.5e-2 and errs[nm + "_mean"] < 6e-3, (nm, errs)
    report("attention_dh32_bwd", tokens=tokens, heads=heads, **errs)


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
def make_model(shape, levels, W=None, seed=None, dropout=0.1):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", 128, levels, 4, n_attention_heads=1, dropout=dropout,
                         downsampling_attention=True, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))
    m.load_state_dict(W if W is not None else unet_attn_weights(shape, levels, seed))
    return m.to(DEV).eval()


def fixture_model(levels, shape):
    w = golden(f"w_unet_attn_l{levels}")
    from tests.unet_attn_weights import fingerprint_matches
    W = unet_attn_weights(shape, levels, int(w["seed"]))
    assert fingerprint_matches(W, w["fingerprint"]), "the weight recipe no longer reproduces the fixture's weights"
    return make_model(shape, levels, W)


def make_bsi(model, shape, k=16):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


@contextlib.contextmanager
def replay_noise(**queues):
    """Feed recorded CPU draws to torch.rand/randn/randperm, in order."""
    qs = {k: list(v) for k, v in queues.items()}

    def pop(name):
        def f(*a, **kw):
            return qs[name].pop(0).to(kw.get("device", DEV))
        return f

    with contextlib.ExitStack() as st:
        for name in qs:
            st.enter_context(mock.patch.object(torch, name, side_effect=pop(name)))
        yield


@pytest.mark.parametrize("case,levels,shape", [("g16_unet_attn_fwd1", 1, (3, 8, 8)), ("g16_unet_attn_fwd2", 2, (3, 16, 16))])
def test_forward_vs_reference(case, levels, shape):
    g = golden(case)
    m = fixture_model(levels, shape)
    with torch.no_grad():
        y = m(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
    err = rel_linf(y, g["out64"])
    report("unet_block_attn_fwd", case=case, rel_linf=err, ref_fp32_vs_fp64=rel_linf(g["out"], g["out64"]))
    bound(f"test_forward_vs_reference:{case}", err, 1e-2)


def test_sampling_vs_reference():
    """Teacher-forced through the reference's sample_history: x_hat of every step from the reference's mu of that step.  (Free
    running, the 8-bit discretisation turns bf16-level differences of x_hat into whole-bin differences of the next mu.)"""
    g = golden("g16_unet_attn_hist")
    k = int(g["k"])
    bsi = make_bsi(fixture_model(1, (3, 8, 8)), (3, 8, 8), k=k)
    t = bsi.default_schedule
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    worst = 0.0
    with torch.no_grad():
        for i in range(k + 1):
            mu_i = g["mus"][i].to(DEV)
            e = rel_linf(bsi._predict_x(mu_i, t_eval[i].repeat(mu_i.shape[0])), g["x_hats"][i])
            worst = max(worst, e)
            bound(f"test_sampling_vs_reference:step{i}", e, 1e-2)
        s = bsi.sample(2, torch.Generator(DEV).manual_seed(0))
    assert torch.isfinite(s).all()
    report("unet_block_attn_hist", worst=worst)


def test_train_loss_gradients_vs_reference():
    """train_loss + .mean().backward() through the HIP training engine vs the reference: loss per sample, every parameter
    gradient (every res_attention tensor included) by relative norm -- exact for tensors up to SKETCH elements, estimated from
    count sketches (~2 %) above."""
    g = golden("g16_unet_attn_train")
    model = fixture_model(1, (3, 8, 8))
    bsi = make_bsi(model, (3, 8, 8))
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = bsi.train_loss(g["x"].to(DEV))
    bound("test_train_loss_gradients_vs_reference:loss", float(((loss.detach().cpu() - g["loss"]).abs() / g["loss"].abs()).max()), 1e-3)
    loss.mean().backward()
    worst, n_attn = (0.0, None), 0
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        ref_norm = float(g["N." + name])
        if "G." + name in g:  # small tensors: the reference gradient itself
            ref = g["G." + name].double()
            assert p.grad.shape == ref.shape, name
            err = float((p.grad.cpu().double() - ref).norm()) / max(ref_norm, 1e-30)
        else:  # count sketches: ||sketch(g) - sketch(ref)|| estimates ||g - ref|| to ~2 % (tests/unet_attn_weights.py)
            err = float((count_sketch(p.grad) - g["K." + name]).norm()) / max(ref_norm, 1e-30)
        worst = max(worst, (err, name))
        n_attn += "res_attention" in name
        bound("test_train_loss_gradients_vs_reference:grad", err, 1e-2)
    assert n_attn == 4 * 6, n_attn
    report("unet_block_attn_grads", worst=worst[0], worst_name=worst[1])


def restated_forward(W, mu, t, levels):
    """fp64 restatement of the reference's forward with downsampling_attention=True: every residual block is followed by
    x + to_out(SDPA(to_qkv(GroupNorm(x)))) with 4 heads (attention.py:32-41, residual_block.py:61-64)."""
    from oracle import unet_oracle as uo
    from oracle.unet_oracle import fourier_features, nyquist_embedding
    W = {k: v.double() for k, v in W.items()}
    F = torch.nn.functional

    def res_attn(x, pre):
        a = F.group_norm(x, 32, W[pre + "res_attention.fn.0.weight"], W[pre + "res_attention.fn.0.bias"], 1e-5)
        qkv = F.conv2d(a, W[pre + "res_attention.fn.1.to_qkv.weight"], W[pre + "res_attention.fn.1.to_qkv.bias"], padding=1)
        b, _, h, w = x.shape
        q, k, v = qkv.reshape(b, 3, 4, 32, h * w).permute(1, 0, 2, 4, 3)
        o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32), -1) @ v  # [b, heads, hw, 32]
        o = o.permute(0, 1, 3, 2).reshape(b, 128, h, w)
        return x + F.conv2d(o, W[pre + "res_attention.fn.1.to_out.weight"], W[pre + "res_attention.fn.1.to_out.bias"], padding=1)

    def block(x, c, pre):
        return res_attn(uo.residual_block(x, c, W, pre, has_dropout_slot=True), pre)

    mu, t = mu.double(), t.double()
    x = torch.cat([mu, fourier_features(mu, FF[0], FF[1], dim=1)], dim=1)
    c = F.silu(F.linear(nyquist_embedding(t, 32, 100), W["pos_map.1.weight"], W["pos_map.1.bias"]))
    c = F.silu(F.linear(c, W["pos_map.3.weight"], W["pos_map.3.bias"]))
    x = F.conv2d(x, W["encode.weight"], W["encode.bias"], padding=1)
    skips = []
    for i in range(levels):
        x = block(x, c, f"u_net.downsampling_blocks.{i}.0.")
        skips.append(x)
    x = block(x, c, "u_net.center_block.0.")
    x = x + uo.attention2d(F.group_norm(x, 32, W["u_net.center_block.1.fn.0.weight"], W["u_net.center_block.1.fn.0.bias"], 1e-5), W,
                           "u_net.center_block.1.fn.1.", 1)
    x = block(x, c, "u_net.center_block.2.")
    for i in range(levels):
        x = block(torch.cat((x, skips.pop()), dim=1), c, f"u_net.upsampling_blocks.{i}.0.")
    return F.conv2d(x, W["decode.weight"], W["decode.bias"])


def test_restatement_matches_reference_fixture():
    """The fp64 restatement used at full size reproduces the reference's fp64 forward (levels 2 fixture)."""
    g = golden("g16_unet_attn_fwd2")
    W = unet_attn_weights((3, 16, 16), 2, int(golden("w_unet_attn_l2")["seed"]))
    with torch.no_grad():
        y = restated_forward(W, g["mu"], g["t"], 2)
    assert rel_linf(y, g["out64"]) < 1e-9


def test_full_size_one_forward_vs_restatement():
    """CIFAR-10 geometry (dim 128, levels 32, 3x32x32: 1024 positions, 66 per-block attentions), B 2, one _predict_x against
    the fp64 restatement.  Bound 2e-3, that of test_full_size_unet_one_forward_vs_oracle (achieved: 2.9e-4)."""
    from oracle import bsi_oracle as bo
    shape, levels = (3, 32, 32), 32
    W = unet_attn_weights(shape, levels, 7)
    m = make_model(shape, levels, W)
    bsi = make_bsi(m, shape, k=128)
    gen = torch.Generator().manual_seed(0)
    mu = torch.randn((2, *shape), generator=gen) * 2
    t = torch.tensor([0.2, 0.9])
    with torch.no_grad():
        got = bsi._predict_x(mu.to(DEV), t.to(DEV)).cpu()
        ref = bo.BSIOracle(lambda a, b: restated_forward(W, a, b, levels).float(), data_shape=shape, k=128).predict_x(mu, t)
    err = rel_linf(got, ref)
    report("unet_block_attn_fullsize", rel_linf=err)
    bound("test_full_size_one_forward_vs_restatement", err, 2e-3)


def test_sample_and_backward_bit_reproducible():
    shape = (3, 16, 16)
    m = make_model(shape, 2, seed=21)
    bsi = make_bsi(m, shape, k=8)
    with torch.no_grad():
        a = bsi.sample(3, torch.Generator(DEV).manual_seed(5))
        b = bsi.sample(3, torch.Generator(DEV).manual_seed(5))
    assert torch.equal(a, b)
    gen = torch.Generator().manual_seed(3)
    x = ((torch.randint(0, 256, (3, *shape), generator=gen).float() / 255) * 2 - 1).to(DEV)
    grads = []
    for _ in range(2):
        m.zero_grad()
        loss = bsi.train_loss(x, torch.Generator(DEV).manual_seed(9))
        loss.mean().backward()
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
    assert torch.equal(grads[0], grads[1])


def test_dptrainer_step_updates_res_attention():
    from bsi_amd.dp import DPTrainer
    shape = (3, 8, 8)
    m = make_model(shape, 1, seed=22).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters() if "res_attention" in n}
    assert len(before) == 4 * 6
    tr = DPTrainer(make_bsi(m, shape), lr=5e-4, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(4)
    x = ((torch.randint(0, 256, (4, *shape), generator=gen).float() / 255) * 2 - 1).to(DEV)
    loss = tr.train_step(x)
    assert torch.isfinite(torch.as_tensor(loss)).all()
    after = dict(m.named_parameters())
    unchanged = [n for n, v in before.items() if torch.equal(after[n].detach(), v)]
    assert not unchanged, unchanged


_DEFAULT_PATH_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, {root!r})
from oracle import unet_oracle as uo
from bsi_amd import BSI, Discretization
from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
from bsi_amd.models.vdm_unet import DenoisingVDMUNet
from bsi_amd.nn import FourierFeatures
shape = (3, 16, 16)
W = uo.unet_random_weights(shape, 128, 2, seed=31, ff=(6, 8))
m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", 128, 2, 4, n_attention_heads=1, dropout=0.1,
                     fourier_features=FourierFeatures(n_min=6, n_max=8))
m.load_state_dict(W)
m = m.cuda().eval()  # no dropout: its seed would come from the process's torch.initial_seed()
bsi = BSI(m, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=8, preconditioning="edm",
          discretization=Discretization.image_8bit()).cuda()
h = hashlib.sha256()
with torch.no_grad():
    h.update(bsi.sample(2, torch.Generator("cuda").manual_seed(1)).cpu().numpy().tobytes())
x = ((torch.randint(0, 256, (2, *shape), generator=torch.Generator().manual_seed(2)).float() / 255) * 2 - 1).cuda()
bsi.train_loss(x, torch.Generator("cuda").manual_seed(3)).mean().backward()
for p in m.parameters():
    h.update(p.grad.cpu().numpy().tobytes())
print(h.hexdigest())
"""


def test_default_unet_bits_unchanged_next_to_attention_model():
    """downsampling_attention=False: sampling and gradient bits of a default UNet run in this process after attention models
    have run (library state, caches, struct fields) equal a fresh process that runs only the default UNet."""
    code = _DEFAULT_PATH_SCRIPT.format(root=ROOT)
    make_model((3, 8, 8), 1, seed=23)(torch.zeros((1, 3, 8, 8), device=DEV), torch.zeros(1, device=DEV))
    ns = {}
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        exec(compile(code, "default_path", "exec"), ns)
    here = buf.getvalue().strip()
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == here
