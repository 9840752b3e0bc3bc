"""DenoisingDiT sampling and training at widths between 128 and 1024 (192, 320, 384, 512, 768, 960; 3, 5, 6, 8, 12 and 15 heads),
and the kernels that choose an instance from the width, at widths that fill their lane vectors only partly.

Kernel level, through the C ABI: bsi_gate_bwd, bsi_ln_mod_bwd and bsi_ln_gate_bwd against fp64 autograd on both sides of every
instance threshold, with the modulation table of a depth-2 model (row stride 12 d) and modulation-gradient targets that start from
non-zero values; bsi_gemm_tn_bf16 / _bias / _pair and bsi_colsum_bf16 at the shapes the engine issues for these widths, dense and on
column slices of wider buffers.  Every output is NaN-filled before the call and followed by a guard region that is compared bit for
bit afterwards; the weight-gradient workspace is NaN-filled before every call.  Bounds: those of tests/test_hip_ops.py.

Engine level: eval forward, train_loss(...).mean().backward() against the fp64 CPU oracle (tests/dit_width_cases.py; its fp32
restatement is held ORACLE_MARGIN inside every bound by tests/test_dit_width_cases_host.py) at the tolerances of BASELINE.md
section 5, plus the same bound on every block of 64 output features of every weight and bias gradient."""
import ctypes as C
import math

import pytest
import torch

from tests import dit_width_cases as wc
from tests.util import bound, max_rel, rel_l2, rel_linf, replay_draws, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BF16 = 0x7FC1       # tests/test_hip_dispatch_edges.py: a quiet NaN whose bits no kernel writes by accident
NAN_F32 = 0x7FC00001
GUARD = 64              # elements behind every output
F64 = torch.float64


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


_KEEP = []  # device buffers stay alive until the test ends (kernels are enqueued asynchronously)


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def dev(t):
    d = t.to(DEV).contiguous()
    _KEEP.append(d)
    return d


class Guarded:
    """An output of `shape` on the GPU followed by GUARD elements; everything holds the NaN pattern unless `init` gives the contents
    a kernel updates in place.  get() checks the guard bit for bit and, for a pure output, that no element kept the pattern."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        self.shape, self.dtype, self.n = tuple(shape), dtype, math.prod(shape)
        self.bits, self.pattern = (torch.int16, NAN_BF16) if dtype == torch.bfloat16 else (torch.int32, NAN_F32)
        self.full = torch.full((self.n + GUARD,), self.pattern, dtype=self.bits, device=DEV)
        self.init = init is not None
        if self.init:
            self.full[:self.n] = init.to(dtype).reshape(-1).contiguous().view(self.bits).to(DEV)
        _KEEP.append(self.full)

    @property
    def ptr(self):
        return C.c_void_p(self.full.data_ptr())

    def at(self, elements):
        return C.c_void_p(self.full.data_ptr() + elements * self.full.element_size())

    def get(self, what):
        h = self.full.cpu()
        assert bool((h[self.n:] == self.pattern).all()), f"{what}: written past the end"
        if not self.init:
            assert not bool((h[:self.n] == self.pattern).any()), f"{what}: elements the kernel never wrote"
        out = h[:self.n].view(self.dtype).reshape(self.shape)
        assert bool(torch.isfinite(out.float()).all()), f"{what}: not finite"
        return out


def nan_bytes(n):
    """n bytes of 0xFF: NaN in fp32 and in bf16 (a slab region that is read before it is written poisons the result)."""
    b = torch.full((max(int(n), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    _KEEP.append(b)
    return b


def off(t, elements):
    return C.c_void_p(t.data_ptr() + elements * t.element_size())


def check_dmod(got, ref, d, own, tag):
    """The chunks in `own` (of the block under test) hold initial value + this call's sums within SUMS; every other float of the
    table -- the other block's half, the other chunks -- keeps its bits."""
    worst = 0.0
    keep = torch.ones(got.shape[1], dtype=torch.bool)
    for c in own:
        o = wc.chunk_offset(d, c)
        keep[o:o + d] = False
        worst = max(worst, rel_linf(got[:, o:o + d], ref[:, o:o + d]))
    assert torch.equal(got[:, keep], ref[:, keep].float()), f"{tag}: modulation gradients outside the kernel's chunks changed"
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# gated-residual and LayerNorm-modulate backward across the instance thresholds
# ----------------------------------------------------------------------------------------------------------------------------------
GATE_CASES = [(d, Bs, t) for d in wc.GATE_D for Bs, t in wc.GATE_ROWS]
FUSED_CASES = [(d, Bs, t) for d in wc.FUSED_D for Bs, t in wc.FUSED_ROWS]


@pytest.mark.parametrize("d,Bs,tokens", GATE_CASES, ids=[f"d{d}_B{b}_t{t}" for d, b, t in GATE_CASES])
def test_gate_bwd_widths(N, d, Bs, tokens):
    c, r = wc.bwd_inputs(d, Bs, tokens), wc.gate_reference(d, Bs, tokens, F64)
    M, stride = c["M"], wc.DEPTH_ROWS * 6 * d
    x = Guarded((M, d), init=r["x2"])
    dmod = Guarded((Bs, stride), init=c["dmod0"])
    dd = Guarded((M, d), torch.bfloat16)
    mod = dev(c["mod"])
    o = wc.chunk_offset(d, wc.G_A)
    N.check(N.lib().bsi_gate_bwd(N.ptr(dev(c["dX"])), N.ptr(dev(c["delta"].to(torch.bfloat16))), x.ptr, off(mod, o), stride, dmod.at(o),
                                 stride, M, d, tokens, dd.ptr, N.stream()))
    e_x = rel_linf(x.get("x"), r["x1"])
    e_dd = rel_linf(dd.get("ddelta").float(), r["ddelta"])
    e_g = check_dmod(dmod.get("dgate"), r["dmod"], d, (wc.G_A,), "gate_bwd")
    report("widths_gate_bwd", d=d, samples=Bs, tokens=tokens, rewind=e_x, ddelta=e_dd, dgate=e_g)
    bound("test_gate_bwd_widths:rewind", e_x, wc.REWIND)
    bound("test_gate_bwd_widths:ddelta", e_dd, wc.DDELTA)
    bound("test_gate_bwd_widths:dgate", e_g, wc.SUMS)


@pytest.mark.parametrize("d,Bs,tokens", GATE_CASES, ids=[f"d{d}_B{b}_t{t}" for d, b, t in GATE_CASES])
def test_ln_mod_bwd_widths(N, d, Bs, tokens):
    c, r = wc.bwd_inputs(d, Bs, tokens), wc.ln_mod_reference(d, Bs, tokens, F64)
    M, stride = c["M"], wc.DEPTH_ROWS * 6 * d
    dX = Guarded((M, d), init=c["dX"])
    dmod = Guarded((Bs, stride), init=c["dmod0"])
    mod = dev(c["mod"])
    N.check(N.lib().bsi_ln_mod_bwd(N.ptr(dev(c["dxn"].to(torch.bfloat16))), N.ptr(dev(c["x_below"])), off(mod, wc.chunk_offset(d, wc.SC_M)),
                                   stride, dmod.at(wc.chunk_offset(d, wc.SH_M)), dmod.at(wc.chunk_offset(d, wc.SC_M)), stride, dX.ptr, M, d,
                                   tokens, 1e-5, N.stream()))
    e_dx = rel_linf(dX.get("dX"), r["dX"])
    e_s = check_dmod(dmod.get("dshift/dscale"), r["dmod"], d, (wc.SH_M, wc.SC_M), "ln_mod_bwd")
    report("widths_ln_mod_bwd", d=d, samples=Bs, tokens=tokens, dX=e_dx, sums=e_s)
    bound("test_ln_mod_bwd_widths:dX", e_dx, wc.DX)
    bound("test_ln_mod_bwd_widths:sums", e_s, wc.SUMS)


@pytest.mark.parametrize("d,Bs,tokens", FUSED_CASES, ids=[f"d{d}_B{b}_t{t}" for d, b, t in FUSED_CASES])
def test_ln_gate_bwd_widths(N, d, Bs, tokens):
    """The three modes of bsi_ln_gate_bwd; the statistics are taken as the forward kernel writes them (fp32 mean and rstd)."""
    c = wc.bwd_inputs(d, Bs, tokens)
    M, stride = c["M"], wc.DEPTH_ROWS * 6 * d
    x64 = wc.fused_reference(d, Bs, tokens, F64)["x"]
    x32, stats = dev(x64.float()), dev(wc.forward_stats(x64))
    mod, dxn, delta = dev(c["mod"]), dev(c["dxn"].to(torch.bfloat16)), dev(c["delta"].to(torch.bfloat16))
    o = lambda ch: wc.chunk_offset(d, ch)  # noqa: E731
    for mode in wc.FUSED_MODES:
        ln, gt = mode != "gate", mode != "ln"
        r = wc.fused_reference(d, Bs, tokens, F64, ln, gt)
        dX = Guarded((M, d), init=c["dX"])
        dmod = Guarded((Bs, stride), init=c["dmod0"])
        dd = Guarded((M, d), torch.bfloat16)
        N.check(N.lib().bsi_ln_gate_bwd(
            N.ptr(dxn) if ln else None, N.ptr(x32) if ln else None, N.ptr(stats) if ln else None, off(mod, o(wc.SC_M)) if ln else None,
            stride, dmod.at(o(wc.SH_M)) if ln else None, dmod.at(o(wc.SC_M)) if ln else None, stride, dX.ptr,
            N.ptr(delta) if gt else None, off(mod, o(wc.G_A)) if gt else None, stride, dmod.at(o(wc.G_A)) if gt else None, stride,
            dd.ptr if gt else None, M, d, tokens, N.stream()))
        e_dx = rel_linf(dX.get("dX"), r["dX"])
        own = ((wc.SH_M, wc.SC_M) if ln else ()) + ((wc.G_A,) if gt else ())
        e_s = check_dmod(dmod.get("dmod"), r["dmod"], d, own, f"ln_gate_bwd/{mode}")
        e_dd = 0.0
        if gt:
            e_dd = rel_linf(dd.get("ddelta").float(), r["ddelta"])
        else:
            assert bool((dd.full.cpu() == NAN_BF16).all()), "ln mode wrote ddelta"
        report("widths_ln_gate_bwd", d=d, samples=Bs, tokens=tokens, mode=mode, dX=e_dx, sums=e_s, ddelta=e_dd)
        bound(f"test_ln_gate_bwd_widths:{mode}:dX", e_dx, wc.DX)
        bound(f"test_ln_gate_bwd_widths:{mode}:sums", e_s, wc.SUMS)
        bound(f"test_ln_gate_bwd_widths:{mode}:ddelta", e_dd, wc.DDELTA)


def test_backward_kernels_refuse_what_they_cannot_run(N):
    """Dummy pointers: refused before anything is followed.  Each message names the offending value."""
    lib, p = N.lib(), C.c_void_p(16)

    def gate(M, d, tokens):
        return lib.bsi_gate_bwd(p, p, p, p, 12 * d, p, 12 * d, M, d, tokens, p, None)

    def ln_mod(M, d, tokens):
        return lib.bsi_ln_mod_bwd(p, p, p, 12 * d, p, p, 12 * d, p, M, d, tokens, 1e-5, None)

    def fused(M, d, tokens):
        return lib.bsi_ln_gate_bwd(p, p, p, p, 12 * d, p, p, 12 * d, p, p, p, 12 * d, p, 12 * d, p, M, d, tokens, None)

    for call, cases in ((gate, ((96, 2052, 32, "d=2052"), (96, 102, 32, "d=102"), (96, 256, 48, "tokens=48"), (100, 256, 64, "M=100"))),
                        (ln_mod, ((96, 2052, 32, "d=2052"), (96, 102, 32, "d=102"), (96, 256, 48, "tokens=48"), (100, 256, 64, "M=100"))),
                        (fused, ((192, 1028, 64, "d=1028"), (192, 256, 96, "tokens=96"), (100, 256, 64, "M=100")))):
        for M, d, tokens, names in cases:
            assert call(M, d, tokens) == -1, (call.__name__, M, d, tokens)
            err = lib.bsi_last_error().decode()
            assert names in err and err.startswith("bsi_" + {"gate": "gate_bwd", "ln_mod": "ln_mod_bwd", "fused": "ln_gate_bwd"}[call.__name__]), err
    # the pair wants whole 256-column tiles of its first problem: 3 * 384 = 1152 is the qkv gradient of a width the engine runs unpaired
    assert lib.bsi_gemm_tn_pair_bf16(p, 1152, p, 1152, p, p, 384, p, 384, p, 384, 512, 384, p, None) == -1
    assert "N1=1152" in lib.bsi_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------------------------
# weight-gradient GEMMs and column sums at the engine's shapes for these widths
# ----------------------------------------------------------------------------------------------------------------------------------
def _slice_of_wider(t, pad, lead):
    """`t` as columns lead .. lead + cols of a bf16 buffer `pad` columns wider whose other columns are NaN; (buffer, pointer, ld)."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    buf[:, lead:lead + cols] = t.to(torch.bfloat16).to(DEV)
    _KEEP.append(buf)
    return buf, off(buf, lead), cols + pad


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("M,Nn,K", wc.TN_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in wc.TN_SHAPES])
def test_gemm_tn_and_colsum_at_engine_shapes(N, M, Nn, K, padded):
    lib = N.lib()
    dY, X = wc.tn_operands(M, Nn, K)
    ref, ref_cs = wc.tn_reference(M, Nn, K, F64)
    if padded:
        _, pP, ldp = _slice_of_wider(dY, wc.PAD_P, 24)
        _, pQ, ldq = _slice_of_wider(X, wc.PAD_Q, 8)
    else:
        pP, ldp, pQ, ldq = N.ptr(dev(dY.to(torch.bfloat16))), Nn, N.ptr(dev(X.to(torch.bfloat16))), K
    ws_bytes = lib.bsi_gemm_tn_workspace_bytes(M, Nn, K)
    errs = {}
    out = Guarded((Nn, K))
    N.check(lib.bsi_gemm_tn_bf16(pP, ldp, pQ, ldq, M, Nn, K, out.ptr, K, 0, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    first = out.get("gemm_tn")
    errs["tn"] = rel_linf(first, ref)
    acc = Guarded((Nn, K), init=first)
    N.check(lib.bsi_gemm_tn_bf16(pP, ldp, pQ, ldq, M, Nn, K, acc.ptr, K, 1, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    errs["tn_accumulate"] = rel_linf(acc.get("gemm_tn accumulate"), 2 * ref)
    out2, cs2 = Guarded((Nn, K)), Guarded((Nn,))
    N.check(lib.bsi_gemm_tn_bias_bf16(pP, ldp, pQ, ldq, M, Nn, K, out2.ptr, K, cs2.ptr, 0, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    errs["tn_bias"] = rel_linf(out2.get("gemm_tn_bias"), ref)
    errs["tn_bias_colsum"] = rel_linf(cs2.get("gemm_tn_bias colsum"), ref_cs)
    acc2, accs = Guarded((Nn, K), init=first), Guarded((Nn,), init=ref_cs)
    N.check(lib.bsi_gemm_tn_bias_bf16(pP, ldp, pQ, ldq, M, Nn, K, acc2.ptr, K, accs.ptr, 1, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    errs["tn_bias_accumulate"] = rel_linf(acc2.get("gemm_tn_bias accumulate"), 2 * ref)
    errs["tn_bias_colsum_accumulate"] = rel_linf(accs.get("gemm_tn_bias colsum accumulate"), 2 * ref_cs)
    cs = Guarded((Nn,))
    N.check(lib.bsi_colsum_bf16(pP, ldp, M, Nn, cs.ptr, 0, N.ptr(nan_bytes(lib.bsi_colsum_workspace_bytes(Nn))), N.stream()))
    errs["colsum"] = rel_linf(cs.get("colsum"), ref_cs)
    report("widths_gemm_tn", M=M, N=Nn, K=K, padded=int(padded), splits=wc.tn_splits(M, Nn, K)[0], **errs)
    for k, v in errs.items():
        bound(f"test_gemm_tn_and_colsum_at_engine_shapes:{k}", v, wc.COLSUM if "colsum" in k else wc.TN)


@pytest.mark.parametrize("M,N1,N2,K", wc.TN_PAIR_SHAPES, ids=[f"{m}x{a}+{b}x{k}" for m, a, b, k in wc.TN_PAIR_SHAPES])
def test_gemm_tn_pair_at_engine_shapes(N, M, N1, N2, K):
    """The qkv and out-projection weight gradients in one launch, as the engine issues it at dim 512 and 768 (ldp1 = N1, ldp2 = N2,
    ldq = K): against fp64, against the two single launches, and twice (bit reproducible)."""
    lib = N.lib()
    (dY1, X1), (dY2, X2) = wc.tn_operands(M, N1, K, 1), wc.tn_operands(M, N2, K, 2)
    r1, r2 = wc.tn_reference(M, N1, K, F64, 1)[0], wc.tn_reference(M, N2, K, F64, 2)[0]
    d1, d2, q1, q2 = (dev(t.to(torch.bfloat16)) for t in (dY1, dY2, X1, X2))
    ws_bytes = lib.bsi_gemm_tn_workspace_bytes(M, N1 + (N2 + 255) // 256 * 256, K)
    runs = []
    for _ in range(2):
        o1, o2 = Guarded((N1, K)), Guarded((N2, K))
        N.check(lib.bsi_gemm_tn_pair_bf16(N.ptr(d1), N1, N.ptr(q1), N1, o1.ptr, N.ptr(d2), N2, N.ptr(q2), N2, o2.ptr, K, M, K,
                                          N.ptr(nan_bytes(ws_bytes)), N.stream()))
        runs.append((o1.get("pair out1"), o2.get("pair out2")))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "the pair launch is not bit reproducible"
    s1, s2 = Guarded((N1, K)), Guarded((N2, K))
    N.check(lib.bsi_gemm_tn_bf16(N.ptr(d1), N1, N.ptr(q1), K, M, N1, K, s1.ptr, K, 0, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    N.check(lib.bsi_gemm_tn_bf16(N.ptr(d2), N2, N.ptr(q2), K, M, N2, K, s2.ptr, K, 0, N.ptr(nan_bytes(ws_bytes)), N.stream()))
    errs = dict(out1=rel_linf(runs[0][0], r1), out2=rel_linf(runs[0][1], r2), out1_vs_single=rel_linf(runs[0][0], s1.get("single 1")),
                out2_vs_single=rel_linf(runs[0][1], s2.get("single 2")))
    report("widths_gemm_tn_pair", M=M, N1=N1, N2=N2, K=K, splits=wc.tn_splits(M, N1 + (N2 + 255) // 256 * 256, K)[0], **errs)
    bound("test_gemm_tn_pair_at_engine_shapes:fp64", max(errs["out1"], errs["out2"]), wc.TN)
    bound("test_gemm_tn_pair_at_engine_shapes:vs_single", max(errs["out1_vs_single"], errs["out2_vs_single"]), wc.PAIR_VS_SINGLE)


# ----------------------------------------------------------------------------------------------------------------------------------
# the engines
# ----------------------------------------------------------------------------------------------------------------------------------
def build(tag, dropout=None):
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    shape, dim, heads, depth, _, _ = wc.GEOMETRIES[tag]
    m = DenoisingDiT(shape, wc.PATCH, dim, depth, heads, dropout=dropout, fourier_features=FourierFeatures(n_min=wc.FF[0], n_max=wc.FF[1]))
    m.load_state_dict(wc.geometry_inputs(tag)[0])
    return m.to(DEV)


def make_bsi(model, shape):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=16, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


@pytest.mark.parametrize("tag", list(wc.GEOMETRIES))
def test_width_vs_fp64_oracle(tag):
    """Eval forward, per-sample and mean loss, and every parameter gradient, whole and per block of 64 output features."""
    shape, dim, heads, depth, B, _ = wc.GEOMETRIES[tag]
    y64, l64, G64 = wc.geometry_oracle(tag, True)
    _, mu, t, x, offs, perm, eps = wc.geometry_inputs(tag)
    model = build(tag).eval()
    with torch.no_grad():
        y = model(mu.to(DEV), t.to(DEV)).cpu()
    model.train()
    bsi = make_bsi(model, shape)
    with replay_draws(DEV, rand=[offs], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(x.to(DEV))
    loss.mean().backward()
    lc = loss.detach().cpu()
    fwd_err = rel_linf(y, y64)
    mean_err = abs(float(lc.double().mean()) / float(l64.mean()) - 1)
    sample_err = max_rel(lc, l64)
    errs, blocks = [], []
    for name, q in model.named_parameters():
        assert q.grad is not None and q.grad.shape == G64[name].shape and bool(torch.isfinite(q.grad).all()), name
        errs.append((rel_l2(q.grad, G64[name]), name))
        if q.grad.ndim == 2 or name.endswith("bias"):
            be = wc.block_errors(q.grad, G64[name])
            blocks.append((max(be), name, be.index(max(be))))
    worst, worst_block = max(errs), max(blocks)
    report("dit_width_vs_fp64_oracle", case=tag, dim=dim, heads=heads, depth=depth, tokens=wc.tokens_of(tag), x_hat=fwd_err, loss_mean=mean_err,
           loss_per_sample=sample_err, worst_grad=worst[0], worst_name=worst[1], worst_block=worst_block[0], worst_block_name=worst_block[1],
           worst_block_index=worst_block[2])
    bound(f"test_width_vs_fp64_oracle:{tag}:x_hat", fwd_err, wc.X_HAT)
    bound(f"test_width_vs_fp64_oracle:{tag}:loss_mean", mean_err, wc.LOSS_MEAN)
    bound(f"test_width_vs_fp64_oracle:{tag}:loss", sample_err, wc.LOSS_SAMPLE)
    failed = [(n, e) for e, n in errs if not e < wc.GRAD] + [(f"{n}[block {i}]", e) for e, n, i in blocks if not e < wc.GRAD]
    assert not failed, failed  # every tensor and block past the bound, not just the first
    for err, name in errs:
        bound(f"test_width_vs_fp64_oracle:{tag}:grad", err, wc.GRAD)
    for err, name, _ in blocks:
        bound(f"test_width_vs_fp64_oracle:{tag}:grad_block64", err, wc.GRAD)


@pytest.mark.parametrize("tag", list(wc.DROPOUT))
def test_width_with_dropout_vs_oracle_with_same_masks(tag):
    """w320 at p = 0.3: hash masks (64 tokens); b768_t256 at p = 0.1: the mask words, which the attention forward computes itself
    because tokens != 16 * heads."""
    from tests.test_hip_dit_heads import against_oracle_with_same_masks
    shape, dim, heads, depth, B, _ = wc.GEOMETRIES[tag]
    W, _, _, x, offs, perm, eps = wc.geometry_inputs(tag)
    against_oracle_with_same_masks("width_" + tag, shape, wc.PATCH, dim, depth, heads, B, wc.DROPOUT[tag], W, (x, offs, perm, eps))


@pytest.mark.parametrize("tag", wc.REPRODUCIBLE)
def test_width_backward_is_bit_reproducible(tag):
    shape = wc.GEOMETRIES[tag][0]
    _, _, _, x, offs, perm, eps = wc.geometry_inputs(tag)
    model = build(tag).train()
    bsi = make_bsi(model, shape)
    runs = []
    for _ in range(2):
        model.zero_grad()
        with replay_draws(DEV, rand=[offs], randperm=[perm], randn=[eps]):
            loss = bsi.train_loss(x.to(DEV))
        loss.mean().backward()
        runs.append((loss.detach().clone(), torch.cat([q.grad.reshape(-1) for q in model.parameters()]).clone()))
    assert bool(torch.isfinite(runs[0][1]).all())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
