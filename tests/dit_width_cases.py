"""Cases of the DenoisingDiT at widths between 128 and 1024, where the kernels fill their lane vectors only partly and the training
engine takes the `dim > 256` path away from the benchmark's 1024: seeded engine geometries with their CPU oracle (fp64, and fp32 to
show what fp32 arithmetic alone costs), a restatement of the backward's dispatch (dit_train.hip bsi_dit_backward, dit_bwd_ops.hip,
gemm_tn.hip tn_splits), and the inputs and references of the memory-bound backward kernels and the weight-gradient GEMMs at those
widths.  CPU only; tests/test_dit_width_cases_host.py vets it, tests/test_hip_dit_widths.py runs the kernels against it."""
import functools

import torch

from tests.dit_patch_cases import GRAD, LOSS_MEAN, LOSS_SAMPLE, ORACLE_MARGIN, X_HAT  # noqa: F401  

PATCH, FF = 2, (6, 8)
# tag: (shape, dim, heads, depth, B, seed); what each one decides:
#   w192        VPL 1 with 48 of 64 lanes; rel_dd off, rel_fc1 on (M = 192 > 128); three heads
#   w320        the first width above 256: VPL 4 with 80 of 256 slots; rel_dd without pair; depth 2: both parity slots of the plane
#               sums and the fused launch of l > 0; five heads
#   w384_dh128  head dim 128 at a width that is no multiple of 256
#   w960        the last width below 1024; fifteen heads
#   s384_t256   the DiT-S block: single-sweep attention backward with qkv bias rows, no pair (384 % 256 != 0)
#   w512_t256   the pair launch at 1536 + 512 columns
#   b768_t256   the DiT-B block, depth 2: the pair launch at 2304 + 768 columns, K = 768
#   w320_m128   M = 128: rel_fc1 off (fc1's bias gradient rides on its weight-gradient GEMM) while rel_dd is on -- the one value of
#               rel_fc1 the rows above do not reach
GEOMETRIES = {
    "w192": ((3, 16, 16), 192, 3, 1, 3, 61),
    "w320": ((3, 16, 16), 320, 5, 2, 3, 62),
    "w384_dh128": ((3, 16, 16), 384, 3, 1, 3, 63),
    "w960": ((3, 16, 16), 960, 15, 1, 3, 64),
    "s384_t256": ((3, 32, 32), 384, 6, 1, 2, 65),
    "w512_t256": ((3, 32, 32), 512, 8, 1, 2, 66),
    "b768_t256": ((3, 32, 32), 768, 12, 2, 2, 67),
    "w320_m128": ((3, 16, 16), 320, 5, 1, 2, 68),
}
DROPOUT = {"w320": 0.3, "b768_t256": 0.1}     # tag -> p of the dropout runs
REPRODUCIBLE = ("w320", "b768_t256")          # two backward runs give equal bits
# block statistic: RMS error inside 64 output features over the RMS of the whole reference tensor.  bf16 noise per element is uniform
# over a tensor, so a correct block reads like the whole tensor (<= GRAD); one wrong column of 64 reads >= 1/8, a missing slab more
BLOCK = 64


def tokens_of(tag):
    shape = GEOMETRIES[tag][0]
    return (shape[1] // PATCH) * (shape[2] // PATCH)


def geometry_inputs(tag):
    """(W, mu, t, x, offset, perm, eps) of a geometry: seeded CPU draws."""
    from oracle import dit_oracle as do
    shape, dim, _, depth, B, seed = GEOMETRIES[tag]
    W = do.dit_random_weights(shape, PATCH, dim, depth, ff=FF, seed=seed)
    g = torch.Generator().manual_seed(seed + 500)
    mu = torch.randn((B, *shape), generator=g) * 2
    t = torch.rand(B, generator=g)
    x = (torch.round(255 * torch.rand((B, *shape), generator=g)) / 255) * 2 - 1
    off = torch.rand((), generator=g)
    perm = torch.randperm(B, generator=g)
    eps = torch.randn((B, *shape), generator=g)
    return W, mu, t, x, off, perm, eps


@functools.lru_cache(maxsize=None)
def geometry_oracle(tag, double):
    """Forward, per-sample train loss and every parameter gradient of the CPU oracle at fp64 (`double`) or fp32.
    Returns (y, loss, {name: grad}); computed once per process and shared (never written to)."""
    from oracle import bsi_oracle as bo
    from oracle import dit_oracle as do
    shape, dim, heads, depth, _, _ = GEOMETRIES[tag]
    W, mu, t, x, off, perm, eps = geometry_inputs(tag)
    dt = torch.float64 if double else torch.float32
    Wr = {k: v.to(dt).requires_grad_(True) for k, v in W.items()}
    f = lambda a, b: do.dit_forward(Wr, a, b, patch_size=PATCH, dim=dim, depth=depth, heads=heads, ff=FF)  # noqa: E731
    with torch.no_grad():
        y = f(mu.to(dt), t.to(dt))
    loss = bo.BSIOracle(f, data_shape=shape, k=16, dtype=dt).train_loss(x.to(dt), off.to(dt), perm.to(dt), eps.to(dt))
    loss.mean().backward()
    return y, loss.detach(), {k: v.grad for k, v in Wr.items()}


def block_errors(got, ref):
    """Per block of BLOCK output features (rows of a 2-D gradient, elements of a bias): RMS error inside the block over the RMS of the
    whole reference tensor.  Returns the list of figures, one per block."""
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = float(ref.pow(2).mean().sqrt().clamp_min(1e-30))
    e = (got - ref).reshape(ref.shape[0], -1)
    return [float(e[i:i + BLOCK].pow(2).mean().sqrt()) / scale for i in range(0, ref.shape[0], BLOCK)]


# ----------------------------------------------------------------------------------------------------------------------------------
# The backward's dispatch, restated
# ----------------------------------------------------------------------------------------------------------------------------------
def vpl(d, fused):
    """float4 vectors per lane of the instance bsi_gate_bwd / bsi_ln_mod_bwd (fused False) or bsi_ln_gate_bwd (fused True) launch at
    width d; None where the entry refuses d."""
    if d % 4 or d < 4 or d > (1024 if fused else 2048):
        return None
    return 1 if d <= 256 else 4 if d <= 1024 else 8


def lane_fill(d, fused):
    """(VPL, slots in use, slots): d / 4 float4 column groups over 64 * VPL lane slots; partly filled where the two differ."""
    v = vpl(d, fused)
    return v, d // 4, 64 * v


def tn_splits(M, N, K, cus=256):
    """gemm_tn.hip tn_splits followed by the rounding of the token range to multiples of 32: (splits, rows per split)."""
    tiles = ((N + 255) // 256) * ((K + 255) // 256)
    max_by_m = max(M // 512, 1)
    best, best_t = 1, 1e30
    for s in range(1, min(16, max_by_m) + 1):
        t = ((tiles * s + cus - 1) // cus) / s
        if t < best_t * 0.9:
            best_t, best = t, s
    per = (M + best - 1) // best
    m_per = (per + 31) // 32 * 32
    return (M + m_per - 1) // m_per, m_per


def dispatch(tag, p=0.0, cus=256):
    """What bsi_dit_backward decides for a geometry at `cus` CUs and dropout p (production settings: no A/B switch set)."""
    shape, dim, heads, depth, B, _ = GEOMETRIES[tag]
    tokens = tokens_of(tag)
    M, dh = B * tokens, dim // heads
    words = tokens == 256 and dh == 64                        # bsi_attention_uses_mask_words
    rel_dd = dim > 256
    rel_fc1 = M > 128 and dim >= 128 and dim % 64 == 0        # bsi_gemm_emits_colsum(M, dim)
    rel_qkv = tokens == 256 and dh == 64 and (p == 0 or words)  # single_sweep: the hash form of the mask stays with two passes
    pair = rel_dd and rel_qkv and dim % 256 == 0
    P = shape[0] * PATCH * PATCH
    kin = P * (1 + 2 * (FF[1] - FF[0] + 1))
    kpad = (kin + 63) // 64 * 64
    gemms = {"dec": (M, (P + 7) // 8 * 8, dim), "fc2": (M, dim, 4 * dim), "fc1": (M, 4 * dim, dim), "ada2": (B, 6 * dim, dim),
             "ada0": (B, dim, dim), "enc": (M, dim, kpad)}
    if pair:
        gemms["pair"] = (M, 3 * dim + (dim + 255) // 256 * 256, dim)
    else:
        gemms["out"], gemms["qkv"] = (M, dim, dim), (M, 3 * dim, dim)
    v, used, slots = lane_fill(dim, True)
    return dict(M=M, tokens=tokens, dh=dh, depth=depth, rel_dd=rel_dd, rel_fc1=rel_fc1, rel_qkv=rel_qkv, pair=pair, vpl=v,
                partly_filled=used < slots, slots=(used, slots), hash_masks=p > 0 and not words,
                mask_ride=p > 0 and words and tokens == 16 * heads and 256 < dim <= 1024,
                tn={k: (*s, *tn_splits(*s, cus)) for k, s in gemms.items()})


# ----------------------------------------------------------------------------------------------------------------------------------
# Kernel cases: gated-residual and LayerNorm-modulate backward
# ----------------------------------------------------------------------------------------------------------------------------------
GATE_D = (4, 12, 100, 192, 252, 256, 260, 320, 768, 1020, 1024, 1028, 1536, 2044, 2048)
GATE_ROWS = ((1, 32), (3, 32), (2, 96))       # (samples, tokens): one slab, one slab per sample, three slabs per sample
FUSED_D = (4, 12, 100, 192, 252, 256, 260, 320, 384, 768, 1020, 1024)
FUSED_ROWS = ((1, 64), (3, 64), (2, 192))
FUSED_MODES = ("both", "ln", "gate")
DEPTH_ROWS, BLOCK_UNDER_TEST = 2, 1            # the modulation table of a depth-2 model: rows of 12 d floats; block 1 is under test
DX, SUMS, DDELTA, REWIND = 2e-5, 1e-5, 4e-3, 1e-6  # tests/test_hip_ops.py test_gate_and_ln_backward / test_fused_ln_gate_backward
# chunk order of a block's six modulation vectors (dit.py:87-92)
SH_A, SC_A, G_A, SH_M, SC_M, G_M = range(6)


def chunk(mod, d, c, block=BLOCK_UNDER_TEST):
    """Chunk c of `block` in a [samples, DEPTH_ROWS * 6 d] table (a view)."""
    o = (block * 6 + c) * d
    return mod[:, o:o + d]


def chunk_offset(d, c, block=BLOCK_UNDER_TEST):
    return (block * 6 + c) * d


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _leaf(t, dtype):
    """A fresh leaf in `dtype` (the cached inputs are shared and stay untouched)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def _layer_norm(x, eps=1e-5):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps)


@functools.lru_cache(maxsize=None)
def bwd_inputs(d, Bs, tokens):
    """Seeded inputs shared by the three kernels at one (d, samples, tokens): the residual stream below the gated add, the bf16 branch
    output delta, the modulation table, the incoming gradient dX, the bf16 gradient dxn of the LayerNorm-modulate output, and the
    non-zero contents the modulation-gradient table starts from."""
    gen = torch.Generator().manual_seed(100003 * d + 101 * Bs + tokens)
    M = Bs * tokens
    r = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    return dict(M=M, rows=torch.arange(M) // tokens, x_below=r(M, d) * 2 + 0.5, delta=bf16r(r(M, d)), mod=r(Bs, DEPTH_ROWS * 6 * d) * 0.3,
                dX=r(M, d), dxn=bf16r(r(M, d)), dmod0=r(Bs, DEPTH_ROWS * 6 * d) * 0.5)


def forward_stats(x):
    """(mean, rstd) per row as the forward LayerNorm kernel writes them: fp32."""
    x32 = x.float()
    mean = x32.mean(dim=1)
    rstd = 1.0 / torch.sqrt(((x32 - mean[:, None]) ** 2).mean(dim=1) + 1e-5)
    return torch.stack((mean, rstd), dim=1).contiguous()


def fused_reference(d, Bs, tokens, dtype, ln=True, gate=True):
    """Autograd of  x = x_below + gate * delta,  xn = LN(x) * (1 + scale) + shift  in `dtype` (fp64: the reference; fp32: what fp32
    arithmetic alone gives).  Returns what bsi_ln_gate_bwd leaves: dX (= dL/dx), ddelta = gate * dX, and the modulation-gradient
    table = its initial contents plus the sums of this call; parts that are switched off leave their targets alone."""
    c = bwd_inputs(d, Bs, tokens)
    rows = c["rows"]
    mod = c["mod"].to(dtype)
    xb = _leaf(c["x_below"], dtype)
    dl = _leaf(c["delta"], dtype)
    g = _leaf(chunk(mod, d, G_A), dtype)
    sh = _leaf(chunk(mod, d, SH_M), dtype)
    sc = _leaf(chunk(mod, d, SC_M), dtype)
    x = torch.addcmul(xb, g[rows], dl)
    x.retain_grad()
    loss = (x * c["dX"].to(dtype)).sum()
    if ln:
        loss = loss + ((_layer_norm(x) * (1 + sc[rows]) + sh[rows]) * c["dxn"].to(dtype)).sum()
    loss.backward()
    dmod = c["dmod0"].to(dtype).clone()
    if ln:
        chunk(dmod, d, SH_M).add_(sh.grad)
        chunk(dmod, d, SC_M).add_(sc.grad)
    if gate:
        chunk(dmod, d, G_A).add_(g.grad)
    return dict(x=x.detach(), dX=x.grad, ddelta=dl.grad if gate else None, dmod=dmod)


def gate_reference(d, Bs, tokens, dtype):
    """bsi_gate_bwd on x2 = x_below + gate * delta with dX = dL/dx2: x is rewound to x_below, ddelta = gate * dX, dgate accumulates."""
    r = fused_reference(d, Bs, tokens, dtype, ln=False, gate=True)
    return dict(x2=r["x"], x1=bwd_inputs(d, Bs, tokens)["x_below"].to(dtype), ddelta=r["ddelta"], dmod=r["dmod"])


def ln_mod_reference(d, Bs, tokens, dtype):
    """bsi_ln_mod_bwd on the rows x_below (it computes the statistics itself): dX += LayerNorm-modulate backward, dshift / dscale
    accumulate."""
    c = bwd_inputs(d, Bs, tokens)
    rows = c["rows"]
    mod = c["mod"].to(dtype)
    x = _leaf(c["x_below"], dtype)
    sh = _leaf(chunk(mod, d, SH_M), dtype)
    sc = _leaf(chunk(mod, d, SC_M), dtype)
    ((_layer_norm(x) * (1 + sc[rows]) + sh[rows]) * c["dxn"].to(dtype)).sum().backward()
    dmod = c["dmod0"].to(dtype).clone()
    chunk(dmod, d, SH_M).add_(sh.grad)
    chunk(dmod, d, SC_M).add_(sc.grad)
    return dict(dX=c["dX"].to(dtype) + x.grad, dmod=dmod)


# ----------------------------------------------------------------------------------------------------------------------------------
# Kernel cases: weight-gradient GEMMs at the shapes the engine issues for the geometries above
# ----------------------------------------------------------------------------------------------------------------------------------
# (M, N, K): out[N, K] = P[M, N]^T Q[M, K].  fc2 and fc1 of w320, its decoder (P = 12 -> 16 columns) and adaLN output layer (M = B);
# qkv of s384_t256 and its patch encoder (84 input columns padded to K = 128); fc2 and qkv of the DiT-B width at 1056 rows, which
# tn_splits cuts into two ragged token ranges (544 + 512)
TN_SHAPES = ((192, 320, 1280), (192, 1280, 320), (192, 16, 320), (3, 1920, 320), (512, 1152, 384), (512, 384, 128),
             (1056, 768, 3072), (1056, 2304, 768))
TN_PAIR_SHAPES = ((512, 1536, 512, 512), (512, 2304, 768, 768), (1056, 2304, 768, 768))  # (M, N1, N2, K)
TN, COLSUM, PAIR_VS_SINGLE = 3e-5, 1e-5, 2e-5  # tests/test_hip_ops.py test_gemm_tn_and_colsum / test_gemm_tn_pair_matches_two_launches
PAD_P, PAD_Q = 64, 40                          # the padded runs: ldp = N + PAD_P, ldq = K + PAD_Q (column slices of wider buffers)


@functools.lru_cache(maxsize=None)
def tn_operands(M, N, K, salt=0):
    """bf16-rounded dY [M, N] and X [M, K]."""
    gen = torch.Generator().manual_seed(7919 * M + 31 * N + K + salt)
    return bf16r(torch.randn((M, N), generator=gen)), bf16r(torch.randn((M, K), generator=gen))


def tn_reference(M, N, K, dtype, salt=0):
    """(dY^T X, colsum(dY)) in `dtype` from the bf16-rounded operands."""
    dY, X = tn_operands(M, N, K, salt)
    return dY.to(dtype).t() @ X.to(dtype), dY.to(dtype).sum(0)
