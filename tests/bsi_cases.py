"""Seeded cases and fp64 restatements for the kernels of bsi_amd/csrc/bsi_ops.hip (behind bsi_amd.BSI) and bsi_amd/csrc/optim.hip
(the clip + AdamW + EMA step of DPTrainer).  Everything here runs on the CPU: tests/test_bsi_cases_host.py vets the cases on a machine
without a GPU, and tests/test_hip_bsi_kernels.py feeds exactly these inputs to the GPU.

Tolerances follow the rule at the top of tests/algo_cases.py.  A kernel made of IEEE add / mul / fma / div / sqrt alone is held to one
fp32 ulp of the largest term of an fp64 reference that rounds where the kernel rounds (every `*_ref` below returns that reference and
the magnitude).  An output behind expf / logf / erff is held to tol(e_ref) per band.  A sum is held to the number of fp32 roundings on
its longest chain (`*_chain` below), all terms being positive."""
import functools
import math

import numpy as np
import torch

from oracle import bsi_oracle as bo
from tests.algo_cases import GUARD, SENTINEL, tol, worst_rel, f32, nextafter  # noqa: F401  (re-exported to the tests)
from tests.algo_cases import F32, F64, ULP, gen

# The parameters of bsi_params as the c_float fields receive them (the reference holds them in fp32 too: bsi.py:127-135)
_P = bo.LogUniformOracle(1e-2, 1e6)
LAMBDA_0, ALPHA_M, ALPHA_R = f32(1e-2), f32(1e6), f32(2e6)
LN_LOW, DELTA = f32(_P.ln_low), f32(_P.delta)
PARAMS = (LAMBDA_0, ALPHA_M, ALPHA_R, LN_LOW, DELTA)
BYTE_SENTINEL, INT_SENTINEL = 0xA5, -777


def worst_scaled(got, ref, mag):
    """max |got - ref| / mag; where mag is exactly 0 (every term is 0), got has to be exactly 0 too (inf otherwise)."""
    got, ref, mag = got.double().flatten(), ref.double().flatten(), mag.double().flatten()
    zero = mag == 0
    if bool((got[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    return float(((got[~zero] - ref[~zero]).abs() / mag[~zero]).max())


def max3(a, b, c):
    return torch.maximum(torch.maximum(a.abs(), b.abs()), c.abs())


def sqrt32(v):
    """The correctly rounded fp32 square root (through fp64, whose rounding to fp32 cannot double-round a square root or a quotient
    of fp32 numbers).  torch.sqrt on the CPU is not correctly rounded in fp32 on every build: some hand long tensors to a vector
    library that is an ulp off, and the kernels' sqrtf is IEEE."""
    return torch.sqrt(v.double()).float()


def div32(a, b):
    return (torch.as_tensor(a, dtype=F32).double() / torch.as_tensor(b, dtype=F32).double()).float()


def rsqrt32(v):
    """1 / sqrt in fp32, two correctly rounded operations (rsqrt_rn of the kernels)."""
    return div32(1.0, sqrt32(v))


# ----------------------------------------------------------------------------------------------
# Row kernels: q_sample, scale_rows, sample_init, predict_combine (+ bwd), sqerr_rows_bwd
# ----------------------------------------------------------------------------------------------
# (rows, B, D): rows = n B with (n, B) in {(1,1), (1,3), (2,3), (5,3)} so that r % B wraps; D around one block of 256 float4; D = 65540
# enters the stride loop over D of row_grid (64 blocks x 256 threads x 4); 65539 rows enter the stride loop over rows (grid.y cap)
ROW_CASES = [(n * B, B, D) for (n, B) in ((1, 1), (1, 3), (2, 3), (5, 3)) for D in (4, 1020, 1024, 1028)] + [(2, 1, 65540), (65539, 3, 4)]
C_STRIDES = (0, 1, 3)


@functools.lru_cache(maxsize=2)
def row_case(rows, B, D):
    """Inputs of every row kernel at one shape.  Rows of x, mu, f, eps and g differ in their mean and every coefficient differs from
    row to row (by at least 1 between neighbours), so that a wrong row index is a large error."""
    g = gen(100000 + 1000 * B + 7 * rows + D)
    r = torch.arange(rows, dtype=F32)
    d = {"x": torch.randn((B, D), generator=g) + 3 * torch.arange(B, dtype=F32)[:, None]}
    for i, k in enumerate(("mu", "f", "eps", "g")):
        d[k] = torch.randn((rows, D), generator=g) + ((r + i) % 7)[:, None]
    d["lam"] = torch.exp(torch.rand(rows, generator=g) * math.log(1e7) + math.log(0.02)) * (1 + r % 3)
    c = torch.arange(3 * rows, dtype=F32)
    d["cs"] = torch.rand(3 * rows, generator=g) * 0.5 + 0.25 + 2 * (c % 13)      # read at r * c_stride
    d["co"] = -(torch.rand(3 * rows, generator=g) * 0.5 + 0.5 + 2 * (c % 11))
    d["w"] = torch.rand(rows, generator=g) * 0.5 + 0.5 + 2 * (r % 5)
    d["gup"] = torch.rand(rows, generator=g) * 0.5 + 0.25 + 2 * (r % 3)
    return d


def coef_rows(c, rows, stride):
    return c[torch.arange(rows) * stride]


def q_sample_ref(x, lam, eps, B):
    """bsi.py:405-420: addcmul((lam - lambda_0) / lam * x, rsqrt(lam), eps) -> (fp64 reference, magnitude, the fp32 CPU sequence)."""
    rows = len(lam)
    a, s = div32(lam - LAMBDA_0, lam), rsqrt32(lam)
    ax = a[:, None] * x[torch.arange(rows) % B]
    se = s.double()[:, None] * eps.double()
    ref = ax.double() + se
    return ref, max3(ax.double(), se, ref), torch.addcmul(ax, s[:, None], eps)


def scale_ref(c, v):
    """c[r] * v[r, :] (bsi_scale_rows, and the two outputs of bsi_predict_combine_bwd)."""
    ref = c.double()[:, None] * v.double()
    return ref, ref.abs(), c[:, None] * v


def sample_init_ref(eps0, lam):
    """bsi.py:325: rsqrt(lam[0]) * eps0."""
    s = rsqrt32(lam[0])
    ref = s.double() * eps0.double()
    return ref, ref.abs(), s * eps0


def combine_ref(mu, f, cs, co):
    """bsi.py:375-388: addcmul(c_skip * mu, c_out, f)."""
    am = cs[:, None] * mu
    bf = co.double()[:, None] * f.double()
    ref = am.double() + bf
    return ref, max3(am.double(), bf, ref), torch.addcmul(am, co[:, None], f)


def sqerr_bwd_ref(x, xh, w, gup, scale, mean, B):
    """d/dx_hat of w[r] scale reduce_D (x[r % B] - x_hat[r])^2 times the upstream gradient: coef (x - x_hat), the coefficient formed
    as ((-2 g) w) scale [/ D] in fp32 like the kernel."""
    rows, D = xh.shape
    coef = (-2.0 * gup) * (w if w is not None else torch.ones(rows)) * scale
    if mean:
        coef = div32(coef, float(D))
    diff = x[torch.arange(rows) % B] - xh
    ref = coef.double()[:, None] * diff.double()
    return ref, ref.abs(), coef[:, None] * diff


# ----------------------------------------------------------------------------------------------
# bsi_refine_step(_philox), bsi_philox_normal / _uint32
# ----------------------------------------------------------------------------------------------
CAP4 = 4096 * 256 * 4  # elements one pass of the capped grids of refine_step / philox covers (4096 blocks x 256 threads x float4)
REFINE_SHAPES = ((1, 4), (1, 1028), (4, 3), (1, 4 * 1048576 + 4), (1, 8 * 1048576 + 1028))  # (rows, D); the last two pass CAP4
REFINE_K = 8
REFINE_STEPS = (0, 4, 7)  # first, a middle and the last step
PHILOX_N = 4 * 1048576 + 1028
PHILOX_SEED = 0x0123456789ABCDEF


@functools.lru_cache(maxsize=None)
def refine_tables():
    """lam, alpha, c_skip, c_out of a schedule of 8 steps (fp32, as BSI.sample hands them to the kernel)."""
    t = torch.linspace(0, 1, REFINE_K + 1)
    lam = torch.exp(DELTA * t + LN_LOW)
    o = bo.BSIOracle(None, data_shape=(1,))
    cs, co, _ = o.edm_coeffs(t)
    return lam, lam.diff(), cs, co


@functools.lru_cache(maxsize=1)
def refine_case(rows, D):
    g = gen(4000 + (rows * D) % 9973)
    n = rows * D
    return tuple(torch.randn(n, generator=g) * s for s in (3.0, 1.0, 1.0))  # mu, f, eps


def refine_ref(mu, f, eps, i, f_is_xhat):
    """bsi.py:331-335.  x_hat = f, or addcmul(c_skip mu, c_out, f); y = x_hat + fl(rsqrt(alpha) eps); mu' = fl(fl(alpha y) + fl(lam_i mu))
    / lam_{i+1}.  Each stage's reference starts from the fp32 value of the stage before -> {name: (ref, magnitude)}."""
    lam, alpha, cs, co = refine_tables()
    if f_is_xhat:
        xh = f.double()
        xh_mag = xh.abs()
    else:
        am = cs[i] * mu
        bf = co[i].double() * f.double()
        xh = am.double() + bf
        xh_mag = max3(am.double(), bf, xh)
    xh32 = xh.float()
    re = rsqrt32(alpha[i]) * eps
    y = xh32.double() + re.double()
    y32 = y.float()
    s = alpha[i] * y32 + lam[i] * mu
    mn = s.double() / lam[i + 1].double()  # the kernel's quotient is this, rounded
    return {"xh": (xh, xh_mag), "y": (y, max3(xh32.double(), re.double(), y)), "mn": (mn, mn.abs())}


# ----------------------------------------------------------------------------------------------
# bsi_sqerr_rows
# ----------------------------------------------------------------------------------------------
SQERR_DS = (4, 252, 256, 1024, 1028, 12288)
SQERR_N, SQERR_B = 2, 3


def sqerr_case(D):
    g = gen(5000 + D)
    rows = SQERR_N * SQERR_B
    x = torch.rand((SQERR_B, D), generator=g) * 2 - 1
    xh = x.repeat(SQERR_N, 1) + 0.05 * (1 + torch.arange(rows, dtype=F32))[:, None] * torch.randn((rows, D), generator=g)
    w = torch.rand(rows, generator=g) + 0.5 + torch.arange(rows, dtype=F32)
    return x, xh, w


def sqerr_ref(x, xh, w, scale, mean):
    s = (x.double().repeat(SQERR_N, 1) - xh.double()).square()
    red = s.mean(1) if mean else s.sum(1)
    return scale * (w.double() if w is not None else 1.0) * red


def sqerr_chain(D):
    """fp32 roundings on the longest chain of sqerr_rows_kernel: a thread adds 4 squares per float4 and ceil(D / 1024) float4 (256
    threads), the wave sum is 6 levels, the four wave sums are added in order (4), then / D, scale * w and the final product (3), and
    each square carries the rounding of its difference twice (2).  All terms are positive: the relative error is below that many
    half-ulps (to first order; 1 % is added for the higher orders)."""
    return 4 * -(-D // 1024) + 6 + 4 + 3 + 2


def chain_limit(count):
    return count * ULP * 1.01


# ----------------------------------------------------------------------------------------------
# bsi_recon_nll
# ----------------------------------------------------------------------------------------------
RECON_KS = (2, 256)
RECON_DS = (1, 3, 255, 256, 257, 1000)
RECON_N, RECON_B = 16, 16  # 256 rows: one band per (k, D)
PAD_BOUNDS = 1  # the table on the device has one more entry than the kernel may read
SIGMA_R = float(rsqrt32(torch.tensor(ALPHA_R)))


def recon_disc(k):
    return bo.Disc(-1.0, 1.0, k)


def recon_edges(k):
    """Indices j of boundaries b[j] (fp32) that lie in bin j in fp32 and in fp64 alike: values exactly on a bin edge that are no
    coin toss."""
    d = recon_disc(k)
    b = d.bin_boundaries(F32)[1:k]
    j = torch.arange(1, k)
    ok = (d.bucketize(b) == d.bucketize(b.double())) & (d.bucketize(b) == j)
    return j[ok]


@functools.lru_cache(maxsize=None)
def recon_case(k, D):
    """x [B, D]: bin centres + U(-0.4, 0.4) dx over bins spread across the range; planted: both extremes, 3.5 dx outside the range on
    either side, one bin past either end (dx outside: the unclamped index is -1 and k), and values exactly on bin edges.
    x_hat [n B, D] is placed relative to the boundary that decides the probability of the bin of x (the inner one for the end bins): z
    standard deviations inside (+) or outside (-) it, |z| of ONE order per row -- in [0.1, 1) for rows r % 4 in (0, 1), in [1, 3.5)
    for r % 4 == 2, with a random sign -- so that every row's sum is made of terms of its own size (an element deep inside its bin
    contributes 1e-8, which is 0 in fp32: a row of those alone cannot be compared relatively by anyone; where D >= 8 a fifth of the
    elements of these rows is such an element).  Rows r % 4 == 3 are 100 to 1000 standard deviations OUTSIDE throughout: the
    probability is 0 in both precisions and the 1e-20 floor takes over."""
    d = recon_disc(k)
    g = gen(6000 + 17 * k + D)
    B, n = RECON_B, RECON_N
    m = B * D
    idx = (torch.linspace(0, k - 1, m).round() if m >= k else torch.randint(0, k, (m,), generator=g).float())[torch.randperm(m, generator=g)]
    x = (d.lo + idx * d.dx + (torch.rand(m, generator=g) * 0.8 - 0.4) * d.dx).to(F32)
    bounds = d.bin_boundaries(F32)
    edges = recon_edges(k)
    special = [d.lo, d.hi, d.lo - 3.5 * d.dx, d.hi + 3.5 * d.dx, d.hi + d.dx, d.lo - d.dx]
    special += [float(bounds[j]) for j in edges[torch.linspace(0, len(edges) - 1, min(4, len(edges))).round().long()]]
    x[:len(special)] = torch.tensor(special, dtype=F32)
    x = x.reshape(B, D)
    bi = d.bucketize(x)                                                   # [B, D]
    right = torch.randint(0, 2, (n * B, D), generator=g).bool()           # which boundary of the bin decides
    bi_r = bi.repeat(n, 1)
    right = (right | (bi_r == 0)) & ~(bi_r == k - 1)
    edge = torch.where(right, bounds[bi_r + 1], bounds[bi_r])
    r = torch.arange(n * B)[:, None]
    u = torch.rand((n * B, D), generator=g)
    zmag = torch.where(r % 4 == 2, 1.0 + 2.5 * u, 0.1 + 0.9 * u)
    sign = torch.randint(0, 2, (n * B, D), generator=g).float() * 2 - 1
    z = zmag * sign
    if D >= 8:
        deep = torch.rand((n * B, D), generator=g) < 0.2
        half = 0.5 * d.dx / SIGMA_R
        z = torch.where(deep, torch.full_like(z, min(5.0, half)), z)
    z = torch.where(r % 4 == 3, -(100.0 + 900.0 * u), z)
    x_hat = (edge + torch.where(right, -1.0, 1.0) * z * SIGMA_R).to(F32)
    return x, x_hat.contiguous(), z


def recon_eval(x, x_hat, k, dtype):
    """bsi.py:230-247 after x_hat, in `dtype` on the fp32 inputs -> [n B].  k = 0: Normal(x_hat, sigma).log_prob(x)."""
    rows, D = x_hat.shape
    xr = x.repeat(rows // len(x), 1).to(dtype)
    m = x_hat.to(dtype)
    sigma = 1.0 / torch.sqrt(torch.tensor(ALPHA_R, dtype=dtype))
    if k == 0:
        logp = -((xr - m) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - math.log(math.sqrt(2 * math.pi))
        return (-logp).sum(dim=1)
    d = recon_disc(k)
    bounds = d.bin_boundaries(F32).to(dtype)
    idx = d.bucketize(x).repeat(rows // len(x), 1)

    def ncdf(v):
        return 0.5 * (1 + torch.erf((v - m) * (1.0 / sigma) / math.sqrt(2)))

    cl = torch.where(idx == 0, torch.zeros((), dtype=dtype), ncdf(bounds[idx]))
    cr = torch.where(idx == k - 1, torch.ones((), dtype=dtype), ncdf(bounds[idx + 1]))
    return (-torch.log(torch.clamp(cr - cl, min=1e-20))).sum(dim=1)


@functools.lru_cache(maxsize=None)
def recon_band(k, D, form):
    """(x, x_hat, ref64, e_ref) of band (k, D); form "disc" or "cont" (k = 0 on the same inputs)."""
    x, x_hat, _ = recon_case(k, D)
    kk = k if form == "disc" else 0
    r64 = recon_eval(x, x_hat, kk, F64)
    return x, x_hat, r64, worst_rel(recon_eval(x, x_hat, kk, F32), r64)


# ----------------------------------------------------------------------------------------------
# bsi_to_uint8
# ----------------------------------------------------------------------------------------------
U8_NS = (1, 255, 257, 1048576 * 4 + 3)
U8_LO, U8_HI = -1.0, 1.0


def u8_planted():
    """The 256 level values with their fp32 neighbours on both sides, and values outside [lo, hi]."""
    lv = (U8_LO + torch.arange(256, dtype=F64) * (U8_HI - U8_LO) / 255).to(F32)
    inf = torch.tensor(math.inf)
    outside = torch.tensor([-1.3, 1.3, -1e30, 1e30, nextafter(U8_LO, -math.inf), nextafter(U8_HI, math.inf)], dtype=F32)
    return torch.cat([lv, torch.nextafter(lv, -inf), torch.nextafter(lv, inf), outside])


def u8_case(n):
    p = u8_planted()
    if n <= len(p):
        return p[torch.linspace(0, len(p) - 1, n).round().long()] if n > 1 else p[255:256].clone()  # n = 1: the top level, 1.0
    x = torch.rand(n, generator=gen(70 + n % 9973)) * 2.6 - 1.3
    pos = torch.linspace(0, n - 1, len(p)).round().long()  # the first and the last element included
    x[pos] = p
    return x


def u8_ref(x):
    return recon_disc(256).to_8bit_image(x)


# ----------------------------------------------------------------------------------------------
# bsi_edm_coeffs, bsi_lambda_to_t, bsi_schedule, bsi_lambda_grid
# ----------------------------------------------------------------------------------------------
COEFF_NS = (1, 255, 256, 257, 1000)
T_DECADES = tuple(range(-6, 0))  # band e: t in [10^e, 10^(e+1)]
EDM_NAMES = ("lam", "c_skip", "c_out", "c_in")


def icdf(t, dtype):
    """bsi.py:83-84: exp(delta t + ln_low), mul and add rounded separately."""
    return torch.exp(DELTA * t.to(dtype) + LN_LOW)


def band_t(e):
    """256 log-uniform times of decade e; the last decade also holds 1.  (t = 0 is in no decade: edm_t() plants it.)"""
    u = torch.rand(256, generator=gen(800 + e), dtype=F64)
    t = (10.0 ** (e + u)).to(F32).clamp(f32(10.0 ** e), f32(10.0 ** (e + 1)))
    return torch.cat([t, torch.ones(1)]) if e == T_DECADES[-1] else t


@functools.lru_cache(maxsize=None)
def edm_t():
    """[(t, band)] per n of COEFF_NS: the points of all decades and t = 0 (band -7), shuffled and dealt out in pieces of those
    lengths (1769 places for 1538 points: every point is run, some twice)."""
    t = torch.cat([torch.zeros(1)] + [band_t(e) for e in T_DECADES])
    band = torch.cat([torch.full((1,), -7)] + [torch.full((len(band_t(e)),), e) for e in T_DECADES])
    order = torch.randperm(len(t), generator=gen(801))
    order = torch.cat([order, order])[:sum(COEFF_NS)]
    assert sum(COEFF_NS) >= len(t)
    out, at = [], 0
    for n in COEFF_NS:
        pick = order[at:at + n]
        out.append((t[pick].clone(), band[pick].clone()))
        at += n
    return out


def edm_eval(t, dtype, lam=None):
    """bsi.py:390-403 per time (from `lam` where given, instead of from t)."""
    lam = icdf(t, dtype) if lam is None else lam.to(dtype)
    alpha = lam - LAMBDA_0
    kappa = 1 + alpha * (alpha / lam)
    return {"lam": lam, "c_skip": alpha / kappa, "c_out": 1.0 / torch.sqrt(kappa), "c_in": torch.sqrt(lam / kappa)}


def to_t_eval(lam, dtype):
    """bsi.py:76-81: cdf and reciprocal pdf of the log-uniform distribution."""
    lam = lam.to(dtype)
    return {"t": (torch.log(lam) - LN_LOW) / DELTA, "rpdf": lam * DELTA}


@functools.lru_cache(maxsize=None)
def edm_band(e):
    """{name: e_ref} of decade e: the four coefficients, the inverse (lambda_to_t of the fp32 lambda) and the round trip
    lambda_to_t(icdf(t)) against t itself."""
    t = band_t(e)
    lo, hi = edm_eval(t, F32), edm_eval(t, F64)
    out = {k: worst_rel(lo[k], hi[k]) for k in EDM_NAMES}
    lam = lo["lam"]
    lo_t, hi_t = to_t_eval(lam, F32), to_t_eval(lam, F64)
    out.update({k: worst_rel(lo_t[k], hi_t[k]) for k in ("t", "rpdf")})
    out["round_trip"] = worst_rel(lo_t["t"], t)
    return out


# At t = 0 lambda is lambda_0 up to the rounding of expf, so alpha = lam - lambda_0 and t' = (log lam - ln_low) / delta are rounding
# noise of either sign in every precision and have no relative error to speak of.  There c_skip is held to the kernel's own lambda
# instead (alpha is an exact difference, then four roundings: below 8 * 2^-24 of the fp64 formula on that lambda -- and this is
# asserted at every t, which pins c_skip where e_ref is large), and t' to an absolute bound: logf within 2 ulp of |ln_low| (2^-21
# each, ln_low = -4.6), the subtraction of ln_low exact, the division one more rounding.
T0_ABS = 2.5 * 2.0 ** -21 / DELTA
OWN_LAM_LIMIT = 8 * ULP

SCHED_K1S = COEFF_NS


def schedule_band_ts(k1):
    """The schedules of band k1: linspace(0, 1, k1) (0.5 alone at k1 = 1) and, below 256 times, seeded sub-intervals of it."""
    base = torch.linspace(0, 1, k1) if k1 > 1 else torch.tensor([0.5])
    out = [base]
    g = gen(9700 + k1)
    while sum(len(s) for s in out) < 256:
        w = 0.5 + 0.5 * float(torch.rand((), generator=g))
        lo = (1 - w) * float(torch.rand((), generator=g))
        out.append((base.double() * w + lo).to(F32))
    return out


def schedule_eval(t, dtype):
    lam = icdf(t, dtype)
    return {"lam": lam, "alpha": lam.diff()}


@functools.lru_cache(maxsize=None)
def schedule_band(k1):
    lo = [schedule_eval(t, F32) for t in schedule_band_ts(k1)]
    hi = [schedule_eval(t, F64) for t in schedule_band_ts(k1)]
    return {n: worst_rel(torch.cat([d[n] for d in lo]), torch.cat([d[n] for d in hi])) for n in ("lam", "alpha")}


GRID_TOTALS = (1, 255, 256, 257, 1000)
GRID_OFFSETS = (0.0, 0.5, nextafter(1.0, 0.0))


def grid_perm(total):
    return torch.randperm(total, generator=gen(900 + total))


def grid_offsets(total):
    """The three offsets and, below 256 points, seeded ones in [0, 1)."""
    out = list(GRID_OFFSETS)
    g = gen(950 + total)
    while len(out) * total < 256:
        out.append(float(torch.rand((), generator=g)))
    return out


def grid_eval(perm, offset, dtype):
    """bsi.py:434-439 -> (t before the exponential, its integer part before the remainder, lambda)."""
    s = perm.to(dtype) / (1 + perm.numel()) + torch.tensor(offset, dtype=F32).to(dtype)
    t = torch.remainder(s, 1)
    return t, torch.floor(s), icdf(t, dtype)


@functools.lru_cache(maxsize=None)
def grid_band(total):
    perm = grid_perm(total)
    lo = torch.cat([grid_eval(perm, o, F32)[2] for o in grid_offsets(total)])
    hi = torch.cat([grid_eval(perm, o, F64)[2] for o in grid_offsets(total)])
    return worst_rel(lo, hi)


# ----------------------------------------------------------------------------------------------
# optim.hip: bsi_grad_sqnorm, bsi_clip_adamw_ema and the segment forms
# ----------------------------------------------------------------------------------------------
ADAM_NS = (1, 3, 4, 5, 1023, 1048576 + 5, 2 * 1048576 + 77)  # the last two pass 1024 x 256 x 4 (norm), the last 8192 x 256 (update)
ADAM_BAND_NS = ADAM_NS[:5]  # the points e_ref is taken over: 1036 per option set, step and output
BASE = dict(ratio=10.0, max_norm=1.0, grad_scale=1.0, lr=5e-4, beta1=0.9, beta2=0.99, eps=1e-8, wd=1e-2, ema=True, ema_w=(1.0, 1.0, 0.25),
            steps=(1, 2, 3))
# ratio: gradient norm (times grad_scale) over max_norm
ADAM_OPTS = {"clip_active": {}, "clip_inactive": dict(ratio=0.1), "no_clip": dict(max_norm=0.0), "grad_scale": dict(grad_scale=0.125),
             "wd0": dict(wd=0.0), "ema_null": dict(ema=False), "ema_weights": dict(ema_w=(-1.0, 0.25, 1.0)), "steps": dict(steps=(1, 2, 1000))}
ADAM_NAMES = ("p", "m", "v", "ema")


def adam_opt(name):
    return {**BASE, **ADAM_OPTS[name]}


def zero_block(n):
    """Elements whose gradient is 0 at every step (v = 0: denom = eps)."""
    return slice(n // 2, n // 2 + max(1, min(300, n // 8))) if n >= 3 else slice(0, 0)


@functools.lru_cache(maxsize=4)
def adam_case(n, name):
    """p0, the initial EMA and the gradients of the three steps; the norm of a gradient times grad_scale is ratio x max_norm
    (x 1 where max_norm is 0) up to rounding."""
    o = adam_opt(name)
    g = gen(11000 + n % 9973)
    p0 = torch.randn(n, generator=g)
    e0 = torch.randn(n, generator=g)
    grads = []
    for s in range(3):
        gr = torch.randn(n, generator=g).double()
        gr[zero_block(n)] = 0
        if not bool(gr.any()):
            gr[0] = 1.0
        target = o["ratio"] * (o["max_norm"] if o["max_norm"] > 0 else 1.0) / o["grad_scale"]
        grads.append((gr * (target / gr.norm())).to(F32))
    return p0, e0, grads


def sq64(g):
    return g.double().square().sum()


def adam_step(state, g, sq, o, i, dtype):
    """One call of the fused kernel, operation for operation (no contraction), in `dtype` on fp32 arguments.  state = (p, m, v, ema);
    sq is the squared norm the kernel is given.  -> (new state, magnitudes each output's error is relative to: the largest term of
    its last sum and the output itself)."""
    def T(v):
        return torch.tensor(v, dtype=F32).to(dtype)

    p, m, v, ema = state
    sqrt = sqrt32 if dtype == F32 else torch.sqrt
    gs, lr, b1, b2, eps, wd, one = T(o["grad_scale"]), T(o["lr"]), T(o["beta1"]), T(o["beta2"]), T(o["eps"]), T(o["wd"]), T(1.0)
    step = o["steps"][i]
    bc1 = torch.tensor(1.0 - f32(o["beta1"]) ** step, dtype=F64).to(dtype)          # formed in double by the host wrapper
    sqrt_bc2 = torch.tensor(math.sqrt(1.0 - f32(o["beta2"]) ** step), dtype=F64).to(dtype)
    coef = gs
    if o["max_norm"] > 0:
        total = sqrt(sq.to(dtype)) * gs
        coef = coef * torch.minimum(T(o["max_norm"]) / (total + T(1e-6)), one)
    stp, decay = lr / bc1, one - lr * wd
    gi = g.to(dtype) * coef
    pd = p * decay
    t1, t2 = b1 * m, (one - b1) * gi
    mi = t1 + t2
    vi = b2 * v + (one - b2) * gi * gi
    denom = sqrt(vi) / sqrt_bc2 + eps
    upd = stp * (mi / denom)
    pi = pd - upd
    mag_p = max3(pd, upd, pi)
    w = o["ema_w"][i]
    if not o["ema"] or w < 0:
        en, mag_e = ema, ema.abs()
    elif w >= 1.0:
        en, mag_e = pi, mag_p
    else:
        en = ema + T(w) * (pi - ema)
        mag_e = torch.maximum(max3(ema, pi, en), mag_p)
    return (pi, mi, vi, en), (mag_p, max3(t1, t2, mi), vi.abs(), mag_e)


def adam_start(n, name, dtype=F32):
    p0, e0, _ = adam_case(n, name)
    return (p0.to(dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), e0.to(dtype))


def adam_ref(state32, n, name, i, sq):
    """Call i in fp64 from the fp32 state the call is given (every call is compared on its own inputs: carried over three calls, the
    error of a moment that cancelled would be measured against a later, smaller magnitude, and the worst of 2 M such ratios has no
    bound that 1 000 points could calibrate)."""
    return adam_step(tuple(t.double() for t in state32), adam_case(n, name)[2][i], sq, adam_opt(name), i, F64)


def _adam_run(n, name):
    grads = adam_case(n, name)[2]
    state = adam_start(n, name)
    out = []
    for i in range(3):
        ref, mags = adam_ref(state, n, name, i, sq64(grads[i]))
        state, _ = adam_step(state, grads[i], sq64(grads[i]).float(), adam_opt(name), i, F32)
        out.append((state, ref, mags))
    return out


_adam_run_small = functools.lru_cache(maxsize=None)(_adam_run)


def adam_run(n, name):
    """Three consecutive calls from zero moments in fp32 on the CPU: [(state after the call, fp64 reference from the state before it,
    magnitudes)].  The squared norm is the fp64 sum, rounded to fp32 for the fp32 run (what a correctly rounded norm kernel hands
    over)."""
    return (_adam_run_small if n <= ADAM_BAND_NS[-1] else _adam_run)(n, name)


@functools.lru_cache(maxsize=None)
def adam_band(name, n):
    """{(call, output): e_ref} of the band n belongs to: the points of ADAM_BAND_NS together, or those of a larger n alone (an update
    is a dozen roundings, and the worst of 2 M elements is several times the worst of 1 000: 6.6e-7 against 1.1e-7 for p)."""
    ns = ADAM_BAND_NS if n in ADAM_BAND_NS else (n,)
    runs = [adam_run(m, name) for m in ns]
    return {(i, k): max(worst_scaled(r[i][0][j], r[i][1][j], r[i][2][j]) for r in runs) for i in range(3) for j, k in enumerate(ADAM_NAMES)}


def decay_only(p0, o, calls):
    """p of the zero-gradient block after `calls` calls, in fp32: p * (1 - lr wd) per call and nothing else."""
    decay = torch.tensor(1.0) - torch.tensor(o["lr"], dtype=F32) * torch.tensor(o["wd"], dtype=F32)
    p = p0.clone()
    for _ in range(calls):
        p = p * decay
    return p


def sqnorm_chain_flat(n):
    """fp32 roundings on the longest chain of bsi_grad_sqnorm: a thread adds 4 squares per float4 and ceil(n4 / threads) float4, one
    more for the ragged tail, 6 levels of the wave sum, 2 of the block sum; the partials are added in double and rounded once."""
    n4 = n // 4
    grid = max(1, min(1024, -(-n4 // 256)))
    return 4 * -(-n4 // (grid * 256)) + 1 + 6 + 2 + 1


# One chunk of a segment: 256 threads x 16 float4 (BSI_SQNORM_CHUNK of include/bsi_hip.h)
CHUNK = 16384
SQNORM_CHAIN_CHUNK = 64 + 6 + 2      # 16 float4 x 4 squares per thread, the wave sum, the block sum
SQNORM_CHAIN_SEGMENTS = SQNORM_CHAIN_CHUNK + 1   # the finish adds the partials in double and rounds once
NSEG = 8200
SPECIAL_LENS = {0: CHUNK + 4, 77: CHUNK - 4, 4100: CHUNK, 8000: 3 * CHUNK + 8, NSEG - 1: CHUNK + 4}


@functools.lru_cache(maxsize=None)
def seg_table():
    """8200 segments of 4 .. 64 elements (a few of CHUNK - 4, CHUNK, CHUNK + 4 and 3 CHUNK + 8), more than 8192 chunks in all.  In
    p / m / v / ema a gap of 4 .. 32 floats lies before, between and behind the segments; the gradient is packed; the partials of the
    segments land in a seeded order of the segments, not in table order.
    -> rows (p_off, g_off, len, my_chunk, out_chunk), floats of p, floats of g, chunks."""
    g = gen(8200)
    lens = (torch.randint(1, 17, (NSEG,), generator=g) * 4).tolist()
    for i, ln in SPECIAL_LENS.items():
        lens[i] = ln
    gaps = (torch.randint(1, 9, (NSEG + 1,), generator=g) * 4).tolist()
    nch = [-(-ln // CHUNK) for ln in lens]
    out_at = [0] * NSEG
    at = 0
    for i in torch.randperm(NSEG, generator=g).tolist():
        out_at[i] = at
        at += nch[i]
    rows, po, go, ch = [], gaps[0], 0, 0
    for i in range(NSEG):
        rows.append((po, go, lens[i], ch, out_at[i]))
        po += lens[i] + gaps[i + 1]
        go += lens[i]
        ch += nch[i]
    return rows, po, go, ch


def seg_index():
    """Positions in p of the elements of g, in the order of g (the gather that makes the flat problem)."""
    rows, *_ = seg_table()
    return torch.cat([torch.arange(po, po + ln) for po, _, ln, _, _ in rows])


def seg_partials64(g):
    """The partial of every chunk, where the table puts it, in fp64."""
    rows, _, _, chunks = seg_table()
    out = torch.zeros(chunks, dtype=F64)
    sq = g.double().square()
    for _, go, ln, _, oc in rows:
        for k in range(-(-ln // CHUNK)):
            out[oc + k] = sq[go + k * CHUNK:go + min(ln, (k + 1) * CHUNK)].sum()
    return out


def philox_uint32(seed, stream, n):
    from oracle import philox_oracle as po
    return po.stream_uint32(seed, stream, n)


def philox_normals(u):
    from oracle import philox_oracle as po
    return po.normals_from_uint32(np.asarray(u))
