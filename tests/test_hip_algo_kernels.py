"""Each kernel of bsi_amd/csrc/algo_ops.hip (behind bsi_amd.VDM and bsi_amd.BFN) through the C ABI against fp64, on the cases of
tests/algo_cases.py (vetted on the CPU by tests/test_algo_cases_host.py).  Plain arithmetic outputs have bounds derived from their
roundings; transcendental outputs follow the tolerance rule of tests/algo_cases.py.  Every output is allocated with 8 guard floats
behind its last element, which have to stay untouched; nullable output pointers are run as the subsets the wrappers use, and the
outputs that remain have to equal the all-pointers call bit for bit."""
import pytest
import torch

from tests import algo_cases as ac
from tests.util import Out, bound, release, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
LE_ULP = 2.0 ** -23 * (1 + 1e-9)  # bound() asserts "<": this is "<= one ulp"


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


_KEEP = []  # device copies stay alive until the test ends (kernels are enqueued asynchronously)


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    release()
    _KEEP.clear()


def dev(t):
    d = t.to(DEV).contiguous()
    _KEEP.append(d)
    return d


def bits(t):
    return t.contiguous().view(torch.int32)


def refused(N, rc, what):
    assert rc != 0, f"{what} was accepted"
    msg = N.lib().bsi_last_error()
    assert msg and what.split(":")[0] in msg.decode(), (what, msg)


# ----------------------------------------------------------------------------------------------
# plain arithmetic kernels
# ----------------------------------------------------------------------------------------------
def test_tgrid(N):
    equal = total_n = 0
    for total in ac.TGRID_TOTALS:
        perm = ac.tgrid_case(total)
        dperm = dev(perm)
        for offset in ac.TGRID_OFFSETS:
            out = Out(total)
            N.check(N.lib().bsi_tgrid(N.ptr(dperm), N.ptr(dev(torch.tensor(offset, dtype=F32))), total, out.ptr, N.stream()))
            t, ref = out.get(), ac.tgrid_ref(perm, offset)
            assert bool(((t >= 0) & (t < 1)).all()), (total, offset)
            # same three fp32 operations (IEEE division, no contraction): one ulp below 1 is the most two correct roundings differ by
            bound("tgrid:abs", float((t - ref).abs().max()), LE_ULP)
            equal += int((bits(t) == bits(ref)).sum())
            total_n += total
    report("algo_kernels_tgrid", bit_equal=equal, values=total_n)


def test_affine_noise(N):
    for n, B, D in ac.AFFINE_CASES:
        x, a, b, eps = ac.affine_case(n, B, D)
        rows = n * B
        out = Out(rows * D)
        N.check(N.lib().bsi_affine_noise(N.ptr(dev(x)), N.ptr(dev(a)), N.ptr(dev(b)), N.ptr(dev(eps)), rows, B, D, out.ptr, N.stream()))
        ref, mag = ac.affine_ref(x, a, b, eps, B)
        got = out.get().reshape(rows, D).double()
        # one fma on fl32(a x): half an ulp of the result; the bound is a whole ulp of the largest term
        bound("affine_noise:ulp", float(((got - ref).abs() / mag.clamp_min(1e-30)).max()), LE_ULP)
    x, a, b, eps = ac.affine_case(1, 1, 8)
    out = Out(8)
    refused(N, N.lib().bsi_affine_noise(N.ptr(dev(x)), N.ptr(dev(a)), N.ptr(dev(b)), N.ptr(dev(eps)), 1, 1, 6, out.ptr, N.stream()),
            "bsi_affine_noise: D = 6")
    assert bool((out.get() == ac.SENTINEL).all())


@pytest.mark.parametrize("n", ac.AXPBYPCZ_NS)
def test_axpbypcz(N, n):
    z, xh, eps, a, b, c = ac.axpbypcz_case(n)
    dz, dx, de, da, db, dc = (dev(v) for v in (z, xh, eps, a, b, c))
    for idx in ac.AXPBYPCZ_IDX:
        out = Out(n)
        N.check(N.lib().bsi_axpbypcz(N.ptr(dz), N.ptr(dx), N.ptr(de), N.ptr(da), N.ptr(db), N.ptr(dc), idx, n, out.ptr, N.stream()))
        ref, mag = ac.axpbypcz_ref(z, xh, eps, a[idx], b[idx], c[idx])
        bound("axpbypcz:ulp", float(((out.get().double() - ref).abs() / mag.clamp_min(1e-30)).max()), LE_ULP)
    if n == ac.AXPBYPCZ_NS[0]:
        out = Out(8)
        refused(N, N.lib().bsi_axpbypcz(N.ptr(dz), N.ptr(dx), N.ptr(de), N.ptr(da), N.ptr(db), N.ptr(dc), 0, 6, out.ptr, N.stream()),
                "bsi_axpbypcz: n = 6")


@pytest.mark.parametrize("lo,hi", ac.CLIP_BOUNDS)
def test_clip_and_backward(N, lo, hi):
    """Forward against torch.clamp on the CPU bit for bit: a NaN stays a NaN (any NaN: the payload torch returns depends on its
    vector width), every other element has the CPU's bits, the sign of a zero included.  Backward against the CPU autograd."""
    for n in ac.CLIP_NS:
        x, grad = ac.clip_case(n, lo, hi)
        y_ref, g_ref = ac.clip_ref(x, grad, lo, hi)
        dx, dg = dev(x), dev(grad)
        out, gout = Out(n), Out(n)
        N.check(N.lib().bsi_clip(N.ptr(dx), lo, hi, n, out.ptr, N.stream()))
        N.check(N.lib().bsi_clip_bwd(N.ptr(dg), N.ptr(dx), lo, hi, n, gout.ptr, N.stream()))
        y, g = out.get(), gout.get()
        nan = torch.isnan(y_ref)
        assert bool(nan.any()) and torch.equal(torch.isnan(y), nan), (n, "NaN inputs have to stay NaN")
        assert torch.equal(bits(y)[~nan], bits(y_ref)[~nan]), (n, lo, hi)
        assert torch.equal(g, g_ref), (n, lo, hi)
        assert float(g[torch.isnan(x)].abs().max()) == 0.0
    out = Out(4)
    refused(N, N.lib().bsi_clip(N.ptr(dx), 1.0, -1.0, 1, out.ptr, N.stream()), "bsi_clip: lo > hi")


@pytest.mark.parametrize("rows,D", ac.PRIOR_CASES)
def test_vdm_prior(N, rows, D):
    x = ac.prior_case(rows, D)
    dx = dev(x)
    for var1 in ac.prior_vars():
        out = Out(rows)
        N.check(N.lib().bsi_vdm_prior(N.ptr(dx), var1, rows, D, out.ptr, N.stream()))
        # an fp32 sum of D positive terms of similar size: D half-ulps at worst, with margin
        bound(f"vdm_prior:rel:D{D}", ac.worst_rel(out.get(), ac.prior_ref(x, var1)), D * 2.0 ** -24 * 4)


# ----------------------------------------------------------------------------------------------
# VDM coefficients
# ----------------------------------------------------------------------------------------------
def run_vdm_coeffs(N, dt, names):
    outs = {k: Out(dt.numel()) for k in names}
    p = [outs[k].ptr if k in outs else None for k in ac.VDM_COEFF_NAMES]
    N.check(N.lib().bsi_vdm_coeffs(N.ptr(dt), dt.numel(), ac.G0, ac.G1, *p, N.stream()))
    return {k: o.get() for k, o in outs.items()}


def test_vdm_coeffs(N):
    e_ref = ac.vdm_coeffs_band()
    report("algo_kernels_e_ref_vdm_coeffs", **e_ref)
    for n in ac.VDM_COEFF_NS:
        t = ac.vdm_coeff_t(n)
        dt = dev(t)
        full = run_vdm_coeffs(N, dt, ac.VDM_COEFF_NAMES)
        ref = ac.vdm_coeffs_eval(t, F64)
        for k in ac.VDM_COEFF_NAMES:
            bound(f"vdm_coeffs:{k}", ac.worst_rel(full[k], ref[k]), ac.tol(e_ref[k]))
        for names in ac.VDM_COEFF_SUBSETS[:-1]:
            part = run_vdm_coeffs(N, dt, names)
            for k in names:
                assert torch.equal(bits(part[k]), bits(full[k])), (n, names, k)
        # gamma around t = 0.5, where torch.lerp changes its formula: snr = exp(-gamma), so a gamma from the other formula (two ulp
        # of gamma away at 0.5, 9.5e-7) moves snr by that much relatively; two correct expf differ by 2 ulp = 2^-22 at the most
        at = torch.isin(t, torch.tensor(ac.HALF3))
        assert int(at.sum()) == (1 if n == 1 else 3)
        ref32 = ac.vdm_coeffs_eval(t[at], F32)["snr"]
        bound("vdm_coeffs:snr_at_half_vs_fp32", ac.worst_rel(full["snr"][at], ref32), 2.0 ** -22)


@pytest.mark.parametrize("kind,k", ac.VDM_SCHEDULES)
def test_vdm_step_coeffs(N, kind, k):
    e_ref = ac.vdm_step_band(kind, k)
    report("algo_kernels_e_ref_vdm_step", kind=kind, k=k, **e_ref)
    for j, ts in enumerate(ac.vdm_step_band_schedules(kind, k)):
        dts = dev(ts)
        ref = ac.vdm_step_eval(ts, F64)
        outs = {name: Out(k) for name in ac.VDM_STEP_NAMES}
        N.check(N.lib().bsi_vdm_step_coeffs(N.ptr(dts), k, ac.G0, ac.G1, *(outs[name].ptr for name in ac.VDM_STEP_NAMES), N.stream()))
        got = {name: o.get() for name, o in outs.items()}
        for name in ac.VDM_STEP_NAMES:
            bound(f"vdm_step:{name}:{kind}{k}", ac.worst_rel(got[name], ref[name]), ac.tol(e_ref[name]))
        if j == 0:  # without dsnr, as the sampler calls it
            outs = {name: Out(k) for name in ac.VDM_STEP_NAMES[:3]}
            N.check(N.lib().bsi_vdm_step_coeffs(N.ptr(dts), k, ac.G0, ac.G1, *(outs[name].ptr for name in ac.VDM_STEP_NAMES[:3]), None,
                                                N.stream()))
            for name, o in outs.items():
                assert torch.equal(bits(o.get()), bits(got[name])), (kind, k, name)


def test_vdm_ancestral_step_vs_oracle(N):
    """bsi_axpbypcz fed the step coefficients at k = 8 is VDMOracle.zs_given_zt_x."""
    ts = ac.vdm_schedule("linear", 8)
    z, x, eps = ac.vdm_chain_case()
    ref64, ref32 = ac.vdm_chain_eval(F64), ac.vdm_chain_eval(F32)
    cz, cx, sd = (torch.empty(8, device=DEV) for _ in range(3))
    N.check(N.lib().bsi_vdm_step_coeffs(N.ptr(dev(ts)), 8, ac.G0, ac.G1, N.ptr(cz), N.ptr(cx), N.ptr(sd), None, N.stream()))
    n = z[0].numel()
    for i in range(8):
        out = Out(n)
        N.check(N.lib().bsi_axpbypcz(N.ptr(dev(z[i])), N.ptr(dev(x[i])), N.ptr(dev(eps[i])), N.ptr(cz), N.ptr(cx), N.ptr(sd), i, n,
                                     out.ptr, N.stream()))
        scale = float(ref64[i].abs().max())
        e_ref = float((ref32[i].double() - ref64[i]).abs().max()) / scale
        bound("vdm_ancestral_step:rel_linf", float((out.get().reshape(3, -1).double() - ref64[i]).abs().max()) / scale, ac.tol(e_ref))


@pytest.mark.parametrize("bins", ac.RECON_BINS)
def test_vdm_recon_nll(N, bins):
    d = ac.recon_disc(bins)
    bounds = dev(d.bin_boundaries(F32))
    for si, std in enumerate(ac.recon_stds()):
        items, e_ref = ac.recon_band(bins, std)
        report("algo_kernels_e_ref_vdm_recon_nll", bins=bins, std=std, e_ref=e_ref)
        for (n, B, D, _), x, x_hat, ref in items:
            out = Out(n * B)
            N.check(N.lib().bsi_vdm_recon_nll(N.ptr(dev(x)), N.ptr(dev(x_hat)), std, N.ptr(bounds), d.lo - d.dx / 2, d.dx, bins, n * B, B,
                                              D, out.ptr, N.stream()))
            got = out.get()
            assert bool(torch.isfinite(got).all()), (bins, std, n, B, D)
            bound(f"vdm_recon_nll:bins{bins}:std{si}", ac.worst_rel(got, ref), ac.tol(e_ref))
    x, x_hat = ac.recon_case(256, 0.05, 1, 1, 4, 0)
    out = Out(1)
    refused(N, N.lib().bsi_vdm_recon_nll(N.ptr(dev(x)), N.ptr(dev(x_hat)), 0.05, N.ptr(bounds), -1.0, 0.1, 4097, 1, 1, 4, out.ptr,
                                         N.stream()), "bsi_vdm_recon_nll: 4097 bins")


# ----------------------------------------------------------------------------------------------
# BFN coefficients
# ----------------------------------------------------------------------------------------------
def run_bfn_coeffs(N, dt, sigma_1, names):
    outs = {k: Out(dt.numel()) for k in names}
    p = [outs[k].ptr if k in outs else None for k in ac.BFN_COEFF_NAMES]
    N.check(N.lib().bsi_bfn_coeffs(N.ptr(dt), dt.numel(), sigma_1, ac.BFN_T_MIN, *p, N.stream()))
    return {k: o.get() for k, o in outs.items()}


@pytest.mark.parametrize("sigma_1", ac.BFN_SIGMAS)
def test_bfn_coeffs(N, sigma_1):
    e_w = ac.bfn_coeffs_band(sigma_1, None)["w"]
    report("algo_kernels_e_ref_bfn_coeffs", sigma_1=sigma_1, band="all", w=e_w)
    for e in ac.BFN_DECADES:
        e_ref = ac.bfn_coeffs_band(sigma_1, e)
        report("algo_kernels_e_ref_bfn_coeffs", sigma_1=sigma_1, band=f"1e{e}", **e_ref)
        t = ac.bfn_band_t(e)
        dt = dev(t)
        full = run_bfn_coeffs(N, dt, sigma_1, ac.BFN_COEFF_NAMES)
        ref = ac.bfn_coeffs_eval(t, sigma_1, F64)
        for k in ac.BFN_COEFF_NAMES[:4]:
            bound(f"bfn_coeffs:{k}:s{sigma_1}:1e{e}", ac.worst_rel(full[k], ref[k]), ac.tol(e_ref[k]))
        bound(f"bfn_coeffs:w:s{sigma_1}", ac.worst_rel(full["w"], ref["w"]), ac.tol(e_w))
        for names in ac.BFN_COEFF_SUBSETS[:-1]:
            part = run_bfn_coeffs(N, dt, sigma_1, names)
            for k in names:
                assert torch.equal(bits(part[k]), bits(full[k])), (e, names, k)
        below = t < ac.f32(ac.BFN_T_MIN)
        if e == ac.BFN_DECADES[0]:
            assert int(below.sum()) == 2 and int((t == ac.f32(ac.BFN_T_MIN)).sum()) >= 1
        for k in ("c_skip", "c_out"):
            assert bool((full[k][below] == 0).all()) and bool((full[k][~below] != 0).all()), (e, k)
    t = dev(ac.bfn_band_t(-1))
    for bad in (0.0, 1.0):
        out = Out(t.numel())
        refused(N, N.lib().bsi_bfn_coeffs(N.ptr(t), t.numel(), bad, ac.BFN_T_MIN, None, None, None, None, out.ptr, N.stream()),
                f"bsi_bfn_coeffs: sigma_1 = {bad}")


@pytest.mark.parametrize("sigma_1", ac.BFN_SCHED_SIGMAS)
@pytest.mark.parametrize("k", ac.BFN_SCHED_KS)
def test_bfn_schedule(N, k, sigma_1):
    e_ref = ac.bfn_schedule_band(sigma_1, k)
    report("algo_kernels_e_ref_bfn_schedule", sigma_1=sigma_1, k=k, **e_ref)
    for j, t in enumerate(ac.bfn_schedule_band_ts(k)):
        dt = dev(t)
        ref = ac.bfn_schedule_eval(t, sigma_1, F64)
        alpha, rho, wdisc = Out(k), Out(k + 1), Out(k)
        N.check(N.lib().bsi_bfn_schedule(N.ptr(dt), k, sigma_1, alpha.ptr, rho.ptr, wdisc.ptr, N.stream()))
        got = {"alpha": alpha.get(), "rho": rho.get(), "wdisc": wdisc.get()}
        assert float(got["rho"][0]) == 1.0
        for name in ("alpha", "rho") + (("wdisc",) if j == 0 else ()):  # wdisc depends on k alone
            bound(f"bfn_schedule:{name}:s{sigma_1}:k{k}", ac.worst_rel(got[name], ref[name]), ac.tol(e_ref[name]))
        if j == 0:  # without wdisc
            a2, r2 = Out(k), Out(k + 1)
            N.check(N.lib().bsi_bfn_schedule(N.ptr(dt), k, sigma_1, a2.ptr, r2.ptr, None, N.stream()))
            assert torch.equal(bits(a2.get()), bits(got["alpha"])) and torch.equal(bits(r2.get()), bits(got["rho"]))
