"""Each entry point of bsi_amd/csrc/bsi_ops.hip (behind bsi_amd.BSI) and bsi_amd/csrc/optim.hip (the clip + AdamW + EMA step) through
the C ABI against fp64, on the cases of tests/bsi_cases.py (vetted on the CPU by tests/test_bsi_cases_host.py).  Kernels of IEEE
operations alone are held to one ulp of the largest term, transcendental outputs to tol(e_ref) per band, sums to the count of fp32
roundings on their longest chain.  Every output is allocated with 8 guard elements behind it, which have to stay untouched; nullable
output pointers are run as the subsets bsi_amd/bsi.py uses, and the outputs that remain have to equal the all-pointers call bit for
bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bsi_cases as bc
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


def P(N):
    return C.byref(N.BSIParams(*bc.PARAMS))


def bits(t):
    return t.contiguous().view(torch.int32)


def refused(N, rc, what, *outs):
    assert rc != 0, f"{what} was accepted"
    msg = N.lib().bsi_last_error()
    assert msg and what.split(":")[0] in msg.decode(), (what, msg)
    for o in outs:
        assert bool((o.get() == o.sentinel).all()), f"{what}: a refused call wrote to its output"


def ulp_check(tag, out, ref, mag, seq32, tally):
    got = out.get().reshape(ref.shape)
    bound(tag, bc.worst_scaled(got, ref, mag), LE_ULP)
    tally[0] += int((bits(got) == bits(seq32)).sum())
    tally[1] += got.numel()
    return got


# ----------------------------------------------------------------------------------------------
# row kernels
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,B,D", bc.ROW_CASES)
def test_row_kernels(N, rows, B, D):
    L, S = N.lib(), N.stream()
    d = bc.row_case(rows, B, D)
    g = {k: dev(v) for k, v in d.items()}
    n = rows * D
    tally = {k: [0, 0] for k in ("q_sample", "scale_rows", "sample_init", "predict_combine", "predict_combine_bwd", "sqerr_rows_bwd")}
    out = Out(n)
    N.check(L.bsi_q_sample(P(N), N.ptr(g["x"]), N.ptr(g["lam"]), N.ptr(g["eps"]), rows, B, D, out.ptr, S))
    ulp_check("row:q_sample:ulp", out, *bc.q_sample_ref(d["x"], d["lam"], d["eps"], B), tally["q_sample"])
    out = Out(n)
    N.check(L.bsi_sample_init(N.ptr(g["eps"]), N.ptr(g["lam"]), rows, D, out.ptr, S))
    ulp_check("row:sample_init:ulp", out, *bc.sample_init_ref(d["eps"], d["lam"]), tally["sample_init"])
    for stride in bc.C_STRIDES:
        cs, co = bc.coef_rows(d["cs"], rows, stride), bc.coef_rows(d["co"], rows, stride)
        out = Out(n)
        N.check(L.bsi_scale_rows(N.ptr(g["mu"]), N.ptr(g["cs"]), stride, rows, D, out.ptr, S))
        ulp_check("row:scale_rows:ulp", out, *bc.scale_ref(cs, d["mu"]), tally["scale_rows"])
        out = Out(n)
        N.check(L.bsi_predict_combine(N.ptr(g["mu"]), N.ptr(g["f"]), N.ptr(g["cs"]), N.ptr(g["co"]), stride, rows, D, out.ptr, S))
        ulp_check("row:predict_combine:ulp", out, *bc.combine_ref(d["mu"], d["f"], cs, co), tally["predict_combine"])
        gf, gm = Out(n), Out(n)
        N.check(L.bsi_predict_combine_bwd(N.ptr(g["g"]), N.ptr(g["cs"]), N.ptr(g["co"]), stride, rows, D, gf.ptr, gm.ptr, S))
        full_f = ulp_check("row:predict_combine_bwd:ulp", gf, *bc.scale_ref(co, d["g"]), tally["predict_combine_bwd"])
        ulp_check("row:predict_combine_bwd:ulp", gm, *bc.scale_ref(cs, d["g"]), tally["predict_combine_bwd"])
        only = Out(n)  # (gf, NULL): the call of BSI's backward
        N.check(L.bsi_predict_combine_bwd(N.ptr(g["g"]), N.ptr(g["cs"]), N.ptr(g["co"]), stride, rows, D, only.ptr, None, S))
        assert torch.equal(bits(only.get().reshape(rows, D)), bits(full_f)), (rows, D, stride)
    for mean, w, scale in ((0, "w", 0.5), (1, "w", 1.0), (1, None, 1.0)):
        out = Out(n)
        N.check(L.bsi_sqerr_rows_bwd(N.ptr(g["x"]), N.ptr(g["mu"]), N.ptr(g[w]) if w else None, N.ptr(g["gup"]), scale, mean, rows, B, D,
                                     out.ptr, S))
        ulp_check("row:sqerr_rows_bwd:ulp", out, *bc.sqerr_bwd_ref(d["x"], d["mu"], d[w] if w else None, d["gup"], scale, mean, B),
                  tally["sqerr_rows_bwd"])
    report("bsi_kernels_rows_bit_equal_to_fp32_cpu", rows=rows, B=B, D=D, **{k: f"{a}/{b}" for k, (a, b) in tally.items()})


def test_row_kernels_refuse_a_row_length_that_is_no_multiple_of_four(N):
    L, S = N.lib(), N.stream()
    g = {k: dev(v) for k, v in bc.row_case(1, 1, 1020).items()}
    out, out2 = Out(8), Out(8)
    refused(N, L.bsi_q_sample(P(N), N.ptr(g["x"]), N.ptr(g["lam"]), N.ptr(g["eps"]), 1, 1, 6, out.ptr, S), "bsi_q_sample: D = 6", out)
    refused(N, L.bsi_scale_rows(N.ptr(g["mu"]), N.ptr(g["cs"]), 1, 1, 6, out.ptr, S), "bsi_scale_rows: D = 6", out)
    refused(N, L.bsi_sample_init(N.ptr(g["eps"]), N.ptr(g["lam"]), 1, 6, out.ptr, S), "bsi_sample_init: D = 6", out)
    refused(N, L.bsi_predict_combine(N.ptr(g["mu"]), N.ptr(g["f"]), N.ptr(g["cs"]), N.ptr(g["co"]), 1, 1, 6, out.ptr, S),
            "bsi_predict_combine: D = 6", out)
    refused(N, L.bsi_predict_combine_bwd(N.ptr(g["g"]), N.ptr(g["cs"]), N.ptr(g["co"]), 1, 1, 6, out.ptr, out2.ptr, S),
            "bsi_predict_combine_bwd: D = 6", out, out2)
    refused(N, L.bsi_sqerr_rows_bwd(N.ptr(g["x"]), N.ptr(g["mu"]), None, N.ptr(g["gup"]), 1.0, 0, 1, 1, 6, out.ptr, S),
            "bsi_sqerr_rows_bwd: D = 6", out)
    refused(N, L.bsi_sqerr_rows(N.ptr(g["x"]), N.ptr(g["mu"]), None, 1.0, 0, 1, 1, 6, out.ptr, S), "bsi_sqerr_rows: D = 6", out)


# ----------------------------------------------------------------------------------------------
# refine step, philox
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", bc.REFINE_SHAPES)
def test_refine_step(N, rows, D):
    L, S = N.lib(), N.stream()
    mu, f, eps = bc.refine_case(rows, D)
    n = rows * D
    dmu, df, de = dev(mu), dev(f), dev(eps)
    lam, alpha, cs, co = (dev(t) for t in bc.refine_tables())
    equal = total = 0
    # every step with and without a ready x_hat; past the cap (where a comparison of 8 M doubles takes a second) each step once
    combos = [(i, fx) for i in bc.REFINE_STEPS for fx in (0, 1)] if n <= bc.CAP4 else list(zip(bc.REFINE_STEPS, (0, 1, 0)))
    for i, fx in combos:
        outs = {k: Out(n) for k in ("xh", "y", "mn")}
        coef = (None, None) if fx else (N.ptr(cs), N.ptr(co))  # BSI.sample hands no coefficients over with an x_hat
        N.check(L.bsi_refine_step(N.ptr(dmu), N.ptr(df), N.ptr(de), N.ptr(lam), N.ptr(alpha), *coef, i, fx, rows, D,
                                  outs["xh"].ptr, outs["y"].ptr, outs["mn"].ptr, S))
        ref = bc.refine_ref(mu, f, eps, i, fx)
        got = {k: o.get() for k, o in outs.items()}
        for k in ("xh", "y", "mn"):
            bound(f"refine_step:{k}:ulp", bc.worst_scaled(got[k], *ref[k]), LE_ULP)
        if fx:
            assert torch.equal(bits(got["xh"]), bits(f))
        equal += int((bits(got["mn"]) == bits(ref["mn"][0].float())).sum())
        total += n
        alone = Out(n)  # without the history outputs
        N.check(L.bsi_refine_step(N.ptr(dmu), N.ptr(df), N.ptr(de), N.ptr(lam), N.ptr(alpha), *coef, i, fx, rows, D, None, None,
                                  alone.ptr, S))
        assert torch.equal(bits(alone.get()), bits(got["mn"])), (rows, D, i, fx)
    report("bsi_kernels_refine_bit_equal_to_rounded_fp64", rows=rows, D=D, mu_next=f"{equal}/{total}")


def test_refine_step_refusals(N):
    L, S = N.lib(), N.stream()
    mu, f, eps = (dev(t) for t in bc.refine_case(1, 1028))
    lam, alpha, cs, co = (dev(t) for t in bc.refine_tables())
    seed = dev(torch.tensor([bc.PHILOX_SEED], dtype=torch.int64))
    out = Out(8)
    refused(N, L.bsi_refine_step(N.ptr(mu), N.ptr(f), N.ptr(eps), N.ptr(lam), N.ptr(alpha), None, None, 0, 0, 1, 8, None, None, out.ptr, S),
            "bsi_refine_step: coefficients missing", out)
    refused(N, L.bsi_refine_step_philox(N.ptr(mu), N.ptr(f), N.ptr(seed), N.ptr(lam), N.ptr(alpha), None, None, 0, 0, 1, 8, None, None,
                                        out.ptr, S), "bsi_refine_step_philox: coefficients missing", out)
    refused(N, L.bsi_refine_step(N.ptr(mu), N.ptr(f), N.ptr(eps), N.ptr(lam), N.ptr(alpha), N.ptr(cs), N.ptr(co), 0, 0, 2, 3, None, None,
                                 out.ptr, S), "bsi_refine_step: 6 elements", out)
    refused(N, L.bsi_philox_normal(N.ptr(seed), 0, 6, out.ptr, S), "bsi_philox_normal: n = 6", out)
    iout = Out(8, dtype=torch.int32, sentinel=bc.INT_SENTINEL)
    refused(N, L.bsi_philox_uint32(N.ptr(seed), 0, 6, iout.ptr, S), "bsi_philox_uint32: n = 6", iout)


def test_philox_past_the_grid_cap(N):
    """The counter is the index of the group of four elements whatever the grid: the first 2^20 elements of a call past the cap of
    4096 blocks equal a call of 2^20 elements, and everything (the tail past the cap included) equals the host restatement -- the
    integers bit for bit, the normals within the absolute bound of tests/test_hip_philox.py."""
    L, S = N.lib(), N.stream()
    n, stream_id = bc.PHILOX_N, 5
    assert n > bc.CAP4
    seed = dev(torch.tensor([bc.PHILOX_SEED], dtype=torch.int64))
    u, u_short = Out(n, dtype=torch.int32, sentinel=bc.INT_SENTINEL), Out(1 << 20, dtype=torch.int32, sentinel=bc.INT_SENTINEL)
    z, z_short = Out(n), Out(1 << 20)
    N.check(L.bsi_philox_uint32(N.ptr(seed), stream_id, n, u.ptr, S))
    N.check(L.bsi_philox_uint32(N.ptr(seed), stream_id, 1 << 20, u_short.ptr, S))
    N.check(L.bsi_philox_normal(N.ptr(seed), stream_id, n, z.ptr, S))
    N.check(L.bsi_philox_normal(N.ptr(seed), stream_id, 1 << 20, z_short.ptr, S))
    gu, gz = u.get(), z.get()
    assert torch.equal(gu[:1 << 20], u_short.get()) and torch.equal(bits(gz[:1 << 20]), bits(z_short.get()))
    ref_u = bc.philox_uint32(bc.PHILOX_SEED, stream_id, n)
    assert np.array_equal(gu.numpy().view(np.uint32), ref_u)
    err = np.abs(gz.numpy().astype(np.float64) - bc.philox_normals(ref_u))
    bound("philox_normal:abs:past_cap", float(err[bc.CAP4:].max()), 4e-6)
    bound("philox_normal:abs", float(err.max()), 4e-6)


def test_refine_step_philox_equals_the_plain_step_past_the_cap(N):
    L, S = N.lib(), N.stream()
    rows, D = bc.REFINE_SHAPES[3]
    n, i = rows * D, 4
    assert n > bc.CAP4
    mu, f, _ = bc.refine_case(rows, D)
    dmu, df = dev(mu), dev(f)
    lam, alpha, cs, co = (dev(t) for t in bc.refine_tables())
    seed = dev(torch.tensor([bc.PHILOX_SEED], dtype=torch.int64))
    eps = Out(n)
    N.check(L.bsi_philox_normal(N.ptr(seed), i, n, eps.ptr, S))
    res = []
    for philox in (False, True):
        outs = [Out(n) for _ in range(3)]
        fn = L.bsi_refine_step_philox if philox else L.bsi_refine_step
        N.check(fn(N.ptr(dmu), N.ptr(df), N.ptr(seed) if philox else eps.ptr, N.ptr(lam), N.ptr(alpha), N.ptr(cs), N.ptr(co), i, 0, rows, D,
                   *(o.ptr for o in outs), S))
        res.append([o.get() for o in outs])
    eps.get()
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b))
    alone = Out(n)
    N.check(L.bsi_refine_step_philox(N.ptr(dmu), N.ptr(df), N.ptr(seed), N.ptr(lam), N.ptr(alpha), N.ptr(cs), N.ptr(co), i, 0, rows, D, None,
                                     None, alone.ptr, S))
    assert torch.equal(bits(alone.get()), bits(res[1][2]))


# ----------------------------------------------------------------------------------------------
# reductions over a row
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", bc.SQERR_DS)
def test_sqerr_rows(N, D):
    L, S = N.lib(), N.stream()
    x, xh, w = bc.sqerr_case(D)
    dx, dxh, dw = dev(x), dev(xh), dev(w)
    rows = len(xh)
    limit = bc.chain_limit(bc.sqerr_chain(D))  # sqerr_chain(D) fp32 roundings on the longest chain, all terms positive
    for mean in (0, 1):
        for ww in (None, w):
            for scale in (0.5, 1.0):
                out = Out(rows)
                N.check(L.bsi_sqerr_rows(N.ptr(dx), N.ptr(dxh), N.ptr(dw) if ww is not None else None, scale, mean, rows, bc.SQERR_B, D,
                                         out.ptr, S))
                bound(f"sqerr_rows:rel:D{D}", bc.worst_rel(out.get(), bc.sqerr_ref(x, xh, ww, scale, mean)), limit)


@pytest.mark.parametrize("k", bc.RECON_KS)
def test_recon_nll(N, k):
    """1.1e-04 (k = 2, D = 1) is the largest e_ref of these bands: a single element three standard deviations outside its bin has a
    probability of 1e-3 that fp32 forms as a difference of two numbers near 1."""
    L, S = N.lib(), N.stream()
    d = bc.recon_disc(k)
    b = d.bin_boundaries(F32)
    bounds = dev(torch.cat([b, b[-1:] + d.dx]))  # PAD_BOUNDS more than the kernel may read
    for D in bc.RECON_DS:
        for form, kk in (("disc", k), ("cont", 0)):
            x, x_hat, ref, e_ref = bc.recon_band(k, D, form)
            report("bsi_kernels_e_ref_recon_nll", k=k, D=D, form=form, e_ref=e_ref)
            rows = len(x_hat)
            out = Out(rows)
            N.check(L.bsi_recon_nll(N.ptr(dev(x)), N.ptr(dev(x_hat)), bc.ALPHA_R, N.ptr(bounds) if kk else None, d.lo - d.dx / 2, d.dx, kk,
                                    rows, len(x), D, out.ptr, S))
            got = out.get()
            assert bool(torch.isfinite(got).all()), (k, D, form)
            bound(f"recon_nll:{form}:k{k}:D{D}", bc.worst_rel(got, ref), bc.tol(e_ref))
    x, x_hat, _, _ = bc.recon_band(k, 3, "disc")
    out = Out(len(x_hat))
    refused(N, L.bsi_recon_nll(N.ptr(dev(x)), N.ptr(dev(x_hat)), bc.ALPHA_R, None, d.lo - d.dx / 2, d.dx, k, len(x_hat), len(x), 3, out.ptr, S),
            "bsi_recon_nll: no bin boundaries", out)


@pytest.mark.parametrize("n", bc.U8_NS)
def test_to_uint8(N, n):
    L, S = N.lib(), N.stream()
    x = bc.u8_case(n)
    out = Out(n, dtype=torch.uint8, sentinel=bc.BYTE_SENTINEL)
    N.check(L.bsi_to_uint8(N.ptr(dev(x)), bc.U8_LO, bc.U8_HI, n, out.ptr, S))
    assert torch.equal(out.get(), bc.u8_ref(x))
    if n == bc.U8_NS[0]:
        for lo, hi in ((1.0, 1.0), (1.0, -1.0)):
            out = Out(8, dtype=torch.uint8, sentinel=bc.BYTE_SENTINEL)
            refused(N, L.bsi_to_uint8(N.ptr(dev(x)), lo, hi, 1, out.ptr, S), "bsi_to_uint8: hi <= lo", out)


# ----------------------------------------------------------------------------------------------
# coefficient tables
# ----------------------------------------------------------------------------------------------
def run_edm(N, dt, names):
    outs = {k: Out(dt.numel()) for k in names}
    N.check(N.lib().bsi_edm_coeffs(P(N), N.ptr(dt), dt.numel(), *(outs[k].ptr if k in outs else None for k in bc.EDM_NAMES), N.stream()))
    return {k: o.get() for k, o in outs.items()}


def test_edm_coeffs_and_lambda_to_t(N):
    L, S = N.lib(), N.stream()
    e_ref = {e: bc.edm_band(e) for e in bc.T_DECADES}
    for e in bc.T_DECADES:
        report("bsi_kernels_e_ref_edm", band=f"1e{e}", **e_ref[e])
    for t, band in bc.edm_t():
        n = t.numel()
        dt = dev(t)
        full = run_edm(N, dt, bc.EDM_NAMES)
        part = run_edm(N, dt, bc.EDM_NAMES[1:])  # (NULL, c_skip, c_out, c_in): BSI._predict_x
        for k in bc.EDM_NAMES[1:]:
            assert torch.equal(bits(part[k]), bits(full[k])), (n, k)
        ref = bc.edm_eval(t, F64)
        # c_skip from the kernel's own lambda: alpha is an exact difference, four roundings follow (tests/bsi_cases.py)
        own = bc.edm_eval(t, F64, lam=full["lam"])["c_skip"]
        bound("edm:c_skip_from_own_lam", bc.worst_rel(full["c_skip"], own), bc.OWN_LAM_LIMIT)
        tt, rp, rt = Out(n), Out(n), Out(n)
        lam32 = bc.icdf(t, F32)
        N.check(L.bsi_lambda_to_t(P(N), N.ptr(dev(lam32)), n, tt.ptr, rp.ptr, S))
        N.check(L.bsi_lambda_to_t(P(N), N.ptr(dev(full["lam"])), n, rt.ptr, None, S))  # the round trip; without rpdf
        got_t = {"t": tt.get(), "rpdf": rp.get()}
        ref_t = bc.to_t_eval(lam32, F64)
        trip = rt.get()
        for e in bc.T_DECADES + (-7,):
            m = band == e
            if not bool(m.any()):
                continue
            eb = e_ref[max(e, bc.T_DECADES[0])]  # t = 0 (band -7): lambda, c_out, c_in and rpdf are as well conditioned as next to it
            for k in ("lam", "c_out", "c_in") + (("c_skip",) if e > -7 else ()):
                bound(f"edm:{k}:1e{e}", bc.worst_rel(full[k][m], ref[k][m]), bc.tol(eb[k]))
            bound(f"lambda_to_t:rpdf:1e{e}", bc.worst_rel(got_t["rpdf"][m], ref_t["rpdf"][m]), bc.tol(eb["rpdf"]))
            if e > -7:
                bound(f"lambda_to_t:t:1e{e}", bc.worst_rel(got_t["t"][m], ref_t["t"][m]), bc.tol(eb["t"]))
                bound(f"lambda_to_t:round_trip:1e{e}", bc.worst_rel(trip[m], t[m]), bc.tol(eb["round_trip"]))
            else:
                bound("lambda_to_t:t:abs_at_0", float((got_t["t"][m].double() - ref_t["t"][m]).abs().max()), bc.T0_ABS)


@pytest.mark.parametrize("k1", bc.SCHED_K1S)
def test_schedule(N, k1):
    L, S = N.lib(), N.stream()
    e_ref = bc.schedule_band(k1)
    report("bsi_kernels_e_ref_schedule", k1=k1, **e_ref)
    for j, t in enumerate(bc.schedule_band_ts(k1)):
        dt = dev(t)
        lam, alpha = Out(k1), Out(k1 - 1)
        N.check(L.bsi_schedule(P(N), N.ptr(dt), k1, lam.ptr, alpha.ptr, S))
        gl, ga = lam.get(), alpha.get()
        ref = bc.schedule_eval(t, F64)
        bound(f"schedule:lam:k{k1}", bc.worst_rel(gl, ref["lam"]), bc.tol(e_ref["lam"]))
        assert torch.equal(bits(ga), bits(gl.diff())), "alpha is the fp32 diff of the kernel's own lambdas"
        if k1 > 1:
            bound(f"schedule:alpha:k{k1}", bc.worst_rel(ga, ref["alpha"]), bc.tol(e_ref["alpha"]))
        if j == 0:  # without alpha
            lam2 = Out(k1)
            N.check(L.bsi_schedule(P(N), N.ptr(dt), k1, lam2.ptr, None, S))
            assert torch.equal(bits(lam2.get()), bits(gl))


@pytest.mark.parametrize("total", bc.GRID_TOTALS)
def test_lambda_grid(N, total):
    L, S = N.lib(), N.stream()
    e_ref = bc.grid_band(total)
    report("bsi_kernels_e_ref_lambda_grid", total=total, e_ref=e_ref)
    perm = bc.grid_perm(total)
    dperm = dev(perm)
    top = float(bc.icdf(torch.ones(1), F64))
    equal = count = 0
    for offset in bc.grid_offsets(total):
        out = Out(total)
        N.check(L.bsi_lambda_grid(P(N), N.ptr(dperm), N.ptr(dev(torch.tensor(offset, dtype=F32))), total, out.ptr, S))
        got = out.get()
        lam32 = bc.grid_eval(perm, offset, F32)[2]
        assert float(got.double().max()) < top and float(got.double().min()) >= bc.LAMBDA_0 * (1 - 8 * bc.ULP), "t before expf in [0, 1)"
        bound(f"lambda_grid:lam:total{total}", bc.worst_rel(got, bc.grid_eval(perm, offset, F64)[2]), bc.tol(e_ref))
        equal += int((bits(got) == bits(lam32)).sum())
        count += total
    report("bsi_kernels_lambda_grid_bit_equal_to_fp32_cpu", total=total, lam=f"{equal}/{count}")


# ----------------------------------------------------------------------------------------------
# optim.hip
# ----------------------------------------------------------------------------------------------
def adam_args(o, i):
    return (o["max_norm"], o["grad_scale"], o["lr"], o["beta1"], o["beta2"], o["eps"], o["wd"], o["steps"][i], o["ema_w"][i])


def workspace(N):
    return dev(torch.empty(N.lib().bsi_sqnorm_workspace_bytes(), dtype=torch.uint8))


@pytest.mark.parametrize("n", bc.ADAM_NS)
def test_flat_optimizer(N, n):
    L, S = N.lib(), N.stream()
    ws = workspace(N)
    z = bc.zero_block(n)
    norm_limit = bc.chain_limit(bc.sqnorm_chain_flat(n))  # that many fp32 roundings on the longest chain of the norm, terms positive
    for name in bc.ADAM_OPTS:
        o = bc.adam_opt(name)
        e_ref = bc.adam_band(name, n)
        p0, e0, grads = bc.adam_case(n, name)
        state = bc.adam_start(n, name)
        bufs = [Out(n, init=t) for t in state]
        for i in range(3):
            dg = dev(grads[i])
            sq = Out(1)
            N.check(L.bsi_grad_sqnorm(N.ptr(dg), n, sq.ptr, N.ptr(ws), S))
            got_sq = sq.get()
            bound(f"grad_sqnorm:rel:n{n}", bc.worst_rel(got_sq, bc.sq64(grads[i]).reshape(1)), norm_limit)
            clip = o["max_norm"] > 0
            ema_ptr = bufs[3].ptr if o["ema"] else None
            N.check(L.bsi_clip_adamw_ema(bufs[0].ptr, N.ptr(dg), bufs[1].ptr, bufs[2].ptr, ema_ptr, n, sq.ptr if clip else None,
                                         *adam_args(o, i), S))
            ref, mags = bc.adam_ref(state, n, name, i, got_sq[0].double())  # from the state and the squared norm the call was given
            new = tuple(b.get() for b in bufs)
            for j, k in enumerate(bc.ADAM_NAMES):
                if k == "ema" and (not o["ema"] or o["ema_w"][i] < 0):
                    assert torch.equal(bits(new[3]), bits(state[3])), (name, i, "the EMA buffer was touched")
                    continue
                bound(f"adam:{k}:{name}:call{i}", bc.worst_scaled(new[j], ref[j], mags[j]), bc.tol(e_ref[i, k]))
            if o["ema"] and o["ema_w"][i] >= 1.0:
                assert torch.equal(bits(new[3]), bits(new[0])), "ema_weight 1 copies the parameters"
            assert bool((new[1][z] == 0).all()) and bool((new[2][z] == 0).all()), "moments of the zero-gradient block"
            assert torch.equal(bits(new[0][z]), bits(bc.decay_only(p0[z], o, i + 1))), "the zero-gradient block moves by the decay alone"
            state = new
    if n >= bc.ADAM_BAND_NS[-1]:
        report("bsi_kernels_e_ref_adam", n=n, **{f"{name}:{k}": max(bc.adam_band(name, n)[i, k] for i in range(3)) for name in bc.ADAM_OPTS
                                                 for k in bc.ADAM_NAMES})


def test_flat_optimizer_refusals(N):
    L, S = N.lib(), N.stream()
    ws = workspace(N)
    n = 1023
    o = bc.adam_opt("clip_active")
    p0, e0, grads = bc.adam_case(n, "clip_active")
    dg = dev(grads[0])
    sq = Out(1)
    bufs = [Out(n) for _ in range(4)]
    ptrs = (bufs[0].ptr, N.ptr(dg), bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n)
    a = list(adam_args(o, 0))
    refused(N, L.bsi_clip_adamw_ema(*ptrs, sq.ptr, *a[:7], 0, a[8], S), "bsi_clip_adamw_ema: step = 0", *bufs)
    refused(N, L.bsi_clip_adamw_ema(*ptrs, None, *a, S), "bsi_clip_adamw_ema: clipping without a squared norm", *bufs)
    refused(N, L.bsi_grad_sqnorm(C.c_void_p(dg.data_ptr() + 4), n - 1, sq.ptr, N.ptr(ws), S), "bsi_grad_sqnorm: pointer offset by 4 bytes", sq)


def test_segment_optimizer(N):
    """The segment forms on 8200 segments (more chunks than either grid cap) with gaps between the segments, a packed gradient and
    the partials in a permuted order."""
    L, S = N.lib(), N.stream()
    rows, n_p, n_g, chunks = bc.seg_table()
    arr = (N.Seg * len(rows))(*[N.Seg(*r) for r in rows])
    tab = dev(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
    idx = bc.seg_index()
    name = "grad_scale"  # bsi_amd/dp.py passes 1 / world here
    o = bc.adam_opt(name)
    e_ref = bc.adam_band(name, n_g)
    p0, e0, grads = bc.adam_case(n_g, name)
    state = bc.adam_start(n_g, name)
    seg_bufs, flat_bufs = [], []
    for t in state:
        full = torch.full((n_p,), bc.SENTINEL)
        full[idx] = t
        seg_bufs.append(Out(n_p, init=full))
        flat_bufs.append(Out(n_g, init=t))
    gap = torch.ones(n_p, dtype=torch.bool)
    gap[idx] = False
    for i in range(3):
        dg = Out(n_g, init=grads[i])  # guard floats behind the packed gradient: a read past a segment's end meets the next segment or these
        part, sq = Out(chunks), Out(1)
        N.check(L.bsi_sqnorm_segments(dg.ptr, N.ptr(tab), len(rows), chunks, part.ptr, S))
        N.check(L.bsi_sqnorm_finish(part.ptr, chunks, sq.ptr, S))
        got_part, got_sq = part.get(), sq.get()
        # 16 float4 x 4 squares per thread, 6 levels of the wave sum, 2 of the block sum: 72 fp32 roundings, terms positive
        bound("sqnorm_segments:partial:rel", bc.worst_rel(got_part, bc.seg_partials64(grads[i])), bc.chain_limit(bc.SQNORM_CHAIN_CHUNK))
        # the finish adds the partials in double and rounds once: 73
        bound("sqnorm_segments:sum:rel", bc.worst_rel(got_sq, bc.sq64(grads[i]).reshape(1)), bc.chain_limit(bc.SQNORM_CHAIN_SEGMENTS))
        args = adam_args(o, i)
        N.check(L.bsi_clip_adamw_ema_segments(seg_bufs[0].ptr, dg.ptr, *(b.ptr for b in seg_bufs[1:]), N.ptr(tab), len(rows), chunks, sq.ptr, *args, S))
        N.check(L.bsi_clip_adamw_ema(flat_bufs[0].ptr, dg.ptr, *(b.ptr for b in flat_bufs[1:]), n_g, sq.ptr, *args, S))
        p_flat = flat_bufs[0].get()
        ref, mags = bc.adam_ref(state, n_g, name, i, got_sq[0].double())
        new = []
        for j, k in enumerate(bc.ADAM_NAMES):
            full = seg_bufs[j].get()
            assert bool((full[gap] == bc.SENTINEL).all()), (k, i, "a gap between two segments was written")
            seg = full[idx]
            flat = p_flat if j == 0 else flat_bufs[j].get()
            assert torch.equal(bits(seg), bits(flat)), (k, i, "the segment form differs from the flat form on the gathered elements")
            bound(f"adam_segments:{k}:call{i}", bc.worst_scaled(seg, ref[j], mags[j]), bc.tol(e_ref[i, k]))
            new.append(seg)
        state = tuple(new)
