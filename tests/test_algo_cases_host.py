"""Conditions on the inputs of tests/test_hip_algo_kernels.py and tests/test_hip_algos_generic.py, checked on the CPU (no GPU
needed): the GPU tests use exactly the cases of tests/algo_cases.py, unfiltered, so what makes a comparison meaningful -- margins
of the fp32 oracle, agreement of the bins in fp32 and fp64, a real std, no clip mask on the verge of flipping -- is held here."""
import math

import pytest
import torch

from oracle import bsi_oracle as bo
from tests import algo_cases as ac
from tests.util import report

F32, F64 = torch.float32, torch.float64


def test_recon_inputs_have_the_same_bin_in_fp32_and_fp64():
    for bins in ac.RECON_BINS:
        d = ac.recon_disc(bins)
        for std in ac.recon_stds():
            items, e_ref = ac.recon_band(bins, std)
            assert sum(len(r) for *_, r in items) >= 256
            seen = torch.zeros(bins, dtype=torch.bool)
            for case, x, x_hat, ref in items:
                i32, i64 = d.bucketize(x), d.bucketize(x.double())
                assert torch.equal(i32, i64), (bins, case)
                assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(x_hat).all())
                seen[i32.flatten()] = True
                n, B, D, _ = case
                if B * D >= 8:  # values outside the range land in the first and the last bin
                    assert i32.flatten()[:6].tolist() == [0, bins - 1, 0, bins - 1, bins - 1, 0]
                    raw = ((x.double().flatten()[:6] + 1 + d.dx / 2) / d.dx).floor().long().tolist()
                    assert raw[4] == bins and raw[5] == -1, "one bin past either end of the range"
            assert bool(seen[0]) and bool(seen[-1]) and int(seen.sum()) >= min(bins, 256)
    for D in ac.RECON_DS:  # every D twice per bin count
        for bins in ac.RECON_BINS:
            assert sum(1 for c in ac.recon_cases(bins) if c[2] == D) >= 2 or bins == 4096 and D in (256, 1000)


def test_step_schedules_have_a_negative_expm1_argument_in_fp32():
    for kind, k in ac.VDM_SCHEDULES:
        scheds = ac.vdm_step_band_schedules(kind, k)
        assert sum(len(s) - 1 for s in scheds) >= 256 and torch.equal(scheds[0], ac.vdm_schedule(kind, k))
        for ts in scheds:
            assert bool((ts[1:] < ts[:-1]).all()), (kind, k, "not decreasing")
            assert float(ac.vdm_step_arg(ts, F32).max()) < 0, (kind, k)
            assert bool(torch.isfinite(ac.vdm_step_eval(ts, F32)["std"]).all())


def test_e_ref_is_finite_and_nonzero_in_a_band_of_every_output():
    bands = {}

    def add(prefix, d):
        for k, v in d.items():
            bands.setdefault(f"{prefix}:{k}", []).append(v)

    add("vdm_coeffs", ac.vdm_coeffs_band())
    for kind, k in ac.VDM_SCHEDULES:
        add("vdm_step", ac.vdm_step_band(kind, k))
    for s1 in ac.BFN_SIGMAS:
        add("bfn_coeffs", ac.bfn_coeffs_band(s1, None))
        for e in ac.BFN_DECADES:
            add("bfn_coeffs", ac.bfn_coeffs_band(s1, e))
    for s1 in ac.BFN_SCHED_SIGMAS:
        for k in ac.BFN_SCHED_KS:
            add("bfn_schedule", ac.bfn_schedule_band(s1, k))
    for bins in ac.RECON_BINS:
        for std in ac.recon_stds():
            add("vdm_recon_nll", {"nll": ac.recon_band(bins, std)[1]})
    for name, vals in bands.items():
        report("algo_cases_e_ref", output=name, lo=min(vals), hi=max(vals))
        assert all(math.isfinite(v) for v in vals), (name, vals)
        assert any(v > 0 for v in vals), name
        assert max(vals) < 0.05, (name, vals)  # a band whose fp32 evaluation is this far off checks nothing


def test_planted_values_are_where_the_cases_say():
    for n in ac.VDM_COEFF_NS[1:]:
        t = ac.vdm_coeff_t(n)
        assert all(bool((t == v).any()) for v in ac.VDM_PLANTED) and bool(((t >= 0) & (t <= 1)).all())
    assert ac.HALF3[0] < 0.5 < ac.HALF3[2]
    t = ac.bfn_band_t(ac.BFN_DECADES[0])
    tm = ac.f32(ac.BFN_T_MIN)
    assert int((t < tm).sum()) == 2 and bool((t == tm).any()) and bool((t == ac.nextafter(tm, 1.0)).any())
    assert bool((ac.bfn_band_t(ac.BFN_DECADES[-1]) == 1).any())
    for lo, hi in ac.CLIP_BOUNDS:
        for n in ac.CLIP_NS:
            x, _ = ac.clip_case(n, lo, hi)
            assert bool(torch.isnan(x).any())
            if n > 1:
                got = x[~torch.isnan(x)]
                for v in ac.clip_planted(lo, hi)[1:]:
                    assert bool((got == v).any()), (n, v)
                assert bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())


GENERIC = [(algo, case) for algo in ("vdm", "bfn") for case in ac.GENERIC_CASES]


@pytest.mark.parametrize("algo,case", GENERIC, ids=[f"{a}-{c[0]}" for a, c in GENERIC])
def test_fp32_oracle_is_within_a_quarter_of_every_fixed_bound(algo, case):
    lo, hi = ac.generic_eval(algo, case, F32), ac.generic_eval(algo, case, F64)
    on_rule = ac.ON_RULE.get((algo, case[0]), ())
    assert set(on_rule) <= set(hi)
    for name, ref in hi.items():
        if ac.generic_bound(name) is None:
            continue
        kind, fixed = ac.generic_bound(name)
        e = ac.metric(kind, lo[name], ref)
        report("algo_cases_generic_fp32_oracle", algo=algo, case=case[0], quantity=name, error=e, bound=fixed)
        assert bool(torch.isfinite(ref).all())
        if name in on_rule:
            assert 0 < e < 0.05 and ac.generic_limit(algo, case, name)[1] == ac.tol(e), (name, e)
        else:
            assert e < fixed / 4, (algo, case[0], name, e, fixed)
            assert ac.generic_limit(algo, case, name) == (kind, fixed)


def test_generic_inputs():
    for algo, case in GENERIC:
        d = ac.generic_draws(algo, case)
        disc = bo.Disc.image_8bit()
        assert torch.equal(disc.bucketize(d["x"]), disc.bucketize(d["x"].double())), (algo, case[0])
        if algo == "bfn":  # sqrt((1 - gamma) / gamma) amplifies the denoiser's rounding at small times
            o = ac.BFNOracle(None, data_shape=ac.GENERIC_SHAPE, sigma_1=ac.BFN_SIGMA_1)
            _, _, lds, B, n = case
            ts = [d["t_iid"]] if not lds else [o.t_grid(d["offset"], d["perm1"], 1, B), o.t_grid(d["offset"], d["perm"], n, B)]
            assert min(float(t.min()) for t in ts) >= 0.05, (case[0], ts)
    for case in ac.GENERIC_CASES[:2]:  # the gradient cases: a clip mask that flips between fp32 and fp64 would dominate the error
        raw = ac.generic_eval("bfn", case, F64)["aux:raw"]
        assert float(torch.minimum((raw - 1).abs(), (raw + 1).abs()).min()) > 1e-4, case[0]
        assert bool((raw.abs() > 1).any()) and bool((raw.abs() < 1).any()), "the case should have clipped and unclipped elements"
    for kind, k in (("linear", ac.GENERIC_K),):  # the sampler's schedule
        assert float(ac.vdm_step_arg(ac.vdm_schedule(kind, k), F32).max()) < 0
