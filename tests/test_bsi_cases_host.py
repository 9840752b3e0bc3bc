"""Conditions on the inputs of tests/test_hip_bsi_kernels.py, checked on the CPU (no GPU needed): the GPU tests use exactly the cases
of tests/bsi_cases.py, unfiltered, so what makes a comparison meaningful -- bins that agree in fp32 and fp64, a gradient norm well
away from the clipping threshold, bands whose fp32 evaluation says something, segments that really pass the grid caps -- is held here."""
import math

import torch

from tests import bsi_cases as bc
from tests.util import report

F32, F64 = torch.float32, torch.float64


def test_row_cases_enter_every_loop_and_tell_rows_apart():
    assert any(D // 4 > 64 * 256 for _, _, D in bc.ROW_CASES), "no case enters the stride loop over D"
    assert any(rows > 65535 for rows, _, _ in bc.ROW_CASES), "no case passes the limit of grid.y"
    assert any(rows > B > 1 for rows, B, _ in bc.ROW_CASES), "r % B never wraps"
    for rows, B, D in bc.ROW_CASES:
        assert D % 4 == 0
        d = bc.row_case(rows, B, D)
        for k in ("lam", "w", "gup"):
            assert bool((d[k] > 0).all())
            if rows > 1:
                assert float(d[k].diff().abs().min()) > 1e-3 * float(d[k].abs().max()) or k == "lam", (k, rows)
        for k in ("cs", "co"):
            for s in bc.C_STRIDES[1:]:
                c = bc.coef_rows(d[k], rows, s)
                assert rows == 1 or float(c.diff().abs().min()) >= 1.0, (k, s)
        if B > 1:
            assert float(d["x"].mean(1).diff().abs().min()) > 1.0


def test_recon_inputs_have_the_same_bin_in_fp32_and_fp64():
    for k in bc.RECON_KS:
        d = bc.recon_disc(k)
        assert len(bc.recon_edges(k)) >= 1
        bounds = d.bin_boundaries(F32)
        for D in bc.RECON_DS:
            x, x_hat, z = bc.recon_case(k, D)
            assert x_hat.shape == (256, D)
            i32, i64 = d.bucketize(x), d.bucketize(x.double())
            assert torch.equal(i32, i64), (k, D)
            flat = x.flatten()
            assert i32.flatten()[:6].tolist() == [0, k - 1, 0, k - 1, k - 1, 0]
            raw = ((flat[:6].double() + 1 + d.dx / 2) / d.dx).floor().long().tolist()
            assert raw[4] == k and raw[5] == -1, "one bin past either end of the range"
            assert bool((flat[2:6].abs() > 1).all()) and bool(torch.isin(flat[6:7], bounds).all()), "outside values, a value on an edge"
            assert bool((i32 == 0).any()) and bool((i32 == k - 1).any()), "both end bins"
            r = torch.arange(256)
            assert bool((z[r % 4 == 3] <= -100).all()), "the rows at the 1e-20 floor"
            for form in ("disc", "cont"):
                _, _, ref, e_ref = bc.recon_band(k, D, form)
                assert bool(torch.isfinite(ref).all()) and math.isfinite(e_ref), (k, D, form)
                report("bsi_cases_e_ref_recon_nll", k=k, D=D, form=form, e_ref=e_ref)
                assert e_ref < 0.05, (k, D, form, e_ref)
                if form == "disc":
                    floor = -D * math.log(1e-20)
                    assert bool(((ref[r % 4 == 3] - floor).abs() < 1e-9 * floor).all()), "rows of probability 0 sit on the floor"
                    assert bool((ref[r % 4 != 3] < 0.5 * floor).all())


def test_to_uint8_inputs():
    p = bc.u8_planted()
    lv = p[:256]
    assert torch.equal(bc.u8_ref(lv[[0, 255]]), torch.tensor([0, 255], dtype=torch.uint8))
    assert bool((p[256:512] < lv).all()) and bool((p[512:768] > lv).all()) and bool((p[768:].abs() > 1).all())
    for n in bc.U8_NS:
        x = bc.u8_case(n)
        assert x.numel() == n
        if n > len(p):
            assert bool(torch.isin(p, x).all())
    assert bc.U8_NS[-1] > 4096 * 256


def test_e_ref_is_finite_and_nonzero_in_a_band_of_every_output():
    bands = {}

    def add(prefix, d):
        for k, v in d.items():
            bands.setdefault(f"{prefix}:{k}", []).append(v)

    for e in bc.T_DECADES:
        assert len(bc.band_t(e)) >= 256
        add("edm", bc.edm_band(e))
    for k1 in bc.SCHED_K1S:
        assert sum(len(t) for t in bc.schedule_band_ts(k1)) >= 256
        add("schedule", {k: v for k, v in bc.schedule_band(k1).items() if k1 > 1 or k != "alpha"})
    for total in bc.GRID_TOTALS:
        assert total * len(bc.grid_offsets(total)) >= 256
        add("lambda_grid", {"lam": bc.grid_band(total)})
    for name in bc.ADAM_OPTS:
        for n in bc.ADAM_NS[4:]:  # the band of the small sizes, and the two large sizes
            for (i, k), v in bc.adam_band(name, n).items():
                if k != "ema" or bc.adam_opt(name)["ema"]:
                    add("adam", {k: v})
    for name, vals in bands.items():
        report("bsi_cases_e_ref", output=name, lo=min(vals), hi=max(vals))
        assert all(math.isfinite(v) for v in vals), (name, vals)
        assert any(v > 0 for v in vals), name
        assert max(vals) < 0.05, (name, vals)  # a band whose fp32 evaluation is this far off checks nothing


def test_times_cover_zero_one_and_every_decade():
    pieces = bc.edm_t()
    assert [len(t) for t, _ in pieces] == list(bc.COEFF_NS)
    t, band = torch.cat([p[0] for p in pieces]), torch.cat([p[1] for p in pieces])
    assert bool((t == 0).any()) and bool((t == 1).any())
    every = torch.cat([torch.zeros(1)] + [bc.band_t(e) for e in bc.T_DECADES])
    assert bool(torch.isin(every, t).all()), "a band point is never run"
    for e in bc.T_DECADES:
        te = t[band == e]
        assert len(te) >= 256 and float(te.min()) >= bc.f32(10.0 ** e) and float(te.max()) <= bc.f32(10.0 ** (e + 1))
    assert bool((t[band == -7] == 0).all())
    # near 0 alpha = lam - lambda_0 cancels: the e_ref of c_skip grows towards small t, which is what the bands are for
    assert bc.edm_band(-6)["c_skip"] > 100 * bc.edm_band(-1)["c_skip"]


def test_lambda_grid_wraps_alike_in_fp32_and_fp64():
    for total in bc.GRID_TOTALS:
        perm = bc.grid_perm(total)
        assert sorted(perm.tolist()) == list(range(total))
        for o in bc.grid_offsets(total):
            t32, w32, _ = bc.grid_eval(perm, o, F32)
            t64, w64, _ = bc.grid_eval(perm, o, F64)
            assert torch.equal(w32.double(), w64), (total, o, "the sum passes 1 in one precision only")
            assert bool(((t32 >= 0) & (t32 < 1)).all()) and float((t32.double() - t64).abs().max()) <= 2.0 ** -23
        assert set(bc.GRID_OFFSETS) <= set(bc.grid_offsets(total))


def test_gradient_norms_are_away_from_the_clipping_threshold():
    for name in bc.ADAM_OPTS:
        o = bc.adam_opt(name)
        for n in bc.ADAM_NS:
            p0, e0, grads = bc.adam_case(n, name)
            z = bc.zero_block(n)
            for g in grads:
                assert bool((g[z] == 0).all()) and (n < 3 or z.stop > z.start)
                if o["max_norm"] > 0:
                    for norm in (float(g.norm()), float(g.double().norm())):
                        ratio = norm * o["grad_scale"] / o["max_norm"]
                        assert ratio > 2 or ratio < 0.5, (name, n, ratio)
                        assert (ratio > 2) == (o["ratio"] > 1)
    assert bc.adam_opt("no_clip")["max_norm"] == 0 and bc.adam_opt("grad_scale")["grad_scale"] == 0.125
    assert bc.ADAM_NS[-2] > 1024 * 256 * 4 and bc.ADAM_NS[-1] > 8192 * 256 and bc.ADAM_NS[-1] % 4


def test_zero_gradient_block_moves_by_the_decay_only():
    o = bc.adam_opt("clip_active")
    n = 1023
    p0, _, _ = bc.adam_case(n, "clip_active")
    z = bc.zero_block(n)
    run = bc.adam_run(n, "clip_active")
    for i in range(3):
        (p, m, v, _), _, _ = run[i]
        assert bool((m[z] == 0).all()) and bool((v[z] == 0).all())
        assert torch.equal(p[z], bc.decay_only(p0[z], o, i + 1))


def test_segment_table_passes_both_chunk_caps_and_leaves_gaps():
    rows, np_, ng, chunks = bc.seg_table()
    assert len(rows) == bc.NSEG == 8200 and chunks > 8192
    assert ng * 4 < 8 << 20, "a few MB"
    lens = [r[2] for r in rows]
    for ln in (bc.CHUNK - 4, bc.CHUNK, bc.CHUNK + 4, 3 * bc.CHUNK + 8):
        assert ln in lens
    assert sum(1 for ln in lens if 4 <= ln <= 64) >= bc.NSEG - 8
    end_p = end_g = end_c = 0
    assert rows[0][0] >= 4
    for i, (po, go, ln, mc, oc) in enumerate(rows):
        assert ln % 4 == 0 and po % 4 == 0 and go % 4 == 0
        assert (i == 0 or 4 <= po - end_p <= 32) and go == end_g and mc == end_c
        end_p, end_g, end_c = po + ln, go + ln, mc + -(-ln // bc.CHUNK)
    assert 4 <= np_ - end_p <= 32 and ng == end_g and chunks == end_c
    assert any(po != go for po, go, *_ in rows)
    slots = sorted((oc, oc + -(-ln // bc.CHUNK)) for _, _, ln, _, oc in rows)
    assert slots[0][0] == 0 and slots[-1][1] == chunks and all(a[1] == b[0] for a, b in zip(slots, slots[1:])), "a permutation of blocks"
    assert sum(1 for _, _, _, mc, oc in rows if mc != oc) > bc.NSEG // 2, "not the identity"
    assert bc.seg_index().numel() == ng
