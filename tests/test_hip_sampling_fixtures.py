"""The DiT sampling kernels outside the GEMMs -- persistent attention, the LayerNorm + modulate passes, the final kernel -- against
the outputs RECORDED from the build before they were last reworked (tests/golden/sampling_kernels.json, written by
tools/record_sampling_fixtures.py): such rework must not change a bit, and the yardstick for that is the earlier build, not the code
under test.  Each attention and LayerNorm case is also held against the fp64 restatement and the bounds of the operator tests
(tests/test_hip_ops.py, tests/test_hip_dispatch_edges.py), so that a wrong record cannot hide a wrong kernel."""
import math

import pytest
import torch

from oracle import dit_oracle as do
from tests import sampling_cases as sc
from tests.util import rel_linf, report

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fixture():
    return sc.load_fixture()


def _attn_ref(qkv, keep=None, p=0.0):
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    sc_ = q @ k.transpose(-1, -2) / math.sqrt(qkv.shape[-1])
    B, T, _, H, dh = qkv.shape
    w = torch.softmax(sc_, -1)
    if keep is not None:
        w = w * keep.reshape(B, H, T, T).double() / (1 - p)
    return (w @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh), torch.logsumexp(sc_, -1)


@pytest.mark.parametrize("case", list(sc.ATTN_CASES))
def test_attention_persistent(N, fixture, case):
    got = sc.run_attention(N, case)
    assert N.lib().bsi_compute_cus() == torch.cuda.get_device_properties(0).multi_processor_count, "a CU reserve was left behind"
    ref, _ = _attn_ref(sc.attn_input(case))
    o = got["out"].double()
    # P is rounded to bf16 before the PV product and O is stored as bf16: 1e-2 of the max, 4e-3 on average
    err, mean = rel_linf(o, ref), float((o - ref).abs().mean() / ref.abs().mean())
    report("sampling_fixture_attention", case=case, rel_linf=err, rel_mean=mean)
    assert err < 1e-2 and mean < 4e-3, (err, mean)
    sc.assert_matches(case, got, fixture)


def test_attention_dropout_lse_instance(N, fixture):
    case, B, heads, p, seed, site = sc.ATTN_DROP
    got = sc.run_attention(N, case)
    keep = torch.empty(B * heads * 256 * 256, dtype=torch.uint8, device=DEV)
    N.check(N.lib().bsi_dropout_mask(p, seed, site, B * heads * 256, 256, N.ptr(keep), N.stream()))
    ref, ref_lse = _attn_ref(sc.attn_input(case), keep.cpu(), p)
    o = got["out"].double()
    err, mean = rel_linf(o, ref), float((o - ref).abs().mean() / ref.abs().mean())
    lse_err = float((got["lse"].double() - ref_lse).abs().max())
    report("sampling_fixture_attention", case=case, rel_linf=err, rel_mean=mean, lse_abs=lse_err)
    assert err < 1e-2 and mean < 4e-3 and lse_err < 2e-3, (err, mean, lse_err)
    sc.assert_matches(case, got, fixture)


@pytest.mark.parametrize("M,shared,upd,write_x", sc.LN_CASES, ids=[sc.ln_id(*a) for a in sc.LN_CASES])
def test_ln_passes(N, fixture, M, shared, upd, write_x):
    d = sc.LN_D
    got = sc.run_ln(N, M, shared, upd, write_x)
    x, d0, d1, mod = sc.ln_inputs(M, shared, upd, write_x)
    rows = (torch.arange(M) // sc.LN_TOKENS) % mod.shape[0]
    x_new = x
    if upd == "two":
        x_new = torch.addcmul(x_new, mod[rows, 0:d], d0)  # fp32 fma in both
    if upd != "none":
        x_new = torch.addcmul(x_new, mod[rows, 2 * d:3 * d], d1)
    # the residual row: exact, and untouched where the pass must not store it
    assert torch.equal(got["x"], x_new if write_x else x)
    md = mod.double()
    ref = torch.addcmul(md[rows, 3 * d:4 * d], md[rows, 4 * d:5 * d] + 1, do.layer_norm(x_new.double()))
    err = float((got["out"].double() - ref).abs().max() / ref.abs().max())
    report("sampling_fixture_ln", case=sc.ln_id(M, shared, upd, write_x), rel_linf=err)
    assert err <= 2 ** -8, err  # fp32 statistics and one bf16 rounding (test_ln_modulate_widths)
    sc.assert_matches(sc.ln_id(M, shared, upd, write_x), got, fixture)


@pytest.mark.parametrize("case", list(sc.ENGINE_CASES))
def test_engine_and_final_kernel(N, fixture, case):
    got = sc.run_engine(N, case)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert float(got["out"].abs().max()) > 0
    sc.assert_matches(case, got, fixture)


def test_training_forward_with_mask_words_from_the_ln_pass(N, fixture):
    got = sc.run_train(N)
    assert bool(torch.isfinite(got["out"]).all())
    sc.assert_matches(sc.TRAIN_CASE[0], got, fixture)
