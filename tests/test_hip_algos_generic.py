"""bsi_amd.VDM and bsi_amd.BFN in fp32 around a generic torch denoiser (the README Conv2d on 3 x 8 x 8) against VDMOracle /
BFNOracle in fp64 with the same weights and the same draws: the fallback branch of both wrappers (self.model -> _PredictCombine
-> _Clip -> _SqErr, and the stride-0 bsi_predict_combine of the samplers), discretization=None, and low_discrepancy_sampling=
False.  Cases, draws and limits come from tests/algo_cases.py; tests/test_algo_cases_host.py has vetted them on the CPU: the fixed
fp32-path bounds (1e-4 on losses and histories, 1e-5 on gradients) hold where the fp32 oracle alone stays within a quarter of them,
and the quantities of algo_cases.ON_RULE follow the tolerance rule."""
import pytest
import torch

from tests import algo_cases as ac
from tests.util import TinyConv, bound, replay_draws

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
CASES = {c[0]: c for c in ac.GENERIC_CASES}


def make(algo, case):
    from bsi_amd import BFN, VDM, Discretization
    _, disc, lds, _, _ = case
    model = TinyConv()
    model.load_state_dict(ac.tinyconv_weights())
    model = model.to(DEV)
    kw = dict(data_shape=ac.GENERIC_SHAPE, k=ac.GENERIC_K, low_discrepancy_sampling=lds,
              discretization=Discretization.image_8bit() if disc == "8bit" else None)
    if algo == "vdm":
        return model, VDM(model, snr_min=ac.SNR_MIN, snr_max=ac.SNR_MAX, **kw).to(DEV)
    return model, BFN(model, sigma_1=ac.BFN_SIGMA_1, **kw).to(DEV)


def check(algo, case, got):
    """Every quantity of `got` against the fp64 oracle, at the limit tests/algo_cases.py gives it."""
    ref = ac.generic_eval(algo, case, F64)
    for name, value in got.items():
        kind, limit = ac.generic_limit(algo, case, name)
        assert value.shape == ref[name].shape, (name, value.shape, ref[name].shape)
        assert bool(torch.isfinite(value).all()), name
        bound(f"generic:{algo}:{case[0]}:{name}", ac.metric(kind, value.detach(), ref[name]), limit)


def grads(model):
    return {"grad:" + k: p.grad for k, p in model.named_parameters()}


@pytest.mark.parametrize("cid", ["8bit", "cont"])
def test_vdm_losses_and_gradients(cid):
    case = CASES[cid]
    _, _, _, B, n = case
    d = ac.generic_draws("vdm", case)
    model, v = make("vdm", case)
    x = d["x"].to(DEV)
    with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm1"]], randn=[d["eps1"][None]]):
        loss = v.train_loss(x)
    loss.mean().backward()
    got = {"train_loss": loss.detach(), **grads(model)}
    with torch.no_grad():
        got["l_prior"] = v.prior_loss(x)
        with replay_draws(DEV, randn=[d["eps_recon"]]):
            got["l_recon"] = v.reconstruction_loss(x, n)
        with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm"]], randn=[d["eps"]]):
            got["l_diff"] = v.inf_diffusion_loss(x, n)
        with replay_draws(DEV, randint=[d["i"]], randn=[d["eps_fin"]]):
            got["l_diff_fin"] = v.finite_diffusion_loss(x, n)
        with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm"]], randn=[d["eps_recon"], d["eps"]]):
            got["elbo"], got["bpd"], extra = v.elbo(x, n, n, estimate_var=True)
        got["bpd_var"] = extra["bpd_var"]
        assert all(torch.equal(extra[k], got[k]) for k in ("l_prior", "l_recon", "l_diff"))
        with replay_draws(DEV, randint=[d["i"]], randn=[d["eps_recon"], d["eps_fin"]]):
            got["fin_elbo"], got["fin_bpd"], extra = v.finite_elbo(x, n, n, estimate_var=True)
        got["fin_bpd_var"] = extra["bpd_var"]
        assert torch.equal(extra["l_diff"], got["l_diff_fin"])
    check("vdm", case, got)


@pytest.mark.parametrize("cid", ["8bit", "cont"])
def test_vdm_sampler(cid):
    case = CASES[cid]
    n, k = case[4], ac.GENERIC_K
    d = ac.generic_draws("vdm", case)
    ref = ac.generic_eval("vdm", case, F64)
    _, v = make("vdm", case)
    ts = torch.linspace(1.0, 0.0, k + 1, device=DEV)
    draws = [d["eps0"], *d["eps_steps"]]
    with torch.no_grad():
        xh, zs = [], []
        for i in range(k):  # one step from the oracle's own z_t (and, for z_s, its x_hat)
            z = ref["zs"][i].float().to(DEV)
            xh.append(v._predict_x(z, ts[i].repeat(n)))
            with replay_draws(DEV, randn=[d["eps_steps"][i]]):
                zs.append(v._sample_zs_given_zt_x(ts[i + 1].repeat(n), z, ts[i].repeat(n), ref["x_hats"][i].float().to(DEV)))
        with replay_draws(DEV, randn=draws):
            hist = v.sample_history(n)
        with replay_draws(DEV, randn=draws):
            smp = v.sample(n)
    assert torch.equal(smp, hist[-1])
    check("vdm", case, {"tf:x_hats": torch.stack(xh), "tf:zs": torch.stack(zs), "x_hats": hist})


@pytest.mark.parametrize("cid", ["8bit", "cont"])
def test_bfn_losses_and_gradients(cid):
    case = CASES[cid]
    _, _, _, B, n = case
    d = ac.generic_draws("bfn", case)
    model, b = make("bfn", case)
    x = d["x"].to(DEV)
    t = torch.linspace(0, 1, ac.GENERIC_K + 1, device=DEV)
    with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm1"]], randn=[d["eps1"]]):
        loss = b.train_loss(x)
    loss.backward()
    got = {"train_loss": loss.detach(), **grads(model)}
    with torch.no_grad():
        with replay_draws(DEV, randn=[d["eps_recon"]]):
            got["l_recon"] = b.reconstruction_loss(x, n)
        with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm"]], randn=[d["eps"]]):
            got["l_latent"] = b.continuous_time_loss(x, n)
        with replay_draws(DEV, randint=[d["i"]], randn=[d["eps_fin"]]):
            got["l_latent_fin"] = b.discrete_time_loss(x, n, t=t)
        with replay_draws(DEV, rand=[d["offset"]], randperm=[d["perm"]], randn=[d["eps_recon"], d["eps"]]):
            got["elbo"], got["bpd"], extra = b.elbo(x, n, n, estimate_var=True)
        got["bpd_var"] = extra["bpd_var"]
        assert all(torch.equal(extra[k], got[k]) for k in ("l_recon", "l_latent"))
        with replay_draws(DEV, randint=[d["i"]], randn=[d["eps_recon"], d["eps_fin"]]):
            got["fin_elbo"], got["fin_bpd"], extra = b.finite_elbo(x, n, n, t=t, estimate_var=True)
        got["fin_bpd_var"] = extra["bpd_var"]
        assert torch.equal(extra["l_latent"], got["l_latent_fin"])
    check("bfn", case, got)


@pytest.mark.parametrize("cid", ["8bit", "cont"])
def test_bfn_sampler(cid):
    case = CASES[cid]
    n, k = case[4], ac.GENERIC_K
    d = ac.generic_draws("bfn", case)
    ref = ac.generic_eval("bfn", case, F64)
    _, b = make("bfn", case)
    t = torch.linspace(0, 1, k + 1, device=DEV)
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    with torch.no_grad():
        xh = [b._predict_x(ref["mus"][i].float().to(DEV), t_eval[i].repeat(n)) for i in range(k + 1)]  # from the oracle's own mu
        with replay_draws(DEV, randn=list(d["eps_steps"])):
            mus, x_hats, ys = b.sample_history(n)
        with replay_draws(DEV, randn=list(d["eps_steps"])):
            smp = b.sample(n)
    assert torch.equal(smp, x_hats[-1])
    check("bfn", case, {"tf:x_hats": torch.stack(xh), "mus": mus, "x_hats": x_hats, "ys": ys})


@pytest.mark.parametrize("algo", ["vdm", "bfn"])
def test_without_low_discrepancy_sampling(algo):
    """low_discrepancy_sampling=False: the times are one rand((B, n)) draw read as [n, B], as in the reference (n = B = 2)."""
    case = CASES["iid"]
    _, _, _, B, n = case
    d = ac.generic_draws(algo, case)
    _, w = make(algo, case)
    x = d["x"].to(DEV)
    with torch.no_grad(), replay_draws(DEV, rand=[d["t_iid"]], randn=[d["eps"]]):
        got = {"l_diff": w.inf_diffusion_loss(x, n)} if algo == "vdm" else {"l_latent": w.continuous_time_loss(x, n)}
    check(algo, case, got)
