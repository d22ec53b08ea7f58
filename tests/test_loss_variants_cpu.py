"""The reference trainer's whole loss import line, its remaining task types and their host-side rules (no GPU)."""
import importlib

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import train_listwise as TL
from tests import loss_variants_ref as R

# the import line of the reference trainer (reactranker/train/train_listwise.py:16-17), name for name
REFERENCE_IMPORT_LINE = ["GaussDisLoss", "evidential_loss_new", "MLEloss", "MLEDisLoss", "Dirichlet_uq", "Listnet_For_evidential",
                         "Listnet_For_Gauss", "ListnetLoss", "Listnet_with_uq", "Listnetlognorm", "Lognorm", "evidential_ranking"]

NEW_TASKS = ["mledis_gaussian", "listnetdis_gauss", "listnetdis_lognorm", "listnet_uq", "evidential", "mle_evidential",
             "mledis_evidential", "listnet_evidential", "dirichlet_uq", "regression_exploss"]

NEW_SYMBOLS = ["rr_mledis_fwd_f32", "rr_mledis_bwd_f32", "rr_listnet_gauss_fwd_f32", "rr_listnet_gauss_bwd_f32",
               "rr_listnet_lognorm_fwd_f32", "rr_listnet_lognorm_bwd_f32", "rr_listnet_evidential_fwd_f32",
               "rr_listnet_evidential_bwd_f32", "rr_listnet_uq_fwd_f32", "rr_listnet_uq_bwd_f32", "rr_dirichlet_uq_fwd_f32",
               "rr_dirichlet_uq_bwd_f32", "rr_nig_fwd_f32", "rr_nig_bwd_f32", "rr_digamma_f32", "rr_lognorm_fwd_f32",
               "rr_lognorm_bwd_f32", "rr_exp_mse_fwd_f32", "rr_exp_mse_bwd_f32"]


def test_the_reference_import_line_imports_as_a_whole():
    mod = importlib.import_module("reactranker_amd.loss")
    missing = [n for n in REFERENCE_IMPORT_LINE if not hasattr(mod, n)]
    assert not missing, missing
    exec("from reactranker_amd.loss import " + ", ".join(REFERENCE_IMPORT_LINE), {})


def test_supported_tasks_cover_the_reference_branches():
    assert set(NEW_TASKS) <= set(TL.SUPPORTED_TASKS)
    assert "mle_dirichlet" not in TL.SUPPORTED_TASKS


def test_mle_dirichlet_is_refused_before_any_launch():
    out = torch.zeros(4, 1)                            # a CPU tensor: any launch attempt would fail differently
    with pytest.raises(ValueError, match="mle_dirichlet"):
        TL.batch_loss("mle_dirichlet", out, [4], torch.zeros(4), None)


def test_annealing_coefficient_is_the_references():
    from reactranker_amd.loss import annealing_coef
    assert annealing_coef(0.5, 2, 5) == 0.5 * (2 / 4) ** 3
    assert annealing_coef(1e-4, 0, 2) == 0.0
    with pytest.raises(ZeroDivisionError):
        annealing_coef(1e-4, 0, 1)


@pytest.mark.parametrize("cls", ["Listnet_with_uq", "Dirichlet_uq"])
def test_one_epoch_raises_zero_division_like_the_reference(cls):
    from reactranker_amd import loss as RL
    with pytest.raises(ZeroDivisionError):
        getattr(RL, cls)()(torch.ones(3), [3], torch.zeros(3), 1e-4, 0, 1, None)


def test_new_entries_are_exported():
    missing = [s for s in NEW_SYMBOLS if s not in _lib.EXPORTED_SYMBOLS]
    assert not missing, missing


def test_numpy_digamma_agrees_with_torch():
    x = np.concatenate([np.linspace(0.05, 1.0, 40), np.linspace(1.0, 50.0, 400), [6.0, 123.4, 1e4]])
    ref = torch.digamma(torch.tensor(x, dtype=torch.float64)).numpy()
    assert np.max(np.abs(R.digamma(x) - ref) / (1 + np.abs(ref))) < 1e-10     # series truncated after x^-10 at x >= 6


def test_numpy_cross_form_agrees_with_torch_broadcasting():
    rng = np.random.default_rng(3)
    M = 37
    mu = rng.standard_normal(M)
    v, b = np.log1p(np.exp(rng.standard_normal((2, M))))
    a = np.log1p(np.exp(rng.standard_normal(M))) + 1.0
    t = rng.standard_normal(M)
    ps = [torch.tensor(x[:, None], dtype=torch.float64, requires_grad=True) for x in (mu, v, a, b)]
    tt = torch.tensor(t)
    om = 2 * ps[3] * (1 + ps[1])
    l = (0.5 * torch.log(R.PI_F32 / ps[1]) - ps[2] * torch.log(om) + (ps[2] + 0.5) * torch.log(ps[1] * (tt - ps[0]) ** 2 + om)
         + torch.lgamma(ps[2]) - torch.lgamma(ps[2] + 0.5) + 0.3 * (torch.abs(tt - ps[0]) * (2 * ps[1] + ps[2]) - 1e-4)).mean()
    gs = torch.autograd.grad(l, ps)
    got = R.nig_cross(mu, v, a, b, t, 0.3, block=8)
    assert abs(got[0] - float(l.detach())) < 1e-12
    for x, g in zip(got[1:], gs):
        assert np.allclose(x, g.numpy().reshape(-1), rtol=1e-10, atol=1e-13)


# the golden keys of every restatement of tests/listwise_variants_ref.py: (value key, input columns, gradient suffixes)
VARIANT_KEYS = {
    "mledis": ("mledis", ["score", "var"], ["_gs", "_gv"]),
    "listnet_gauss": ("lgauss", ["score", "var"], ["_gs", "_gv"]),
    "listnet_lognorm": ("llognorm", ["pos", "var"], ["_gs", "_gv"]),
    "listnet_evidential": ("levid", ["score", "nu", "alpha"], ["_gs", "_gv", "_ga"]),
    "listnet_uq": ("uq", ["pos"], ["_g"]),
    "dirichlet_uq": ("dir", ["conc"], ["_g"]),
}


@pytest.mark.parametrize("case", ["single", "tiny", "c32", "c64", "ragged", "long"])
@pytest.mark.parametrize("kind", list(VARIANT_KEYS))
def test_listwise_restatements_reproduce_the_reference_vectors(kind, case, golden_dir):
    """tests/listwise_variants_ref.py against the reference's own float32 run (tests/golden/loss_variants.npz), values and
    every gradient: |loss - ref| / |ref| and max |g - ref| / max |ref| (absolute where the reference is exactly zero, as for
    the score gradient of a one-candidate list).  Evaluated in float32 the restatement is the reference's operation, in
    blocks of 50 rows so that the blocked sums are what is checked: 1e-6, a dozen float32 roundings of 6e-8.  Evaluated in
    float64 it sits where float32 rounding puts the reference: 1e-5, the project's parity bound."""
    import os
    from tests import listwise_variants_ref as LV
    V = np.load(os.path.join(golden_dir, "loss_variants.npz"))
    mc, ep, eps = V["uq_args"].tolist()
    coef = mc * (ep / (eps - 1)) ** 3
    key, cols, sfx = VARIANT_KEYS[kind]
    P = case + "."
    for dtype, bound in ((torch.float32, 1e-6), (torch.float64, 1e-5)):
        loss, grads = LV.variant_loss(kind, [V[P + c] for c in cols], V[P + "scope"].tolist(), V[P + "targets"], coef,
                                      dtype=dtype, block=50)
        ref = float(V[P + key].reshape(-1)[0])
        assert abs(loss - ref) / (abs(ref) or 1.0) <= bound, (dtype, loss, ref)
        for g, s in zip(grads, sfx):
            r = V[P + key + s].astype(np.float64).reshape(-1)
            assert g.shape == r.shape
            assert np.max(np.abs(g - r)) / (np.max(np.abs(r)) or 1.0) <= bound, (dtype, s)
