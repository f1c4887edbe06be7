"""The CPU oracle against the independent NumPy restatement (tests/numpy_restatement.py) AWAY from the reference's float
defaults: Farneback's pyrScale, TVL1's tau / lambda / theta / scaleStep, Brox's alpha / gamma / scale_factor.  The GPU
parity tests for these parameters (tests/test_*_params_gpu.py) take the oracle as their reference; this file is what says
that the oracle reads them as a second, separately written restatement does.  No GPU needed.

Every comparison is the one the default-parameter test of the same algorithm uses (tests/test_oracle_tvl1.py,
test_oracle_farneback.py, test_oracle_brox.py): the bounds are theirs, for the reasons given there.  Every case also has to
differ from the oracle's default-parameter flow by more than 1e-3 px, so that a restatement (or an oracle) that ignored the
parameter could not pass."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import numpy_restatement as NR

DISCRIMINATION = 1e-3


def _set(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _moves(flow, default_flow):
    assert np.isfinite(flow).all()
    assert np.max(np.abs(flow - default_flow)) > DISCRIMINATION


# ------------------------------------------------------------------------------------------------ Farneback

@pytest.mark.parametrize("pyr_scale,levels", [(0.8, 6), (0.3, 2)])
def test_farneback_pyr_scale(oracle, pyr_scale, levels):
    """160x128, frames 8 apart (12 px of motion: the coarse levels matter).  0.8 keeps all 5 + 1 levels (128 * 0.8^5 = 41.9),
    0.3 keeps 2 (128 * 0.09 = 11.5 < 32)."""
    w, h = 160, 128
    clip = SynthClip(w, h, 12)
    f0, f1 = clip.frame(0), clip.frame(8)
    scale, n = 1.0, 1
    while n <= 5 and w * scale * pyr_scale >= 32 and h * scale * pyr_scale >= 32:
        scale, n = scale * pyr_scale, n + 1
    assert n == levels
    a = oracle.farneback_calc(f0, f1, _set(oracle.farneback_default_params(), pyr_scale=pyr_scale))
    _moves(a, oracle.farneback_calc(f0, f1))
    b = NR.farneback_calc(f0, f1, pyr_scale=pyr_scale)
    assert np.max(np.abs(a - b)) <= 2e-4  # test_oracle_farneback.py: same op order; Gaussian taps / matrix inverse differ in the last ulp


# ------------------------------------------------------------------------------------------------ TVL1

TVL1_SETS = {
    "tau": dict(tau=0.1),
    "lambda": dict(lambda_=0.05),
    "theta": dict(theta=0.5),
    "scale_step_half": dict(scale_step=0.5),   # an exact 2x resize
    "scale_step_0.6": dict(scale_step=0.6),
    "all": dict(tau=0.1, lambda_=0.05, theta=0.5, scale_step=0.6),
}


@pytest.mark.parametrize("name", list(TVL1_SETS))
def test_tvl1_parameters(oracle, name):
    w, h = 64, 48
    clip = SynthClip(w, h, 3)
    f0, f1 = clip.frame(0), clip.frame(2)
    kw = TVL1_SETS[name]
    flow_c, tr = oracle.tvl1_calc(f0, f1, _set(oracle.tvl1_default_params(), **kw), want_trace=True)
    _moves(flow_c, oracle.tvl1_calc(f0, f1))
    flow_n, iters_n = NR.tvl1_calc(f0, f1, **{{"lambda_": "lam"}.get(k, k): v for k, v in kw.items()})
    assert tr.nscales == len(iters_n)
    assert [r[:5] for r in tr.iters_table()] == iters_n
    assert np.max(np.abs(flow_c - flow_n)) <= 1e-5  # test_oracle_tvl1.py: same float32 op order; only the double reduction order differs


# ------------------------------------------------------------------------------------------------ Brox

BROX_SETS = {
    "alpha": dict(alpha=0.05),
    "gamma": dict(gamma=5.0),
    "alpha_gamma0": dict(alpha=1.0, gamma=0.0),
    "scale_factor_half": dict(scale_factor=0.5),
    "scale_factor_0.9": dict(scale_factor=0.9),
    "all": dict(alpha=0.05, gamma=5.0, scale_factor=0.6),
}


@pytest.mark.parametrize("name", list(BROX_SETS))
def test_brox_parameters(oracle, name):
    w, h = 40, 32
    clip = SynthClip(w, h, 6)
    f0, f1 = clip.frame(0), clip.frame(1)
    kw = BROX_SETS[name]
    p = _set(oracle.brox_default_params(), **kw)
    if "scale_factor" in kw:
        assert oracle.brox_pyramid_sizes(w, h, p) == NR.brox_pyramid_sizes(w, h, kw["scale_factor"])
    a = oracle.brox_calc(f0, f1, p)
    _moves(a, oracle.brox_calc(f0, f1))
    b = NR.brox_calc(f0, f1, **kw)
    assert np.max(np.abs(a - b)) <= 1e-5  # test_oracle_brox.py
