"""The oracle's analytic backward against float64 autograd on every case of the regime matrix (tests/f64_regimes.py):
SH degrees 0..3 with 16 coefficients, clamped colours, scale modifiers, precomputed colours / covariances, off-cone
Gaussians, saturated opacities, unnormalised quaternions and the depth loss."""
import numpy as np
import pytest

import f64_regimes as R
from helpers import assert_grads_close


@pytest.mark.parametrize("name", R.CASES)
def test_oracle_backward_matches_float64_regime(oracle, name):
    r = R.regime(name)
    f, g = R.oracle_run(oracle, r)
    want, stats, img = R.f64_run(f, r)
    R.regime_count(r, f, want, stats, got=g)
    masked, report = R.masked_rows(r, f, stats)
    keep = np.ones(f["color"].shape[1] * f["color"].shape[2], bool)
    keep[R.flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])] = False
    dc = np.abs(img.numpy() - f["color"]).reshape(3, -1)[:, keep]
    print(f"  {report}; colour max diff outside the flipped pixels {dc.max():.2e}")
    assert dc.max() < 5e-6
    worst = assert_grads_close(g, want, tol=R.TOL, tag=f"oracle vs float64 [{name}]", masked=masked, keys=R.grad_keys(r))
    print(f"  worst tensor-wide error {worst:.2e}")
