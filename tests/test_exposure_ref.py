"""The CPU mirror of the exposure-compensated loss (tests/exposure_ref.py) is a sound yardstick: its float32 results
agree with the same ops in float64 far inside the 1e-4 bar the GPU tests use, the identity reproduces the loss
oracle, and its Adam mirror lowers the loss of a gain-mismatched pair.  No GPU."""
import numpy as np
import pytest
import torch

import exposure_ref as er
from util import max_err_over_max


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("h,w", [(7, 5), (16, 16), (17, 33), (37, 53), (64, 64), (270, 480)])
def test_fp32_mirror_agrees_with_fp64(h, w, masked):
    c, t, E, mask = er.make_case(h, w)
    mask = mask if masked else None
    a = er.case(h, w, masked)[4] if (h, w) in er.SHAPES else er.mirror(c, t, E, mask)
    b = er.mirror(c, t, E, mask, dtype=torch.float64)
    errs = {k: max_err_over_max(a[k], b[k]) for k in ("dL_dcolor", "dL_dexposure", "corrected")}
    errs.update({k: abs(a[k] - b[k]) / max(1.0, abs(b[k])) for k in ("loss", "l1", "ssim_mean")})
    print((h, w), "masked" if masked else "plain", {k: f"{v:.1e}" for k, v in errs.items()})
    # the mirror's own rounding, two orders below the GPU tests' 1e-4 gradient bar
    assert all(v <= 1e-5 for v in errs.values()), errs


def test_identity_exposure_reproduces_the_loss_oracle():
    lo = er.loss_oracle()
    c, t, _, _ = er.make_case(37, 53)
    eye = er.identity()
    want_loss, want_grad, want_l1, want_ssim = lo.combined_loss_and_grad(c.numpy(), t.numpy(), 0.2)
    for E in (None, eye):
        got = er.mirror(c, t, E, None)
        assert abs(got["loss"] - want_loss) <= 1e-7 and abs(got["l1"] - want_l1) <= 1e-7
        assert abs(got["ssim_mean"] - want_ssim) <= 1e-6
        assert max_err_over_max(got["dL_dcolor"], want_grad) <= 1e-6
        assert np.array_equal(got["corrected"], c.numpy())


def test_mask_semantics():
    """Means over all 3 H W elements; no gradient where the mask is 0; an all-zero mask is a perfect score."""
    c, t, E, mask = er.make_case(17, 33)
    got = er.mirror(c, t, E, mask)
    off = (mask == 0).numpy()
    assert off.any() and not got["dL_dcolor"][off].any()
    zero = er.mirror(c, t, E, torch.zeros_like(mask))
    assert zero["l1"] == 0.0 and abs(zero["ssim_mean"] - 1.0) <= 1e-6
    assert not zero["dL_dcolor"].any() and not zero["dL_dexposure"].any()


def test_mirror_adam_steps_lower_the_loss():
    """A target that is the image under a gain: twenty Adam steps on the exposure, from the identity, lower the loss."""
    c, _, _, mask = er.make_case(17, 33)
    target = (1.3 * c + 0.05).contiguous()
    row, adam, losses = er.identity(), er.AdamMirror(er.identity()), []
    for _ in range(20):
        m = er.mirror(c, target, row, mask)
        losses.append(m["loss"])
        row = adam.step(m["dL_dexposure"], 0.01)
    final = er.mirror(c, target, row, mask)["loss"]
    assert final < losses[-1] < losses[0] and final < 0.8 * losses[0], (losses[0], final)
