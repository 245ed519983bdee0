"""The comparison helper of the per-kernel GPU suite (test_unet_kernels_gpu.close) on the CPU: it must fail on NaN / inf
outputs, on a single element far outside tolerance and on a shape mismatch, and pass a reference perturbed within tolerance."""
import pytest
import torch

from test_unet_kernels_gpu import CLOSE_CEILING, close

RTOL = ATOL = 4e-3


def ref_and_copy():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1000, 320, generator=g)
    return ref, ref.clone()


def test_all_nan_fails():
    ref, got = ref_and_copy()
    got.fill_(float("nan"))
    with pytest.raises(AssertionError, match="non-finite 320000"):
        close(got, ref, RTOL, ATOL, "all nan")


@pytest.mark.parametrize("val", [float("inf"), float("-inf"), float("nan")])
def test_single_non_finite_element_fails(val):
    ref, got = ref_and_copy()
    got[999, 319] = val
    with pytest.raises(AssertionError, match=r"worst element \(999, 319\)"):
        close(got, ref, RTOL, ATOL, "one non-finite")


def test_nan_tail_rows_fail():
    ref, got = ref_and_copy()
    got[-2:] = float("nan")             # a missed store of a ragged tail: 640 elements, under 1e-4 of a larger tensor too
    big_ref = torch.cat([ref] * 8)
    big_got = torch.cat([ref] * 7 + [got])
    with pytest.raises(AssertionError):
        close(big_got, big_ref, RTOL, ATOL, "nan tail")


def test_one_element_at_ten_tolerances_fails():
    ref, got = ref_and_copy()
    got[3, 7] = ref[3, 7] + 10 * (ATOL + RTOL * ref[3, 7].abs())
    with pytest.raises(AssertionError, match=r"worst element \(3, 7\)"):
        close(got, ref, RTOL, ATOL, "10x")


def test_few_large_errors_fail():
    ref, got = ref_and_copy()
    got[:3, :3] = 1e4                   # 9 elements = 2.8e-5 of the tensor: under the 1e-4 fraction, over the ceiling
    with pytest.raises(AssertionError):
        close(got, ref, RTOL, ATOL, "block")


def test_shape_mismatch_fails():
    ref, got = ref_and_copy()
    with pytest.raises(AssertionError, match="shape"):
        close(got[:, :1], ref, RTOL, ATOL, "broadcast")
    with pytest.raises(AssertionError, match="shape"):
        close(got.view(320, 1000), ref, RTOL, ATOL, "reshaped")


def test_within_tolerance_passes():
    ref, got = ref_and_copy()
    g = torch.Generator().manual_seed(1)
    got += 0.9 * (ATOL + RTOL * ref.abs()) * (2 * torch.rand(ref.shape, generator=g) - 1)
    close(got, ref, RTOL, ATOL, "perturbed")
    close(got.half(), ref, RTOL, ATOL, "16-bit storage")


def test_rare_outliers_under_the_ceiling_pass():
    ref, got = ref_and_copy()
    got[0, :20] = ref[0, :20] + 0.9 * CLOSE_CEILING * (ATOL + RTOL * ref[0, :20].abs())    # 20 elements = 6e-5 of the tensor
    close(got, ref, RTOL, ATOL, "rare outliers")
    got[1, :20] = got[0, :20]                                                                  # 40 = 1.25e-4: over the fraction
    with pytest.raises(AssertionError, match="frac bad"):
        close(got, ref, RTOL, ATOL, "too many outliers")
