"""_check_infill on fabricated count vectors (no GPU): what the in-fill solvers publish in counts[..., 3] is an iteration count
or one of three negative codes, and every code is an error with its own message."""
import pytest
import torch

from diffusionhandles_amd import depth_transform as DT


def test_counts_pass():
    DT._check_infill(torch.tensor([0, 17, 920, 19999], dtype=torch.int32))
    DT._check_infill(torch.zeros(0, dtype=torch.int32))


def test_barrier_timeout_keeps_its_error():
    with pytest.raises(RuntimeError, match="grid barrier timed out") as ei:
        DT._check_infill(torch.tensor([12, -1, 40], dtype=torch.int32))
    assert not isinstance(ei.value, DT.InfillNotConverged)


def test_iteration_cap_is_its_own_error():
    assert DT.INFILL_NOT_CONVERGED == -2
    with pytest.raises(DT.InfillNotConverged, match="iteration cap"):
        DT._check_infill(torch.tensor([12, 40, -2], dtype=torch.int32))
    assert issubclass(DT.InfillNotConverged, RuntimeError)


def test_breakdown_is_an_error():
    assert DT.INFILL_BREAKDOWN == -3
    with pytest.raises(DT.InfillNotConverged, match="broke down"):
        DT._check_infill(torch.tensor([-3], dtype=torch.int32))


def test_unknown_negative_code_is_an_error():
    with pytest.raises(RuntimeError, match="unknown failure code -7"):
        DT._check_infill(torch.tensor([5, -7], dtype=torch.int32))
