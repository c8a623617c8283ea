"""The host side every ragged wrapper shares (unet_watermark_amd/_device.py), as far as it runs without a device: the capacities
derived from host descriptors, and the refusal of a workspace query that answered 0."""
import numpy as np
import pytest
import torch

from unet_watermark_amd import _device as D
from unet_watermark_amd.data import DESC_DTYPE


def test_ragged_capacities_of_host_records():
    descs = np.array([(0, 3, 5), (15, 0, 7), (15, 4, 2)], DESC_DTYPE)
    assert D.ragged_capacities(descs) == {"max_pixels": 15, "rows": 7, "total_pixels": 23}
    with pytest.raises(ValueError):
        D.ragged_capacities(np.zeros(0, DESC_DTYPE))


def test_workspace_of_zero_bytes_raises_the_librarys_message(monkeypatch):
    class Lib:
        @staticmethod
        def uwm_last_error():
            return b"uwm_x_workspace_bytes: n must be >= 1"
    monkeypatch.setattr(D.L, "lib", lambda: Lib)
    before = set(D._WORKSPACE)
    with pytest.raises(RuntimeError, match="uwm_x_workspace_bytes: n must be >= 1"):
        D.workspace("x", torch.device("cpu"), 0)
    with pytest.raises(ValueError, match="n must be >= 1"):
        D.workspace("x", torch.device("cpu"), 0, ValueError)
    assert set(D._WORKSPACE) == before
