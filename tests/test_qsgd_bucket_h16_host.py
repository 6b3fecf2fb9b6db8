"""The 16-bit bucketed encoders' argument errors that need no GPU: a value_format that names no 16-bit format is
refused by the library before anything else is looked at, and the Plan wrappers refuse an fp64 arena."""

import pytest
import torch

from omnifed_amd import _lib, codec


@pytest.mark.parametrize("fmt", (0, 3, -1))
def test_bad_value_format_is_einval(fmt):
    L = _lib.lib()
    calls = (lambda: L.omf_qsgd_encode_bucketed_h16(None, None, fmt, 1.0, 4, 64, None, 0, 0, None, None, None, None),
             lambda: L.omf_qsgd_norms_bucketed_h16(None, None, fmt, 1.0, 64, None, None),
             lambda: L.omf_qsgd_encode_bucketed_packed_h16(None, None, fmt, 1.0, 4, 64, None, 0, 0, None, None, None, None))
    for call in calls:
        assert call() == _lib.OMF_EINVAL
        assert b"value_format" in L.omf_last_error()


@pytest.mark.parametrize("method", ("qsgd_encode_bucketed", "qsgd_encode_bucketed_packed"))
def test_fp64_arena_is_refused(method):
    x = torch.zeros(64, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):  # the dtype is checked before the plan is touched
        getattr(codec.Plan, method)(None, x, 4, 64)
    with pytest.raises(ValueError, match="float64"):
        codec.Plan.qsgd_norms_bucketed(None, x, 64)
