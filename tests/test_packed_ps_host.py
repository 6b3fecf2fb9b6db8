"""omf_qsgd_decode_sum_packed without a GPU: the symbol is bound, and the argument checks that need no
device come before any device work."""

import ctypes

from omnifed_amd import _lib
from omnifed_amd.build import build


def test_symbol_is_bound():
    assert "omf_qsgd_decode_sum_packed" in _lib.SIGNATURES
    build()
    assert hasattr(_lib.lib(), "omf_qsgd_decode_sum_packed")


def test_refusals_before_any_device_work():
    build()
    L = _lib.lib()
    one = (ctypes.c_void_p * 1)(None)
    # no plan
    assert L.omf_qsgd_decode_sum_packed(None, one, one, 1, 16, None, 0, 0.0, None) == _lib.OMF_EINVAL
    assert b"plan" in L.omf_last_error()
    # no client (checked first: the message names it even without a plan)
    assert L.omf_qsgd_decode_sum_packed(None, one, one, 0, 16, None, 0, 0.0, None) == _lib.OMF_EINVAL
    assert b"nclients" in L.omf_last_error()
    assert L.omf_qsgd_decode_sum_packed(None, one, one, -3, 16, None, 0, 0.0, None) == _lib.OMF_EINVAL
    assert b"nclients" in L.omf_last_error()
