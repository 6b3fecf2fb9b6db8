"""The host side of bucketed QSGD on the bit-packed wire: the ``QSGDBucketedPackedCompression`` ``LayerState`` and
its validation, the compressor's opt-in and its refused combinations, the config key.  No GPU."""

import numpy as np
import pytest

from omnifed_amd import codec
from omnifed_amd.hybrid.communicator import global_grpc_compression as wire
from omnifed_amd.hybrid.compression import QSGD_BUCKETED_PACKED_COMPRESSION_NAME, QSGDQuantCompression


def _layer(n=300, d=128, level=16):
    b = codec.packed_bits(level)
    norms = np.arange(1, -(-n // d) + 1, dtype=np.float32)
    return wire.qsgd_bucketed_packed_layer_from_payload("w", (n,), bytes(-(-n * b // 8)), norms, level, d)


@pytest.mark.parametrize("level,b", ((16, 6), (256, 10), (100, 8)))
def test_layer_fields_and_wire_size(level, b):
    L = _layer(level=level)
    assert L.compression_type == QSGD_BUCKETED_PACKED_COMPRESSION_NAME == "QSGDBucketedPackedCompression"
    assert (list(L.param_shape), list(L.original_shape), L.width, L.level) == ([128], [300], b, level)
    assert (L.values_dtype, L.meta_tensor_dtype) == (f"packed.u{b}", "torch.float32")
    assert len(L.values_data) == -(-300 * b // 8)
    assert np.array_equal(np.frombuffer(L.meta_tensor, dtype="<f4"), [1.0, 2.0, 3.0])
    assert wire._validate_layer(L) is None
    assert wire.wire_size([L])["payload_bytes"] == -(-300 * b // 8) + 12


@pytest.mark.parametrize("bad,match", (
    (lambda L: L.param_shape.__setitem__(0, 100), "bucket size"),
    (lambda L: setattr(L, "meta_tensor", L.meta_tensor[:8]), "bucket norms"),
    (lambda L: setattr(L, "width", 8), "width"),
    (lambda L: setattr(L, "values_data", L.values_data[:-1]), "224 bytes"),
    (lambda L: setattr(L, "values_data", b""), "missing values_data"),
))
def test_validate_layer_errors(bad, match):
    L = _layer()
    bad(L)
    with pytest.raises(ValueError, match=match):
        wire._validate_layer(L)


def test_opt_in_and_refused_combinations():
    with pytest.raises(ValueError, match="bucket_size"):
        QSGDQuantCompression(bit_width=4, bucket_packed=True)
    with pytest.raises(ValueError, match="bucket_size"):
        QSGDQuantCompression(bit_width=4, bucket_size=256, bucket_packed=True, rng="mt19937")
    with pytest.raises(ValueError, match="bucket_packed"):
        wire.build_global_compressor(enabled=True, scheme="topk", bucket_packed=True)
    with pytest.raises(ValueError, match="bucket_packed"):
        wire.build_global_compressor(enabled=True, scheme="qsgd", bucket_packed=True)
    assert not QSGDQuantCompression(bit_width=4, bucket_size=256).bucket_packed  # off unless asked for
    comp = wire.hybrid_global_compressor_from_cfg({"engine": {"hybrid": {"global_compression": {
        "enabled": True, "scheme": "qsgd", "bit_width": 4, "bucket_size": 128, "bucket_packed": True}}}})
    assert comp.bucket_size == 128 and comp.bucket_packed and not comp.packed_wire
