"""The host side of QSGD with bucket norms: the bucket-norm arena's layout, the bucketed ``LayerState`` and
its validation, the compressor's refused combinations.  No GPU."""

import numpy as np
import pytest

from omnifed_amd import codec
from omnifed_amd.hybrid.communicator import global_grpc_compression as wire
from omnifed_amd.hybrid.compression import QSGD_BUCKETED_COMPRESSION_NAME, QSGDQuantCompression


@pytest.mark.parametrize("d", codec.BUCKET_SIZES)
def test_bucket_layout_counts_every_bucket(d):
    sizes = [1, d - 1, d, d + 1, 3 * d + 7]
    boff, nb = codec.bucket_layout(sizes, d)
    counts = [len({i // d for i in range(n)}) for n in sizes]  # brute force: the distinct buckets of a tensor
    assert counts == [1, 1, 1, 2, 4]
    assert boff == [sum(counts[:t]) for t in range(len(sizes))] and nb == sum(counts)


@pytest.mark.parametrize("d", (0, 1, 32, 96, 8192, -64))
def test_bad_bucket_sizes_raise(d):
    with pytest.raises(ValueError, match="bucket_size"):
        codec.bucket_layout([100], d)
    with pytest.raises(ValueError, match="bucket_size"):
        QSGDQuantCompression(bit_width=4, bucket_size=d)


@pytest.mark.parametrize("kw", ({"packed_wire": True}, {"rng": "mt19937"}))
def test_refused_constructor_combinations(kw):
    with pytest.raises(ValueError, match="bucket_size"):
        QSGDQuantCompression(bit_width=4, bucket_size=256, **kw)
    with pytest.raises(ValueError, match="bucket_size"):
        wire.build_global_compressor(enabled=True, scheme="topk", bucket_size=256)
    comp = wire.hybrid_global_compressor_from_cfg({"engine": {"hybrid": {"global_compression": {
        "enabled": True, "scheme": "qsgd", "bit_width": 4, "bucket_size": 128}}}})
    assert comp.bucket_size == 128 and comp.s == 4


def _layer(n=300, d=128, width=8, level=16, norms=None, payload=None):
    norms = np.arange(1, -(-n // d) + 1, dtype=np.float32) if norms is None else norms
    payload = bytes(n * width // 8) if payload is None else payload
    return wire.qsgd_bucketed_layer_from_payload("w", (n,), payload, norms, width, level, d)


def test_layer_fields_and_wire_size():
    L = _layer()
    assert L.compression_type == QSGD_BUCKETED_COMPRESSION_NAME == "QSGDBucketedCompression"
    assert (list(L.param_shape), list(L.original_shape), L.width, L.level) == ([128], [300], 8, 16)
    assert (L.values_dtype, L.meta_tensor_dtype) == ("torch.int8", "torch.float32")
    assert np.array_equal(np.frombuffer(L.meta_tensor, dtype="<f4"), [1.0, 2.0, 3.0])
    assert wire._validate_layer(L) is None
    assert wire.wire_size([L])["payload_bytes"] == 300 + 12


@pytest.mark.parametrize("bad,match", (
    (lambda L: L.param_shape.__setitem__(0, 100), "bucket size"),
    (lambda L: L.param_shape.append(128), "bucket size"),
    (lambda L: setattr(L, "meta_tensor", L.meta_tensor[:8]), "bucket norms"),
    (lambda L: setattr(L, "meta_tensor", L.meta_tensor + bytes(4)), "bucket norms"),
    (lambda L: setattr(L, "width", 16), "width"),
    (lambda L: setattr(L, "level", 0), "level"),
    (lambda L: setattr(L, "values_data", L.values_data[:299]), "299 bytes"),
    (lambda L: setattr(L, "values_data", b""), "missing values_data"),
))
def test_validate_layer_errors(bad, match):
    L = _layer()
    bad(L)
    with pytest.raises(ValueError, match=match):
        wire._validate_layer(L)

