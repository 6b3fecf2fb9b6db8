"""Host side of max-scaled bucketed QSGD: the rotation's signs, the compressor's argument checks, the seed's range."""

import pytest
import torch

from omnifed_amd import codec
from omnifed_amd.hybrid.communicator.global_grpc_compression import (build_global_compressor,
                                                                      hybrid_global_compressor_from_cfg)
from omnifed_amd.hybrid.compression.qsgd import QSGDQuantCompression, encode_bucketed

RS = 20171


def test_signs():
    a, b = codec.rotation_signs(RS, 3, 0, 4096), codec.rotation_signs(RS + 1, 3, 0, 4096)
    assert set(a.tolist()) == {-1, 1}
    assert torch.equal(a, codec.rotation_signs(RS, 3, 0, 4096))  # deterministic in (seed, tensor, element)
    assert torch.equal(a[100:1000], codec.rotation_signs(RS, 3, 100, 900))
    assert not torch.equal(a, b) and not torch.equal(a, codec.rotation_signs(RS, 4, 0, 4096))
    for s in (a, b):
        assert 1792 <= int((s == -1).sum()) <= 2304  # +- 8 sigma of 4096 fair bits


@pytest.mark.parametrize("seed", [-1, 2 ** 31, 1.5, True])
def test_rotation_seed_range(seed):
    with pytest.raises(ValueError, match="rotation_seed"):
        codec.rotation_signs(seed, 0, 0, 4)


@pytest.mark.parametrize("kw", [dict(bucket_norm="max"), dict(bucket_norm="max", bucket_size=64, bucket_packed=True),
                                dict(bucket_norm="max", bucket_size=64, rng="mt19937"),
                                dict(bucket_norm="linf", bucket_size=64), dict(rotate=True, bucket_size=64),
                                dict(rotate=True), dict(bucket_norm="max", bucket_size=64, rotate=True, rotation_seed=-1),
                                dict(bucket_norm="max", bucket_size=64, rotate=True, rotation_seed=2 ** 31),
                                dict(bucket_norm="max", bucket_size=64, rotation_seed=1.5)])
def test_compressor_refuses(kw):
    with pytest.raises(ValueError):
        QSGDQuantCompression(bit_width=4, **kw)


def test_half_tensors_refused_and_builder_fields():
    with pytest.raises(ValueError, match="float32"):
        encode_bucketed([torch.zeros(64, dtype=torch.bfloat16)], 4, 64, torch.device("cpu"), norm="max")
    with pytest.raises(ValueError, match="scheme='qsgd'"):
        build_global_compressor(enabled=True, scheme="topk", bucket_norm="max")
    cfg = {"engine": {"hybrid": {"global_compression": {"enabled": True, "scheme": "qsgd", "bit_width": 4,
                                                        "bucket_size": 512, "bucket_norm": "max"}}}}
    comp = hybrid_global_compressor_from_cfg(cfg)
    assert (comp.bucket_norm, comp.bucket_size, comp.s, comp.bucket_packed) == ("max", 512, 4, False)
    assert build_global_compressor(enabled=True, scheme="qsgd", bucket_size=512).bucket_norm == "l2"  # the default
    cfg["engine"]["hybrid"]["global_compression"].update(bucket_rotate=True, rotation_seed=77)
    comp = hybrid_global_compressor_from_cfg(cfg)
    assert (comp.rotate, comp.rotation_seed, comp.wire_rotation_seed) == (True, 77, 77)


def test_layer_builder_fields():
    import numpy as np

    from omnifed_amd.hybrid.communicator.global_grpc_compression import (_check_bucketed_fields,
                                                                          qsgd_bucketed_layer_from_payload)
    scales = np.arange(3, dtype=np.float32)
    L = qsgd_bucketed_layer_from_payload("w", (130,), bytes(130), scales, 8, 16, 64, rotation_seed=77)
    assert L.compression_type == "QSGDRotatedBucketedCompression" and list(L.param_shape) == [64, 77]
    assert (L.width, L.level, list(L.original_shape)) == (8, 16, [130]) and L.meta_tensor == scales.tobytes()
    _check_bucketed_fields(L)
    plain = qsgd_bucketed_layer_from_payload("w", (130,), bytes(130), scales, 8, 16, 64)
    assert plain.compression_type == "QSGDBucketedCompression" and list(plain.param_shape) == [64]
    del L.param_shape[1:]  # a rotated layer without its seed
    with pytest.raises(ValueError):
        _check_bucketed_fields(L)
