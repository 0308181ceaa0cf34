"""Host side of the fp16 inference storage (round 6), CPU only: the activation buffer's storage
type, the descriptors' f16 flag and the one-storage-type-per-launch rule (ops._same_storage), and
the chain's exactness test of the residual-fold scale in the storage type (engine._storage_exact),
and the refusal of fp16 buffers by the builders of the bf16-only glue kernels (ops._bf16_only).
The kernels themselves are tested on the GPU (tests/test_gpu_fp16.py)."""
import pytest
import torch

from image_super_resolution_amd import engine, ops

F16, BF16 = torch.float16, torch.bfloat16


def test_act_buffer_storage_type():
    a = ops.ActBuffer.alloc(1, 5, 7, 32, 1, "cpu", dtype=F16)
    assert a.t.dtype == F16 and a.f16 == 1 and (a.ha, a.wa) == (ops.round_up(5, ops.TILE_H), 32)
    assert ops.ActBuffer.alloc(1, 5, 7, 32, 1, "cpu").f16 == 0  # bf16 stays the default
    x = torch.randn(1, 32, 5, 7)
    a.set_nchw(x)
    assert a.t.dtype == F16 and torch.equal(a.to_nchw(), x.to(F16).float())
    assert a.outside_valid().abs().max().item() == 0.0
    with pytest.raises(TypeError):
        ops.ActBuffer.alloc(1, 5, 7, 32, 1, "cpu", dtype=torch.float32)


def test_conv_desc_takes_its_storage_from_the_launch():
    xh = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu", dtype=F16)
    yh = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu", dtype=F16)
    wh = torch.zeros(64 * 64 * 9, dtype=F16)
    assert ops.conv3x3_desc(xh, 64, wh, None, 64, yh).f16 == 1
    xb = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu")
    yb = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu")
    assert ops.conv3x3_desc(xb, 64, wh.to(BF16), None, 64, yb).f16 == 0
    for args in ((xb, wh, yb), (xh, wh.to(BF16), yh), (xh, wh, yb)):
        with pytest.raises(TypeError):
            ops.conv3x3_desc(args[0], 64, args[1], None, 64, args[2])
    with pytest.raises(TypeError):  # a residual of the other storage type
        ops.conv3x3_desc(xh, 64, wh, None, 64, yh, r1=xb, s1=0.2)


def test_fold_scale_exactness_per_storage_type():
    # add_rate 0.2 -> 1/s1 = 5: exact in both; 1/0.3 is in neither; 1/0.15 = 6.666.. likewise
    for f16 in (0, 1):
        assert engine._storage_exact(1 / 0.2, f16)
        assert not engine._storage_exact(1 / 0.3, f16)
    # 1 + 2^-9 has 9 mantissa bits: exact in fp16 (10), not in bf16 (7)
    v = 1 + 2 ** -9
    assert engine._storage_exact(v, 1) and not engine._storage_exact(v, 0)


def _glue_builders(monkeypatch):
    """(name, call) per bf16-only descriptor builder; call(dtype) builds one descriptor with every
    ActBuffer of that storage type.  convert_desc wants a device tensor for its NCHW side, which
    the storage check does not concern: the device check is stubbed out for it."""
    monkeypatch.setattr(ops, "_require_gpu", lambda t, what: None)

    def buf(dt, c=64, h=16, w=32, **kw):
        return ops.ActBuffer.alloc(1, h, w, c, 1, "cpu", dtype=dt, **kw)

    bn = torch.nn.BatchNorm2d(64)
    st = ops.BNState(64, "cpu")
    return [
        ("ew_combine_desc", lambda dt: ops.ew_combine_desc(buf(dt), buf(dt), 64, b=buf(dt), m=buf(dt))),
        ("pixel_shuffle2_desc", lambda dt: ops.pixel_shuffle2_desc(buf(dt, 16, 32, 64), buf(dt, 64), 16)),
        ("pixel_unshuffle2_desc", lambda dt: ops.pixel_unshuffle2_desc(buf(dt, 64), buf(dt, 16, 32, 64, ha=64, wa=64),
                                                                       64, m=buf(dt, 16, 32, 64, ha=64, wa=64))),
        ("convert_desc", lambda dt: ops.convert_desc(torch.zeros(1, 3, 16, 32), buf(dt, 16), m=buf(dt, 16))),
        ("pool_desc", lambda dt: ops.pool_desc(buf(dt, 64, 32, 64, ha=64, wa=64), buf(dt), 64,
                                               buf(dt, 64, 32, 64, ha=64, wa=64))),
        ("bn_desc", lambda dt: ops.bn_desc(buf(dt), buf(dt), 64, st, bn, r1=buf(dt), r2=buf(dt), dz=buf(dt))),
    ]


@pytest.mark.parametrize("name", ["ew_combine_desc", "pixel_shuffle2_desc", "pixel_unshuffle2_desc", "convert_desc",
                                  "pool_desc", "bn_desc"])
def test_glue_builders_are_bf16_only(name, monkeypatch):
    """The elementwise / layout / pool / BatchNorm kernels read bf16 bits (load8_bf16): their
    descriptor builders refuse an fp16 ActBuffer by name and still take bf16."""
    call = dict(_glue_builders(monkeypatch))[name]
    with pytest.raises(TypeError, match=rf"{name}: .*bf16 only"):
        call(F16)
    assert call(BF16) is not None


def test_glue_builders_refuse_one_fp16_operand_among_bf16():
    y, a = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu"), ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu")
    mh = ops.ActBuffer.alloc(1, 16, 32, 64, 1, "cpu", dtype=F16)
    with pytest.raises(TypeError, match="bf16 only"):
        ops.ew_combine_desc(y, a, 64, m=mh)
    with pytest.raises(TypeError, match="bf16 only"):
        ops.bn_desc(y, a, 64, ops.BNState(64, "cpu"), torch.nn.BatchNorm2d(64), r2=mh)
    with pytest.raises(TypeError, match="bf16 only"):  # refused before the device check of the NCHW side
        ops.convert_desc(torch.zeros(1, 3, 16, 32), mh)
