"""Host-side pieces that need no GPU: Preprocessor contract, resize_by_factor (the reference's own
test cases, tests/test_transforms.py:6-28), take()."""
import numpy as np
import pytest

from empanada_napari_amd.preprocess import (Preprocessor, is_raw_input, normalize, normalize_params, padded_hw, plan_raw,
                                            resize_by_factor)


@pytest.mark.parametrize('image,scale,expected', [
    ([[10., 20.], [30., 40.]], 1, [[10., 20.], [30., 40.]]),
    ([[10., 20.], [30., 40.]], 0.5, [[10., 12.5, 17.5, 20.], [15., 17.5, 22.5, 25.], [25., 27.5, 32.5, 35.], [30., 32.5, 37.5, 40.]]),
    ([[10., 20.], [30., 40.]], 2, [[25.]])])
def test_resize_by_factor_reference_cases(image, scale, expected):
    out = resize_by_factor(np.array(image), scale)
    assert out.shape == np.array(expected).shape
    assert np.array_equal(out, expected)


def test_resize_shapes_and_dtype():
    img = (np.arange(35 * 51) % 251).astype(np.uint8).reshape(35, 51)
    out = resize_by_factor(img, 2)
    assert out.shape == (18, 26) and out.dtype == np.uint8
    assert out.shape[0] * 2 >= 35 and out.shape[1] * 2 >= 51      # volume_dataset.py:48-49


def test_preprocessor_contract():
    p = Preprocessor(mean=0.57571, std=0.12765)
    img8 = np.array([[0, 255], [128, 64]], dtype=np.uint8)
    t = p(img8)['image']
    assert tuple(t.shape) == (1, 2, 2) and t.dtype.is_floating_point
    np.testing.assert_allclose(t[0].numpy(), (img8.astype(np.float32) - 0.57571 * 255) / (0.12765 * 255), rtol=1e-6)
    img16 = (img8.astype(np.uint16) * 257)
    np.testing.assert_allclose(p(img16)['image'][0].numpy(), t[0].numpy(), rtol=1e-5, atol=1e-5)   # iinfo(dtype).max scaling (Q14)
    with pytest.raises(Exception, match='cannot be float'):
        p(img8.astype(np.float32))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_plan_raw_constants_are_normalize_params(dtype):
    """the raw route's (sub, mul) are normalize_params' fp32 values, bit for bit (what the model call receives is
    float(fp32), an exact conversion)"""
    p = Preprocessor(mean=0.57571, std=0.12765)
    plan = plan_raw(p, dtype, (250, 230), 16)
    sub, mul = normalize_params(p.mean, p.std, np.iinfo(dtype).max)
    assert sub.dtype == mul.dtype == np.float32
    assert (plan.sub, plan.mul) == (float(sub), float(mul))
    assert np.float32(plan.sub).tobytes() == sub.tobytes() and np.float32(plan.mul).tobytes() == mul.tobytes()
    assert plan == plan_raw(p, np.dtype(dtype), (250, 230), 16)
    with pytest.raises(AttributeError):
        plan.sub = 0.0      # immutable


def test_plan_raw_padding():
    p = Preprocessor(mean=0.5, std=0.25)
    assert plan_raw(p, np.uint8, (250, 230), 16).pad_to == (256, 240) == padded_hw(250, 230, 16)
    assert plan_raw(p, np.uint8, (256, 240), 16).pad_to == (256, 240) == padded_hw(256, 240, 16)
    assert padded_hw(1, 17, 16) == (16, 32) and padded_hw(33, 7, 1) == (33, 7) and padded_hw(129, 128, 128) == (256, 128)


def test_raw_route_qualification():
    p = Preprocessor(mean=0.5, std=0.25)
    for dtype in (np.uint8, np.uint16):
        img = np.zeros((4, 6), dtype)
        assert is_raw_input(img) and is_raw_input(img, 1)
        assert not is_raw_input(img, 2) and not is_raw_input(img, 0.5)      # native scale only
        assert not is_raw_input(img.tolist()) and not is_raw_input(memoryview(img))      # numpy arrays only
    for dtype in (np.int16, np.float32, np.int8, np.uint32, np.float64, bool):
        assert not is_raw_input(np.zeros((4, 6), dtype)), dtype
        assert plan_raw(p, dtype, (4, 6), 16) is None, dtype


def test_take():
    from empanada_napari_amd.inference import take
    v = np.arange(24).reshape(2, 3, 4)
    assert np.array_equal(take(v, 1, 0), v[1]) and np.array_equal(take(v, 2, 1), v[:, 2]) and np.array_equal(take(v, 3, 2), v[:, :, 3])
