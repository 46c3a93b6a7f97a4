"""A/B of the rewritten glue kernels against the kernels they replace, each through its C-ABI entry with the switch set per call
in one process: the second form of the fused stem against the first (EMP_STEM_POOL_LEGACY=1; EMP_STEM_POOL_GRID = 1, 2 and
unset), the 4 x 4 form of the four-pixel bilinear kernel against the 1 x 4 form (EMP_BILINEAR_UP4_LEGACY=1) and against
the one-pixel kernel, the four-output PointRend up-sampler against the one-output kernel (EMP_PR_UP2X_LEGACY=1), logits and keys.
Every comparison is of bits; there is no tolerance.  Every output buffer carries GC.GUARD sentinel elements behind its end and,
where its row stride exceeds C, junk in the pad channels, all of which must come back untouched.  The shapes and why they were
chosen: tests/glue_ab_case.py; that they reach what they are named for: tests/test_glue_ab_case_host.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import glue_ab_case as GC
import layers_case as LC

pytestmark = pytest.mark.gpu

F16 = 0          # EMP_OP_F16


def _abi():
    from empanada_napari_amd import _abi
    return _abi


def _stream():
    return _abi().stream_ptr(torch.device('cuda:0'))


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


class _env:
    """an environment switch that the library reads per call"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# ----------------------------------------------------------------------------
# fused stem
# ----------------------------------------------------------------------------
def _stem(dimg, dw, db, shape, dtype, legacy, grid):
    H, W, vh, vw = shape
    n = GC.N * (H // 4) * (W // 4) * 64
    out = torch.full((n + GC.GUARD,), LC.F16_SENTINEL, dtype=torch.float16, device='cuda:0')
    sub, mul = LC.NORMALISE[dtype]
    with _env('EMP_STEM_POOL_LEGACY', '1' if legacy else None), _env('EMP_STEM_POOL_GRID', grid):
        _abi().check(_abi().load().emp_op_stem_pool(_ptr(dimg), dtype, float(sub), float(mul), GC.N, H, W, vh, vw, _ptr(dw), _ptr(db),
                                                   _ptr(out), F16, _stream()), 'emp_op_stem_pool')
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[n:] == np.float16(LC.F16_SENTINEL)).all(), 'written behind the buffer'
    return a[:n].view(np.uint16)


@pytest.mark.parametrize('dtype', LC.STEM_DTYPES, ids=['f32', 'u8', 'u16'].__getitem__)
@pytest.mark.parametrize('shape', GC.STEM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem_pool_new_against_legacy(shape, dtype):
    H, W, vh, vw = shape
    seed = 7000 + 10 * (H + W + vh + vw) + dtype
    img = LC.stem_image(dtype, GC.N, vh, vw, seed)
    w, b = LC.stem_weights(7, 64, seed)
    if img.dtype == np.uint16:
        img = img.view(np.int16)
    dimg, dw, db = torch.from_numpy(img).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    want = _stem(dimg, dw, db, shape, dtype, legacy=True, grid=None)
    f = want.view(np.float16)
    assert np.isfinite(f).all() and (f > 0).any() and (f == 0).any()
    for grid in GC.STEM_GRIDS:
        got = _stem(dimg, dw, db, shape, dtype, legacy=False, grid=grid)
        np.testing.assert_array_equal(got, want, err_msg=f'second form, EMP_STEM_POOL_GRID={grid}')
    np.testing.assert_array_equal(_stem(dimg, dw, db, shape, dtype, legacy=True, grid='1'), want, err_msg='first form, one workgroup')


# ----------------------------------------------------------------------------
# bilinear: four-pixel kernel
# ----------------------------------------------------------------------------
def _bilinear(dx, shape, in_ld, out_ld, junk, variant, legacy):
    """-> (return code, the (N*H*W, out_ld) buffer as uint16 on the host after the call, its guard)"""
    C_, h, w, H, W = shape
    out = torch.from_numpy(junk.copy()).cuda()
    with _env('EMP_BILINEAR_UP4_LEGACY', '1' if legacy else None):
        rc = _abi().load().emp_op_bilinear_ac_nhwc(_ptr(dx), GC.N, h, w, C_, in_ld, _ptr(out), H, W, out_ld, F16, variant, _stream())
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    return rc, a[:GC.N * H * W * out_ld].reshape(-1, out_ld), a[GC.N * H * W * out_ld:]


@pytest.mark.parametrize('name', list(GC.UP4_CASES))
def test_bilinear_up4_new_against_legacy(name):
    abi = _abi()
    shape, in_pad, out_pad, takes = GC.UP4_CASES[name]
    C_, h, w, H, W = shape
    in_ld, out_ld = C_ + in_pad, C_ + out_pad
    x = GC.up4_input(shape, seed=H * W + C_)
    buf = np.full((GC.N, h, w, in_ld), np.inf, np.float16)       # pad channels of the input: never read
    buf[..., :C_] = x
    dx = torch.from_numpy(buf.view(np.int16)).cuda()
    junk = np.random.default_rng(7).integers(0, 1 << 15, GC.N * H * W * out_ld + GC.GUARD).astype(np.int16)
    body = junk[:GC.N * H * W * out_ld].reshape(-1, out_ld)
    results = {}
    for variant, legacy in ((0, False), (0, True), (1, False), (2, False), (2, True)):
        rc, got, guard = _bilinear(dx, shape, in_ld, out_ld, junk, variant, legacy)
        what = f'{name} variant {variant} legacy {legacy}'
        np.testing.assert_array_equal(guard, junk[body.size:], err_msg=f'{what}: written behind the buffer')
        if variant == 2 and not (GC.takes_1x4(*shape) if legacy else takes):
            assert rc != 0, f'{what}: not refused'
            with pytest.raises(abi.EmpError, match='four-pixel'):
                abi.check(rc, 'emp_op_bilinear_ac_nhwc')
            np.testing.assert_array_equal(got, body, err_msg=f'{what}: a refused call wrote')
            continue
        abi.check(rc, 'emp_op_bilinear_ac_nhwc')
        np.testing.assert_array_equal(got[:, C_:], body[:, C_:], err_msg=f'{what}: pad channels written')
        results[(variant, legacy)] = got[:, :C_].copy()
    one = results[(1, False)]
    assert np.isfinite(one.view(np.float16)).all()
    for key, got in results.items():
        np.testing.assert_array_equal(got, one, err_msg=f'{name}: variant {key[0]}, legacy {key[1]} against the one-pixel kernel')
    assert ((2, False) in results) == takes


# ----------------------------------------------------------------------------
# PointRend x2 up-sampler with keys
# ----------------------------------------------------------------------------
def _up2x(dx, shape, offset, legacy):
    N, Cc, h, w = shape
    n_out, n_keys = N * Cc * 4 * h * w, N * 4 * h * w
    out = torch.full((offset + n_out + GC.GUARD,), 12345.0, dtype=torch.float32, device='cuda:0')
    keys = torch.full((offset + n_keys + GC.GUARD,), -7777, dtype=torch.int32, device='cuda:0')
    assert out.data_ptr() % 16 == 0 and keys.data_ptr() % 16 == 0
    with _env('EMP_PR_UP2X_LEGACY', '1' if legacy else None):
        _abi().check(_abi().load().emp_pr_upsample2x_keys(_ptr(dx), N, Cc, h, w, _ptr(out, offset), _ptr(keys, offset), _stream()),
                     'emp_pr_upsample2x_keys')
    torch.cuda.synchronize()
    o, k = out.cpu().numpy().view(np.uint32), keys.cpu().numpy().view(np.uint32)
    return o, k


@pytest.mark.parametrize('offset', GC.UP2X_OFFSETS, ids=['aligned', 'one_float_past'])
@pytest.mark.parametrize('shape', GC.UP2X_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample2x_keys_new_against_legacy(shape, offset):
    N, Cc, h, w = shape
    x = GC.up2x_input(shape, seed=h * w + Cc)
    dx = torch.from_numpy(x).cuda()
    new_o, new_k = _up2x(dx, shape, offset, legacy=False)
    old_o, old_k = _up2x(dx, shape, offset, legacy=True)
    n_out, n_keys = N * Cc * 4 * h * w, N * 4 * h * w
    # the legacy kernel wrote every element and nothing else
    sent_o, sent_k = np.float32(12345.0).view(np.uint32), np.uint32(np.int32(-7777).view(np.uint32))
    assert (old_o[:offset] == sent_o).all() and (old_o[offset + n_out:] == sent_o).all()
    assert (old_k[:offset] == sent_k).all() and (old_k[offset + n_keys:] == sent_k).all()
    assert not (old_k[offset:offset + n_keys] >> 31).any()
    # whole buffers, guards and the floats in front of the view included
    np.testing.assert_array_equal(new_o, old_o, err_msg='logits')
    np.testing.assert_array_equal(new_k, old_k, err_msg='keys')
