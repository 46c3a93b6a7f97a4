"""The convolution fence: the MFMA convolution kernels that stage both operands by LDS-DMA (csrc/conv_igemm.hip,
conv_igemm256.hip, conv_igemm_s64.hip, conv3x3c64.hip, conv16x3p.hip, sharing csrc/igemm_common.h) pinned through their C
entries to the bits they produced when tests/conv_fence.json was recorded.  No tolerance: sha256 of every packed weight image
and of every output buffer, the spare columns behind each row included, so a store outside the channel slice shows.  These
kernels have no atomics and the split-K path adds its partial sums in a fixed order.

Two geometries: N=3, H=9, W=11 (297 pixels: two 256-pixel tiles, the second ragged) and N=1, H=5, W=7 (one partial tile).
  fp16 (emp_conv2d_nhwc_f16), tile forced by `variant`: the 128 x 128 / 128 x 64 / 64 x 64 tiles with register staging, LDS-DMA
      and LDS-DMA + transposed epilogue, the half tile, the deep-ring 64 x 64 tile, the register-weight 3x3 tile; on the
      256 x 256 tile 2 K-tiles (no pipeline), 4 (the shortest ring: the 64-byte-row kernel), 8 (the shortest the whole-line
      kernel takes), a dilated 3x3 of 512 channels (16 slabs > 8: a group-major walk, taps in the padding), a stride-2 3x3 and a
      stride-2 1x1 (taps walked on the 4-K-tile ring), each with Cout 256 / 512, plain / packed weights, residual, per-image bias and relu on / off;
  emp_conv1x1_dual_nhwc_f16: automatic tile and the 256 x 256 tile, plain / packed, a stride-2 second source of odd size;
  fp16x3 over hl32 maps (emp_conv2d_hl32_f16x3): 4 K steps (the minimum) and a dilated 3x3, act 0 / 1 / 2, fp32 / hl32 output,
      no / fp32 / hl32 residual, per-image bias, Cout 512 with a second destination; its split-K form with S = 2, 4, 8
      (splits that start inside a tap among them); emp_x3p_pack_weights, emp_hl32_from_f32, emp_hl32_to_f32.
The back-to-back instantiation of the 256 x 256 kernel is reachable through the network only (tests/test_gpu_forward_fence.py
case fp16-pdl-b1-1024); the EMP_CONV256_MODE instantiations are read from the environment once per process.

A change that shares, moves or renames code of these kernels must leave every entry equal.
``python tests/test_gpu_conv_fence.py --record`` rewrites the file; it is re-recorded ONLY by a change that means to alter the
numerics (another summation order, another rounding), from two recordings in two fresh processes that agree, and its header
names the commit and the compiler it was recorded with."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FENCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_fence.json')

SHAPES = {'n3h9w11': (3, 9, 11), 'n1h5w7': (1, 5, 7)}
PAD = 8           # spare channels behind every output row
PAD_HL32 = 32     # (an hl32 row is made of whole 32-channel blocks)
CMAX = 512        # channels of the shared fp16 input / residual buffers
CMAX32 = 2048     # channels of the shared fp32 / hl32 input map
PACKED = 1 << 20
T256 = 4 << 4

# (name, Cin, k, stride, pad, dil)
CASES256 = [('c64k1', 64, 1, 1, 0, 1), ('c128k1', 128, 1, 1, 0, 1), ('c256k1', 256, 1, 1, 0, 1), ('c512k3d2', 512, 3, 1, 2, 2),
            ('c128k3s2', 128, 3, 2, 1, 1), ('c128k1s2', 128, 1, 2, 0, 1)]      # (a strided 1x1 walks taps on the 4-K-tile ring)
# the other tiles: (name, Cin, Cout, k, stride, pad, dil, act, res, bias, bias_n)
CASES_TILE = [('c64k1-o128', 64, 128, 1, 1, 0, 1, 1, False, True, False),
              ('c128k3s2-o128', 128, 128, 3, 2, 1, 1, 0, True, True, True),
              ('c512k3d2-o256', 512, 256, 3, 1, 2, 2, 1, False, True, False),       # a group-major walk on every tile
              ('c64k1-o72', 64, 72, 1, 1, 0, 1, 2, True, False, False),             # a ragged cout tile (not the half tile's)
              ('c64k3-o64', 64, 64, 3, 1, 1, 1, 1, False, True, False)]
VARIANTS_TILE = {f't{t}s{s}': 16 * t + s for t in (1, 2, 3) for s in (1, 2, 3)}
VARIANTS_TILE.update({'t5': 5 << 4, 't7': 7 << 4})
# (name, Cin, Cin2, stride2); the stride-2 case runs on a geometry of its own
CASES_DUAL = [('c64+64s1', 64, 64, 1), ('c128+256s2', 128, 256, 2)]
DUAL_S2_GEOM = (2, 12, 20, 23, 39)      # N, H, W, H2, W2: a source of odd size under 480 pixels (two tiles, the second ragged)
# (name, Cin, k, pad, dil)
CASES_X3P = [('c128k1', 128, 1, 0, 1), ('c64k3d2', 64, 3, 2, 2)]
# split-K: (name, Cin, k, pad, dil, the S the rule gives on one pixel tile)
CASES_KSPLIT = [('c2048k1', 2048, 1, 0, 1, 8), ('c1024k1', 1024, 1, 0, 1, 4), ('c512k1', 512, 1, 0, 1, 2), ('c256k3d2', 256, 3, 2, 2, 8),
                ('c64k3', 64, 3, 1, 1, 2)]

GROUPS = ([('tile', v, None) for v in VARIANTS_TILE] + [('c64', None, None)] + [('t256', c[0], None) for c in CASES256] +
          [('dual', c[0], None) for c in CASES_DUAL] + [('x3p', c[0], None) for c in CASES_X3P] +
          [('ksplit', c[0], None) for c in CASES_KSPLIT] + [('hl32', None, None)])

_CACHE = {}


def _randn(seed, shape):
    """seeded normals from numpy's frozen legacy stream (the same on every machine and numpy version)"""
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _dev(seed, shape, dtype, scale=1.0):
    import torch
    from gpu_common import dev
    return _cached(('t', seed, shape, dtype, scale), lambda: torch.from_numpy(_randn(seed, shape) * np.float32(scale)).to(dtype).to(dev()))


def _out_dims(H, W, k, stride, pad, dil):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _api():
    from gpu_common import dev
    from empanada_napari_amd import _abi
    return _abi.load(), _abi, _abi.stream_ptr(dev())


# ---------------------------------------------------------------------------------------------------------------- fp16
def _w16(Cin, Cout, k, Cin2=0):
    """(Cout, k*k*Cin + Cin2) fp16 weights"""
    import torch
    K = k * k * Cin + Cin2
    return _dev(7000 + 10 * Cin + Cout + k + Cin2, (Cout, K), torch.float16, 1.0 / np.sqrt(K))


def _w16_packed(Cin, Cout, k, Cin2=0):
    """the 256 x 256 tile's packed image of _w16 and its hash"""
    import torch

    def make():
        lib, _abi, st = _api()
        w = _w16(Cin, Cout, k, Cin2)
        wp = torch.zeros_like(w)
        _abi.check(lib.emp_conv256_pack_weights(_abi.ptr(w), _abi.ptr(wp), Cout, k * k, Cin, Cin2, st), 'pack256')
        torch.cuda.synchronize()
        return wp, _sha(wp)

    return _cached(('wp', Cin, Cout, k, Cin2), make)


def _conv16(shape, Cin, Cout, k, stride, pad, dil, act, res, bias, bias_n, variant):
    """one launch of emp_conv2d_nhwc_f16 on a channel slice of the shape's shared input -> sha256 of the whole output buffer"""
    import torch
    from gpu_common import dev
    lib, _abi, st = _api()
    p = _abi.ptr
    N, H, W = SHAPES[shape]
    Ho, Wo = _out_dims(H, W, k, stride, pad, dil)
    x = _dev(11, (N, H, W, CMAX + PAD), torch.float16)
    w = _w16_packed(Cin, Cout, k)[0] if variant & PACKED else _w16(Cin, Cout, k)
    b = _dev(13, (CMAX,), torch.float32, 0.1)[:Cout] if bias else None
    bn = _dev(14, (N, Cout), torch.float32, 0.1) if bias_n else None
    r = _dev(15, (N * H * W, CMAX + PAD), torch.float16) if res else None
    out = torch.full((N * Ho * Wo, Cout + PAD), 7.0, dtype=torch.float16, device=dev())
    _abi.check(lib.emp_conv2d_nhwc_f16(p(x), N, H, W, Cin, CMAX + PAD, p(w), p(b), p(bn), p(r), CMAX + PAD if res else 0, p(out), Cout + PAD,
                                       Cout, k, k, stride, pad, dil, act, variant, st), f'conv2d variant {variant}')
    torch.cuda.synchronize()
    return _sha(out)


def _cases_tile(vname, shape):
    variant = VARIANTS_TILE[vname]
    for name, Cin, Cout, k, stride, pad, dil, act, res, bias, bias_n in CASES_TILE:
        if variant == 5 << 4 and Cout % 128:
            continue
        yield (f'{vname}-{shape}-{name}',
               lambda a=(Cin, Cout, k, stride, pad, dil, act, res, bias, bias_n): _conv16(shape, *a, variant))


def _cases_c64(shape):
    """the register-weight 3x3 tile (variant tile 6) and the deep-ring 64 x 64 tile on its shapes"""
    for C in (64, 128):
        for act in (0, 1, 2):
            for vname, variant in (('t6', 6 << 4), ('t7', 7 << 4)):
                yield (f'{vname}-{shape}-c{C}k3-o{C}-act{act}',
                       lambda C=C, act=act, variant=variant: _conv16(shape, C, C, 3, 1, 1, 1, act, False, True, False, variant))


def _cases_t256(cname, shape):
    _, Cin, k, stride, pad, dil = next(c for c in CASES256 if c[0] == cname)
    for Cout in (256, 512):
        yield f't4-{cname}-o{Cout}-pack', lambda Cout=Cout: _w16_packed(Cin, Cout, k)[1]
        for packed in (0, 1):
            for res in (0, 1):
                for bias_n in (0, 1):
                    for relu in (0, 1):
                        yield (f't4{"p" if packed else ""}-{shape}-{cname}-o{Cout}-res{res}-bn{bias_n}-relu{relu}',
                               lambda a=(Cin, Cout, k, stride, pad, dil, relu, bool(res), True, bool(bias_n)), v=T256 | (PACKED if packed else 0):
                               _conv16(shape, *a, v))


def _dual(geom, Cin, Cin2, s2, Cout, relu, variant):
    import torch
    from gpu_common import dev
    lib, _abi, st = _api()
    p = _abi.ptr
    N, H, W, H2, W2 = geom
    x = _dev(21, (N, H, W, CMAX + PAD), torch.float16)
    x2 = _dev(22, (N, H2, W2, Cin2 + PAD), torch.float16)
    w = _w16_packed(Cin, Cout, 1, Cin2)[0] if variant & PACKED else _w16(Cin, Cout, 1, Cin2)
    b = _dev(13, (CMAX,), torch.float32, 0.1)[:Cout]
    out = torch.full((N * H * W, Cout + PAD), 7.0, dtype=torch.float16, device=dev())
    _abi.check(lib.emp_conv1x1_dual_nhwc_f16(p(x), N, H, W, Cin, CMAX + PAD, p(x2), H2, W2, Cin2, Cin2 + PAD, s2, p(w), p(b), p(out),
                                             Cout + PAD, Cout, relu, variant, st), f'dual variant {variant}')
    torch.cuda.synchronize()
    return _sha(out)


def _cases_dual(cname, shape):
    _, Cin, Cin2, s2 = next(c for c in CASES_DUAL if c[0] == cname)
    if s2 == 2:      # one geometry of its own: a 23 x 39 source sampled at stride 2 under a 12 x 20 output
        if shape != 'n3h9w11':
            return
        geom, gname = DUAL_S2_GEOM, 'n2h12w20'
    else:
        N, H, W = SHAPES[shape]
        geom, gname = (N, H, W, H, W), shape
    for Cout in (256, 512):
        yield f'dual-{cname}-o{Cout}-pack', lambda Cout=Cout: _w16_packed(Cin, Cout, 1, Cin2)[1]
        for vname, variant in (('auto', 0), ('t4', T256), ('t4p', T256 | PACKED)):
            for relu in (0, 1):
                yield (f'dual-{vname}-{gname}-{cname}-o{Cout}-relu{relu}',
                       lambda Cout=Cout, relu=relu, variant=variant: _dual(geom, Cin, Cin2, s2, Cout, relu, variant))


# -------------------------------------------------------------------------------------------------------- fp16x3 / hl32
def _hl32_map(shape):
    """the shape's fp32 map (rows, CMAX32 + 32) as hl32 rows: (tensor of 2 * ld halfs per row, ld)"""
    import torch
    from gpu_common import dev

    def make():
        lib, _abi, st = _api()
        N, H, W = SHAPES[shape]
        ld = CMAX32 + PAD_HL32
        x = _dev(31, (N * H * W, CMAX32), torch.float32)
        h = torch.zeros((N * H * W, 2 * ld), dtype=torch.float16, device=dev())
        _abi.check(lib.emp_hl32_from_f32(_abi.ptr(x), _abi.ptr(h), N * H * W, CMAX32, CMAX32, ld, st), 'hl32_from_f32')
        torch.cuda.synchronize()
        return h, ld

    return _cached(('hl32', shape), make)


def _x3p_image(Cin, Cout, k):
    """packed fp16x3 weight image of seeded (Cout, K) fp32 weights, and its hash"""
    import torch
    from gpu_common import dev

    def make():
        lib, _abi, st = _api()
        K = k * k * Cin
        w = _dev(8000 + Cin + Cout + k, (Cout, K), torch.float32, 1.0 / np.sqrt(K))
        img = torch.zeros((2 * Cout * K,), dtype=torch.float16, device=dev())
        _abi.check(lib.emp_x3p_pack_weights(_abi.ptr(w), _abi.ptr(img), Cout, K, st), 'x3p pack')
        torch.cuda.synchronize()
        return img, _sha(img)

    return _cached(('x3p', Cin, Cout, k), make)


def _x3p(shape, Cin, Cout, k, pad, dil, act, out_fmt, resf, bias_n, ksplit=False, split2=0):
    """one launch of emp_conv2d_hl32_f16x3 (or its split-K form) -> sha256 of the output buffer(s); resf: 0 none, 1 fp32, 2 hl32"""
    import torch
    from gpu_common import dev
    lib, _abi, st = _api()
    p = _abi.ptr
    N, H, W = SHAPES[shape]
    Ho, Wo = _out_dims(H, W, k, 1, pad, dil)
    M = N * Ho * Wo
    x, ld = _hl32_map(shape)
    img = _x3p_image(Cin, Cout, k)[0]
    b = _dev(13, (CMAX,), torch.float32, 0.1)[:Cout]
    bn = _dev(14, (N, Cout), torch.float32, 0.1) if bias_n else None
    r, r_ld = None, 0
    if resf == 1:
        r, r_ld = _dev(33, (N * H * W, CMAX + PAD), torch.float32), CMAX + PAD
    elif resf == 2:      # (any fp16 bits are a valid hl32 row: hi and lo halves are read as they lie)
        r, r_ld = _dev(34, (N * H * W, 2 * (CMAX + PAD_HL32)), torch.float16, 0.5), CMAX + PAD_HL32

    def buf(C):
        if out_fmt:
            return torch.full((M, 2 * (C + PAD_HL32)), 7.0, dtype=torch.float16, device=dev()), C + PAD_HL32
        return torch.full((M, C + PAD), 7.0, dtype=torch.float32, device=dev()), C + PAD

    out, o_ld = buf(split2 if split2 else Cout)
    if not ksplit:
        _abi.check(lib.emp_conv2d_hl32_f16x3(p(x), N, H, W, Cin, ld, p(img), p(b), p(bn), p(r), r_ld, 1 if resf == 2 else 0, p(out), o_ld,
                                             out_fmt, Cout, k, k, 1, pad, dil, act, st), 'conv2d_hl32_f16x3')
        torch.cuda.synchronize()
        return _sha(out)
    out2, o2_ld = buf(Cout - split2) if split2 else (None, 0)
    scratch = _cached('scratch', lambda: torch.zeros((8 << 20,), dtype=torch.float32, device=dev()))      # 32 MiB
    _abi.check(lib.emp_conv2d_hl32_f16x3_ksplit(p(x), N, H, W, Cin, ld, p(img), p(b), p(bn), p(r), r_ld, 1 if resf == 2 else 0, p(out), o_ld,
                                                out_fmt, p(out2), o2_ld, split2, Cout, k, k, 1, pad, dil, act, p(scratch),
                                                scratch.numel() * 4, st), 'conv2d_hl32_f16x3_ksplit')
    torch.cuda.synchronize()
    return _sha(out) + ('+' + _sha(out2) if split2 else '')


def _cases_x3p(cname, shape):
    _, Cin, k, pad, dil = next(c for c in CASES_X3P if c[0] == cname)
    yield f'x3p-{cname}-o256-pack', lambda: _x3p_image(Cin, 256, k)[1]
    yield f'x3p-{cname}-o512-pack', lambda: _x3p_image(Cin, 512, k)[1]
    for act in (0, 1, 2):
        for out_fmt in (0, 1):
            for resf in (0, 1, 2):
                yield (f'x3p-{shape}-{cname}-o256-act{act}-fmt{out_fmt}-res{resf}',
                       lambda a=(act, out_fmt, resf): _x3p(shape, Cin, 256, k, pad, dil, *a, False))
    yield f'x3p-{shape}-{cname}-o256-act1-fmt0-res1-bn', lambda: _x3p(shape, Cin, 256, k, pad, dil, 1, 0, 1, True)
    yield f'x3p-{shape}-{cname}-o256-act0-fmt1-res2-bn', lambda: _x3p(shape, Cin, 256, k, pad, dil, 0, 1, 2, True)
    # Cout 512 with the second destination at cout 256 (the split-K entry carries it; too few K steps here for the rule to split)
    for out_fmt in (0, 1):
        yield (f'x3p-{shape}-{cname}-o512-split256-act1-fmt{out_fmt}',
               lambda out_fmt=out_fmt: _x3p(shape, Cin, 512, k, pad, dil, 1, out_fmt, 0, False, ksplit=True, split2=256))


def _cases_ksplit(cname, shape):
    _, Cin, k, pad, dil, S = next(c for c in CASES_KSPLIT if c[0] == cname)
    yield f'x3p-{cname}-o256-pack', lambda: _x3p_image(Cin, 256, k)[1]
    for act, out_fmt, resf, bias_n in ((0, 0, 0, False), (1, 1, 2, True), (2, 0, 1, False), (1, 1, 0, False)):
        yield (f'ksplit{S}-{shape}-{cname}-o256-act{act}-fmt{out_fmt}-res{resf}{"-bn" if bias_n else ""}',
               lambda a=(act, out_fmt, resf, bias_n): _x3p(shape, Cin, 256, k, pad, dil, *a, ksplit=True))
    if shape == 'n1h5w7':
        yield f'x3p-{cname}-o512-pack', lambda: _x3p_image(Cin, 512, k)[1]
        yield (f'ksplit-{shape}-{cname}-o512-split256-act1-fmt0',
               lambda: _x3p(shape, Cin, 512, k, pad, dil, 1, 0, 0, False, ksplit=True, split2=256))


def _cases_hl32(shape):
    """fp32 rows -> hl32 rows -> fp32 rows, a channel slice of wider rows both ways"""
    import torch
    from gpu_common import dev

    def back():
        lib, _abi, st = _api()
        h, ld = _hl32_map(shape)
        rows = h.shape[0]
        o = torch.full((rows, 96 + PAD), 7.0, dtype=torch.float32, device=dev())
        _abi.check(lib.emp_hl32_to_f32(_abi.ptr(h), _abi.ptr(o), rows, 96, ld, 96 + PAD, st), 'hl32_to_f32')
        torch.cuda.synchronize()
        return _sha(o)

    yield f'hl32-from-f32-{shape}', lambda: _sha(_hl32_map(shape)[0])
    yield f'hl32-to-f32-{shape}', back


def group_cases(kind, name, _unused, shape):
    """the entries of one group: (name in the fence file, what computes its hash)"""
    if kind == 'tile':
        return _cases_tile(name, shape)
    if kind == 'c64':
        return _cases_c64(shape)
    if kind == 't256':
        return _cases_t256(name, shape)
    if kind == 'dual':
        return _cases_dual(name, shape)
    if kind == 'x3p':
        return _cases_x3p(name, shape)
    if kind == 'ksplit':
        return _cases_ksplit(name, shape)
    return _cases_hl32(shape)


def run_group(kind, name, unused, shape):
    return {n: compute() for n, compute in group_cases(kind, name, unused, shape)}


def _fence():
    with open(FENCE) as f:
        return json.load(f)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('kind,name,unused', GROUPS, ids=[k + ('-' + n if n else '') for k, n, _ in GROUPS])
def test_conv_equals_the_recorded_fence(kind, name, unused, shape):
    want = _fence()['cases']
    got = run_group(kind, name, unused, shape)
    missing = [k for k in got if k not in want]
    assert not missing, f'not in the fence file: {missing[:5]} of {len(missing)}'
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, f'{len(diff)} of {len(got)} differ from the fence, first {diff[:5]}'


def test_no_entry_of_the_fence_file_goes_unchecked():
    names = {n for kind, name, u in GROUPS for shape in SHAPES for n, _ in group_cases(kind, name, u, shape)}
    assert names == set(_fence()['cases']), sorted(names ^ set(_fence()['cases']))[:5]


def _record(out_path, parent):
    import subprocess
    import conftest  # noqa: F401  (imports the package the way the suite does)
    hipcc = [line for line in subprocess.run(['hipcc', '--version'], capture_output=True, text=True).stdout.splitlines()
             if 'HIP version' in line or 'clang version' in line]
    doc = {'parent_commit': parent, 'hipcc_version': ' | '.join(hipcc), 'cases': {}}
    for kind, name, u in GROUPS:
        for shape in SHAPES:
            doc['cases'].update(run_group(kind, name, u, shape))
        print('recorded', kind, name, len(doc['cases']), flush=True)
    with open(out_path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', action='store_true')
    ap.add_argument('--out', default=FENCE)
    ap.add_argument('--parent', default='unknown', help='hash of the commit whose sources the library was built from')
    a = ap.parse_args()
    if not a.record:
        sys.exit('run under pytest, or with --record')
    _record(a.out, a.parent)
