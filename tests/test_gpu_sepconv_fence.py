"""The separable-conv fence: the three fused "depthwise waves + MFMA waves" kernels (csrc/sepconv.hip, sepconv_precise.hip,
sepconv_x3.hip, sharing csrc/sepconv_common.h) pinned through their C entries to the bits they produced when
tests/sepconv_fence.json was recorded.  No tolerance: sha256 of the packed weights and of every output buffer (the padding
columns of a feature map's rows included, so a store outside the channel slice shows).

Every reachable combination of family (sepconv5 / sepconvp / sepconv_x3), depthwise 3x3 / 5x5, Cout 128 / 256, feature map /
head with 1 or 2 planes (5x5 only), hi + lo pointwise weights on / off (sepconvp, Cout 128), activation 0 / 1 / 2, at the
smallest channel count a family takes and the next chunk count up (128 and 192 fp16 channels, 64 and 96 fp32 channels), on
  N=2, H=93, W=170: 264 tiles of 8 x 16 -- more than the 256 workgroups of the persistent grid, so some workgroups take a
                    second tile and the halo ring wraps across tiles; ragged bottom rows and right columns;
  N=1, H=5,  W=7:   one partial tile, every other workgroup idle (there also once per group without a bias).
The input is a channel slice of a wider buffer (in_ld = C_max + 8).

A change that shares, moves or renames code of these kernels must leave every entry equal.
``python tests/test_gpu_sepconv_fence.py --record`` rewrites the file; it is re-recorded ONLY by a change that means to alter
the numerics (another summation order, another rounding), from two recordings in two fresh processes that agree, and its
header names the commit and the compiler it was recorded with."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FENCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sepconv_fence.json')

SHAPES = {'n2h93w170': (2, 93, 170), 'n1h5w7': (1, 5, 7)}
CHANNELS = {'sepconv5': (128, 192), 'sepconvp': (128, 192), 'x3': (64, 96)}
# mode -> (depthwise size, head planes)
MODES = {'k3': (3, 0), 'k5': (5, 0), 'k5head1': (5, 1), 'k5head2': (5, 2)}
GROUPS = [(fam, mode, ws) for fam, wss in (('sepconv5', (0,)), ('sepconvp', (0, 1)), ('x3', (0,))) for ws in wss for mode in MODES]
PAD = 8      # spare channels behind the input slice and behind every output row

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


def _input(fam, shape):
    """(N,H,W,C_max + PAD) map of the family's element type, shared by both channel counts and every case of the shape"""
    import torch
    from gpu_common import dev
    N, H, W = SHAPES[shape]
    ld = CHANNELS[fam][1] + PAD
    dt = torch.float32 if fam == 'x3' else torch.float16
    return _cached(('x', dt, shape), lambda: torch.from_numpy(_randn(11, (N, H, W, ld))).to(dt).to(dev()))


def _weights(fam, ks, C, Cout, ws):
    """device operands of one block: (dw, pw, bias, head_w, head_b, hashes of the packed buffers)"""
    import torch
    from gpu_common import dev
    from empanada_napari_amd import _abi

    def make():
        lib, st = _abi.load(), _abi.stream_ptr(dev())
        seed = 1000 * ks + C + Cout
        dw = torch.from_numpy(_randn(seed, (ks * ks, C)) / ks).to(dev())                     # (k*k, C)
        pw = torch.from_numpy(_randn(seed + 1, (Cout, C)) / np.float32(np.sqrt(C))).to(dev())
        bias = torch.from_numpy(_randn(seed + 2, (Cout,)) * np.float32(0.1)).to(dev())
        hw = torch.from_numpy(_randn(seed + 3, (2, Cout)) / np.float32(np.sqrt(Cout))).to(dev())
        hb = torch.from_numpy(_randn(seed + 4, (2,))).to(dev())
        packs = {}
        if fam == 'sepconv5':      # fp16 taps as they are, fp16 pointwise weights in fragment order
            dwp = dw.to(torch.float16)
            pw16 = pw.to(torch.float16).contiguous()
            pwp = torch.zeros_like(pw16)
            _abi.check(lib.emp_sepconv5x5_pack_pw(_abi.ptr(pw16), C, C, Cout, _abi.ptr(pwp), st), 'sepconv5 pack')
        elif fam == 'sepconvp':
            dwp = torch.zeros_like(dw)
            _abi.check(lib.emp_sepconvp_pack_dw(_abi.ptr(dw), ks, C, _abi.ptr(dwp), st), 'sepconvp pack_dw')
            pwp = torch.zeros(((2 if ws else 1) * Cout, C), dtype=torch.float16, device=dev())
            pack = lib.emp_sepconvp_ws_pack_pw if ws else lib.emp_sepconvp_pack_pw
            _abi.check(pack(_abi.ptr(pw), C, C, Cout, _abi.ptr(pwp), st), 'sepconvp pack_pw')
            packs['dw'] = _sha(dwp)
        else:
            dwp = torch.zeros_like(dw)
            pwp = torch.zeros((2 * C * Cout,), dtype=torch.float16, device=dev())
            _abi.check(lib.emp_sepconv_x3_pack(_abi.ptr(dw), _abi.ptr(pw), ks, C, Cout, _abi.ptr(dwp), _abi.ptr(pwp), st), 'x3 pack')
            packs['dw'] = _sha(dwp)
        torch.cuda.synchronize()
        packs['pw'] = _sha(pwp)
        return dwp, pwp, bias, hw, hb, packs

    return _cached(('w', fam, ks, C, Cout, ws), make)


def _run(fam, ks, hc, ws, shape, C, Cout, act, with_bias=True):
    """one launch through the family's C entry -> sha256 of the whole output buffer"""
    import torch
    from gpu_common import dev
    from empanada_napari_amd import _abi
    lib, st, p = _abi.load(), _abi.stream_ptr(dev()), _abi.ptr
    N, H, W = SHAPES[shape]
    x = _input(fam, shape)
    in_ld = x.shape[-1]
    dwp, pwp, bias, hw, hb, _ = _weights(fam, ks, C, Cout, ws)
    b = bias if with_bias else None
    odt = torch.float32 if fam == 'x3' else torch.float16
    out_ld = Cout + PAD
    out = None if hc else torch.full((N, H, W, out_ld), 7.0, dtype=odt, device=dev())
    hout = torch.full((N, hc, H * W), 7.0, dtype=torch.float32, device=dev()) if hc else None
    hwd, hbd = (hw[:hc].contiguous(), hb[:hc].contiguous()) if hc else (None, None)
    o_ld = 0 if hc else out_ld
    if fam == 'sepconv5' and ks == 3:
        rc = lib.emp_sepconv3x3_nhwc_f16(p(x), N, H, W, C, in_ld, p(dwp), p(pwp), p(b), Cout, act, p(out), o_ld, st)
    elif fam == 'sepconv5':
        rc = lib.emp_sepconv5x5_nhwc_f16(p(x), N, H, W, C, in_ld, p(dwp), p(pwp), p(b), Cout, act, p(out), o_ld, p(hwd), p(hbd), hc,
                                         p(hout), st)
    elif fam == 'sepconvp':
        entry = lib.emp_sepconvp_ws_nhwc_f16 if ws else lib.emp_sepconvp_nhwc_f16
        rc = entry(p(x), N, H, W, C, in_ld, ks, p(dwp), p(pwp), p(b), Cout, act, p(out), o_ld, p(hwd), p(hbd), hc, p(hout), st)
    else:
        rc = lib.emp_sepconv_x3_nhwc_f32(p(x), N, H, W, C, in_ld, p(dwp), p(pwp), p(b), Cout, act, p(out), o_ld, p(hwd), p(hbd), hc,
                                         p(hout), ks, st)
    _abi.check(rc, f'{fam} k{ks} head{hc} ws{ws}')
    torch.cuda.synchronize()
    return _sha(hout if hc else out)


def group_cases(fam, mode, ws, shape):
    """the entries of one (family, mode, weight-split, shape) group: (name in the fence file, what computes its hash)"""
    ks, hc = MODES[mode]
    name = fam + ('-ws' if ws else '')
    for Cout in ((128,) if ws else (128, 256)):
        for C in CHANNELS[fam]:
            for k in (('pw',) if fam == 'sepconv5' else ('dw', 'pw')):      # (shared by the groups of the same depthwise size)
                yield f'{name}-k{ks}-c{C}-o{Cout}-pack-{k}', lambda C=C, Cout=Cout, k=k: _weights(fam, ks, C, Cout, ws)[5][k]
            for act in (0, 1, 2):
                yield f'{name}-{mode}-{shape}-c{C}-o{Cout}-act{act}', lambda C=C, Cout=Cout, act=act: _run(fam, ks, hc, ws, shape, C, Cout, act)
    if shape == 'n1h5w7':
        C = CHANNELS[fam][0]
        yield f'{name}-{mode}-{shape}-c{C}-o128-act1-nobias', lambda: _run(fam, ks, hc, ws, shape, C, 128, 1, with_bias=False)


def run_group(fam, mode, ws, shape):
    return {name: compute() for name, compute in group_cases(fam, mode, ws, shape)}


def _fence():
    with open(FENCE) as f:
        return json.load(f)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('fam,mode,ws', GROUPS, ids=[f'{f}{"-ws" if w else ""}-{m}' for f, m, w in GROUPS])
def test_sepconv_equals_the_recorded_fence(fam, mode, ws, shape):
    want = _fence()['cases']
    got = run_group(fam, mode, ws, shape)
    missing = [k for k in got if k not in want]
    assert not missing, f'not in the fence file: {missing[:5]} of {len(missing)}'
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, f'{len(diff)} of {len(got)} differ from the fence, first {diff[:5]}'


def test_no_entry_of_the_fence_file_goes_unchecked():
    names = {name for fam, mode, ws in GROUPS for shape in SHAPES for name, _ in group_cases(fam, mode, ws, shape)}
    assert names == set(_fence()['cases']), sorted(names ^ set(_fence()['cases']))[:5]


def _record(out_path, parent):
    import subprocess
    import conftest  # noqa: F401  (imports the package the way the suite does)
    hipcc = [line for line in subprocess.run(['hipcc', '--version'], capture_output=True, text=True).stdout.splitlines()
             if 'HIP version' in line or 'clang version' in line]
    doc = {'parent_commit': parent, 'hipcc_version': ' | '.join(hipcc), 'cases': {}}
    for fam, mode, ws in GROUPS:
        for shape in SHAPES:
            doc['cases'].update(run_group(fam, mode, ws, shape))
        print('recorded', fam, mode, ws, len(doc['cases']), flush=True)
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
