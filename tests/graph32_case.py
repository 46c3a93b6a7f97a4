"""The fp32 / fp16x3 forward (csrc/pdl_net32.hip run32) map by map: bounds, a CPU stand-in of the engine and planted defects
(tests/test_graph32_case_host.py, tests/test_gpu_graph32_layers.py).  No GPU.

oracle.pdl_model.Graph32Walk recomputes every buffer of a forward from the engine's own input buffers in float64 and describes
the launch that made it; ``bound`` turns that description into the per-element bound of the kernel, none of them taken from a
kernel's output:

* 'conv' / 'sep' (c32, the fused separable block): fp16x3 -> x3_range_case.reference(case, operands) as it stands; fp32 mode ->
  layers_case.conv32_ref_bound.  Accepted: |got - ref| <= min(worst, f rss), f = x3_range_case.RSS_HOST (3) for the CPU stand-in
  and RSS_GPU (6) on the device -- the factors of the operand-range tests, not refitted.  An hl32 output adds u(result)
  (reference's out_fmt).  'tiles': the fused head's partial sums, one such launch per cout tile.
* glue kernels: layers_case's bounds (stems, bilinear, average pool, gemv, fp32 depthwise, head_finish) and pointrend_case's
  (2x up-sampling, point sampling, the predictor = head1x1).  Max-pool, copies, the hl32 copy of p5 and every zero pad: exact.
* what the end of a forward no longer holds is forced through its producer: 'conv_prop' / 'conv_gated' (RegNetY's in-place
  gate), 'chain' (PointRend's sampled rows, overwritten by the fc layers): each launch's own bound at the expected input
  plus the input's bound through |w|.
* 'selection': integer -- distinct cells inside the plane, every selected key <= every unselected key (ties at the boundary
  either way), and every unselected cell's key bit-equal to the key recomputed from the logits stored there.

StandIn runs the same walk in float32 (torch CPU kernels: another summation order than the engine's, the same formats) and
stores what it yields under the engine's names -- the oracle's fp32 forward in the engine's buffers.  DEFECTS plants one wrong
site at a time in it."""
import numpy as np
import torch
import torch.nn.functional as F

import layers_case as LC
import pointrend_case as PC
import x3_range_case as X3
from oracle import pdl_model

ALLOW = ('pr.keys', 'pr.topk', 'pr.idx')      # work buffers of the selection: checked through 'selection', not element by element
OUTPUTS = ('sem_logits', 'ctr_hmp', 'offsets')


def _rows(t):
    """(N,C,H,W) -> (N*H*W, C) float64 numpy"""
    t = torch.as_tensor(t)
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()


def _nchw(rows, N, H, W):
    return np.ascontiguousarray(rows.reshape(N, H, W, -1).transpose(0, 3, 1, 2))


def _conv_bound(d):
    c, p = d['case'], d['p']
    r = X3.reference(c, p) if d['family'] == 'x3' else LC.conv32_ref_bound(c, p)
    Ho, Wo = X3.out_hw(c)
    out = {k: _nchw(v, c['N'], Ho, Wo) for k, v in r.items()}
    if d.get('ps_cout'):      # cout block q = dy * 2 + dx of pixel (y, x) -> pixel (2y + dy, 2x + dx)
        co = d['ps_cout']
        out = {k: v.reshape(c['N'], 2, 2, co, Ho, Wo).transpose(0, 3, 4, 1, 5, 2).reshape(c['N'], co, 2 * Ho, 2 * Wo) for k, v in out.items()}
    if 'rows' in d:      # PointRend's rows as a (1, 1, rows, C) map
        out = {k: np.ascontiguousarray(v[0, :, 0, :].T) for k, v in out.items()}
    return out


def _chain(stages):
    """PointRend's sampled rows through fc layers: each launch's bound at the expected rows + the bound so far (and the fp32
    rounding of the expected rows) through |w|; the coarse and pad columns keep the sample's -> (rows, bound), (R, ld)"""
    s0 = stages[0]
    x = PC.point_rows_ref(s0['feat'], s0['C'], s0['coarse'], s0['idx'], s0['H2'], s0['W2'], s0['ld'])
    e = PC.sample_bound(x, s0['feat'], s0['C'], s0['coarse'], False)
    for st in stages[1:]:
        b, w = _conv_bound(st), np.abs(np.asarray(st['w'], np.float64))
        Cf = b['ref'].shape[1]
        e = np.concatenate([b['worst'] + (e + LC.U * np.abs(x)) @ w.T, e[:, Cf:]], 1)
        x = np.concatenate([b['ref'], x[:, Cf:]], 1)
    return x, e


def bound(d, value):
    """description -> dict(ref, worst, rss) in the layout of the walk's value; rss is None where the bound has one form only"""
    k = d['kind']
    if k in ('conv', 'sep'):
        return _conv_bound(d)
    if k == 'tiles':
        bs = [_conv_bound(t) for t in d['tiles']]
        return {key: np.stack([_rows(b[key]).reshape(b[key].shape[0], -1, b[key].shape[1]) for b in bs]) for key in ('ref', 'worst', 'rss')}
    if k == 'chain':
        x, e = _chain(d['stages'])
        c0, c1 = d['channels']
        return dict(ref=x[:, c0:c1], worst=e[:, c0:c1], rss=None)
    if k == 'conv_prop':      # a launch whose input map is gone: its own bound at the expected input + that input's bound through |w|
        b, bu = _conv_bound(d['inner']), _conv_bound(d['upstream'])
        w = np.asarray(d['w'], np.float64)
        eu = bu['worst'] + LC.U * np.abs(bu['ref'])
        return dict(ref=b['ref'], worst=b['worst'] + np.einsum('oc,nchw->nohw', np.abs(w), eu),
                    rss=b['rss'] + np.sqrt(np.einsum('oc,nchw->nohw', w * w, (bu['rss'] + LC.U * np.abs(bu['ref'])) ** 2)))
    if k == 'conv_gated':      # the launch's output times the engine's own gate (gate_mul: layers_case's 12 U |ref| + 2^-126)
        bu = _conv_bound(d['inner'])
        sig = 1.0 / (1.0 + np.exp(-np.asarray(d['gate'], np.float64)))
        ref = bu['ref'] * sig
        eg = 12 * LC.U * np.abs(ref) + LC.TINY32
        return dict(ref=ref, worst=bu['worst'] * sig * (1 + 12 * LC.U) + eg, rss=bu['rss'] * sig * (1 + 12 * LC.U) + eg)
    v = value.double().numpy()
    if k in ('exact', 'zero'):
        return dict(ref=v, worst=np.zeros_like(v), rss=None)
    if k in ('stem', 'stem_pool'):
        im = d['image']
        ref, S, T = LC.stem_ref(im['x'].double().numpy(), LC.IMG_F32, d['H'], d['W'], d['taps'], d['b'], d['k'])
        if k == 'stem':
            e = LC.stem_conv_bound(ref, S, T, d['k'], LC.F32, False)
        else:
            ref, e = LC.stem_pool_ref_bound(ref, S, T, LC.F32)
        return dict(ref=ref.transpose(0, 3, 1, 2), worst=e.transpose(0, 3, 1, 2), rss=None)
    if k == 'bilinear':
        ref = LC.bilinear_ref(d['x'], d['H'], d['W'])
        e = LC.bilinear_e32(d['x'], d['H'], d['W'])[None] + 0 * ref
        return dict(ref=ref.transpose(0, 3, 1, 2), worst=e.transpose(0, 3, 1, 2), rss=None)
    if k == 'avgpool':
        ref, e = LC.avgpool_ref_bound(d['x'], LC.HL32 if d['hl32'] else LC.F32)
        return dict(ref=ref, worst=e, rss=None)
    if k == 'gemv':
        ref, e = LC.gemv_ref_bound(d['x'], d['w'], d['b'], d['relu'])
        return dict(ref=ref, worst=e, rss=None)
    if k == 'dw':
        ref, e = LC.dw_ref_bound(d['x'], d['taps'], d['k'])
        return dict(ref=ref.transpose(0, 3, 1, 2), worst=e.transpose(0, 3, 1, 2), rss=None)
    if k == 'fuse':
        ref, A = LC.fuse_ref(d['a'], d['b'], d['c'], d['coef'], d['mode'])
        return dict(ref=ref.transpose(0, 3, 1, 2), worst=LC.fuse_e32(A).transpose(0, 3, 1, 2), rss=None)
    if k == 'head_finish':
        ref, e = LC.head_finish_ref_bound(d['part'], d['b'])
        N, C, H, W = v.shape
        return dict(ref=_nchw(ref, N, H, W), worst=_nchw(e, N, H, W), rss=None)
    if k == 'head1x1':
        ref, e = PC.predictor_ref(d['rows'], d['w'], d['b'])
        N, C, H, W = v.shape
        return dict(ref=_nchw(ref, N, H, W), worst=_nchw(e, N, H, W), rss=None)
    if k == 'sample':
        rows = PC.point_rows_ref(d['feat'], d['C'], d['coarse'], d['idx'], d['H2'], d['W2'], d['ld'])
        e = PC.sample_bound(rows, d['feat'], d['C'], d['coarse'], False)
        c0, c1 = d['channels']
        return dict(ref=rows[:, c0:c1], worst=e[:, c0:c1], rss=None)
    if k in ('upsample_but', 'refined'):
        ref = PC.upsample_ref(d['x'])
        e = np.full_like(ref, PC.upsample_bound(d['x']))
        if k == 'refined':
            lg, le = PC.predictor_ref(d['rows'], d['w'], d['b'])
            N, ncls = ref.shape[:2]
            idx = np.asarray(d['idx'])
            rf, ef = ref.reshape(N, ncls, -1), e.reshape(N, ncls, -1)
            for n in range(N):
                rf[n][:, idx[n]] = lg.reshape(N, idx.shape[1], ncls)[n].T
                ef[n][:, idx[n]] = le.reshape(N, idx.shape[1], ncls)[n].T
        return dict(ref=ref, worst=e, rss=None)
    raise KeyError(k)


def family(name, d):
    """the map family a ratio is reported under"""
    for key, fam in (('encoder.', 'encoder'), ('.aspp', 'aspp'), ('pooled', 'aspp'), ('.poolfeat', 'aspp'), ('.bias_n', 'aspp'), ('p5.hl32', 'aspp'),
                     ('.stage', 'decoder'), ('_fpn.', 'bifpn'), ('_decoder.', 'decoder'), ('p2f', 'bifpn'), ('pr.', 'pointrend'), ('sem_logits', 'pointrend')):
        if key in name:
            return fam
    return 'stem' if name in ('p1', 'stem') else 'heads'


def selection_faults(d, idx, target):
    """the 'selection' description against the engine's indices (N, k) and the refined logits (N, ncls, H2, W2) -> list of faults"""
    keys, k, plane = np.asarray(d['keys']), d['k'], d['plane']
    idx = np.asarray(idx)
    out = []
    for n in range(idx.shape[0]):
        sel = idx[n]
        if sel.min() < 0 or sel.max() >= plane or len(np.unique(sel)) != k:
            out.append(f'image {n}: the selected cells are not {k} distinct cells of the plane')
            continue
        mask = np.zeros(plane, bool)
        mask[sel] = True
        if k < plane and keys[n][mask].max() > keys[n][~mask].min():
            out.append(f'image {n}: a selected key {keys[n][mask].max():#x} is above an unselected one {keys[n][~mask].min():#x}')
        want = PC.keys_ref(np.asarray(target, np.float32)[n:n + 1])[0].view(np.uint32).astype(np.int64)
        bad = int((want[~mask] != keys[n][~mask]).sum())
        if bad:
            out.append(f'image {n}: {bad} unselected keys are not the keys of the logits stored there')
    return out


def check(name, d, value, got, factor):
    """-> dict(name, family, viol, worst (largest |err| / worst), rss (largest |err| / rss, None without one), n)"""
    b = bound(d, value)
    got = np.asarray(torch.as_tensor(got).double().numpy())
    ref = b['ref']
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    vref = value.double().numpy()
    if d['kind'] not in ('refined',):      # the oracle's expectation and the bound module's reference are two float64 evaluations
        assert np.abs(vref - ref).max() <= 1e-9 * max(1.0, float(np.abs(ref).max())), (name, float(np.abs(vref - ref).max()))
    accept = b['worst'] if b['rss'] is None else np.minimum(b['worst'], factor * b['rss'])
    err = np.abs(got - ref)
    bad = ~(err <= accept)
    if d['kind'] == 'upsample_but':      # an inner step: at most k cells per image are refined, the others are the plain up-sampling
        # ... and a refined cell holds the point head's logits of that cell; where k is the whole plane every cell must
        N, ncls = got.shape[:2]
        plain = ~bad.reshape(N, ncls, -1).any(1)
        x, e = _chain(d['stages'])
        lg, le = PC.predictor_ref(x, d['w'], d['b'])
        le = le + (e + LC.U * np.abs(x)) @ np.abs(np.asarray(d['w'], np.float64)).T
        g = got.reshape(N, ncls, -1).transpose(0, 2, 1).reshape(-1, ncls)
        rh = (np.abs(g - lg) / le).max(1).reshape(N, -1)      # per cell, against the point head
        ru = (err / np.maximum(b['worst'], 1e-300)).reshape(N, ncls, -1).max(1)      # per cell, against the plain up-sampling
        head = rh <= 1.0
        ok = head if d['k'] >= d['plane'] else (plain | head)
        viol = int((~ok).sum()) + int(((~plain).sum(1) > d['k']).sum())
        rw = float(rh.max()) if d['k'] >= d['plane'] else float(np.minimum(rh, ru).max())
        return dict(name=name, family=family(name, d), viol=viol, worst=rw, rss=None, n=int(got.size), kind=d['kind'])
    tiny = 1e-300
    if b['worst'].max() > 0:
        rw = float((err / np.maximum(b['worst'], tiny)).max())
    else:      # an exact operator
        rw = float('inf') if err.max() > 0 else 0.0
    rr = None if b['rss'] is None else float((err / np.maximum(b['rss'], tiny)).max())
    return dict(name=name, family=family(name, d), viol=int(bad.sum()), worst=rw, rss=rr, n=int(got.size), kind=d['kind'],
                channels=d.get('channels'))


def slice_of(buf, d):
    """the part of the engine's buffer a yield speaks about"""
    t = torch.as_tensor(buf)
    if 'rows' in d and d['kind'] in ('sample', 'conv', 'chain'):
        t = t[:d['rows']]
    if d.get('channels') is not None:
        c0, c1 = d['channels']
        t = t[:, c0:c1]
    return t


def run_walk(P, cfg, image, has, fmt, get, precision, render_steps, interp, factor):
    """-> (rows, names yielded, faults of the selection)"""
    w = pdl_model.Graph32Walk(P, cfg, image, has, fmt, get, precision, render_steps, interp)
    rows, seen, faults = [], set(), []
    for name, value, d in w.walk():
        seen.add(name)
        if d['kind'] == 'selection':
            faults += selection_faults(d, value, get(d['out']))
            continue
        rows.append(check(name, d, value, slice_of(get(name), d), factor))
    return rows, seen, faults


# ----------------------------------------------------------------------------
# the CPU stand-in
# ----------------------------------------------------------------------------
X3_DEFAULT = dict(stem_fused=True, fuse_ds=True, hl=False, small_aspp=True, sep_fused=True, head='fused')
X3_PLANES = dict(X3_DEFAULT, hl=True)
X3_OFF = dict(stem_fused=False, fuse_ds=False, hl=False, small_aspp=False, sep_fused=False, head='pw')
X3_PART = dict(X3_DEFAULT, sep_fused=False, head='part')
F32 = dict(X3_OFF)


class StandIn:
    """The walk in float32 under the engine's names, with the schedule ``flags`` (run32's rules restated for the decisions the
    walk reads off the map list) and at most one planted defect."""

    def __init__(self, P, cfg, image, precision, flags, render_steps=2, interp=False, defect=None):
        self.P, self.cfg, self.image, self.x3, self.flags = P, cfg, image, precision == 'fp16x3', flags
        self.precision, self.RS, self.interp, self.defect = precision, render_steps, interp, defect
        self.maps, self.planted = {}, None
        regnet, bifpn = str(cfg.get('encoder', 'resnet50')).startswith('regnet'), 'BiFPN' in cfg.get('arch', '')
        # run32 opens the plane region on a ResNet whose low-level skips all leave below layer3 (x3_planes_complete)
        self.hl = bool(self.x3 and flags['hl'] and not regnet and (bifpn or max(cfg['low_level_stages']) <= 2))
        self.N = image['x'].shape[0]
        self.run()

    # ---- the schedule ----
    def has(self, name):
        f, x3 = self.flags, self.x3
        if name == 'stem':
            return not (x3 and f['stem_fused'])
        if name.endswith('.ds'):
            return not (x3 and f['fuse_ds'] and not (self.hl and name.startswith('encoder.layer4.')))
        if name.endswith('.f32'):
            return self.hl
        if name == 'p5.hl32':
            return bool(x3 and f['small_aspp'] and not self.hl and self.cfg['ins_decoder'])
        head = name.split('.')[0] in ('semantic_head', 'ins_center', 'ins_xy')
        if name.endswith('.dw'):
            return not (x3 and (f['head'] == 'fused' if head else f['sep_fused']))
        if name.endswith('.part'):
            return f['head'] == 'part'
        if name.endswith('.pw'):
            return f['head'] == 'pw'
        return name in self.maps

    def fmt(self, name):
        f = self.flags
        if not self.hl:
            return 0
        if name in ('p5.hl32',) or name.endswith('.aspp.cat'):
            return 1
        if name.startswith(('encoder.layer3.', 'encoder.layer4.')) and not name.endswith('.f32'):
            return 0 if (name == 'encoder.layer3.0.c2' and f['fuse_ds']) else 1
        return 0

    def get(self, name):
        if name not in self.maps and name.startswith('pr.'):
            self.pointrend_last()
        return self.maps[name]

    # ---- storing what the walk yields ----
    def store(self, name, value, d):
        v = value.to(torch.float32)
        if d['kind'] in ('conv', 'sep') and d.get('out_fmt'):      # (the gated and forced kinds of a RegNetY never sit in hl32 maps)
            v = pdl_model._pair(v)
        v = v.double()
        if d.get('channels') is None:
            self.maps[name] = v
            return
        c0, c1 = d.get('channels') or (0, v.shape[1])
        if name not in self.maps:
            shape = list(v.shape)
            shape[1] = self.width(name, d)
            self.maps[name] = torch.zeros(shape, dtype=torch.float64)
        self.maps[name][:v.shape[0], c0:c1] = v

    def width(self, name, d):
        if name.endswith('.aspp.cat'):
            return 4 * (d['channels'][1] - d['channels'][0])
        if name.startswith('pr.x'):
            return d['ld'] if 'ld' in d else d['case']['Cin']
        if '_decoder.cat' in name:      # BiFPN decoder: [transposed conv | skip]
            return 2 * (d['channels'][1] - d['channels'][0])
        P, x3 = self.P, self.x3      # a stage's concat buffer: run32's cpad
        dec, i = name.split('.stage')[0], int(name.split('.stage')[1][0])
        A = P[f'{dec}.aspp.convs.0.0'][0].shape[0]
        xch = A if i == 0 else P[f'{dec}.fuse.0.0.sepconv.1'][0].shape[0]
        return pdl_model._up(xch + P[f'{dec}.project.{i}.0'][0].shape[0], 32 if x3 else 16)

    def run(self):
        w = pdl_model.Graph32Walk(self.P, self.cfg, self.image, self.has, self.fmt, self.get, self.precision, self.RS, self.interp,
                                  dtype=torch.float32)
        for name, value, d in w.walk():
            if d['kind'] == 'selection':
                continue
            if d['kind'] == 'upsample_but':
                value = self.pointrend_step(self.maps[self._pr_src(name)], 2 * value.shape[2] // 2, store=False)
            elif d['kind'] == 'refined':
                value = self.maps['sem_logits']
            if self.defect is not None:
                bad = DEFECTS[self.defect](self, name, d, value)
                if bad is not None:
                    value, self.planted = bad, (name, d.get('channels'))
            if name == 'sem_logits':
                self.maps[name] = value.double()
            elif not name.startswith('pr.x'):      # (the row buffers are the stand-in's own: pointrend_step)
                self.store(name, value, d)
        if not self.interp:
            self.maps['ctr_hmp'], self.maps['offsets'] = self.maps['ins_center.out'], self.maps['ins_xy.out']

    def _pr_src(self, name):
        st = int(name[len('pr.sem'):])
        return 'semantic_head.out' if st == 0 else f'pr.sem{st - 1}'

    # ---- PointRend in float32 (oracle.pdl_model.point_rend_forward, one step, keeping the engine's buffers) ----
    def semx_name(self):
        if 'BiFPN' in self.cfg.get('arch', ''):
            return 'semantic_decoder.out'
        return 'semantic_decoder.stage%d.out' % (len(self.cfg['low_level_stages']) - 1)

    def pointrend_step(self, src, _unused, store):
        P, cfg = self.P, self.cfg
        coarse, semx = self.maps['semantic_head.out'].float(), self.maps[self.semx_name()].float()
        up = F.interpolate(src.float(), scale_factor=2.0, mode='bilinear', align_corners=False)
        N, ncls, hh, ww = up.shape
        k = min(hh * ww, cfg['subdivision_num_points'])
        keys = torch.from_numpy(PC.keys_ref(up.numpy()))
        idx = torch.topk(keys, k, dim=1, largest=False)[1]
        coords = PC.point_coords(idx.numpy(), hh, ww)
        if self.defect == 'pr_neighbour' and store:      # point 0 of image 0 sampled at its right-hand neighbour's centre
            coords[0, 0, 0] += 1.0 / ww
            self.planted = ('pr.x0', None)
        Cf = semx.shape[1]
        ldp = pdl_model._up(Cf + ncls, 16)
        fine = pdl_model.point_sample(semx, coords).permute(0, 2, 1).reshape(N * k, Cf)
        cs = pdl_model.point_sample(coarse, coords).permute(0, 2, 1).reshape(N * k, ncls)
        X = [torch.zeros(N * k, ldp), torch.zeros(N * k, ldp)]
        for x in X:
            x[:, :Cf], x[:, Cf:Cf + ncls] = fine, cs
        cur = 0
        for f in range(cfg['num_fc']):
            w, b = P[f'semantic_pr.point_head.fc_layers.{f}.0']
            w = torch.from_numpy(np.asarray(w, np.float32).reshape(w.shape[0], -1))
            X[cur ^ 1][:, :Cf] = F.relu(X[cur][:, :w.shape[1]] @ w.T + torch.from_numpy(np.asarray(b, np.float32)))
            cur ^= 1
        w, b = P['semantic_pr.point_head.predictor']
        w = torch.from_numpy(np.asarray(w, np.float32).reshape(ncls, -1))
        logits = X[cur][:, :w.shape[1]] @ w.T + torch.from_numpy(np.asarray(b, np.float32))
        out = up.reshape(N, ncls, hh * ww).scatter(2, idx.unsqueeze(1).expand(-1, ncls, -1), logits.view(N, k, ncls).permute(0, 2, 1)).view(N, ncls, hh, ww)
        if store:
            self.maps['pr.keys'] = keys.numpy().view(np.uint32).astype(np.int64)
            self.maps['pr.keys'] = torch.from_numpy(self.maps['pr.keys'])
            self.maps['pr.idx'] = idx
            self.maps['pr.x0'], self.maps['pr.x1'] = X[0].double(), X[1].double()
            self.maps['sem_logits'] = out.double()
        return out

    def pointrend_last(self):
        src = 'semantic_head.out' if self.RS == 1 else f'pr.sem{self.RS - 2}'
        self.pointrend_step(self.maps[src], None, store=True)

    def heads(self):
        return {k: self.maps[k] for k in OUTPUTS}


# ----------------------------------------------------------------------------
# planted defects: name -> f(stand-in, buffer name, description, clean value) -> the wrong value, or None where it does not apply
# ----------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.asarray(a, np.float32))


def _d_aspp_dilation(s, name, d, v):
    A = v.shape[1]
    if name != 'semantic_decoder.aspp.cat' or d.get('channels') != (2 * A, 3 * A):
        return None
    r = s.cfg['atrous_rates'][0]      # branch 2 with branch 1's rate
    w, b = s.P['semantic_decoder.aspp.convs.2.0']
    src = _f32(d['p']['x'][..., :w.shape[1]]).permute(0, 3, 1, 2)      # the launch's own input: p5 or its hl32 copy
    return F.relu(F.conv2d(src, _f32(w), _f32(b), 1, r, r))


def _d_hi_only(s, name, d, v):
    if name != 'encoder.layer3.0.c2' or not s.fmt('encoder.layer3.0.c1'):
        return None
    w, b = s.P['encoder.layer3.0.conv2']
    c1 = s.maps['encoder.layer3.0.c1'].float().half().float()      # the hi half alone
    stride = d['case']['stride']
    return F.relu(F.conv2d(c1, _f32(w), _f32(b), stride, d['case']['pad'], d['case']['dil']))


def _d_bias_image0(s, name, d, v):
    if name != 'semantic_decoder.aspp' or s.N < 2:
        return None
    bn = s.maps['semantic_decoder.bias_n'].float()
    return F.relu(v.float() * 0 + _pre_act_aspp(s) + bn[:1, :, None, None])


def _pre_act_aspp(s):
    A = s.P['semantic_decoder.aspp.convs.0.0'][0].shape[0]
    w, b = s.P['semantic_decoder.aspp.project.0']
    w = np.asarray(w, np.float32).reshape(A, 5 * A)[:, :4 * A]
    return F.conv2d(s.maps['semantic_decoder.aspp.cat'].float(), _f32(w)[:, :, None, None], _f32(b))


def _d_residual_from_input(s, name, d, v):
    """the first block of the second stage: its last launch adds the block's INPUT where the shortcut map is due"""
    if 'regnet' in s.cfg:
        if name != 'encoder.stage2.block1':
            return None
        w, b = s.P[name + '.bottleneck.c.0']
        y = F.conv2d(s.maps[name + '.b'].float(), _f32(w), _f32(b))
        inp = s.maps['encoder.stage1.block%d' % s.cfg['regnet']['depths'][0]]
    else:
        if name != 'encoder.layer2.0':
            return None
        w, b = s.P[name + '.conv3']
        y = F.conv2d(s.maps[name + '.c2'].float(), _f32(w), _f32(b))
        if not s.has(name + '.ds'):
            y = y + _f32(s.P[name + '.downsample.0'][1])[None, :, None, None]
        inp = s.maps['encoder.layer1.2']
    # the kernel's read of the block's input through the shortcut's geometry: row m, channel co at m * ld + co of the input's rows
    flat = inp.float().permute(0, 2, 3, 1).reshape(-1)
    N, C, H, W = y.shape
    ld = inp.shape[1]
    pos = (torch.arange(N * H * W)[:, None] * ld + torch.arange(C)[None, :]).clamp(max=flat.numel() - 1)
    return F.relu(y + flat[pos].view(N, H, W, C).permute(0, 3, 1, 2))


def _d_se_gate_skipped(s, name, d, v):
    """RegNetY: the first block's grouped map left ungated"""
    if d['kind'] != 'conv_gated' or s.planted is not None:
        return None
    return v.float() / torch.sigmoid(_f32(d['gate']))


def _d_align_corners(s, name, d, v):
    # the semantic decoder's first up-sampling that is not a same-size copy
    if not (name.startswith('semantic_decoder.stage') and name.endswith('.cat')) or d['kind'] != 'bilinear' or s.planted is not None:
        return None
    return F.interpolate(_f32(d['x']).permute(0, 3, 1, 2), size=(d['H'], d['W']), mode='bilinear', align_corners=False)


def _d_cat_pad(s, name, d, v):
    if d['kind'] != 'zero' or s.planted is not None:      # the first concat buffer that has a pad
        return None
    v = v.clone().float()
    v[-1, 0, 1, 2] = 1e-3
    return v


def _d_projection_offset(s, name, d, v):
    if name != 'semantic_decoder.stage0.cat' or d['kind'] != 'conv' or not s.cfg['ins_decoder']:
        return None
    lp_ins = s.P['instance_decoder.project.0.0'][0].shape[0]
    return torch.roll(v.float(), lp_ins % v.shape[1] or 1, 1)      # written from the offset the other decoder's width gives


DEFECTS = {
    'aspp_dilation': _d_aspp_dilation,
    'hl32_hi_only': _d_hi_only,
    'bias_n_image0': _d_bias_image0,
    'residual_from_input': _d_residual_from_input,
    'align_corners_false': _d_align_corners,
    'cat_pad_nonzero': _d_cat_pad,
    'projection_offset': _d_projection_offset,
    'pr_neighbour': lambda s, name, d, v: None,      # planted inside pointrend_step
    'se_gate_skipped': _d_se_gate_skipped,
}


def head_figures(bad, clean):
    """the figures the head-level tests assert (max |d| over max(1, rms) for the centre map and the offsets, the largest
    difference of the semantic probabilities), a defective stand-in against the clean one"""
    out = {}
    for k in ('ctr_hmp', 'offsets'):
        a, b = bad[k], clean[k]
        out[k] = float((a - b).abs().max()) / max(1.0, float(b.pow(2).mean().sqrt()))
    pa, pb = (torch.sigmoid(t) if t.shape[1] == 1 else torch.softmax(t, 1) for t in (bad['sem_logits'], clean['sem_logits']))
    out['sem_prob'] = float((pa - pb).abs().max())
    out['sem_share_over_1e3'] = float(((pa - pb).abs() > 1e-3).float().mean())
    return out


def image_of(x, H=None, W=None):
    """x (N, vh, vw) normalised float32 tensor [to be run at the padded size H x W]"""
    return dict(x=x, H=H or x.shape[1], W=W or x.shape[2])
