"""Which kernel serves a launch, recorded without a GPU: ops.gather_gemm / ops.gather_wgrad run on CPU tensors with ops._L replaced
by a stand-in that forwards the size and query functions to the real libefgh_hip.so and, for every other efgh_* entry point, records
the call and launches nothing.  tests/test_routes_host.py compares the table this produces with tests/golden/routes.json.

Per case the table holds: the entry points called, in order (or, when the call raises, the exception type alone); the profile
lists the launch was appended to, each with its flops / bytes value and its (mode, M, N, T, C); a digest of every argument handed to
the library (descriptor fields verbatim, pointers as (argument tensor, byte offset), 'tmp' for a buffer the dispatch made itself);
the answers of stats_rows / pool_fusable / lazy_capable / wgrad_lazy_capable; the return value.

The stand-in answers EFGH_WROTE_OUT when it is handed an efgh_wgrad_out_desc, so that the `done` path of gather_wgrad is taken.
The input transform a 2-D Winograd forward keeps for its weight gradient travels as the caller's own nets/fn.py hands it over:
gather_gemm(keep_v=) receives it, gather_wgrad(pre_v=) takes it - a buffer the dispatch made, so it stays 'tmp' in the digests."""
import ctypes
import base64
import hashlib
import itertools
import json
import os
import sys

import torch

from lattice_capture import typed_args

QUERIES = ('_supported', '_workspace', '_tiles', '_stats_rows', '_grid_m', '_groups', 'efgh_last_error', 'efgh_version')
LISTS = ('PROFILE', 'PROFILE_WGRAD', 'PROFILE_WINO', 'PROFILE_WINO_WGRAD', 'PROFILE_WINO2D', 'PROFILE_WINO2D_GEMM', 'PROFILE_THIN',
         'PROFILE_DED')
OFF_IN_TURN = ('USE_WINO', 'USE_WINO2D', 'USE_C4', 'USE_SMALLC', 'USE_THIN', 'USE_WINO_WGRAD', 'PLANE_DMA', 'POOL_FUSED', 'POOL_HALF')
THRESHOLDS = ('WINO2D_MIN_C', 'WINO2D_MIN_C_WGRAD', 'WINO2D_MIN_C_TRAIN', 'SC_MIN_PIXELS_32')
# (name, switches, TLS.train_step, grid): the full grid under the default switches, a thinned one (every family, both sides of every
# threshold) for the variants
SETTINGS = ([('default', {}, False, 'full'), ('default train_step', {}, True, 'full')]
            + [(k + ' off', {k: False}, i % 2 == 1, 'thin') for i, k in enumerate(OFF_IN_TURN)]
            + [('PLANES_SPLIT', {'PLANES_SPLIT': True}, True, 'thin'), ('KSPLIT_MAX_ROWS 0', {'KSPLIT_MAX_ROWS': 0}, False, 'thin'),
               ('thresholds 0', {k: 0 for k in THRESHOLDS}, True, 'thin')])
GRIDS = {'full': ((4, 16, 32, 64, 128, 256), ((1, 1), (3, 5), (4, 4), (7, 9), (8, 8), (13, 16), (16, 11), (200, 320))),
         'thin': ((4, 16, 32, 64, 128), ((7, 9), (8, 8), (200, 320)))}
z = torch.zeros


def g3x3(B, H, W, s=1):
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    return (B, H, W, Ho, Wo, s, s, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)], Ho, Wo, 1, 1, 0, 0)


def g1x1(B, H, W):
    return (B, H, W, H, W, 1, 1, [0], [0], H, W, 1, 1, 0, 0)


class _Ev:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


class Capture:
    """the stand-ins, installed for the life of a `with` block"""

    def __init__(self):
        from efgh_amd import _C, ops
        self._C, self.ops = _C, ops
        self.real = _C.lib()
        self.calls, self.digest, self.tensors, self.lists_hit = [], [], {}, set()

    def __getattr__(self, name):            # the library stand-in
        if any(q in name for q in QUERIES):
            return getattr(self.real, name)

        def entry(*args):
            args = typed_args(getattr(self.real, name), args)
            self.calls.append(name)
            self.digest.append([name] + [self._arg(a) for a in args])
            return 1 if any(isinstance(getattr(a, '_obj', None), self._C.WgradOutDesc) for a in args) else 0
        return entry

    def _ptr(self, p):
        if not p:
            return None
        for name in sorted(self.tensors):
            t = self.tensors[name]
            s = t.untyped_storage()
            if s.data_ptr() <= p < s.data_ptr() + max(s.nbytes(), 1):
                return [name, p - t.data_ptr()]
        return 'tmp'

    def _arg(self, a):
        a = getattr(a, '_obj', a)
        if isinstance(a, ctypes.Structure):
            return {f: self._ptr(getattr(a, f)) if ty is ctypes.c_void_p else self._arg(getattr(a, f)) for f, ty in a._fields_}
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value)
        if isinstance(a, ctypes.Array):
            return list(a)
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        return a

    def __enter__(self):
        ops, _C = self.ops, self._C
        self.saved = [(ops, '_L', ops._L), (ops, '_st', ops._st), (_C, 'stream_ptr', _C.stream_ptr), (torch.cuda, 'Event', torch.cuda.Event)]
        self.saved += [(ops, k, getattr(ops, k)) for k in LISTS + OFF_IN_TURN + THRESHOLDS
                       + ('PLANES_SPLIT', 'KSPLIT_MAX_ROWS', 'BN_BWD_FUSED', 'BN_BWD_FUSED_2D', 'FOLD_UNPACK', 'W2V_KEEP')]
        ops._L = lambda: self
        ops._st = _C.stream_ptr = lambda: 0
        torch.cuda.Event = _Ev
        for k in LISTS:
            setattr(ops, k, [])
        self.train_step = ops.TLS.train_step
        return self

    def __exit__(self, *exc):
        for o, k, v in self.saved:
            setattr(o, k, v)
        self.ops.TLS.train_step = self.train_step

    def run(self, fn, tensors, sw=None):
        """one case -> [entry points | exception type, digest hash of (profile records, arguments, return value)]"""
        ops = self.ops
        self.tensors = {k: v for k, v in tensors.items() if torch.is_tensor(v)}
        del self.calls[:], self.digest[:]
        old = {k: getattr(ops, k) for k in (sw or {})}
        for k, v in (sw or {}).items():
            setattr(ops, k, v)
        try:
            r = fn()
            ret = list(r.shape) if torch.is_tensor(r) else r
            calls = '+'.join(self.calls)
        except Exception as e:           # (the parent launches before it rejects an unserved pool: the exception type alone)
            return [type(e).__name__, '']
        finally:
            for k, v in old.items():
                setattr(ops, k, v)
            prof = [(k, e[2], list(e[3])) for k in LISTS for e in getattr(ops, k)]
            self.lists_hit.update(p[0] for p in prof)
            for k in LISTS:
                del getattr(ops, k)[:]
        return [calls, _h([prof, self.digest, ret])]


def _h(x):
    return base64.b64encode(hashlib.sha1(json.dumps(x, sort_keys=True, default=str).encode()).digest()[:3]).decode()


NA = ['not applicable', '']


def _answers(*a):
    """stats_rows / pool_fusable / lazy_capable / wgrad_lazy_capable of a shape"""
    return ['answers', _h(list(a))]


def _gemm(cap, A, lda, C, T, Wp, N, M, out, ldo, sw=None, **kw):
    names = dict(kw, A=A, Wp=Wp, out=out)
    for k in ('lazy', 'bn_bwd'):
        o = kw.get(k)
        for f in getattr(o, '__slots__', ()):
            names[k + '.' + f] = getattr(o, f)
    return cap.run(lambda: cap.ops.gather_gemm(A, lda, C, T, Wp, N, M, out, ldo, **kw), names, sw)


def _wgrad(cap, A, lda, C, T, N, M, G, ldg, dWp, sw=None, **kw):
    names = dict(kw, A=A, G=G, dWp=dWp)
    names.pop('pre_v', None)         # (the forward's own buffer, not an argument of the layer: 'tmp')
    if kw.get('unpack') is not None:
        names['unpack.dW'] = kw['unpack'][0]
    o = kw.get('lazy')
    for f in getattr(o, '__slots__', ()):
        names['lazy.' + f] = getattr(o, f)
    return cap.run(lambda: cap.ops.gather_wgrad(A, lda, C, T, N, M, G, ldg, dWp, **kw), names, sw)


def grid_cases(cap, grid):
    """channels^2 x maps x {3x3 stride 1, 3x3 stride 2, 1x1} x {plain, statistics, pool} and the weight gradient"""
    ops = cap.ops
    chans, maps = GRIDS[grid]
    for C, N, (H, W) in itertools.product(chans, chans, maps):
        for geom in (g3x3(2, H, W), g3x3(2, H, W, 2), g1x1(2, H, W)):
            B, Ho, Wo, T = 2, geom[9], geom[10], len(geom[7])
            M = B * Ho * Wo
            tag = 'C%d N%d %dx%d s%d T%d' % (C, N, H, W, geom[5], T)
            A, Wp, out = z(B, H, W, C), z(N, T, C), z(B, Ho, Wo, N)
            pf = ops.pool_fusable(1, C, N, geom)
            rows = ops.stats_rows(1, C, N, geom, M)
            yield tag + ' answers', _answers(rows, pf, ops.lazy_capable(1, C, N, geom), ops.wgrad_lazy_capable(1, C, N, geom),
                                           ops.pool_fusable(1, C, N, geom, stats=out), ops.pool_fusable(1, C, N, geom, residual=out))
            yield tag + ' plain', _gemm(cap, A, C, C, T, Wp, N, M, out, N, mode=1, geom=geom)
            # (with statistics a thin shape goes to another family; pool: only what pool_fusable accepts, the rest is among the
            # special cases)
            yield tag + ' stats', _gemm(cap, A, C, C, T, Wp, N, M, out, N, mode=1, geom=geom, stats=z(max(rows, 1), 2, N))
            po = z(B, Ho if pf == 'h' else Ho // 2, Wo // 2, N)
            yield tag + ' pool', _gemm(cap, A, C, C, T, Wp, N, M, po, N, mode=1, geom=geom, pool=pf) if pf else NA
            yield tag + ' wgrad', _wgrad(cap, A, C, C, T, N, M, out, N, z(N, T, C), mode=1, geom=geom)


def _convt_geoms(B, H, W, ph=1, oph=1):
    """the four output-parity classes of a stride-2 ConvTranspose2d(k=3) (layers.conv_transpose2d)"""
    Ho, Wo = (H - 1) * 2 - 2 * ph + 3 + oph, (W - 1) * 2 - 2 * ph + 3 + oph
    for cy in range(2):
        for cx in range(2):
            taps = [(a, b) for a in range(3) if (cy + ph - a) % 2 == 0 for b in range(3) if (cx + ph - b) % 2 == 0]
            Hv, Wv = (Ho - cy + 1) // 2, (Wo - cx + 1) // 2
            yield (B, H, W, Hv, Wv, 1, 1, [(cy + ph - a) // 2 for a, _ in taps], [(cx + ph - b) // 2 for _, b in taps], Ho, Wo, 2, 2, cy, cx)


def special_cases(cap):
    """the launches the grid does not reach (see the conditions on the case list in tests/test_routes_host.py)"""
    from efgh_amd.nets.fn import BnSrc
    ops = cap.ops
    i32 = torch.int32
    # linear rows: mode 0, no geometry (N == 4 and C == 4 are thin SHAPES, but the thin kernels serve mode 1 only)
    for C, N in ((64, 64), (16, 4), (4, 16), (4, 4), (256, 12), (32, 32)):
        M = 500
        yield 'linear C%d N%d' % (C, N), _gemm(cap, z(M, C), C, C, 1, z(N, 1, C), N, M, z(M, N), N, mode=0)
        yield 'linear C%d N%d stats' % (C, N), _gemm(cap, z(M, C), C, C, 1, z(N, 1, C), N, M, z(M, N), N, mode=0,
                                                       stats=z(ops.stats_rows(0, C, N, None, M), 2, N))
        yield 'linear C%d N%d wgrad' % (C, N), _wgrad(cap, z(M, C), C, C, 1, N, M, z(M, N), N, z(N, 1, C), mode=0)
        yield 'linear C%d N%d answers' % (C, N), _answers(ops.stats_rows(0, C, N, None, M), ops.pool_fusable(0, C, N, None),
                                                         ops.lazy_capable(0, C, N, None), ops.wgrad_lazy_capable(0, C, N, None))
    # transposed convolution: the four parity classes (osh = osw = 2)
    for C, N in ((64, 64), (128, 128), (16, 4), (4, 4)):
        for geom in _convt_geoms(1, 8, 8):
            T, M = len(geom[7]), geom[3] * geom[4]
            tag = 'convT C%d N%d class %d%d' % (C, N, geom[13], geom[14])
            A, Wp, out = z(1, 8, 8, C), z(N, T, C), z(1, 16, 16, N)
            yield tag, _gemm(cap, A, C, C, T, Wp, N, M, out, N, mode=1, geom=geom)
            yield tag + ' stats', _gemm(cap, A, C, C, T, Wp, N, M, out, N, mode=1, geom=geom, stats=z(ops.stats_rows(1, C, N, geom, M), 2, N))
            yield tag + ' wgrad', _wgrad(cap, A, C, C, T, N, M, out, N, z(N, T, C), mode=1, geom=geom)
            yield tag + ' answers', _answers(ops.stats_rows(1, C, N, geom, M), ops.pool_fusable(1, C, N, geom), ops.lazy_capable(1, C, N, geom),
                                           ops.wgrad_lazy_capable(1, C, N, geom))
    # BCL blur (mode 2): both sides of every k-split condition, with and without alias_mask
    def blur(tag, M=1000, T=15, C=128, N=64, nb=None, **kw):
        tab = z(M, 16, dtype=i32)
        bias = None if nb == 0 else z(nb or N)
        return 'blur ' + tag, _gemm(cap, z(M, C), C, C, T, z(N, T, C), N, M, z(M, N), N, mode=2, table=tab, bias=bias, act=1, **kw)
    yield blur('ksplit')
    yield blur('ksplit alias_mask', alias_mask=True)
    yield blur('ksplit no bias', nb=0)
    yield blur('ksplit offsets', a_off=0, out_off=0, flops=123.0)
    yield blur('rows at the limit', M=16384)
    yield blur('rows above the limit', M=16385)
    yield blur('rows above the limit alias_mask', M=16385, alias_mask=True)
    yield blur('T 14', T=14)
    yield blur('N 6', N=6)
    yield blur('K 960', C=64)
    yield blur('K 1080', C=72)
    yield blur('short bias', nb=60)
    yield blur('batch', batch=(1, 0, 0, 0))
    yield blur('scale', scale=z(64))
    yield blur('shift', shift=z(64))
    yield blur('residual', residual=z(1000, 64), ldr=64)
    yield blur('stats', stats=z(ops.stats_rows(2, 128, 64, None, 1000), 2, 64))
    yield blur('M_dev', M_dev=z(1, dtype=torch.int64))
    yield 'blur wgrad', _wgrad(cap, z(1000, 128), 128, 128, 15, 64, 1000, z(1000, 64), 64, z(64, 15, 128), mode=2, table=z(1000, 16, dtype=i32))
    # the batched correlation launch (ops.corr_head): mode 3 with batch strides
    B, h, wc, wr = 2, 8, 40, 48
    wp_, segw = wr + 2 * (wr // 8), (wc + 31) // 32
    nseg, wpitch, T = ops.ceil4((wc + segw - 1) // segw), wp_ + segw, 1
    geom = (1, h, wpitch, 1, wp_, 1, 1, [], [], 1, wp_, 1, 1, 0, 0)
    yield 'corr batch', _gemm(cap, z(B, h, wpitch, 16), 16, segw * 16, h, z(B, nseg, h, segw * 16), nseg, wp_, z(B, wp_, nseg), nseg, mode=3,
                              geom=geom, flops=7.0, batch=(B, h * wpitch * 16, nseg * h * segw * 16, wp_ * nseg))
    yield 'corr bwd batch', _gemm(cap, z(B, 128, 64), 64, 64, 1, z(B, 40, 64), 40, 128, z(B, 128, 40), 40, mode=0, flops=9.0,
                                  batch=(B, 128 * 64, 40 * 64, 128 * 40))
    # M_dev on a shape each family would serve without it
    for C, N in ((128, 128), (64, 64), (16, 16), (4, 32), (4, 4), (8, 8)):
        g = g3x3(1, 16, 16)
        yield 'M_dev C%d N%d' % (C, N), _gemm(cap, z(1, 16, 16, C), C, C, 9, z(N, 9, C), N, 256, z(1, 16, 16, N), N, mode=1, geom=g,
                                              M_dev=z(1, dtype=torch.int64))
        yield 'batch C%d N%d' % (C, N), _gemm(cap, z(1, 16, 16, C), C, C, 9, z(N, 9, C), N, 256, z(1, 16, 16, N), N, mode=1, geom=g,
                                              batch=(1, 0, 0, 0))
    # MODE_BLUR_R: plain, and with each argument it rejects
    Hn, F = 1000, 65
    def blur_r(tag, tshape=(Hn, 68), tdt=i32, **kw):
        return 'blur_r ' + tag, _gemm(cap, z(Hn, 32), 32, 32, F, z(64, F * 32), 64, Hn, z(Hn, 64), 64, mode=ops.MODE_BLUR_R,
                                      table=z(*tshape, dtype=tdt), **kw)
    yield blur_r('plain')
    yield blur_r('bias act offsets', bias=z(64), act=1, slope=0.1, a_off=0, out_off=0, flops=5.0)
    yield blur_r('narrow table', tshape=(Hn, 66))
    yield blur_r('short table', tshape=(Hn - 1, 68))
    yield blur_r('int64 table', tdt=torch.int64)
    for k, v in (('geom', g3x3(1, 16, 16)), ('batch', (1, 0, 0, 0)), ('M_dev', z(1, dtype=torch.int64)), ('scale', z(64)), ('shift', z(64)),
                 ('residual', z(Hn, 64)), ('stats', z(8, 2, 64)), ('alias_mask', True), ('pool', True),
                 ('bn_bwd', BnSrc(z(Hn, 64), None, z(64), z(64), z(64), z(64), 1, 0.0, Hn, 64)),
                 ('lazy', ops.LazyAct(z(32), z(32), 1, 0.0))):
        yield blur_r('rejects ' + k, **{k: v})
    yield 'blur_r wgrad', _wgrad(cap, z(Hn, 32), 32, 32, F, 64, Hn, z(Hn, 64), 64, z(64, F, 32), mode=ops.MODE_BLUR_R, table=z(Hn, 68, dtype=i32))
    yield 'blur_r wgrad unpack', _wgrad(cap, z(Hn, 32), 32, 32, F, 64, Hn, z(Hn, 64), 64, z(64, F, 32), mode=ops.MODE_BLUR_R,
                                        table=z(Hn, 68, dtype=i32), unpack=(z(64, 32, F), 64, F, 32, 32, 32 * F, F, 1, list(range(16)), False))
    # lazy / pre_v / pre_gy, pool, bn_bwd, unpack, the kept transform: on routes that take them and on routes that do not
    g, M = g3x3(1, 16, 16), 256
    T2 = 16
    for C, N in ((128, 128), (256, 128), (64, 64), (64, 128), (16, 64), (32, 64), (32, 32), (16, 16), (4, 32), (4, 4), (8, 8), (16, 4)):
        tag = 'C%d N%d ' % (C, N)
        A, Wp, out = z(1, 16, 16, C), z(N, 9, C), z(1, 16, 16, N)
        lazy = ops.LazyAct(z(C), z(C), 1, 0.0)
        yield tag + 'lazy', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, mode=1, geom=g, lazy=lazy)
        yield tag + 'lazy M_dev', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, mode=1, geom=g, lazy=lazy, M_dev=z(1, dtype=torch.int64))
        yield tag + 'pre_v', _gemm(cap, None, C, C, 9, Wp, N, M, out, N, mode=1, geom=g, pre_v=z(T2, 36, C))
        yield tag + 'wgrad lazy', _wgrad(cap, A, C, C, 9, N, M, out, N, z(N, 9, C), mode=1, geom=g, lazy=lazy)
        yield tag + 'wgrad pre_gy', _wgrad(cap, A, C, C, 9, N, M, None, N, z(N, 9, C), mode=1, geom=g, pre_gy=z(T2, 36, N))
        for pool in (True, 'h'):
            po = z(1, 16 if pool == 'h' else 8, 8, N)
            # (a fresh weight: fa9984f packs its Winograd image, which is cached on the weight, before it rejects the launch)
            yield tag + 'pool %s' % pool, _gemm(cap, A, C, C, 9, z(N, 9, C), N, M, po, N, mode=1, geom=g, pool=pool)
            yield tag + 'pool %s stride 2' % pool, _gemm(cap, A, C, C, 9, z(N, 9, C), N, 64, z(1, 4, 4, N), N, mode=1, geom=g3x3(1, 16, 16, 2),
                                                         pool=pool)
        for y in (None, z(1, 16, 16, N)):
            for sw in ({'BN_BWD_FUSED': True, 'BN_BWD_FUSED_2D': True}, {'BN_BWD_FUSED': False, 'BN_BWD_FUSED_2D': False}, {}):
                src = BnSrc(z(1, 16, 16, N), y, z(N), z(N), z(N), z(N), 1, 0.1, M, N)
                t = tag + 'bn_bwd y=%s %s' % (y is not None, sorted(sw.items()))
                yield t, _gemm(cap, A, C, C, 9, Wp, N, M, out, N, sw, mode=1, geom=g, bn_bwd=src)
                yield t + ' out_off', _gemm(cap, A, C, C, 9, Wp, N, M, z(1, 16, 16, N + 4), N + 4, sw, mode=1, geom=g, bn_bwd=src, out_off=4)
                yield t + ' stats', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, sw, mode=1, geom=g, bn_bwd=src,
                                          stats=z(ops.stats_rows(1, C, N, g, M), 2, N))
                yield t + ' misfit', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, sw, mode=1, geom=g,
                                           bn_bwd=BnSrc(z(1, 16, 16, N), y, z(N), z(N), z(N), z(N), 1, 0.1, M + 1, N))
        for fold in (True, False):
            up = (z(N, C, 3, 3), N, 9, C, C, C * 9, 9, 1, list(range(9)), fold)
            yield tag + 'wgrad unpack FOLD_UNPACK=%s' % fold, _wgrad(cap, A, C, C, 9, N, M, out, N, z(N, 9, C), {'FOLD_UNPACK': fold},
                                                                    mode=1, geom=g, unpack=up)
        # the transform kept by the forward (keep_v=), handed to the weight gradient where that runs on the 2-D Winograd path, as
        # nets/fn.py does; then without it (a second backward)
        slot = []
        yield tag + 'forward keeps', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, mode=1, geom=g, keep_v=slot)
        kept = {'pre_v': slot[0]} if (slot and ops.wgrad_route(1, C, N, 9, g) == 'wino2d') else {}
        yield tag + 'wgrad finds kept', _wgrad(cap, A, C, C, 9, N, M, out, N, z(N, 9, C), mode=1, geom=g, **kept)
        yield tag + 'wgrad kept gone', _wgrad(cap, A, C, C, 9, N, M, out, N, z(N, 9, C), mode=1, geom=g)
        yield tag + 'wgrad W2V_KEEP off', _gemm(cap, A, C, C, 9, Wp, N, M, out, N, {'W2V_KEEP': False}, mode=1, geom=g)
    # 16- / 32-channel launches on a channel slice at an offset of 2 floats (not 16-byte aligned), with and without statistics
    for C, N in ((16, 16), (32, 16), (16, 32), (32, 32)):
        for k in ('a_off', 'out_off', 'res_off'):
            for st in (False, True):
                A, out, res = z(1, 16, 16, C + 4), z(1, 16, 16, N + 4), z(1, 16, 16, N + 4)
                kw = dict(mode=1, geom=g, residual=res, ldr=N + 4, stats=z(ops.stats_rows(1, C, N, g, M), 2, N) if st else None)
                kw[k] = 2
                yield 'slice C%d N%d %s=2 stats=%s' % (C, N, k, st), _gemm(cap, A, C + 4, C, 9, z(N, 9, C), N, M, out, N + 4, **kw)
        A = z(1, 16, 16, C + 4)
        yield 'slice C%d N%d wgrad lda' % (C, N), _wgrad(cap, A, C + 2, C, 9, N, M, z(1, 16, 16, N), N, z(N, 9, C), mode=1, geom=g)
        yield 'slice C%d N%d wgrad A' % (C, N), _wgrad(cap, A.view(-1)[2:], C + 4, C, 9, N, M, z(1, 16, 16, N), N, z(N, 9, C), mode=1, geom=g)
        yield 'slice C%d N%d wgrad G' % (C, N), _wgrad(cap, A, C + 4, C, 9, N, M, z(1, 16, 16, N + 1).view(-1)[2:], N, z(N, 9, C), mode=1, geom=g)
    for N in (4, 32, 64):          # the 4-channel input layers: the stencil and the small-channel weight gradient need 16-byte rows too
        A = z(1, 16, 16, 8)
        yield 'slice C4 N%d wgrad lda' % N, _wgrad(cap, A, 6, 4, 9, N, M, z(1, 16, 16, N), N, z(N, 9, 4), mode=1, geom=g)
        yield 'slice C4 N%d wgrad A' % N, _wgrad(cap, A.view(-1)[2:], 8, 4, 9, N, M, z(1, 16, 16, N), N, z(N, 9, 4), mode=1, geom=g)
        yield 'slice C4 N%d wgrad dWp' % N, _wgrad(cap, A, 8, 4, 9, N, M, z(1, 16, 16, N), N, z(N * 36 + 4)[2:], mode=1, geom=g)


def table():
    """{'names': {grid: [case names]}, 'calls': [distinct call sequences], 'records': [distinct [calls index, digest]],
    'settings': {setting: [records index per case]}, 'lists': the profile lists reached}"""
    names, seqs, recs, settings = {}, {}, {}, {}
    with Capture() as cap:
        ops = cap.ops
        for name, sw, train, grid in SETTINGS:
            ops.TLS.train_step = train
            for k, v in sw.items():
                setattr(ops, k, v)
            rows = list(grid_cases(cap, grid)) + list(special_cases(cap))
            for k in sw:
                setattr(ops, k, next(v for o, kk, v in cap.saved if o is ops and kk == k))
            got = [r[0] for r in rows]
            assert len(set(got)) == len(got), [n for n in got if got.count(n) > 1][:5]
            assert names.setdefault(grid, got) == got, (name, 'the case list depends on the switches')
            settings[name] = [recs.setdefault((seqs.setdefault(c, len(seqs)), h), len(recs)) for _, (c, h) in rows]
    return {'names': names, 'calls': sorted(seqs, key=seqs.get), 'records': [list(r) for r in sorted(recs, key=recs.get)],
            'settings': settings, 'lists': sorted(cap.lists_hit)}


def _default_ids(t_names, ids, names):
    """the record of each case of `names` in the 'default' setting (whose case list, the full grid, holds every name)"""
    at = dict(zip(t_names, ids))
    return [at[n] for n in names]


def _wrap(s, n=120):
    return [s[i:i + n] for i in range(0, len(s), n)]


def pack(t):
    """table() -> the compact form kept in tests/golden/routes.json.  The case names: one hash per grid.  The records, in the order
    the 'default' setting meets them: one character each for the call sequence, four for the digest (both wrapped).  'default':
    {record: [positions, each as the step from the one before]} of the cases that repeat an earlier record (every other case has the
    next new one).  Every other setting: the
    [position, record] pairs where it differs from 'default' at the case of the same name."""
    assert len(t['calls']) <= 94 and SETTINGS[0][0] == 'default'
    full, ids0 = t['names'][SETTINGS[0][3]], t['settings']['default']
    settings, seen, last = {'default': {}}, 0, {}
    for i, r in enumerate(ids0):
        if r == seen:
            seen += 1
        else:
            settings['default'].setdefault(str(r), []).append(i - last.get(r, 0))
            last[r] = i
    for name, _, _, grid in SETTINGS[1:]:
        base = _default_ids(full, ids0, t['names'][grid])
        settings[name] = [x for i, (a, b) in enumerate(zip(base, t['settings'][name])) if a != b for x in (i, b)]
    return {'names': {g: [len(n), _h(n)] for g, n in t['names'].items()}, 'calls': t['calls'],
            'record_calls': _wrap(''.join(chr(35 + c) for c, _ in t['records'])),
            'record_digests': _wrap(''.join(h.ljust(4, '.') for _, h in t['records'])),
            'settings': settings, 'lists': t['lists']}


def unpack(f, names):
    """the compact form and the case names {grid: [names]} of the code under test -> what table() returns, but for the names"""
    seq, dig = ''.join(f['record_calls']), ''.join(f['record_digests'])
    records = [[ord(c) - 35, dig[4 * i:4 * i + 4].rstrip('.')] for i, c in enumerate(seq)]
    full = names[SETTINGS[0][3]]
    rep, ids0 = {}, []
    for r, steps in f['settings']['default'].items():
        pos = 0
        for st in steps:
            pos += st
            rep[pos] = int(r)
    nrep = 0
    for i in range(len(full)):
        nrep += i in rep
        ids0.append(rep[i] if i in rep else i - nrep)
    settings = {'default': ids0}
    for name, _, _, grid in SETTINGS[1:]:
        ids, d = _default_ids(full, ids0, names[grid]), f['settings'][name]
        for pos, rec in zip(d[::2], d[1::2]):
            ids[pos] = rec
        settings[name] = ids
    return {'calls': f['calls'], 'records': records, 'settings': settings, 'lists': f['lists']}


def dumps(f, width=120):
    """compact JSON, broken after a comma outside a string once a line is `width` long (so that the file can be read and diffed)"""
    out, line, in_str = [], '', False
    for ch in json.dumps(f, separators=(',', ':')):
        line += ch
        in_str ^= ch == '"'
        if ch == ',' and not in_str and len(line) >= width:
            out.append(line)
            line = ''
    return '\n'.join(out + [line]) + '\n'


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t = table()
    packed = pack(t)
    back = unpack(json.loads(dumps(packed)), t['names'])
    assert all(back[k] == t[k] for k in back), 'pack / unpack do not round-trip'
    open(sys.argv[1], 'w').write(dumps(packed))
