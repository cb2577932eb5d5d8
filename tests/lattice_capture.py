"""How lattice.build_pyramid_batched plans, enqueues and escalates the levels of a pyramid, recorded without a GPU: the function
runs on CPU tensors with _C.lib replaced by a stand-in that forwards the sizing queries to the real libefgh_hip.so, records every
other efgh_lattice_* call and launches nothing.  A build call gets its scripted (H, ERR) words and per-sample bases written into
the level's info block, as the kernels would leave them.  tests/test_lattice_plans_host.py compares what this produces with
tests/golden/lattice_plans.json.

Per build the record holds: every recorded call in order (scalars verbatim, floats as their float32 bits, a pointer as the level
array it points into - 'L<n>' is the n-th level allocated by that build - or None, 'other' for anything else: the input cloud, the
radius-r workspace); of every level returned its plan as (kind, buckets, slots, big), capacities, H, seg, n_alias, radius, F, ld;
STATS and the signature's _SIZES / _HASH_LEVELS / _BIG_LEVELS / _CLEAN after the build; the log messages; the PROFILE entries'
byte counts; the exception type when the build raises.

`python tests/lattice_capture.py --write` rewrites the fixture, `--dump FILE` writes the full records (to diff two trees)."""
import base64
import ctypes
import hashlib
import json
import logging
import numbers
import os
import struct
import sys

import torch

QUERIES = ('_bytes', '_len', '_buckets', '_workspace', '_capacity', '_max_entries', 'efgh_last_error', 'efgh_version')
ARRAYS = ('bary_pm', 'emg_pm', 'off_pm', 'list', 'vseg', 'pts_next_buf', 'vsid', 'info', 'alist', '_ws', '_zeroed', 'nbr')
SCALES = (1.0, 0.75, 0.5, 0.25, 0.125)
HS = (1500, 1100, 600, 200, 50)           # the vertex count the stand-in reports per level (+ 3 per build of the scenario)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lattice_plans.json')


class _Ev:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


def plan_of(mode):
    """a level's plan as [kind, buckets, slots, big], whether it is the named tuple or one of the plain tuples ('hash', slots),
    ('part', buckets, slots), ('part', buckets, slots, big) that the code before the named tuple kept"""
    if mode[0] == 'hash':
        return ['hash', 0, int(mode[1] if len(mode) == 2 else mode[2]), False]
    return [mode[0], int(mode[1]), int(mode[2]), bool(len(mode) > 3 and mode[3])]


def typed_args(fn, args):
    """the arguments of a library call as its argtypes (from include/efgh_hip.h) convert them: a plain number or None becomes the
    instance of the declared scalar or void-pointer type, so a record tells a pointer from a size and a float by its fp32 bits;
    a value the declared type refuses raises here as it would in the call"""
    assert len(fn.argtypes) == len(args), (fn.__name__, len(args))
    return [t(a) if issubclass(t, ctypes._SimpleCData) and (a is None or isinstance(a, numbers.Real)) else a
            for t, a in zip(fn.argtypes, args)]


class Capture(logging.Handler):
    """the stand-ins, installed for the life of a `with` block"""

    def __init__(self):
        logging.Handler.__init__(self, logging.INFO)
        from efgh_amd import _C, lattice
        self._C, self.lat = _C, lattice
        self.real = _C.lib()
        self.calls, self.levels, self.logs, self.built = [], [], [], {}
        self.script, self.scales, self.shift, self.zero_buckets = {}, SCALES, 0, None

    def emit(self, record):
        self.logs.append(record.getMessage())

    def __getattr__(self, name):            # the library stand-in
        if name == 'efgh_lattice_part_buckets':
            return lambda n: 0 if self.zero_buckets == getattr(n, 'value', n) else self.real.efgh_lattice_part_buckets(n)
        if any(q in name for q in QUERIES):
            return getattr(self.real, name)

        def entry(*args):
            args = typed_args(getattr(self.real, name), args)
            self.calls.append([name[len('efgh_lattice_'):]] + [self._arg(a) for a in args])
            if name in ('efgh_lattice_part_build', 'efgh_lattice_level_build'):
                self._counts(args)
            return 0
        return entry

    def _counts(self, args):
        """what the build kernels leave in the info block of the level allocated last: H, ERR and the samples' vertex bases"""
        lv = self.levels[-1]
        assert lv.info.data_ptr() in [a.value for a in args if isinstance(a, ctypes.c_void_p)]
        l = self.scales.index(round(args[7].value, 6))
        nth = self.built[l] = self.built.get(l, -1) + 1
        B = args[6].value
        err, H = self.script.get((nth, l), (0, None))
        H = HS[l] + self.shift if H is None else H
        lv.info[self.lat.INFO_H], lv.info[self.lat.INFO_ERR] = H, err
        for b in range(B):
            lv.info[self.lat.INFO_SEG + b] = H * b // B

    def _ptr(self, p):
        if not p:
            return None
        for i, lv in enumerate(self.levels):
            for k in ARRAYS:
                t = getattr(lv, k, None)
                if t is not None and t.numel() and t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                    return 'L%d.%s' % (i, k)
        return 'other'

    def _arg(self, a):
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value)
        if isinstance(a, ctypes.c_float):
            return 'f%08x' % struct.unpack('<I', struct.pack('<f', a.value))[0]
        if isinstance(a, ctypes._SimpleCData):
            return a.value
        return repr(a)

    def __enter__(self):
        _C, lat = self._C, self.lat
        self.saved = [(_C, 'lib', _C.lib), (_C, 'require_cuda', _C.require_cuda), (_C, 'stream_ptr', _C.stream_ptr),
                      (lat, '_level_arrays', lat._level_arrays), (lat, 'ESCALATION_DECAY', lat.ESCALATION_DECAY),
                      (lat, 'PROFILE', lat.PROFILE), (torch.cuda, 'Event', torch.cuda.Event)]
        self.saved_dicts = [(d, dict(d)) for d in (lat._SIZES, lat._HASH_LEVELS, lat._BIG_LEVELS, lat._CLEAN, lat.STATS)]
        real_arrays = lat._level_arrays

        def level_arrays(*a, **kw):
            lv = real_arrays(*a, **kw)
            self.levels.append(lv)
            return lv
        _C.lib = lambda: self
        _C.require_cuda = lambda *t: None
        _C.stream_ptr = lambda: 0
        lat._level_arrays = level_arrays
        torch.cuda.Event = _Ev
        lat._log.addHandler(self)
        self.log_level = lat._log.level
        lat._log.setLevel(logging.INFO)
        return self

    def __exit__(self, *exc):
        for o, k, v in self.saved:
            setattr(o, k, v)
        for d, v in self.saved_dicts:
            d.clear()
            d.update(v)
        self.lat._log.removeHandler(self)
        self.lat._log.setLevel(self.log_level)

    def reset(self):
        """a fresh process as far as the lattice module's per-signature state goes"""
        lat = self.lat
        for d, _ in self.saved_dicts:
            d.clear()
        lat.STATS.update(speculative=0, level_by_level=0, reenqueued=0)
        lat.ESCALATION_DECAY, lat.PROFILE = 64, None
        self.shift, self.zero_buckets = 0, None

    def build(self, B=2, N=512, scales=SCALES, script=None, **kw):
        """one build_pyramid_batched call -> its record.  script: {(n, level): (ERR, H or None)} for the n-th build of that level
        within the call"""
        lat = self.lat
        del self.calls[:], self.levels[:], self.logs[:]
        self.built, self.script, self.scales = {}, script or {}, tuple(round(s, 6) for s in scales)
        pc = torch.zeros(B, 3, N)
        key = (None, B, N, tuple(float(s) for s in scales))
        rec = {}
        try:
            out = lat.build_pyramid_batched(pc, scales, **kw) if B > 1 else lat.build_pyramid(pc[0], scales, **kw)
            rec['levels'] = [[plan_of(lv._mode), list(lv._caps), lv.n_in, lv.H, list(lv.seg_in), list(lv.seg), lv.n_alias, lv.radius,
                              lv.F, lv.ld, list(lv.nbr.shape), lv.off_pm is None, lv._ws is None, lv._geom is None, lv._zeroed is None]
                             for lv in out]
        except Exception as e:
            rec['raised'] = type(e).__name__
        rec['calls'] = [list(c) for c in self.calls]
        rec['state'] = [dict(lat.STATS), lat._SIZES.get(key), sorted(lat._HASH_LEVELS.get(key, ())), sorted(lat._BIG_LEVELS.get(key, ())),
                        lat._CLEAN.get(key)]
        rec['logs'] = list(self.logs)
        if lat.PROFILE is not None:
            rec['profile'] = [[e[2], e[3]] for e in lat.PROFILE]
        self.shift += 3
        return rec


def scenarios(cap):
    """(name, [record per build]) of every scenario"""
    lat = cap.lat
    key = (None, 2, 512, SCALES)

    def run(name, *builds):
        cap.reset()
        recs = []
        for b in builds:
            if callable(b):
                b()
            else:
                recs.append(cap.build(**b))
        return name, recs

    def preset(hashed=(), big=(), decay=None, forget_sizes=False):
        def go():
            lat._HASH_LEVELS[key], lat._BIG_LEVELS[key], lat._CLEAN[key] = set(hashed), set(big), 0
            if decay is not None:
                lat.ESCALATION_DECAY = decay
            if forget_sizes:
                lat._SIZES.clear()
        return go

    clean = {}
    yield run('clean', clean, clean, clean)
    yield run('one sample', dict(B=1), dict(B=1))
    yield run('three scales', dict(scales=SCALES[:3]), dict(scales=SCALES[:3]))
    yield run('need_off False', dict(need_off=False), dict(need_off=False))
    radii = dict(radii=(1, 2, 3, 2, 1))
    yield run('radii on partitioned levels', radii, radii)
    yield run('radii on hash levels', clean, preset(hashed=(1, 2, 3)), radii, preset(hashed=(1, 2, 3), forget_sizes=True), radii)
    yield run('radii on big levels', clean, preset(big=(1, 2)), radii, preset(big=(1, 2), forget_sizes=True), radii)
    yield run('profile', lambda: setattr(lat, 'PROFILE', []), clean, clean, dict(script={(0, 2): (1, None)}))
    # the speculative path
    yield run('speculative: count beyond capacity', clean, dict(script={(0, 2): (1, 9000)}), clean)
    yield run('speculative: overflow, then again', clean, dict(script={(0, 1): (4, None)}), clean, dict(script={(0, 1): (4, None)}), clean)
    yield run('speculative: overflow twice in one call', clean, dict(script={(0, 1): (4, None), (1, 1): (4, None)}), clean)
    yield run('speculative: overflow three times in one call', clean, dict(script={(0, 1): (4, None), (1, 1): (4, None), (2, 1): (4, None)}),
              clean)
    yield run('speculative: three levels overflow in turn', clean, dict(script={(0, 0): (4, None), (1, 1): (4, None), (2, 2): (4, None)}), clean)
    yield run('speculative: two levels overflow at once', clean, dict(script={(0, 1): (4, None), (0, 3): (4, None)}), clean)
    yield run('speculative: key range too wide', clean, dict(script={(0, 1): (12, None)}), clean)
    yield run('speculative: overflow and a count beyond capacity', clean, dict(script={(0, 1): (4, None), (0, 3): (1, None)}), clean)
    yield run('speculative: overflow of a hash level', clean, preset(hashed=(2,)), dict(script={(0, 2): (4, None)}), clean)
    yield run('speculative: alias cap', clean, dict(script={(0, 2): (2, None)}), clean)
    # the level-by-level path
    yield run('level by level: overflow', dict(script={(0, 1): (4, None)}), clean)
    yield run('level by level: overflow twice', dict(script={(0, 1): (4, None), (1, 1): (4, None)}), clean)
    yield run('level by level: overflow three times', dict(script={(0, 1): (4, None), (1, 1): (4, None), (2, 1): (4, None)}), clean)
    yield run('level by level: key range too wide', dict(script={(0, 1): (12, None)}), clean)
    yield run('level by level: overflow and a count beyond capacity', dict(script={(0, 1): (4, None), (0, 3): (1, None)}), clean)
    yield run('level by level: hash and big levels kept', preset(hashed=(1,), big=(0,)), clean, clean)
    yield run('level by level: alias cap', dict(script={(0, 0): (2, None)}), clean)
    # de-escalation: the sequence test_escalations_expire_after_clean_builds asserts on the GPU
    yield run('escalations expire', clean, preset(hashed=(1,), big=(0,), decay=2), *[clean] * 7)
    yield run('escalations do not expire with decay 0', clean, preset(hashed=(1,), big=(0,), decay=0), *[clean] * 3)
    yield run('an overflow resets the clean count', clean, preset(big=(0,), decay=2), clean, dict(script={(0, 2): (4, None)}), clean, clean)
    # more points than the partitioned build takes: the hash plan, its table sized from the estimate once there is one
    yield run('no buckets on level 0', lambda: setattr(cap, 'zero_buckets', 1024), clean, clean)
    yield run('no buckets on level 0, hash level overflows', lambda: setattr(cap, 'zero_buckets', 1024), clean, dict(script={(0, 0): (4, None)}))
    yield run('new signature', clean, clean, dict(B=3), dict(N=256), clean, dict(B=3), dict(N=256))


def _h(x):
    return base64.b64encode(hashlib.sha1(json.dumps(x, sort_keys=True, default=str).encode()).digest()[:6]).decode()


def table(full=False):
    """{'calls': [distinct entry-point sequences], 'scenarios': {name: [[calls index, digest of the whole record] per build]}}"""
    seqs, out, dump = {}, {}, {}
    with Capture() as cap:
        for name, recs in scenarios(cap):
            assert name not in out
            dump[name] = recs
            out[name] = [[seqs.setdefault('+'.join(c[0] for c in r['calls']), len(seqs)), _h(r)] for r in recs]
    if full:
        return dump
    return {'calls': sorted(seqs, key=seqs.get), 'scenarios': out}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:2] == ['--dump']:
        json.dump(table(True), open(sys.argv[2], 'w'), indent=1, sort_keys=True, default=str)
    elif sys.argv[1:2] == ['--write']:
        with open(GOLDEN, 'w') as f:
            f.write(json.dumps(table(), indent=0, separators=(',', ':')) + '\n')
    else:
        sys.exit(__doc__)
