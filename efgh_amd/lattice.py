"""Device-side permutohedral lattice pyramid (replaces GenerateData.__call__,
nets/generate_data.py:117-193, which the reference runs on the CPU inside forward).

All samples of a batch are built by ONE launch sequence per level (efgh_lattice_level_build / _neighbors); every sample
keeps its own lattice (own key ranges, own vertex numbering).  The number of vertices of a level - the number of points of
the next one - lives in device memory, so when the sizes of a previous call with the same (batch, points, scales) signature
are known the whole pyramid is enqueued without a host read-back between levels (capacities = previous sizes + 25 %) and
the five counts come back in ONE read; a count that does not fit its capacity (flagged by the device) falls back to the
level-by-level path, which reads each count before sizing the next level."""
import collections
import logging
import math

import numpy as np
import torch

from . import _C

EXPECTED_STD = 4 * math.sqrt(2 / 3)            # generate_data.py:19
ALIAS_CAP = 4096                               # aliased neighbour hits recorded per level (lattice.hip k_neighbors)
INFO_H, INFO_ERR, INFO_ALIAS, INFO_SEG = 0, 1, 2, 4          # include/efgh_hip.h EFGH_LATTICE_INFO_*

PROFILE = None          # bench.py: list of (start_event, end_event, algorithmic_bytes, 'lattice build') per pyramid
_SIZES = {}             # (device, B, N, scales) -> vertex counts of the last build with that signature
_BIG_LEVELS = {}        # the same key -> levels where a bucket of the partitioned build overflowed: built with the big-bucket kernel from then on
_HASH_LEVELS = {}       # the same key -> levels where that overflowed as well: they take the hash build
_CLEAN = {}             # the same key -> consecutive clean speculative builds since the last change of the escalation sets
# An outlier frame must not pin a signature to the slow plans for the rest of the process: after this many clean builds in a row
# the most expensive escalation of the signature is taken back one step (hash -> big buckets -> regular) and the cheaper plan gets
# another try (a renewed overflow costs one re-enqueue of the pyramid and resets the count)
ESCALATION_DECAY = 64
STATS = {'speculative': 0, 'level_by_level': 0, 'reenqueued': 0}      # pyramids by path (tests, bench --rotate-inputs)
_log = logging.getLogger('efgh_amd.lattice')
RADII = (1, 2, 3)                              # BCL neighbourhood radii served (the second column of scale_map)


def filter_size(r):
    """taps of a radius-r BCL filter: (r+1)^4 - r^4 (bilateralNN.py get_filter_size, d = 3)"""
    return (r + 1) ** 4 - r ** 4


def table_ld(F):
    """row stride of a neighbour table of F taps: F neighbour columns + ceil(F/32) alias-mask words, rounded up to 4 (16 at F = 15)"""
    return (F + (F + 31) // 32 + 3) // 4 * 4


_OFFSETS = {}


def filter_offsets(r):
    """(off [F][4] int32, inv [F] int64) of a radius-r filter in the reference's tap order (generate_data.py:44-52).

    A tap is a vector of step counts i = (i0, i1, i2, i3), 0 <= i_d <= r, along the four lattice directions 4 e_d - (1,1,1,1);
    i3 may only be nonzero when one of i0..i2 is zero (the cuboid walk takes one step along the last direction otherwise), so
    the taps are the (r+1)^4 - r^4 such vectors in lexicographic order of (i0, i1, i2, i3), and off = 4 i - sum(i).
    inv[t] is the tap with off[inv[t]] = -off[t] (the set is symmetric)"""
    r = int(r)
    got = _OFFSETS.get(r)
    if got is None:
        rows = []
        for i0 in range(r + 1):
            for i1 in range(r + 1):
                for i2 in range(r + 1):
                    for i3 in range(r + 1 if 0 in (i0, i1, i2) else 1):
                        i = np.array([i0, i1, i2, i3])
                        rows.append(4 * i - i.sum())
        off = np.array(rows, dtype=np.int32)
        assert len(off) == filter_size(r)
        pos = {tuple(o): t for t, o in enumerate(off.tolist())}
        inv = np.array([pos[tuple((-off[t]).tolist())] for t in range(len(off))], dtype=np.int64)
        got = _OFFSETS[r] = (off, inv)
    return got


def check_radii(radii, nlevels):
    """radii per level (None: all 1) as a tuple of ints; anything outside RADII raises EfghError naming the level"""
    if radii is None:
        return (1,) * nlevels
    radii = list(radii)
    if len(radii) != nlevels:
        raise _C.EfghError('BCL radii: %d values for %d levels' % (len(radii), nlevels))
    out = []
    for l, r in enumerate(radii):
        if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or r != int(r) or int(r) not in RADII:
            raise _C.EfghError('BCL neighbourhood radius %r on level %d: radius 1, 2 or 3 is served' % (r, l))
        out.append(int(r))
    return tuple(out)


_DEV_OFFSETS = {}


def _dev_offsets(r, dev):
    k = (r, dev)
    t = _DEV_OFFSETS.get(k)
    if t is None:
        t = _DEV_OFFSETS[k] = torch.from_numpy(filter_offsets(r)[0]).to(dev)
    return t


class LatticeLevel:
    """one pyramid level; the arrays cover all samples (sample-major); seg_in / seg hold the per-sample offsets of input
    points / vertices (host lists, len B+1).

    point-major device arrays (16 B per point): bary_pm, emg_pm (float32 [n][4]), off_pm (int32 [n][4]);
    per vertex: nbr [H][ld] (F = filter_size(radius) neighbours + alias-mask words; [H][16] at radius 1), vseg [H][2] + list [4n] (vertex -> ascending flat positions
    4p + r), pts_next [3][H]; info = the level's device counters (INFO_*), alist = aliased neighbour records.
    _src = (pts, cstride, sid, pps, scale): the points the level was built from, kept for the point query (OutPoints.locate) - the
    previous level's arrays, or the [3][B N] form of the cloud for level 0 (for B = 1 a VIEW of the caller's cloud: it must not be
    overwritten before the first query); _index: the vertex index of the level, built on the first query."""
    __slots__ = ('n_in', 'H', 'bary_pm', 'emg_pm', 'off_pm', 'nbr', 'vseg', 'list', 'pts_next_buf', 'info', 'alist',
                 'seg_in', 'seg', 'vsid', '_ws', '_caps', '_mode', '_geom', '_zeroed', 'n_alias', 'radius', 'F', 'ld',
                 '_src', '_index')

    def vertex_index(self):
        """the persistent vertex index (efgh_lattice_index_build): key integer -> vertex row and the per-sample key boxes, whichever
        plan built the level; made on the first call, kept"""
        if self._index is None:
            from . import ops
            pts, cstride, sid, pps, s = self._src
            self._index = ops.lattice_index(pts, cstride, sid, pps, len(self.seg) - 1, s, self.list, self.vseg, self.vsid, self.info,
                                            self.H)
        return self._index

    # the reference's (4, n) / (3, H) arrays as views
    @property
    def bary(self):
        return self.bary_pm[:self.n_in].t()

    @property
    def emg(self):
        return self.emg_pm[:self.n_in].t()

    @property
    def off(self):
        if self.off_pm is None:
            raise _C.EfghError('this lattice was built with need_off=False (inference): lattice_offset was not produced')
        return self.off_pm[:self.n_in].t()

    @property
    def pts_next(self):
        return self.pts_next_buf[:, :self.H]

    def sample(self, b):
        """per-sample view with LOCAL indices, exactly the reference's per-sample arrays"""
        p0, p1, h0, h1 = self.seg_in[b], self.seg_in[b + 1], self.seg[b], self.seg[b + 1]
        out = _SampleView()
        out.n_in, out.H = p1 - p0, h1 - h0
        out.bary = self.bary[:, p0:p1]
        out.emg = self.emg[:, p0:p1]
        out.off = self.off[:, p0:p1] - h0
        nb = self.nbr[h0:h1, :self.F]
        out.nbr = torch.where(nb >= 0, nb - h0, nb)
        out.pts_next = self.pts_next[:, h0:h1]
        return out


class _SampleView:
    __slots__ = ('n_in', 'H', 'bary', 'emg', 'off', 'nbr', 'pts_next')



class OutPoints:
    """where the slice step of a BCL puts lattice features (bilateralNN.py:251-257 out_barycentric / out_lattice_offset): bary
    [n_out][4] float32 and off [n_out][4] int32, point-major like LatticeLevel.bary_pm / off_pm, off in GLOBAL row indices of the
    level's [H]-row arrays (sample-major).  The inverse of off (vseg, list: what the slice's backward walks) is built on first
    use; that is also the one time the count of offsets outside [0, H) is read, and a nonzero count raises EfghError.
    Out points made by `locate` (a lattice query of arbitrary points) may hold -1 = the lattice has no such vertex: that corner
    contributes nothing, forward and backward, and the other weights are not renormalised (the blur treats a missing neighbour the
    same way).  They carry the query's device counters; the count of left-out offsets must then EQUAL the absent corners."""
    __slots__ = ('n_out', 'H', 'bary', 'off', '_vseg', '_list', '_counters', '_missing')

    def __init__(self, bary, off, H, vseg=None, lst=None, counters=None):
        _C.require_cuda(bary, off)
        if bary.dtype != torch.float32 or off.dtype != torch.int32 or bary.dim() != 2 or bary.shape[1] != 4 or \
                tuple(off.shape) != tuple(bary.shape) or bary.shape[0] < 1 or int(H) < 1:
            raise _C.EfghError('OutPoints: bary [n_out][4] float32 and off [n_out][4] int32 of one shape, n_out >= 1, H >= 1 expected, '
                               'got %s %s / %s %s' % (tuple(bary.shape), bary.dtype, tuple(off.shape), off.dtype))
        self.bary, self.off = bary.contiguous(), off.contiguous()
        self.n_out, self.H = int(bary.shape[0]), int(H)
        self._vseg, self._list = vseg, lst
        self._counters, self._missing = counters, None           # (counters: absent corners are expected - set by locate only)

    @classmethod
    def locate(cls, lv, pts, sid=None):
        """arbitrary points on a built level: pts (3, M) or (B, 3, M) float32 on the device, in the frame of the cloud handed to
        build_pyramid(_batched) (the level's own scale is applied inside, as the build applies it); sid: int32 [M], the sample of
        every point of the (3, M) form (None: sample 0 of a one-sample level); the (B, 3, M) form puts M points on every sample.
        The weights are constants (generate_data.py:119); off holds -1 where the lattice has no vertex at a corner, see missing()"""
        from . import ops
        _C.require_cuda(pts, sid)
        _C.require_f32(pts)
        B = len(lv.seg) - 1
        if pts.dim() == 3 and pts.shape[0] == B and pts.shape[1] == 3 and pts.shape[2] >= 1 and sid is None:
            M = pts.shape[2]
            q, cstride, pps, n_q = pts.detach().permute(1, 0, 2).reshape(3, B * M).contiguous(), B * M, M, B * M
        elif pts.dim() == 2 and pts.shape[0] == 3 and pts.shape[1] >= 1 and (sid is not None or B == 1):
            q = pts.detach()
            if q.stride(1) != 1 or q.stride(0) < q.shape[1]:
                q = q.contiguous()
            cstride, pps, n_q = q.stride(0), q.shape[1], q.shape[1]
            if sid is not None and (sid.dtype != torch.int32 or tuple(sid.shape) != (n_q,) or not sid.is_contiguous()):
                raise _C.EfghError('OutPoints.locate: sid = int32 [%d], contiguous, expected, got %s %s' % (n_q, tuple(sid.shape), sid.dtype))
        else:
            raise _C.EfghError('OutPoints.locate: points (3, M), with sid [M] on a level of more than one sample, or (%d, 3, M) expected '
                               'on this level of %d sample(s), got %s' % (B, B, tuple(pts.shape)))
        bary, off, counters = ops.lattice_locate(lv.vertex_index(), q, cstride, sid, pps, n_q, lv._src[4], B, lv.H, lv.info)
        return cls(bary, off, lv.H, counters=counters)

    def missing(self):
        """(absent corners, points without any corner) of located points - one read, kept; (0, 0) for out points that were not
        located (theirs hold none, or lists() raises)"""
        if self._missing is None:
            self._missing = (0, 0) if self._counters is None else tuple(self._counters.tolist())
        return self._missing

    @classmethod
    def of_level(cls, lv):
        """the level's own points: its arrays as they are, the build's own vseg / list - nothing is launched"""
        if lv.off_pm is None:
            raise _C.EfghError('this lattice was built with need_off=False (inference): lattice_offset was not produced')
        return cls(lv.bary_pm[:lv.n_in], lv.off_pm[:lv.n_in], lv.H, lv.vseg, lv.list)

    @classmethod
    def select(cls, lv, idx):
        """rows idx (int tensor, any order, repetition allowed) of the level's points: a subset or another ordering without a
        lattice query"""
        if lv.off_pm is None:
            raise _C.EfghError('this lattice was built with need_off=False (inference): lattice_offset was not produced')
        idx = torch.as_tensor(idx, device=lv.bary_pm.device).long().reshape(-1)
        return cls(lv.bary_pm[:lv.n_in].index_select(0, idx), lv.off_pm[:lv.n_in].index_select(0, idx), lv.H)

    def lists(self):
        """(vseg [H][2], list): every vertex's flat positions 4p + r into these out points, ascending"""
        if self._vseg is None:
            from . import ops
            vseg, lst, err = ops.offsets_invert(self.off, self.H)
            if self._counters is None:
                bad, expected = int(err.item()), 0                  # the one read of the error word
            else:                                  # located points: the left-out entries are the query's absent corners, no other
                bad, expected, none = torch.cat([err, self._counters]).tolist()          # (one transfer)
                self._missing = (expected, none)
            if bad != expected:
                raise _C.EfghError('OutPoints: %d lattice offsets outside [0, %d) (the reference would wrap a -1 to the last vertex; '
                                   'here that is an error)%s' % (bad, self.H, ', %d absent corners located' % expected if expected else ''))
            self._vseg, self._list = vseg, lst
        return self._vseg, self._list


def _pow2ceil(v):
    return 1 << max(0, int(v) - 1).bit_length()


# how a level is built.  kind 'part': the entries are dealt into `buckets` buckets and every bucket is grouped in LDS in a table of
# `slots` slots, big: with the big-bucket kernel behind it (one more launch; spatially dense sweeps need it).  kind 'hash': the
# global hash insert into a table of `slots` entries (0 = its default table); buckets = 0, big = False
Plan = collections.namedtuple('Plan', 'kind buckets slots big')


def _as_plan(mode):
    """a Plan from what a caller hands in: a Plan, ('hash', slots), ('part', buckets, slots) or ('part', buckets, slots, big)"""
    if isinstance(mode, Plan):
        return mode
    if mode[0] == 'hash':
        return Plan('hash', 0, mode[1], False)
    return Plan('part', mode[1], mode[2], len(mode) > 3 and bool(mode[3]))


def _plan(L, n_cap, h_est, hashed=False, big=False):
    """the Plan of a level of n_cap points expecting ~h_est vertices (None: unknown).  hashed / big: the level's escalation state
    (_HASH_LEVELS / _BIG_LEVELS).  More points than the partitioned build's bucket limit (~2.8 M) take the hash build as well"""
    nb = 0 if hashed else L.efgh_lattice_part_buckets(n_cap)
    if nb:
        return Plan('part', nb, 2048 if h_est is None else min(2048, max(64, _pow2ceil(2.5 * h_est / nb + 64))), big)
    # hash table sized for the expected vertex count (load <= 1/2) instead of the worst case 4 * n_cap keys
    return Plan('hash', 0, 0 if h_est is None else max(4096, 1 << (2 * h_est - 1).bit_length()), False)


def _state(key, l):
    """(hashed, big) of level l of a signature, as _plan takes them"""
    return l in _HASH_LEVELS[key], l in _BIG_LEVELS[key]


def _escalate(key, l, err, plan):
    """level l, built by the partitioned `plan`, overflowed (ERR bit 2: a bucket with more entries than its window, a table too
    small): it is escalated for this signature - first to the build with the big-bucket kernel, then to the hash build.  A key range
    too wide for the partitioned build's entry word (bit 3) is not a bucket problem: the big-bucket kernel cannot fix it, the level
    goes straight to the hash build.  Returns the name of the build the level takes from now on"""
    to_hash = bool(err & 8) or plan.big
    (_HASH_LEVELS if to_hash else _BIG_LEVELS)[key].add(l)
    _CLEAN[key] = 0
    return 'hash' if to_hash else 'big-bucket'


def _relax(key):
    """the counterpart of _escalate, after a clean speculative build: once ESCALATION_DECAY of them have passed in a row the most
    expensive escalation of the signature is taken back one step"""
    forced, bigl = _HASH_LEVELS[key], _BIG_LEVELS[key]
    _CLEAN[key] = _CLEAN.get(key, 0) + 1
    if not (forced or bigl) or ESCALATION_DECAY <= 0 or _CLEAN[key] < ESCALATION_DECAY:
        return
    _CLEAN[key] = 0
    if forced:
        l = max(forced)
        forced.discard(l)
        bigl.add(l)
        _log.info('lattice %s: level %d back from the hash build to the big-bucket build after %d clean builds', key, l, ESCALATION_DECAY)
    else:
        l = max(bigl)
        bigl.discard(l)
        _log.info('lattice %s: level %d back to the regular partitioned build after %d clean builds', key, l, ESCALATION_DECAY)


def _ctrl_bytes(L, n_cap, B, mode):
    """bytes of the zero-initialised control block of a level: info, and for the partitioned build its `zeroed` area"""
    info_b = (4 * (INFO_SEG + B) + 255) // 256 * 256
    return info_b, (L.efgh_lattice_part_zeroed_bytes(n_cap) if mode[0] == 'part' else 0)


def _level_arrays(L, dev, n_cap, h_cap, B, mode=('hash', 0), ctrl=None, need_off=True):
    """arrays of one level.  ctrl: a ZEROED uint8 tensor of sum(_ctrl_bytes) bytes (one fill serves all levels of a pyramid);
    None = allocate and zero one here.  need_off=False (partitioned build only): lattice_offset is not produced"""
    lv = LatticeLevel()
    lv._mode = mode = _as_plan(mode)
    lv._src = lv._index = None
    lv.radius, lv.F, lv.ld = 1, 15, 16
    lv.bary_pm = torch.empty((n_cap, 4), dtype=torch.float32, device=dev)
    lv.emg_pm = torch.empty((n_cap, 4), dtype=torch.float32, device=dev)
    lv.off_pm = torch.empty((n_cap, 4), dtype=torch.int32, device=dev) if (need_off or mode.kind == 'hash') else None
    if mode.kind == 'part':       # every bucket owns a fixed window of the list array
        lv.list = torch.empty(L.efgh_lattice_part_list_len(n_cap, mode.buckets), dtype=torch.int32, device=dev)
        ws_bytes = L.efgh_lattice_part_workspace_bytes(n_cap, h_cap, B, mode.buckets, mode.slots)
    else:
        lv.list = torch.empty(4 * n_cap, dtype=torch.int32, device=dev)
        ws_bytes = L.efgh_lattice_workspace_bytes(n_cap, h_cap, B)
    lv.vseg = torch.empty((h_cap, 2), dtype=torch.int32, device=dev)
    lv.pts_next_buf = torch.empty((3, h_cap), dtype=torch.float32, device=dev)
    lv.vsid = torch.empty(h_cap, dtype=torch.int32, device=dev)
    info_b, zero_b = _ctrl_bytes(L, n_cap, B, mode)
    if ctrl is None:
        ctrl = torch.zeros(info_b + zero_b, dtype=torch.uint8, device=dev)
    lv.info = ctrl[:4 * (INFO_SEG + B)].view(torch.int32)
    lv._zeroed = ctrl[info_b:info_b + zero_b] if zero_b else None
    lv.alist = torch.empty((ALIAS_CAP, 2), dtype=torch.int32, device=dev)
    lv._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lv._caps = (n_cap, h_cap)
    return lv


def _launch_build(L, lv, pts, cstride, n_dev, sid, pps, B, s, st):
    n_cap, h_cap = lv._caps
    head = (_C.ptr(pts), cstride, _C.ptr(n_dev), n_cap, _C.ptr(sid), pps, B, s)
    lv._geom = (pts, cstride, n_dev, sid, pps, s)          # (kept alive for the neighbours call)
    lv._src = (pts, cstride, sid, pps, s)                  # (kept with the level: OutPoints.locate)
    plan = lv._mode
    if plan.kind == 'part':
        _C.check(L.efgh_lattice_part_build(*head, _C.ptr(lv.bary_pm), _C.ptr(lv.emg_pm), _C.ptr(lv.list), h_cap, _C.ptr(lv.info),
                                           _C.ptr(lv._ws), _C.ptr(lv._zeroed), plan.buckets, plan.slots,
                                           0 if lv.off_pm is None else 1, 1 if plan.big else 0, st))
    else:
        _C.check(L.efgh_lattice_level_build(*head, EXPECTED_STD * s, _C.ptr(lv.bary_pm), _C.ptr(lv.emg_pm), _C.ptr(lv.off_pm),
                                            _C.ptr(lv.list), h_cap, _C.ptr(lv.vseg), _C.ptr(lv.pts_next_buf), _C.ptr(lv.vsid),
                                            _C.ptr(lv.info), _C.ptr(lv._ws), plan.slots, st))


def _launch_neighbors(L, lv, B, h_rows, st):
    n_cap, h_cap = lv._caps
    plan = lv._mode
    lv.nbr = torch.empty((h_rows, 16), dtype=torch.int32, device=lv.info.device)
    if lv.radius != 1 and plan.kind != 'part':
        _launch_neighbors_r(L, lv, B, h_rows, st)          # (the hash build left its vertex records: its radius-1 probes are not needed)
        return
    if plan.kind == 'part':
        pts, cstride, n_dev, sid, pps, s = lv._geom
        _C.check(L.efgh_lattice_part_neighbors(
            _C.ptr(lv._ws), _C.ptr(pts), cstride, _C.ptr(n_dev), n_cap, _C.ptr(sid), pps, B, s, EXPECTED_STD * s, h_cap,
            _C.ptr(lv.info), h_rows, _C.ptr(lv.nbr), _C.ptr(lv.alist), ALIAS_CAP, _C.ptr(lv.off_pm), _C.ptr(lv.vseg),
            _C.ptr(lv.pts_next_buf), _C.ptr(lv.vsid), plan.buckets, plan.slots, st))
        if lv.radius != 1:              # (that launch also emitted the vertex records the radius-r probes start from)
            _launch_neighbors_r(L, lv, B, h_rows, st)
            return
    else:
        _C.check(L.efgh_lattice_level_neighbors(_C.ptr(lv._ws), n_cap, h_cap, B, _C.ptr(lv.info), _C.ptr(lv.vsid), h_rows,
                                                _C.ptr(lv.nbr), _C.ptr(lv.alist), ALIAS_CAP, plan.slots, st))
    lv._geom = lv._zeroed = None


def _launch_neighbors_r(L, lv, B, h_rows, st):
    """the F = filter_size(radius) blur neighbours of a level (efgh_lattice_neighbors_r), behind whichever build served it"""
    pts, cstride, n_dev, sid, pps, s = lv._geom
    dev = lv.info.device
    lv.nbr = torch.empty((h_rows, lv.ld), dtype=torch.int32, device=dev)
    ws = torch.empty(L.efgh_lattice_neighbors_r_workspace(h_rows, B), dtype=torch.uint8, device=dev)
    _C.check(L.efgh_lattice_neighbors_r(_C.ptr(pts), cstride, _C.ptr(sid), pps, B, s, _C.ptr(lv.list), _C.ptr(lv.vseg),
                                        _C.ptr(lv.vsid), _C.ptr(lv.info), h_rows, _C.ptr(_dev_offsets(lv.radius, dev)), lv.F, lv.ld,
                                        _C.ptr(lv.nbr), _C.ptr(ws), st))
    lv._geom = lv._zeroed = None


def _enqueue(L, lv, src, N, B, s, st, exact=False):
    """build and neighbours of one level from its source (pts, cstride, n_dev, sid, n_cap) -> (the next level's source, ERR).
    exact: the vertex count H is read back between the two (a host sync) - the neighbour table gets H rows and the next level
    exactly H points; a partitioned build that overflowed (ERR bit 2) gets no neighbours and no next source (None)"""
    pts, cstride, n_dev, sid, _ = src
    h_cap = lv._caps[1]
    _launch_build(L, lv, pts, cstride, n_dev, sid, N, B, s, st)
    if not exact:           # the count stays on the device: capacities stand in for it
        _launch_neighbors(L, lv, B, h_cap, st)
        return (lv.pts_next_buf, h_cap, lv.info[INFO_H:], lv.vsid, h_cap), 0
    H, err = lv.info[:2].tolist()
    if err & 4 and lv._mode.kind == 'part':
        return None, err
    _launch_neighbors(L, lv, B, H, st)
    return (lv.pts_next_buf, h_cap, None, lv.vsid, H), err


def _finish(lv, host, n_in, seg_in, B):
    if host[INFO_ERR] & 2:
        raise _C.EfghError('lattice: more than %d aliased neighbour hits on one level' % ALIAS_CAP)
    H = host[INFO_H]
    lv.n_alias = host[INFO_ALIAS]      # (on the host with the one read-back: a level without aliased hits - every real sweep - needs no patch launch)
    lv.n_in, lv.H, lv.seg_in = n_in, H, seg_in
    lv.seg = list(host[INFO_SEG:INFO_SEG + B]) + [H]
    lv._ws = None                      # scratch no longer needed (the stream orders its reuse)
    if lv.nbr.shape[0] != H:
        lv.nbr = lv.nbr[:H]


def _speculative(L, dev, key, prev, src, scales, radii, B, N, need_off, st, e1):
    """the whole pyramid enqueued with capacities from `prev`, the vertex counts of the previous build of this signature (+ 25 %),
    no read-back between levels, the counts back in ONE read.  Returns (levels, False); (None, False) when the batch has to take
    the level-by-level path - a vertex count beyond its capacity (ERR bit 0); or (None, True) when a partitioned level overflowed
    and was escalated: the pyramid is to be enqueued once more (levels behind the first overflow were built on its garbage)"""
    # capacities and plans of all levels first: their control blocks (device counters, first-seen bitmaps) are zeroed by ONE fill.
    # Tables are sized for the expected vertex count
    caps, nc = [], src[4]
    for l, hp in enumerate(prev):
        hc = min(4 * nc, hp + hp // 4 + 1024)
        caps.append((nc, hc, _plan(L, nc, hc, *_state(key, l))))
        nc = hc
    sizes = [_ctrl_bytes(L, nc_, B, plan) for nc_, _, plan in caps]
    ctrl = torch.zeros(sum(a + b for a, b in sizes), dtype=torch.uint8, device=dev)
    lvs, coff = [], 0
    for s, r, (n_cap, h_cap, plan), (ib, zb) in zip(scales, radii, caps, sizes):
        lv = _level_arrays(L, dev, n_cap, h_cap, B, plan, ctrl[coff:coff + ib + zb], need_off)
        _set_radius(lv, r)
        coff += ib + zb
        src, _ = _enqueue(L, lv, src, N, B, s, st)
        lvs.append(lv)
    if e1 is not None:
        e1.record()              # (before the read-back: the events bracket the launches only)
    host = torch.stack([lv.info for lv in lvs]).cpu().tolist()           # the one host sync of the pyramid
    if not any(h[INFO_ERR] & 5 for h in host):
        n_in, seg_in = B * N, [b * N for b in range(B + 1)]
        for lv, h in zip(lvs, host):
            _finish(lv, h, n_in, seg_in, B)
            n_in, seg_in = lv.H, lv.seg
        _relax(key)
        return lvs, False
    over = [l for l, (h, lv) in enumerate(zip(host, lvs)) if h[INFO_ERR] & 4 and lv._mode.kind == 'part']
    if not over or any(h[INFO_ERR] & 1 for h in host):
        return None, False
    l, err = over[0], host[over[0]][INFO_ERR]
    _log.warning('lattice %s: level %d %s; escalated to the %s build, pyramid re-enqueued', key, l,
                 'has a key range too wide for the partitioned build' if err & 8 else 'overflowed a bucket',
                 _escalate(key, l, err, lvs[l]._mode))
    return None, True


def _level_by_level(L, dev, key, src, scales, radii, B, N, need_off, st):
    """each level's count is read before the next level is sized (exact capacities); a partitioned level that overflows is
    escalated and built again on the spot"""
    out, seg_in = [], [b * N for b in range(B + 1)]
    for l, (s, r) in enumerate(zip(scales, radii)):
        n, nxt = src[4], None
        while nxt is None:
            plan = _plan(L, n, None, *_state(key, l))
            lv = _level_arrays(L, dev, n, 4 * n, B, plan, None, need_off)
            _set_radius(lv, r)
            nxt, err = _enqueue(L, lv, src, N, B, s, st, exact=True)
            if nxt is None:
                _escalate(key, l, err, plan)
        _finish(lv, lv.info.cpu().tolist(), n, seg_in, B)
        out.append(lv)
        src, seg_in = nxt, lv.seg
    return out


def build_pyramid_batched(pc, scales, radii=None, need_off=True):
    """pc: (B,3,N) fp32 CUDA tensor -> list of LatticeLevel (one per scale).  radii: the BCL neighbourhood radius per level
    (scale_map's second column; None = 1 everywhere): a level of radius r gets a neighbour table of filter_size(r) taps.
    need_off=False: lattice_offset (`off`) is left out - the splat walks the vertex lists, only its backward reads `off` (inference
    saves a gather pass and three arrays per level)."""
    _C.require_cuda(pc)
    radii = check_radii(radii, len(scales))
    L = _C.lib()
    dev = pc.device
    B, _, N = pc.shape
    assert pc.dtype == torch.float32 and pc.size(1) == 3 and B >= 1 and N >= 1
    src = (pc.permute(1, 0, 2).reshape(3, B * N).contiguous(), B * N, None, None, B * N)
    st = _C.stream_ptr()
    scales = [float(s) for s in scales]
    key = (dev.index, B, N, tuple(scales))
    e0 = e1 = None
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    out = None
    prev = _SIZES.get(key)
    _HASH_LEVELS.setdefault(key, set())
    _BIG_LEVELS.setdefault(key, set())
    for _ in range(3 if prev is not None else 0):
        out, again = _speculative(L, dev, key, prev, src, scales, radii, B, N, need_off, st, e1)
        if not again:
            break
        STATS['reenqueued'] += 1
    if out is not None:
        STATS['speculative'] += 1
    else:
        STATS['level_by_level'] += 1
        out = _level_by_level(L, dev, key, src, scales, radii, B, N, need_off, st)
        if e1 is not None:
            e1.record()
    _SIZES[key] = [lv.H for lv in out]
    if PROFILE is not None:
        by = 0.0
        for lv in out:          # reads N*3*4, writes N*(4*4 + 4*4 + 4*8) + 15*H*8 + 4*H*4
            by += lv.n_in * 12.0 + lv.n_in * 64.0 + lv.H * (lv.F * 8 + 16.0)
        PROFILE.append((e0, e1, by, 'lattice build'))
    return out


def _set_radius(lv, r):
    lv.radius, lv.F = r, filter_size(r)
    lv.ld = table_ld(lv.F)


def build_pyramid(pc, scales, radii=None):
    """pc: (3,N) fp32 CUDA tensor (one sample).  Returns a list of LatticeLevel."""
    assert pc.dim() == 2 and pc.size(0) == 3
    return build_pyramid_batched(pc.unsqueeze(0), scales, radii)
