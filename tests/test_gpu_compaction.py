"""The stable compaction of the point preparation (count, scan, compact: csrc/prep.hip) through the C ABI, at the sizes where a scan or
a rank can go wrong: a lone lane, a wave edge, a block edge, and 256 / 257 blocks (the second chunk of the single-block scan of the block
counts holds one block).  The kept rows and their count equal numpy's flatnonzero of the contract's predicate exactly
(tests/sweeps_contract.py, tests/voxel_contract.py, the one-line box for plain rows); `keep` lives between two sentinel frames, and what
lies past the count is not written; plain [n, 4] rows and a one-identity sweep set over the same rows give the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import sweeps_contract as SC
from tests import voxel_contract as VC

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 65536, 65537)
R = 50.0                                                     # exact in float32
FRAME, SENTINEL = 64, -77777
EGO = (0.8, 2.7)
i32, f32, f64 = ctypes.c_int32, ctypes.c_float, ctypes.c_double


def _C():
    from efgh_amd import _C as C
    return C


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


class Framed(object):
    """an int32 buffer of n entries between two frames of sentinels"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * FRAME,), SENTINEL, dtype=torch.int32, device='cuda')
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * FRAME)

    def kept(self, count):
        """the first `count` entries, after checking that nothing else was written"""
        b = self.buf.cpu().numpy()
        assert 0 <= count <= self.n
        assert (b[:FRAME] == SENTINEL).all() and (b[FRAME + count:] == SENTINEL).all()
        return b[FRAME:FRAME + count]


@functools.lru_cache(maxsize=None)
def mix(n):
    """[n, 4] float32 rows of which about half lie in the box (x, y uniform in +-R sqrt 2), with planted rows where they fit: exactly
    -R (kept), exactly +R (dropped), the float below +R (kept), NaN, +inf and -inf in x (dropped)"""
    rng = np.random.default_rng(100 + n)
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(-R * np.sqrt(2), R * np.sqrt(2), (n, 2))
    p[:, 2] = rng.uniform(-2, 2, n)
    p[:, 3] = 0.5
    below = np.nextafter(np.float32(R), np.float32(0))
    for k, x in enumerate((-R, R, below, np.nan, np.inf, -np.inf)):
        at = 5 + 11 * k
        if at < n:
            p[at, 0], p[at, 1] = x, (-R if k == 0 else 1.5)                  # (the row at -R stands at -R in y too)
    p.setflags(write=False)
    return p


def box(p, flip=False):
    """the one-line box of plain float32 rows (loader_utils.py:182-187): numpy compares float32 with float32(radius)"""
    s, r = np.float32(-1 if flip else 1), np.float32(R)
    with np.errstate(invalid='ignore'):
        x, y = p[:, 0] * s, p[:, 1] * s
        return (x >= -r) & (x < r) & (y >= -r) & (y < r)


def radius_filter(p_dev, n, pre=None, flip=False):
    C = _C()
    L = C.lib()
    keep, count = Framed(n), torch.full((1,), SENTINEL, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.efgh_prep_filter_blocks(i32(n)), dtype=torch.int32, device='cuda')
    C.check(L.efgh_prep_radius_filter(C.ptr(p_dev), C.ptr(pre), i32(n), i32(1 if flip else 0), f32(R), C.ptr(scratch), keep.ptr,
                                      C.ptr(count), C.stream_ptr()))
    return keep.kept(int(count.item()))


class Set(object):
    """a sweep set staged by hand: packed rows, offsets, [K][3][4] matrices, identity flags -> the leading C arguments"""

    def __init__(self, sweeps, Ms=()):
        C = _C()
        self.K, self.stride = len(sweeps), sweeps[0].shape[1]
        self.pts = dev(np.concatenate(sweeps, axis=0))
        self.n_total = int(self.pts.shape[0])
        off = np.zeros(self.K + 1, np.int32)
        off[1:] = np.cumsum([s.shape[0] for s in sweeps])
        M = np.stack([np.eye(4)[:3]] + [np.asarray(m, np.float64)[:3] for m in Ms])
        ident = np.zeros(self.K, np.int32)
        ident[0] = 1
        self.off, self.M, self.ident = dev(off), dev(M), dev(ident)
        self.args = (C.ptr(self.pts), i32(self.stride), C.ptr(self.off), C.ptr(self.M), C.ptr(self.ident), i32(self.K),
                     i32(self.n_total))


def sweeps_filter(ss, n, pre=None, flip=False, ego=None):
    C = _C()
    L = C.lib()
    keep, count = Framed(n), torch.full((1,), SENTINEL, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.efgh_prep_filter_blocks(i32(n)), dtype=torch.int32, device='cuda')
    ex, ey = ego if ego is not None else (0., 0.)
    C.check(L.efgh_prep_sweeps_filter(*ss.args, C.ptr(pre), i32(n), i32(1 if flip else 0), f64(R), f32(ex), f32(ey), C.ptr(scratch),
                                      keep.ptr, C.ptr(count), C.stream_ptr()))
    return keep.kept(int(count.item()))


@pytest.mark.parametrize('n', SIZES)
def test_radius_filter_of_plain_rows(n):
    p = mix(n)
    p_dev = dev(p)
    want = np.flatnonzero(box(p)).astype(np.int32)
    if n > 5 + 11 * 5:                                                       # every planted row is in, and decided as stated
        assert np.isin([5, 27], want).all() and not np.isin([16, 38, 49, 60], want).any()
    assert np.array_equal(radius_filter(p_dev, n), want)
    assert np.array_equal(radius_filter(p_dev, n, flip=True), np.flatnonzero(box(p, flip=True)))
    pre = np.random.default_rng(n).permutation(n).astype(np.int32)           # candidates in another order: the kept SOURCE rows
    assert np.array_equal(radius_filter(p_dev, n, pre=dev(pre)), pre[box(p[pre])])
    every = p.copy()
    every[:, :2] = np.clip(np.nan_to_num(every[:, :2], nan=0., posinf=0., neginf=0.) * 0.5, -R / 2, R / 2)
    assert np.array_equal(radius_filter(dev(every), n), np.arange(n))
    none = p.copy()
    none[:, 0] = 2 * R
    assert radius_filter(dev(none), n).size == 0


@pytest.mark.parametrize('n', SIZES)
def test_sweeps_filter_one_identity_sweep(n):
    p = mix(n)
    for flip in (False, True):
        want = SC.chain([p], [], np.eye(4), n, radius=R, flip_xy=flip)['keep']
        assert np.array_equal(want, np.flatnonzero(box(p, flip)))            # the two contracts agree on one float32 sweep
        assert np.array_equal(sweeps_filter(Set([p]), n, flip=flip), want)
    every = p.copy()
    every[:, :2] = np.clip(np.nan_to_num(every[:, :2], nan=0., posinf=0., neginf=0.) * 0.5, -R / 2, R / 2)
    assert np.array_equal(sweeps_filter(Set([every]), n), np.arange(n))
    none = p.copy()
    none[:, 0] = 2 * R
    assert sweeps_filter(Set([none]), n).size == 0


def three_sweeps(n):
    """own sweep (the planted rows live here: identity, nothing is rounded), an EMPTY sweep, and a third sweep under a rigid transform
    whose positions keep clear of +-R by more than the contract's bound on them; a few rows inside the ego box everywhere"""
    n3 = n // 3
    own = mix(n)[:n - n3].copy()
    third = mix(n + 1)[:n3].copy()
    M = VC.rigid(2)
    M[:3, 3] = (1.1, -0.2, 0.03)
    own[3::7, :2] *= np.float32(0.01)                                        # |x| < 0.8 and |y| < 2.7: inside the ego box
    third[3::7, :2] *= np.float32(0.01)
    third[~np.isfinite(third).all(axis=1), :2] = (3.0, 4.0)                  # (the planted NaN and inf stay with the own sweep)
    q = SC.positions([own[:1], third], [M])[0][1:]
    third[(np.abs(np.abs(q[:, :2]) - R) <= 1e-6).any(axis=1), :2] = (3.0, 4.0)     # (1e-6 is far above the bound, ~1e-14 here)
    return [own, np.zeros((0, 4), np.float32), third], [np.eye(4), M]


@pytest.mark.parametrize('n', SIZES)
def test_sweeps_filter_three_sweeps_with_an_ego_box(n):
    sweeps, Ms = three_sweeps(n)
    q, b1, _ = SC.positions(sweeps, Ms)
    n_own = sweeps[0].shape[0]
    with np.errstate(invalid='ignore'):
        clear = np.abs(np.abs(q[n_own:, :2]) - R) > b1[n_own:, :2]
    assert clear.all() and sum(s.shape[0] for s in sweeps) == n              # no rounding of a transformed position decides
    want = SC.chain(sweeps, Ms, np.eye(4), n, ego_box=EGO, radius=R)['keep']
    if n >= 255:
        assert 0 < want.size < n and (want >= n_own).any()
    assert np.array_equal(sweeps_filter(Set(sweeps, Ms), n, ego=EGO), want)


@pytest.mark.parametrize('n', SIZES)
def test_voxel_keep_with_a_keep_list_and_a_device_count(n):
    C = _C()
    L = C.lib()
    v = 0.25
    rng = np.random.default_rng(200 + n)
    side = max(1, int(round((n / 12.8) ** (1 / 3.0))))                       # (2 side)^3 ~ n / 1.6 voxels: about half the rows are firsts
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = VC.centre(rng.integers(-side, side, (n, 3)), v)               # voxel centres: exact in float32, far from every face
    for k, x in enumerate((np.nan, np.inf, -np.inf)):
        if 7 + 13 * k < n:
            p[7 + 13 * k, k] = x                                             # unrepresentable: kept alone
    keep_in = rng.permutation(n).astype(np.int32)
    n_dev = n - (n + 4) // 5                                                 # fewer candidates on the device than the capacity
    assert n_dev < n
    cand = keep_in[:n_dev]
    want = cand[VC.keep(p[cand, :3].astype(np.float64), v)] if n_dev else cand
    out, counts = Framed(n), torch.full((2,), SENTINEL, dtype=torch.int32, device='cuda')
    ws = torch.empty(L.efgh_prep_voxel_workspace(i32(n)), dtype=torch.uint8, device='cuda')
    p_dev, k_dev, nd = dev(p), dev(keep_in), dev(np.array([n_dev], np.int32))
    C.check(L.efgh_prep_voxel_keep(C.ptr(p_dev), i32(4), i32(n), C.ptr(k_dev), i32(n), C.ptr(nd), f64(v), C.ptr(ws), out.ptr,
                                   C.ptr(counts), C.stream_ptr()))
    count, exhausted = (int(c) for c in counts.cpu())
    assert exhausted == 0
    assert np.array_equal(out.kept(count), want)
    if n >= 255:
        assert 0.2 * n_dev < count < 0.8 * n_dev


@pytest.mark.parametrize('n', SIZES)
def test_plain_rows_equal_a_one_identity_sweep_set(n):
    from efgh_amd.data import preproc_gt
    C = _C()
    L = C.lib()
    p = mix(n)
    p_dev, ss = dev(p), Set([p])
    T = dev(np.ascontiguousarray(preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)['rand_init_l'][:3]))
    for flip in (False, True):
        a, b = radius_filter(p_dev, n, flip=flip), sweeps_filter(ss, n, flip=flip)
        assert np.array_equal(a, b)
        n_keep = int(a.size)
        n_sel = min(n_keep, 4096)
        num_points = n_sel + 37                                              # the zero-pad columns are compared too
        keep = dev(a) if n_keep else torch.zeros(1, dtype=torch.int32, device='cuda')
        sel = dev(np.random.default_rng(n).permutation(n_keep)[:n_sel].astype(np.int32)) if n_sel else None
        outs = []
        for kind in ('plain', 'sweeps'):
            o32 = torch.full((3, num_points), float('nan'), dtype=torch.float32, device='cuda')
            o64 = torch.full((3, num_points), float('nan'), dtype=torch.float64, device='cuda')
            tail = (C.ptr(sel), i32(n_sel), i32(1 if flip else 0), C.ptr(T), i32(num_points), C.ptr(o32), C.ptr(o64), C.stream_ptr())
            if kind == 'plain':
                C.check(L.efgh_prep_gather_transform(C.ptr(p_dev), C.ptr(keep), *tail))
            else:
                C.check(L.efgh_prep_sweeps_gather_transform(*ss.args, C.ptr(keep), i32(n_keep), *tail))
            outs.append((o32.cpu().numpy(), o64.cpu().numpy()))
        (a32, a64), (b32, b64) = outs
        assert np.isfinite(a64).all()
        assert np.array_equal(a32.view(np.int32), b32.view(np.int32)) and np.array_equal(a64.view(np.int64), b64.view(np.int64))
        assert np.array_equal(a32.view(np.int32), a64.astype(np.float32).view(np.int32))
        pad = T.cpu().numpy()[:, 3:4]
        assert np.array_equal(a64[:, n_sel:], np.broadcast_to(pad, (3, 37)))
