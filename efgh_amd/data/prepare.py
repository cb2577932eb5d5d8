"""GPU-side sample preparation: drop-in for the reference's `ProcessKITTIODOM` /
`ProcessRELLIS` / `ProcessKITTIRAW` / `ProcessNUSC` callables (data_loader/kitti_odom_loader.py:237-273,
rellis3d_loader.py:292-339, kitti_raw_loader.py:227-263, nusc_loader.py:227-262), the `preproc_*` helpers they call
(data_loader/loader_utils.py:63-202), and the loaders' multi-sweep accumulation as a `SweepSet` the point kernels read
without ever building the accumulated float64 cloud.

Same constructor (`args` dict), same `__call__(pcd, img, calibs, posej_T_posei, fname, rand_init=None)` and the same
return tuple `(pc[:3], img, calib, A, gts, fname)` — but the pixel and point work runs in libefgh_hip.so
(csrc/prep.hip) and the results are CUDA tensors (no CPU fallback).  Host code keeps what is O(1) per sample: the random
mis-calibration draw, 4x4 matrix algebra in float64, and the geometry of the two Pillow operations
(`Image.rotate(expand=True)` -> 16.16 affine coefficients, `Image.resize` BICUBIC -> integer coefficient tables),
restated from Pillow's published algorithm so that the kernels reproduce its pixels exactly.

One deliberate difference: the reference sub-samples with `np.random.choice(..., replace=False)` (numpy's global
Mersenne stream).  Here the subset is `sampled_indices` when given (parity tests pass the reference's draw) and a
`torch.randperm` on the device otherwise.
"""
import ctypes
import math
import random
from math import cos, pi, sin

import numpy as np
import torch

from .. import _C
from .._C import ptr


def _L():
    return _C.lib()


def _st():
    return _C.stream_ptr()


# ------------------------------------------------------------------------------------------------
# host-side O(1) pieces
# ------------------------------------------------------------------------------------------------
def rand_init_params(rand_init, rpy_range, xyz_range, t_range):
    """loader_utils.py:63-79 (python `random`, 7 draws in this order)"""
    if rand_init is not None:
        return tuple(rand_init)
    if rpy_range is None or xyz_range is None or t_range is None:
        raise ValueError('rand_init_params: neither rand_init nor the ranges are given')
    rr = (random.random() * 2. - 1.) * pi * rpy_range
    rp = (random.random() * 2. - 1.) * pi * rpy_range
    ry = (random.random() * 2. - 1.) * pi * rpy_range
    tx = (random.random() * 2. - 1.) * xyz_range
    ty = (random.random() * 2. - 1.) * xyz_range
    tz = (random.random() * 2. - 1.) * xyz_range
    rt = (random.random() * 2. - 1.) * pi * t_range
    return rr, rp, ry, tx, ty, tz, rt


def _rpy(roll, pitch, yaw):            # numpy_utils.py:519-548
    ym = np.array([[cos(yaw), -sin(yaw), 0], [sin(yaw), cos(yaw), 0], [0, 0, 1]])
    pm = np.array([[cos(pitch), 0, sin(pitch)], [0, 1, 0], [-sin(pitch), 0, cos(pitch)]])
    rm = np.array([[1, 0, 0], [0, cos(roll), -sin(roll)], [0, sin(roll), cos(roll)]])
    R4 = np.eye(4)
    R4[:3, :3] = ym @ pm @ rm
    return R4


def preproc_gt(rr, rp, ry, tx, ty, tz, rt, posej_T_posei=np.eye(4)):
    """loader_utils.py:81-102 (float64 on the host)"""
    ltrs = np.eye(4)
    ltrs[:3, 3] = (tx, ty, tz)
    rand_init_l = np.array(_rpy(rr, rp, ry) @ ltrs)
    rand_init_c = np.array([[cos(rt), -sin(rt), 0], [sin(rt), cos(rt), 0], [0, 0, 1]])
    return {'rand_init_l': rand_init_l, 'rand_init_c': rand_init_c,
            'sensor2_T_sensor1': posej_T_posei @ np.linalg.inv(rand_init_l),
            'intrinsic_sensor2': np.array(np.linalg.inv(rand_init_c))}


def _fix16(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_plan(w, h, angle_deg):
    """Pillow `Image.rotate(angle, expand=True)` NEAREST: ((nw, nh), six 16.16 coefficients) of the destination->source map
    (Image.py:rotate, Geometry.c:affine_fixed); the 0/90/180/270 fast paths are the same map with exact coefficients."""
    angle = angle_deg % 360.0
    one, half = 65536, 32768
    if angle == 0:
        return (w, h), (one, 0, half, 0, one, half)
    if angle == 180:
        return (w, h), (-one, 0, (w - 1) * one + half, 0, -one, (h - 1) * one + half)
    if angle == 90:                      # counter-clockwise: out[y][x] = in[x][w-1-y]
        return (h, w), (0, -one, (w - 1) * one + half, one, 0, half)
    if angle == 270:                     # out[y][x] = in[h-1-x][y]
        return (h, w), (0, one, half, -one, 0, (h - 1) * one + half)
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tf(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    cx, cy = w / 2, h / 2
    m[2], m[5] = tf(-cx, -cy)
    m[2] += cx
    m[5] += cy
    xx, yy = zip(*[tf(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))])
    nw = math.ceil(max(xx)) - math.floor(min(xx))
    nh = math.ceil(max(yy)) - math.floor(min(yy))
    m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return (nw, nh), (_fix16(m[0]), _fix16(m[1]), _fix16(m[2] + m[0] * 0.5 + m[1] * 0.5),
                      _fix16(m[3]), _fix16(m[4]), _fix16(m[5] + m[3] * 0.5 + m[4] * 0.5))


_COEFF_CACHE = {}


def resample_tables(in_size, out_size, device):
    """Pillow Resample.c:precompute_coeffs + normalize_coeffs_8bpc (bicubic, a = -0.5, 22 fractional bits)"""
    key = (in_size, out_size, str(device))
    hit = _COEFF_CACHE.get(key)
    if hit is not None:
        return hit
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)

    def bicubic(x):
        x = abs(x)
        if x < 1.0:
            return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * -0.5
        return 0.0

    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax)
    val = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    _COEFF_CACHE[key] = val
    return val


# ------------------------------------------------------------------------------------------------
# device ops (uint8 (H,W,3) images)
# ------------------------------------------------------------------------------------------------
def _as_dev_u8(img, device):
    t = torch.as_tensor(np.ascontiguousarray(img)) if not torch.is_tensor(img) else img
    if t.dim() == 3 and t.shape[2] != 3:                 # (3,H,W) -> (H,W,3), as the reference helpers accept
        t = t.permute(1, 2, 0)
    t = t.to(device=device, dtype=torch.uint8).contiguous()
    _C.require_cuda(t)
    return t


def rotate_expand(img, angle_deg):
    h, w = img.shape[:2]
    (nw, nh), coef = rotate_plan(w, h, float(angle_deg))
    out = torch.empty((nh, nw, 3), dtype=torch.uint8, device=img.device)
    c6 = (ctypes.c_int64 * 6)(*coef)
    _C.check(_L().efgh_prep_affine_nearest_u8(ptr(img), h, w, c6, ptr(out), nh, nw, _st()))
    return out


def crop_image(img, target_hw, init=False):
    """numpy_utils.py:447-472 (zero pad up to the target, then crop: centred, or from the origin when `init`)"""
    h, w = img.shape[:2]
    th, tw = int(target_hw[0]), int(target_hw[1])
    ph, pw = max(h, th), max(w, tw)
    i0, j0 = int(math.floor((ph - h) / 2.)), int(math.floor((pw - w) / 2.))
    i, j = (0, 0) if init else (int(math.floor((ph - th) / 2.)), int(math.floor((pw - tw) / 2.)))
    out = torch.empty((th, tw, 3), dtype=torch.uint8, device=img.device)
    _C.check(_L().efgh_prep_crop_pad_u8(ptr(img), h, w, i - i0, j - j0, ptr(out), th, tw, _st()))
    return out


def resize_image(img, target_hw):
    """numpy_utils.py:474-486: `Image.resize((W, H))`, default BICUBIC with antialiasing, two 8-bit passes"""
    th, tw = int(target_hw[0]), int(target_hw[1])
    cur = img
    for axis, size in ((1, tw), (0, th)):                # horizontal pass first, as Pillow does
        h, w = cur.shape[:2]
        if size == (w if axis else h):
            continue
        bounds, kk, ksize = resample_tables(w if axis else h, size, img.device)
        out = torch.empty((h, size, 3) if axis else (size, w, 3), dtype=torch.uint8, device=img.device)
        _C.check(_L().efgh_prep_resample_u8(ptr(cur), h, w, axis, size, ptr(bounds), ptr(kk), ksize, ptr(out), _st()))
        cur = out
    return cur.clone() if cur is img else cur


def _chw_and_mask(img, want_chw=True, want_mask=False):
    h, w = img.shape[:2]
    chw = torch.empty((3, h, w), dtype=torch.uint8, device=img.device) if want_chw else None
    mask = torch.empty((1, h, w), dtype=torch.uint8, device=img.device) if want_mask else None
    _C.check(_L().efgh_prep_hwc_to_chw_u8(ptr(img), h, w, ptr(chw), ptr(mask), _st()))
    return chw, mask


# ------------------------------------------------------------------------------------------------
# photometric jitter (not in the reference): torchvision's ColorJitter on PIL images, byte for byte (csrc/jitter.hip)
# ------------------------------------------------------------------------------------------------
JITTER_OPS = ('brightness', 'contrast', 'saturation', 'hue')          # EFGH_JITTER_* of include/efgh_hip.h, in this order


class JitterParams(object):
    """One drawn jitter, for `color_jitter` / `preproc_img(jitter=...)`, for tests and for replay.
    order      the op names (of JITTER_OPS, each at most once) in the order they are applied
    factors    one float per op: the blend factor of brightness / contrast / saturation (>= 0), the hue value in [-0.5, 0.5]
    hue_shift  what is added to H (mod 256): int(hue * 255), truncated toward zero; 0 without hue"""
    __slots__ = ('order', 'factors', 'hue_shift')

    def __init__(self, order=(), factors=()):
        order, factors = tuple(order), tuple(factors)
        if len(order) != len(factors):
            raise _C.EfghError('JitterParams: %d ops with %d factors' % (len(order), len(factors)))
        for op in order:
            if op not in JITTER_OPS or order.count(op) != 1:
                raise _C.EfghError('JitterParams: op %r is not one of %s, or appears twice' % (op, ', '.join(JITTER_OPS)))
        self.order, self.factors, self.hue_shift = order, tuple(_jitter_value(op, f) for op, f in zip(order, factors)), 0
        if 'hue' in order:
            self.hue_shift = int(self.factors[order.index('hue')] * 255)

    def __repr__(self):
        return 'JitterParams(order=%r, factors=%r)' % (self.order, self.factors)


def _jitter_value(op, f):
    try:
        v = float(f)
    except (TypeError, ValueError):
        raise _C.EfghError('%s: expected a number, got %r' % (op, f))
    ok = -0.5 <= v <= 0.5 if op == 'hue' else (v >= 0. and math.isfinite(v))
    if not ok:
        raise _C.EfghError('%s: %r is outside %s' % (op, f, '[-0.5, 0.5]' if op == 'hue' else '[0, inf)'))
    return v


class ColorJitter(object):
    """torchvision's `ColorJitter(brightness, contrast, saturation, hue)`: a float x is the range [max(0, 1 - x), 1 + x] (hue:
    [-x, x], 0 <= x <= 0.5), a pair is the range itself; a component that is 0 or None is left out.
    `.sample()` draws with Python's `random`, and the sequence of draws is part of the contract: with n ops present, first the order,
    a Fisher-Yates shuffle of the present ops taken in JITTER_OPS order (for i = n-1 down to 1: j = int(random.random() * (i + 1)),
    swap entries i and j), then one factor lo + (hi - lo) * random.random() per present op, in JITTER_OPS order.  No op: no draw."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.ranges = {}
        for op, v in zip(JITTER_OPS, (brightness, contrast, saturation, hue)):
            r = self._range(op, v)
            if r is not None:
                self.ranges[op] = r

    @staticmethod
    def _range(op, v):
        is_hue = op == 'hue'
        if v is None:
            return None
        if isinstance(v, (tuple, list)):
            if len(v) != 2:
                raise _C.EfghError('%s: a range is a pair (lo, hi), got %r' % (op, v))
            lo, hi = _jitter_value(op, v[0]), _jitter_value(op, v[1])
            if lo > hi:
                raise _C.EfghError('%s: the range %r is empty' % (op, v))
            return lo, hi
        x = _jitter_value(op, v)
        if x < 0.:
            raise _C.EfghError('%s: %r is negative (a single number x means the range [-x, x])' % (op, v))
        if x == 0.:
            return None
        return (-x, x) if is_hue else (max(0., 1. - x), 1. + x)

    def sample(self):
        order = [op for op in JITTER_OPS if op in self.ranges]
        present = list(order)
        for i in range(len(order) - 1, 0, -1):
            j = int(random.random() * (i + 1))
            order[i], order[j] = order[j], order[i]
        drawn = {}
        for op in present:
            lo, hi = self.ranges[op]
            drawn[op] = lo + (hi - lo) * random.random()
        return JitterParams(order, [drawn[op] for op in order])


def color_jitter(img, params, device='cuda'):
    """`params` (a JitterParams) applied to a uint8 RGB image, (H,W,3) or (3,H,W), array or tensor -> uint8 (H,W,3) on the device.
    Two launches at most (the sum of L for contrast's mean, then every op per pixel); the result is a new tensor, the input is
    never written.  With no ops nothing is launched and the image itself (on the device, (H,W,3)) is returned."""
    if not isinstance(params, JitterParams):
        raise _C.EfghError('color_jitter: params is a JitterParams (ColorJitter(...).sample()), got %r' % (params,))
    img = _as_dev_u8(img, device)
    n_ops = len(params.order)
    if n_ops == 0:
        return img
    if img.dim() != 3 or img.shape[2] != 3 or img.numel() == 0:
        raise _C.EfghError('color_jitter: image of shape %s, expected (H, W, 3) or (3, H, W), not empty' % (tuple(img.shape),))
    n = int(img.shape[0]) * int(img.shape[1])
    ops = (ctypes.c_int32 * n_ops)(*[JITTER_OPS.index(op) for op in params.order])
    fac = (ctypes.c_float * n_ops)(*params.factors)
    out = torch.empty_like(img)
    partials = None
    if 'contrast' in params.order:
        partials = torch.empty(_L().efgh_prep_jitter_partials(n), dtype=torch.int64, device=img.device)
        _C.check(_L().efgh_prep_jitter_sum(ptr(img), n, ops, fac, n_ops, params.hue_shift, ptr(partials), _st()))
    _C.check(_L().efgh_prep_jitter_apply(ptr(img), n, ops, fac, n_ops, params.hue_shift, ptr(partials), ptr(out), _st()))
    return out


def preproc_img(img, gts, raw_cam_img_size, rellis=False, device='cuda', jitter=None):
    """loader_utils.py:104-130 (KITTI) / :132-158 (`rellis=True`: the raw view is a resize, not a crop).
    `jitter` (not in the reference; None: off, and nothing runs differently): a JitterParams applied once to the decoded image, in
    front of the raw view, the rotation and the resize, so 'in', 'raw' and 'rot' agree and the borders stay black."""
    raw_hw = (int(raw_cam_img_size[0]), int(raw_cam_img_size[1]))
    img = _as_dev_u8(img, device)
    if jitter is not None:
        img = color_jitter(img, jitter, device)
    img_raw = resize_image(img, raw_hw) if rellis else crop_image(img, raw_hw, init=True)
    rc = gts['rand_init_c']
    rot_deg = math.degrees(np.arctan2(rc[1, 0], rc[0, 0]))                       # numpy_utils.py:436
    img_rot = crop_image(rotate_expand(img, rot_deg), raw_hw)
    half = (int(img_rot.shape[0] / 2), int(img_rot.shape[1] / 2))
    small = resize_image(img_rot, half)
    th, tw = int(raw_hw[0] / 2), int(raw_hw[1] / 2)
    img_in = torch.empty((3, th, tw), dtype=torch.float32, device=img.device)
    oy, ox = int(math.floor((th - half[0]) / 2.)), int(math.floor((tw - half[1]) / 2.))
    _C.check(_L().efgh_prep_u8_to_f32_chw_pad(ptr(small), half[0], half[1], oy, ox, ptr(img_in), th, tw, _st()))
    raw_chw, _ = _chw_and_mask(img_raw)
    rot_chw, mask = _chw_and_mask(img_rot, want_mask=True)
    return {'in': img_in, 'raw': raw_chw, 'rot': rot_chw, 'img_mask': mask}


def lidar_line_indices(n_points, reduce_to):
    """the index list of `reduce_lidar_line` (loader_utils.py:162-175) incl. its python negative indexing"""
    rate = 64 / reduce_to
    line_num = int(n_points / 64)
    lo, hi = int(-line_num / 2), int(line_num / 2)
    rows = np.array([i for i in range(64) if i % rate == 0], np.int64)
    idx = (rows[:, None] * line_num + np.arange(lo, hi, dtype=np.int64)[None, :]).reshape(-1)
    return np.where(idx < 0, idx + n_points, idx).astype(np.int32)


def _subsample(n_keep, num_points, sampled_indices, device):
    """loader_utils.py:189-196: num_points of the n_keep survivors without replacement -> (index tensor, num_points), or all of
    them (the caller zero-pads) -> (None, n_keep)"""
    if num_points >= n_keep:
        return None, n_keep
    if sampled_indices is None:
        sel = torch.randperm(n_keep, device=device)[:num_points].to(torch.int32)
    else:
        sel = torch.as_tensor(np.asarray(sampled_indices)).to(device=device, dtype=torch.int32)
        assert sel.numel() == num_points
    return sel, num_points


# ------------------------------------------------------------------------------------------------
# thinning on a voxel grid (efgh_prep_voxel_keep / efgh_prep_sweeps_voxel_keep, csrc/prep.hip)
# ------------------------------------------------------------------------------------------------
def _check_voxel_size(voxel_size):
    try:
        v = float(voxel_size)
    except (TypeError, ValueError):
        raise _C.EfghError('voxel_size: expected a positive finite edge length, got %r' % (voxel_size,))
    if not (v > 0. and math.isfinite(v)):
        raise _C.EfghError('voxel_size: expected a positive finite edge length, got %r' % (voxel_size,))
    return v


def _read_counts(counts):
    """the one host read of a thinned sample: (kept count, table-exhausted flag)"""
    return [int(c) for c in counts.cpu()]


def _upload_T(gts, device, wait=True):
    """rows 0..2 of rand_init_l as float64 on the device.  `wait=False` stages through pinned memory and copies asynchronously, so
    the thinning path waits for the device once per sample, at `_read_counts`"""
    T = torch.from_numpy(np.ascontiguousarray(np.asarray(gts['rand_init_l'], np.float64)[:3, :]))
    return T.to(device) if wait else T.pin_memory().to(device, non_blocking=True)


class _Rows(object):
    """What the point chain runs over, for the three steps that read points: a SweepSet, or a resident [rows, 3 | 4] float32 tensor.
    `pts` the points on the device, `rows` their number, `set` the SweepSet or None, and per step (filter, thin, gather) the name of the
    entry point with the C arguments that describe the points to it."""

    def __init__(self, src, device=None):
        if isinstance(src, SweepSet):
            self.set, self.rows = src, src.n_total
            self.pts, a = src._args(device)
            self.filter, self.thin, self.gather = (('efgh_prep_sweeps_' + step, a) for step in ('filter', 'voxel_keep', 'gather_transform'))
        else:
            self.set, self.pts, self.rows = None, src, int(src.shape[0])
            self.filter, self.gather = ('efgh_prep_radius_filter', (ptr(src),)), ('efgh_prep_gather_transform', (ptr(src),))
            self.thin = ('efgh_prep_voxel_keep', (ptr(src), int(src.shape[1]), self.rows))
        self.device = self.pts.device

    def call(self, step, *args):
        name, lead = step
        _C.check(getattr(_L(), name)(*lead, *args, _st()))


def _voxel_thin(src, keep, n, n_dev, voxel_size):
    """of the candidates keep[0 .. n) (None: rows 0 .. n-1; `n_dev`: their count on the device, None: n) the first row of every
    occupied voxel, in order -> (int32 tensor, count).  `src` is a _Rows."""
    v = _check_voxel_size(voxel_size)
    nbytes = _L().efgh_prep_voxel_workspace(n)
    if nbytes < 0:
        raise _C.EfghError('voxel thinning: %d candidate rows, supported are fewer than 2^29' % n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    out = torch.empty(n, dtype=torch.int32, device=src.device)
    counts = torch.empty(2, dtype=torch.int32, device=src.device)
    src.call(src.thin, ptr(keep), n, ptr(n_dev), v, ptr(ws), ptr(out), ptr(counts))
    n_keep, exhausted = _read_counts(counts)
    if exhausted:
        raise _C.EfghError('voxel thinning: the hash table of %d candidate rows ran out of slots (a bug: it is sized at load <= 0.5)' % n)
    return out, n_keep


def voxel_keep(points, voxel_size, keep=None, device='cuda'):
    """Thin a cloud on a voxel grid of edge `voxel_size`: the rows whose voxel no earlier row occupies (first seen wins, so the own
    sweep of a SweepSet wins over its neighbours), ascending, int32 on the device.  A row with a NaN or inf coordinate, or more than
    2^20 voxels from the origin, is kept alone.  `points` is a SweepSet (rows of its concatenation, positions in the own sweep's
    frame) or a [n, 3 | 4] float32 array or tensor; `keep` optionally restricts and orders the candidates (e.g.
    `SweepSet.kept_indices()`).  The representative is an input row, so per-point data can be carried through the indices."""
    _check_voxel_size(voxel_size)
    if isinstance(points, SweepSet):
        src = _Rows(points, device)
    else:
        p = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32)) if not torch.is_tensor(points) else points
        if p.dim() != 2 or p.shape[1] not in (3, 4) or p.shape[0] < 1:
            raise _C.EfghError('voxel_keep: points has shape %s, expected [n, 3] or [n, 4] with n >= 1' % (tuple(p.shape),))
        p = p.to(device=device, dtype=torch.float32).contiguous()
        _C.require_cuda(p)
        src = _Rows(p)
    rows = src.rows
    if keep is not None:
        keep = torch.as_tensor(np.asarray(keep)) if not torch.is_tensor(keep) else keep
        if keep.dim() != 1 or keep.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
            raise _C.EfghError('voxel_keep: keep is a 1-D integer index list, got %s of shape %s' % (keep.dtype, tuple(keep.shape)))
        keep = keep.to(device=src.device, dtype=torch.int32).contiguous()
        rows = int(keep.numel())
        if rows == 0:
            return keep
    out, n_keep = _voxel_thin(src, keep, rows, None, voxel_size)
    return out[:n_keep]


# ------------------------------------------------------------------------------------------------
# multi-sweep accumulation: host helpers (float64, the reference's product order) and the sweep set
# ------------------------------------------------------------------------------------------------
SWEEPS_MAX = 64          # K of efgh_prep_sweeps_* (include/efgh_hip.h)


def accumulation_indices(seq_i, n_frames, num, skip):
    """`search_for_accumulation` (kitti_odom_loader.py:160-190, rellis3d_loader.py:218-245) as index lists: up to `num` frames
    seq_i -/+ skip*c, c = 1, 2, ..., stopping at the first one past either end of the sequence.  Returns (prev, next)."""
    def walk(stride):
        out, counter = [], 0
        while len(out) < num:
            counter += 1
            seq_j = seq_i + stride * counter
            if seq_j < 0 or seq_j >= n_frames:
                break
            out.append(seq_j)
        return out
    return walk(-skip), walk(skip)


def accumulation_transform(P_oi, P_oj, Tr=None):
    """sweep j -> frame of sweep i: `inv(P_oi) @ P_oj` (rellis3d_loader.py:220,237); with the KITTI calibration `Tr`,
    `Tr_inv @ P_ij @ Tr` evaluated left to right as kitti_odom_loader.py:185 does (Tr_inv = inv(Tr), loader_utils.py:46)"""
    P_ij = np.linalg.inv(P_oi) @ P_oj
    if Tr is None:
        return P_ij
    return np.linalg.inv(Tr) @ P_ij @ Tr


def nusc_accumulation_transform(P_io, P_oj, P_lidar_vehicle, P_vehicle_lidar):
    """nusc_loader.py:113-114"""
    P_ij = np.dot(P_io, P_oj)
    return np.dot(np.dot(P_lidar_vehicle, P_ij), P_vehicle_lidar)


def nusc_walk(record, get, direction, num, skip):
    """the `counter % skip` walk of `lidar_frame_accumulation` (nusc_loader.py:99-123) along record[direction] ('next' or
    'prev') with `get(token)` in place of `nusc.get('sample_data', token)`: the tokens whose sweeps are accumulated, in order"""
    out, counter, lidar = [], 1, record
    while len(out) < num:
        if lidar[direction] == '':
            break
        if counter % skip != 0:
            counter += 1
            lidar = get(lidar[direction])
            continue
        out.append(lidar[direction])
        counter += 1
        lidar = get(lidar[direction])
    return out


class SweepSet(object):
    """The own sweep plus neighbouring sweeps, each with the 4x4 float64 transform into the own sweep's frame: what the
    reference's `get_accumulated_pc` / `accumulate_lidar_points` concatenate into one float64 cloud, kept as the float32
    sweeps it was read from.  `preproc_pcd` and the Process classes take it in place of an array; the kernels compute the
    float64 positions on the fly (csrc/prep.hip), so the accumulated cloud is never built unless `.accumulated()` asks.

    sweeps      [n_k, 3 | 4] float32 arrays or tensors (one column count for all), the own sweep first; n_k = 0 is allowed
                for every sweep but the own one
    transforms  one 4x4 float64 matrix per further sweep (`accumulation_transform`, `nusc_accumulation_transform`)
    own_order   optional permutation of the own sweep (the reference shuffles it, kitti_odom_loader.py:197)
    ego_box     (x_half, y_half): drop what lies strictly inside, per sweep, before the transform (nusc_loader.py:88-93
                uses (0.8, 2.7))
    Uploads happen once, at the first use: the packed points, and one buffer with offsets, matrices and flags."""

    def __init__(self, sweeps, transforms=None, own_order=None, ego_box=None):
        sweeps = list(sweeps)
        transforms = [] if transforms is None else list(transforms)
        if not 1 <= len(sweeps) <= SWEEPS_MAX:
            raise _C.EfghError('SweepSet: %d sweeps, supported are 1 .. %d' % (len(sweeps), SWEEPS_MAX))
        if len(transforms) != len(sweeps) - 1:
            raise _C.EfghError('SweepSet: %d sweeps need %d transforms (none for the own sweep), got %d'
                               % (len(sweeps), len(sweeps) - 1, len(transforms)))
        self._sweeps = []
        for k, sw in enumerate(sweeps):
            if not torch.is_tensor(sw):
                sw = np.ascontiguousarray(sw, dtype=np.float32)
            if sw.ndim != 2 or sw.shape[1] not in (3, 4) or (self._sweeps and sw.shape[1] != self._sweeps[0].shape[1]):
                raise _C.EfghError('SweepSet: sweep %d has shape %s, expected [n, 3] or [n, 4] with one column count for all'
                                   % (k, tuple(sw.shape)))
            self._sweeps.append(sw)
        self.lengths = [int(sw.shape[0]) for sw in self._sweeps]
        self.stride = int(self._sweeps[0].shape[1])
        self.K = len(sweeps)
        self.n_total = sum(self.lengths)
        if self.lengths[0] < 1:
            raise _C.EfghError('SweepSet: the own sweep is empty')
        if self.n_total >= 1 << 29:
            raise _C.EfghError('SweepSet: %d points, supported are fewer than 2^29' % self.n_total)
        self.M = np.zeros((self.K, 3, 4), np.float64)
        self.M[0] = np.eye(4)[:3]
        for k, T in enumerate(transforms):
            T = np.asarray(T, np.float64)
            if T.shape != (4, 4):
                raise _C.EfghError('SweepSet: transform %d has shape %s, expected (4, 4)' % (k, T.shape))
            self.M[k + 1] = T[:3]
        self.own_order = None
        if own_order is not None:
            order = np.asarray(own_order, np.int64)
            if order.shape != (self.lengths[0],) or not np.array_equal(np.sort(order), np.arange(self.lengths[0])):
                raise _C.EfghError('SweepSet: own_order is not a permutation of the own sweep')
            self.own_order = order
        self.ego_box = None
        if ego_box is not None:
            self.ego_box = (float(ego_box[0]), float(ego_box[1]))
            if not (self.ego_box[0] > 0. and self.ego_box[1] > 0.):
                raise _C.EfghError('SweepSet: ego_box is (x_half, y_half), both positive')
        self._staged = None

    def _stage(self, device):
        """(points tensor, descriptor tensor, pointers of offsets / matrices / flags) on `device`"""
        device = torch.device(device)
        if self._staged is not None and self._staged[0] == device:
            return self._staged[1]
        sweeps = list(self._sweeps)
        if not any(torch.is_tensor(sw) for sw in sweeps):
            if self.own_order is not None:
                sweeps[0] = sweeps[0][self.own_order]
            pts = torch.from_numpy(np.concatenate(sweeps, axis=0) if self.K > 1 else np.ascontiguousarray(sweeps[0]))
            pts = pts.to(device)
        else:
            sweeps = [torch.as_tensor(sw).to(device=device, dtype=torch.float32) for sw in sweeps]
            if self.own_order is not None:
                sweeps[0] = sweeps[0][torch.from_numpy(self.own_order).to(device)]
            pts = (torch.cat(sweeps, dim=0) if self.K > 1 else sweeps[0]).contiguous()
        _C.require_cuda(pts)
        off = np.zeros(self.K + 1, np.int32)
        off[1:] = np.cumsum(self.lengths)
        ident = np.zeros(self.K, np.int32)
        ident[0] = 1
        desc = torch.from_numpy(np.frombuffer(self.M.tobytes() + off.tobytes() + ident.tobytes(), np.uint8).copy()).to(device)
        base = desc.data_ptr()
        st = (pts, desc, _C.c_void_p(base + 96 * self.K), _C.c_void_p(base), _C.c_void_p(base + 96 * self.K + 4 * (self.K + 1)))
        self._staged = (device, st)
        return st

    def _args(self, device):
        pts, _, off, M, ident = self._stage(device)
        return pts, (ptr(pts), self.stride, off, M, ident, self.K, self.n_total)

    def kept_indices(self, radius=50., lidar_line=None, flip_xy=False, device='cuda', voxel_size=None):
        """rows of the concatenation (own sweep first, before the ego box) that `preproc_pcd` keeps, in its order: int32 on
        the device.  For carrying per-point data (intensity, labels) through the same selection.  `voxel_size`: thinned on
        that grid after the ego box and the radius (`voxel_keep`)."""
        _, keep, n_keep = _keep_rows(self, device, lidar_line, radius, flip_xy, voxel_size)
        return keep[:n_keep]

    def accumulated(self, device='cuda'):
        """the accumulated cloud itself, [n, 3] float64 on the device: what `get_accumulated_pc` (kitti_odom_loader.py:192-225)
        returns, or `accumulate_lidar_points(...)[:3].T` with the ego box (nusc_loader.py:126-146,156)"""
        pts, a = self._args(device)
        keep, n = None, self.n_total
        if self.ego_box is not None:
            keep, count = _filter(_Rows(self, device), None, n, False, None)
            n = int(count.item())
        out = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
        if n > 0:
            _C.check(_L().efgh_prep_sweeps_materialize(*a, ptr(keep), n, ptr(out), _st()))
        return out


def _filter(src, pre, n, flip_xy, radius):
    """stable compaction of the candidates pre[0 .. n) (None: rows 0 .. n-1) of a _Rows by ego box and radius
    -> (keep [n] int32, count [1] int32)"""
    keep = torch.empty(n, dtype=torch.int32, device=src.device)
    count = torch.zeros(1, dtype=torch.int32, device=src.device)
    scratch = torch.empty(_L().efgh_prep_filter_blocks(n), dtype=torch.int32, device=src.device)
    if src.set is None:
        box = (radius,)
    else:
        ex, ey = src.set.ego_box if src.set.ego_box is not None else (0., 0.)
        box = (0. if radius is None else radius, ex, ey)
    src.call(src.filter, ptr(pre), n, 1 if flip_xy else 0, *box, ptr(scratch), ptr(keep), ptr(count))
    return keep, count


def _keep_rows(points, device, lidar_line, radius, flip_xy, voxel_size=None):
    """(lidar-line reduction,) ego box and radius filter (and voxel thinning) of a SweepSet or a resident [n, 4] tensor
    -> (its _Rows, keep int32 tensor, n_keep)"""
    if voxel_size is not None:
        _check_voxel_size(voxel_size)
    ego = isinstance(points, SweepSet) and points.ego_box is not None
    if lidar_line is not None and ego:
        raise _C.EfghError('preproc_pcd: lidar_line with an ego_box is not supported: the line reduction indexes the '
                           'concatenated cloud, whose length after the ego box is known on the device only')
    src = _Rows(points, device)                          # (a sweep set is uploaded here, at its first use)
    n, keep, count = src.rows, None, None
    if lidar_line is not None:
        idx = lidar_line_indices(n, lidar_line)
        if idx.size == 0:
            raise _C.EfghError('preproc_pcd: lidar_line on %d points leaves none' % n)
        keep = torch.from_numpy(idx).to(src.device)
        n = int(keep.numel())
    if radius is not None or ego:
        # float32 rows alone (an array, or an all-identity set) stay float32 in the reference, where numpy compares with float32(radius)
        r = radius if radius is None or (src.set is not None and src.set.K > 1) else float(np.float32(radius))
        keep, count = _filter(src, keep, n, flip_xy, r)
    if voxel_size is not None:                           # the filter's count stays on the device: the thinning reads it there
        keep, n = _voxel_thin(src, keep, n, count, voxel_size)
    elif count is not None:
        n = int(count.item())                            # one host read per sample: the caller's branch depends on it
    elif keep is None:
        keep = torch.arange(n, dtype=torch.int32, device=src.device)
    return src, keep, n


def preproc_pcd(pcd, gts, num_points, lidar_line=None, radius=50., sampled_indices=None, flip_xy=False, device='cuda',
                want_float64=False, voxel_size=None):
    """loader_utils.py:160-202: (lidar-line reduction,) radius filter, sub-sample without replacement (or zero pad),
    homogeneous transform by `rand_init_l` in float64.  Returns (3, num_points) float32 on the device
    (the reference's float64 rows are cast by the training loop, iterater.py:29).
    `pcd` is a SweepSet (the chain runs on the concatenated index space, efgh_prep_sweeps_*) or an array or tensor of [n, 4] rows
    (efgh_prep_radius_filter / efgh_prep_gather_transform) or [n, 3] rows (the KITTI-raw and nuScenes readers: a SweepSet of one).
    `voxel_size` (not in the reference; None: off, and nothing runs differently): after the radius filter, keep the first row of
    every occupied voxel of that edge (`voxel_keep`), then sub-sample or zero-pad what is left."""
    if voxel_size is not None:
        _check_voxel_size(voxel_size)
    if not isinstance(pcd, SweepSet):
        p = torch.as_tensor(np.ascontiguousarray(pcd, dtype=np.float32)) if not torch.is_tensor(pcd) else pcd
        p = p.to(device=device, dtype=torch.float32).contiguous()
        _C.require_cuda(p)
        assert p.dim() == 2 and p.shape[1] in (3, 4)
        pcd = SweepSet([p]) if p.shape[1] == 3 else p    # [n, 3] rows are read at stride 3
    src, keep, n_keep = _keep_rows(pcd, device, lidar_line, radius, flip_xy, voxel_size)
    sel, n_sel = _subsample(n_keep, num_points, sampled_indices, src.device)
    T = _upload_T(gts, src.device, wait=voxel_size is None)
    out32 = torch.empty((3, num_points), dtype=torch.float32, device=src.device)
    out64 = torch.empty((3, num_points), dtype=torch.float64, device=src.device) if want_float64 else None
    rows_kept = (n_keep,) if src.set is not None else ()            # a sweep set checks `sel` against the kept rows
    src.call(src.gather, ptr(keep), *rows_kept, ptr(sel), n_sel, 1 if flip_xy else 0, ptr(T), num_points,
             ptr(out32), ptr(out64))
    return (out32, out64) if want_float64 else out32


# ------------------------------------------------------------------------------------------------
# the reference's callables
# ------------------------------------------------------------------------------------------------
class _Process(object):
    rellis = False
    has_lidar_line = True

    def __init__(self, args):
        self.raw_cam_img_size = args['raw_cam_img_size']
        self.lidar_line = args['lidar_line'] if self.has_lidar_line else None
        self.num_points = args['num_points']
        self.device = args.get('DEVICE', 'cuda')
        self.voxel_size = args.get('voxel_size')         # optional (not in the reference): thin on a voxel grid, see preproc_pcd
        if self.voxel_size is not None:
            _check_voxel_size(self.voxel_size)
        self.color_jitter = None                         # optional (not in the reference): training only, see ColorJitter
        if args['test'] is False:
            self.l_rot_range = args['dclb']['l_rot_range']
            self.l_trs_range = args['dclb']['l_trs_range']
            self.c_rot_range = args['dclb']['c_rot_range']
            if args.get('color_jitter') is not None:
                try:
                    self.color_jitter = ColorJitter(**args['color_jitter'])
                except TypeError:
                    raise _C.EfghError("args['color_jitter']: expected a dict with keys of %s, got %r" % (JITTER_OPS, args['color_jitter']))
        else:
            self.l_rot_range, self.l_trs_range, self.c_rot_range = None, None, None

    def _calib(self, calibs):
        raise NotImplementedError

    def _run(self, pcd, img, calib, posej_T_posei, rand_init, sampled_indices):
        """the body all four callables share; `pcd` is an array or a SweepSet, `calib` the camera matrix as it is returned"""
        rr, rp, ry, tx, ty, tz, rt = rand_init_params(rand_init, self.l_rot_range, self.l_trs_range, self.c_rot_range)
        gts = preproc_gt(rr, rp, ry, tx, ty, tz, rt, posej_T_posei)
        jitter = self.color_jitter.sample() if self.color_jitter is not None else None       # (after rand_init_params's seven draws)
        imgs = preproc_img(img, gts, self.raw_cam_img_size, self.rellis, self.device, jitter)
        pc = preproc_pcd(pcd, gts, self.num_points, self.lidar_line, sampled_indices=sampled_indices,
                         flip_xy=self.rellis, device=self.device, voxel_size=self.voxel_size)
        gts['img_raw'], gts['img_rot'], gts['img_mask'] = imgs['raw'], imgs['rot'], imgs['img_mask']
        A = np.array([[1, 0, -self.raw_cam_img_size[1] / 2], [0, 1, -self.raw_cam_img_size[0] / 2], [0, 0, 1]])
        gts['cam_T_velo'] = np.linalg.inv(A) @ gts['intrinsic_sensor2'] @ A @ calib @ gts['sensor2_T_sensor1']
        return pc, imgs['in'], calib, A, gts

    def __call__(self, pcd, img, calibs, posej_T_posei, fname, rand_init=None, sampled_indices=None):
        return self._run(pcd, img, self._calib(calibs)[:3, :], posej_T_posei, rand_init, sampled_indices) + (fname,)


class ProcessKITTIODOM(_Process):
    """data_loader/kitti_odom_loader.py:237-273"""

    def _calib(self, calibs):
        return calibs['P2'] @ calibs['Tr']


class ProcessRELLIS(_Process):
    """data_loader/rellis3d_loader.py:292-339: the sweep is first rotated by diag(-1,-1,1) (an exact sign flip, folded
    into the point kernels) and the calibration carries its inverse"""
    rellis = True

    def _calib(self, calibs):
        R = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        return calibs['P'] @ calibs['Tr'] @ np.linalg.inv(R)


class ProcessKITTIRAW(_Process):
    """data_loader/kitti_raw_loader.py:227-263: no pose between sweep and image (`posej_T_posei` = I), the calibration is
    `calibs.T_cam2_velo` / `T_cam3_velo` chosen by `cam` and returned as it is; the reader hands over [n, 3] rows"""

    def __call__(self, pcd, img, calibs, cam, fname, rand_init=None, sampled_indices=None):
        if cam not in ('image_02', 'image_03'):
            raise ValueError("ProcessKITTIRAW: cam is 'image_02' or 'image_03', got %r" % (cam,))
        calib = calibs.T_cam2_velo if cam == 'image_02' else calibs.T_cam3_velo
        return self._run(pcd, img, calib, np.eye(4), rand_init, sampled_indices) + (fname,)


class ProcessNUSC(_Process):
    """data_loader/nusc_loader.py:227-262: no lidar-line reduction, pose and camera matrix come in `calibs`, and the token
    pair is returned in place of a file name"""
    has_lidar_line = False

    def __init__(self, args):
        super().__init__(args)
        self.is_test = args['test']

    def __call__(self, pcd, img, calibs, tokeni_tokenj, rand_init=None, sampled_indices=None):
        return self._run(pcd, img, calibs['T_cam_velo'], calibs['posej_T_posei'], rand_init, sampled_indices) + (tokeni_tokenj,)
