"""Scoring predicted calibrations WITHOUT ground truth (csrc/score.hip): the mutual information between a
per-point scalar of the cloud (the reflectance of column 4, or a range) and the image grey level under the projected point (Pandey
et al., "Automatic extrinsic calibration of vision and lidar by maximizing mutual information"), for K candidate poses per sample in
one call.  The number peaks where the two sensors agree.  Not in the reference; off unless called.

    poses, names = stage_poses(pred, calib)            # (B,4,3,4): the initial pose and the three cascade stages
    s = score(pcd, image, poses)                       # value = pcd[:, 3], 32 x 32 bins
    s.mi, s.nmi, s.count                               # (B,K) float64, float64, int32
    s.best()                                           # (B,) the candidate with the largest mi
    around = candidates_around(pred['cam_T_velo'], rot_deg=(0.5, 0.5, 0.5), trans=(0.05, 0.05, 0.05))      # (B,729,3,4)

Pixel convention, image and matrices are `fuse`'s: the image is the one the matrices project into (`raw_cam_img_size`).  A point
counts iff it is in frame under its candidate and its value is not NaN.  `score` itself asks nothing about occlusion - which points a
nearer surface hides changes with the candidate; `score_visible` (score_vis.py) puts a depth test per candidate in front of the
same histogram.

MI of a sparse histogram is biased UPWARDS when the count n is small (with n points on bins^2 cells the plug-in estimate of an
independent pair is about (bins - 1)^2 / (2 n) nats, not 0), so candidates with very different `count` are not comparable as they
are: `miller_madow(score(..., want_hist=True))` (score_vis.py) applies the standard correction from `count` and `hist`, and
`score_visible` returns it as `mi_mm`.  No effect on registration accuracy is claimed or was measured."""
import math

import numpy as np
import torch

from .. import _C
from .fuse import _cloud_dims, _finite_nonneg, _image_u8, _on_the_clouds_device, _u8_hwc
from .fuse import _fail as _fuse_fail

BINS = (8, 16, 32, 64)
MAX_CANDIDATES = 4096
STAGES = ('eh_cam_T_velo', 'efh_cam_T_velo', 'efgh_cam_T_velo')
BY = ('mi', 'nmi', 'hx', 'hy', 'hxy')


class Score:
    """device tensors of one `score` call: mi, nmi, hx, hy, hxy float64 (B,K) in nats (x: the value, y: the grey level) | count
    int32 (B,K): the points that counted | hist int32 (B,K,bins,bins) [value bin][grey bin], or None"""
    __slots__ = BY + ('count', 'hist')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def best(self, by='mi'):
        """(B,) int64: the candidate with the largest `by` (the first of equals)"""
        if by not in BY:
            raise _C.EfghError('Score.best: by = %r is none of %s' % (by, ', '.join(BY)))
        return torch.argmax(getattr(self, by), dim=1)


def _checked_poses(who, pc, cam_T_velo):
    """the cloud and the candidate matrices -> (B, N, K, T (B,K,3,4)); the head of `_checked`, and all `visible_mask` needs of it"""
    def _fail(what):
        _fuse_fail(what, who)
    B, N = _cloud_dims(pc, who)
    T = cam_T_velo
    if not torch.is_tensor(T):
        _fail('cam_T_velo: expected a tensor, got %s (stage_poses stacks the matrices of a `pred` dict)' % type(T).__name__)
    if T.dtype not in (torch.float32, torch.float64):
        _fail('cam_T_velo: dtype %s, expected float32 or float64' % T.dtype)
    if T.dim() == 3:
        T = T[:, None]
    if T.dim() != 4 or T.shape[0] != B or T.shape[1] < 1 or tuple(T.shape[2:]) != (3, 4):
        _fail('cam_T_velo: expected (%d, K >= 1, 3, 4) or (%d, 3, 4), got %s' % (B, B, tuple(cam_T_velo.shape)))
    K = T.shape[1]
    if K > MAX_CANDIDATES:
        _fail('cam_T_velo: K = %d candidates, at most %d a call' % (K, MAX_CANDIDATES))
    return B, N, K, T


def _checked(who, pc, img, cam_T_velo, value, value_range, bins, min_depth, more=None):
    """the argument checks `score`, `score_soft` and their `_visible` forms share, every one in front of any launch -> (B, N, K,
    T (B,K,3,4), img, H, W, value, lo, hi).  `more(B, K, H, W)`, if given, runs in front of the device check, which stays the last"""
    def _fail(what):
        _fuse_fail(what, who)
    B, N, K, T = _checked_poses(who, pc, cam_T_velo)
    img, H, W = _image_u8(img, B, who)
    if value is None:
        if pc.shape[1] < 4:
            _fail('value: None takes pc[:, 3], and the cloud has %d rows' % pc.shape[1])
        value = pc[:, 3]
    if not torch.is_tensor(value):
        _fail('value: expected a tensor or None, got %s' % type(value).__name__)
    if value.dtype not in (torch.float32, torch.uint8):
        _fail('value: dtype %s, expected float32 or uint8' % value.dtype)
    if tuple(value.shape) != (B, N):
        _fail('value: expected (%d, %d), got %s' % (B, N, tuple(value.shape)))
    if value.dtype == torch.uint8:
        lo, hi = 0.0, 256.0
    else:
        try:
            lo, hi = (float(v) for v in value_range)
        except (TypeError, ValueError):
            _fail('value_range: %r, expected (lo, hi)' % (value_range,))
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            _fail('value_range: %r, expected finite lo < hi' % (value_range,))
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins not in BINS:
        _fail('bins: %r, supported are %s (the counters live in LDS)' % (bins, ', '.join(map(str, BINS))))
    _finite_nonneg('min_depth', min_depth, who)
    if more is not None:
        more(B, K, H, W)
    _on_the_clouds_device(pc, (('img', img), ('cam_T_velo', T), ('value', value)), who, 'the scoring')
    return B, N, K, T, img, H, W, value, lo, hi


def _kernel_inputs(pc, value, T, img):
    """the checked arguments as the kernels read them (call with the cloud's device current): a cloud with unit point stride, a
    float32 value with unit stride, float64 matrices (B,K,3,4) contiguous, a uint8 (B,H,W,3) image"""
    if pc.stride(2) != 1:
        pc = pc.contiguous()
    if value.dtype == torch.uint8:
        value = value.to(torch.float32)                          # exact
    elif value.stride(1) != 1:
        value = value.contiguous()
    P = T.detach().to(torch.float64).contiguous()                # float32 -> float64 is exact
    return pc, value, P, _u8_hwc(img)


def score(pc, img, cam_T_velo, value=None, value_range=(0.0, 1.0), bins=32, min_depth=0.0, want_hist=False):
    """pc float32 (B, C >= 3, N) | img as in `fuse` | cam_T_velo (B,K,3,4), or (B,3,4) for K = 1, of either float width | value
    float32 (B,N) binned over value_range = (lo, hi), or uint8 (B,N) binned over (0, 256); None: pc[:, 3] | bins 8, 16, 32 or 64
    -> Score.  Inputs are never written, outputs are new tensors, nothing is read back to the host."""
    B, N, K, T, img, H, W, value, lo, hi = _checked('score', pc, img, cam_T_velo, value, value_range, bins, min_depth)

    dev = pc.device
    L, st = _C.lib(), _C.stream_ptr
    with torch.cuda.device(dev):
        pc, value, P, img = _kernel_inputs(pc, value, T, img)
        hist = torch.empty((B, K, bins, bins), dtype=torch.int32, device=dev)      # (counts stay below 2^31: N does)
        out = torch.empty((B, K, 5), dtype=torch.float64, device=dev)
        count = torch.empty((B, K), dtype=torch.int32, device=dev)
        _C.check(L.efgh_score_hist(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                   _C.ptr(img), H, W, int(bins), lo, hi, float(min_depth), _C.ptr(hist), st()))
        _C.check(L.efgh_score_mi(_C.ptr(hist), B, K, int(bins), _C.ptr(out), _C.ptr(count), st()))
    return Score(count=count, hist=hist if want_hist else None, **{k: out[:, :, i] for i, k in enumerate(BY)})


def stage_poses(pred, calib=None):
    """the candidates a forward hands back: `calib` (the initial pose, if given) and the cascade's eh_ / efh_ / efgh_cam_T_velo of
    a `pred` dict, each (B,3,4) and exactly the matrix `fuse` accepts for the image at raw_cam_img_size -> ((B,K,3,4), names)"""
    if not isinstance(pred, dict):
        raise _C.EfghError('stage_poses: pred: expected the dict of a forward, got %s' % type(pred).__name__)
    names = [k for k in STAGES if pred.get(k) is not None]
    if len(names) != len(STAGES):
        raise _C.EfghError('stage_poses: pred: no %s' % ', '.join(k for k in STAGES if k not in names))
    mats = [pred[k] for k in names]
    if calib is not None:
        mats, names = [calib] + mats, ['calib'] + names
    for k, m in zip(names, mats):
        if not torch.is_tensor(m) or m.dim() != 3 or tuple(m.shape[1:]) != (3, 4) or m.shape[0] != mats[-1].shape[0]:
            raise _C.EfghError('stage_poses: %s: expected a (B,3,4) tensor, got %s' % (k, tuple(m.shape) if torch.is_tensor(m) else type(m).__name__))
    wide = torch.float64 if any(m.dtype == torch.float64 for m in mats) else mats[-1].dtype
    return torch.stack([m.detach().to(device=mats[-1].device, dtype=wide) for m in mats], 1), tuple(names)


def perturbations(rot_deg, trans, steps=1, device=None):
    """the 4x4 rigid perturbations D_j of `candidates_around` as one float64 tensor (K,4,4) on `device`, built with torch ops there;
    D_0 is the identity.  The grid is {-steps .. steps} on every axis whose entry of rot_deg (three Euler angles in degrees,
    D = [Rz Ry Rx | t]) or trans (metres) is not zero, scaled by that entry; after the identity the rest follows in lexicographic
    order"""
    try:
        scale = [float(v) for v in rot_deg] + [float(v) for v in trans]
    except (TypeError, ValueError):
        scale = []
    if len(scale) != 6 or len(tuple(rot_deg)) != 3 or not all(math.isfinite(v) for v in scale):
        raise _C.EfghError('candidates_around: rot_deg = %r and trans = %r: three finite numbers each' % (rot_deg, trans))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise _C.EfghError('candidates_around: steps = %r, expected an integer >= 1' % (steps,))
    steps = int(steps)
    axes = [a for a in range(6) if scale[a] != 0.0]
    K = (2 * steps + 1) ** len(axes)
    if K > MAX_CANDIDATES:
        raise _C.EfghError('candidates_around: %d axes with %d values each are %d candidates, at most %d'
                           % (len(axes), 2 * steps + 1, K, MAX_CANDIDATES))
    f64 = dict(dtype=torch.float64, device=device)
    p = torch.zeros((K, 6), **f64)
    if axes:
        line = torch.arange(-steps, steps + 1, **f64)
        grid = torch.cartesian_prod(*([line] * len(axes))).reshape(K, len(axes))
        mid = K // 2                                             # the all-zero row of the lexicographic order goes first
        grid = torch.cat([grid[mid:mid + 1], grid[:mid], grid[mid + 1:]])
        p[:, axes] = grid * torch.tensor([scale[a] for a in axes], **f64)
    return _rigid(torch.deg2rad(p[:, :3]), p[:, 3:])


def _rigid(r, t):
    """r (K,3) Euler angles in radians, t (K,3) -> (K,4,4) float64 [Rz Ry Rx | t], with torch ops (differentiable in r and t)"""
    (cx, cy, cz), (sx, sy, sz) = torch.cos(r).unbind(1), torch.sin(r).unbind(1)
    zero, one = torch.zeros_like(cx), torch.ones_like(cx)
    rows = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, t[:, 0]], [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, t[:, 1]],
            [-sy, cy * sx, cy * cx, t[:, 2]], [zero, zero, zero, one]]
    return torch.stack([torch.stack(row, 1) for row in rows], 1)


def candidates_around(P, rot_deg, trans, steps=1):
    """P (B,3,4) of either float width -> (B,K,3,4) float64 on P's device: P D_j with D_j the rigid perturbations of the LiDAR frame
    on the grid of `perturbations`.  Candidate 0 is P itself, bit for bit; at most 4096 candidates."""
    if not torch.is_tensor(P) or P.dim() != 3 or tuple(P.shape[1:]) != (3, 4) or P.dtype not in (torch.float32, torch.float64):
        raise _C.EfghError('candidates_around: P: expected a float (B,3,4) tensor, got %s'
                           % ('%s %s' % (P.dtype, tuple(P.shape)) if torch.is_tensor(P) else type(P).__name__))
    D = perturbations(rot_deg, trans, steps, P.device)
    P64 = P.detach().to(torch.float64)
    out = torch.matmul(P64[:, None], D[None])                   # (B,1,3,4) x (1,K,4,4)
    out[:, 0] = P64                                              # the unperturbed pose: P, not P times a computed identity
    return out
