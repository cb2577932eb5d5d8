"""What csrc/fuse.hip computes, restated in numpy float64 (include/efgh_hip.h states it in words).  Every operation is element-wise
and in the stated order; there is no `@` anywhere, because a BLAS may fuse a multiply and an add.  The GPU results are held to
this BIT FOR BIT (tests/test_gpu_fuse.py); tests/test_fuse_host.py holds this file to properties that are not taken from it."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BEHIND, OUT_OF_FRAME, OCCLUDED, VISIBLE = 0, 1, 2, 3


def project(pc, T, H, W, min_depth=0.0):
    """pc (C >= 3, N) float32, T 3x4 -> dict of per-point u, v (float64), d (float32), front, frame (bool), r, c (int64, 0 where
    not in frame)"""
    pc = np.asarray(pc)
    assert pc.dtype == np.float32
    T = np.asarray(T, dtype=np.float64).reshape(12)
    px, py, pz = pc[0].astype(np.float64), pc[1].astype(np.float64), pc[2].astype(np.float64)
    with np.errstate(all='ignore'):
        x = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3]
        y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7]
        w = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11]
        u, v = x / w, y / w
        d = w.astype(np.float32)
        front = (w > min_depth) & (w < np.inf) & (np.abs(x) < np.inf) & (np.abs(y) < np.inf)
        frame = front & (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(H))
    c = np.where(frame, u, 0.0).astype(np.int64)              # (int)u: truncation of a non-negative value
    r = np.where(frame, v, 0.0).astype(np.int64)
    return {'u': u, 'v': v, 'd': d, 'front': front, 'frame': frame, 'r': r, 'c': c}


def keys(p):
    """float32 depth bits << 32 | point index, for every point (meaningful where p['frame'])"""
    return (p['d'].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(p['d'].shape[0], dtype=np.uint64)


def zbuffer(pc, T, H, W, radius=0, min_depth=0.0):
    """-> uint64 (H, W): the smallest key over all in-frame points whose (2 radius + 1)^2 window, clipped, holds the pixel"""
    p = project(pc, T, H, W, min_depth)
    k = keys(p)
    z = np.full(H * W, EMPTY, dtype=np.uint64)
    idx = np.nonzero(p['frame'])[0]
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            rr, cc = p['r'][idx] + dr, p['c'][idx] + dc
            ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            np.minimum.at(z, rr[ok] * W + cc[ok], k[idx][ok])
    return z.reshape(H, W)


def _lerp2(a, b, c, d, tx, ty):
    top = a + (b - a) * tx
    bot = c + (d - c) * tx
    val = top + (bot - top) * ty
    return (val + 0.5).astype(np.int64).astype(np.uint8)


def resolve(pc, T, img, zbuf, bilinear=True, min_depth=0.0, rel_tol=0.0, abs_tol=0.0):
    """img uint8 (H, W, 3), zbuf of `zbuffer` -> state uint8 (N,), rgb uint8 (N, 3), uv float32 (N, 2)"""
    H, W = img.shape[:2]
    p = project(pc, T, H, W, min_depth)
    n = p['d'].shape[0]
    state = np.where(p['frame'], OCCLUDED, np.where(p['front'], OUT_OF_FRAME, BEHIND)).astype(np.uint8)
    f = p['frame']
    r, c = p['r'][f], p['c'][f]
    zmin = (zbuf[r, c] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(all='ignore'):
        bound = zmin.astype(np.float64) * (1.0 + float(rel_tol)) + float(abs_tol)
        vis = p['d'][f].astype(np.float64) <= bound
    state[np.nonzero(f)[0][vis]] = VISIBLE
    rgb = np.zeros((n, 3), dtype=np.uint8)
    if not bilinear:
        rgb[f] = img[r, c]
    else:
        fx, fy = p['u'][f] - 0.5, p['v'][f] - 0.5
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        xi, yi = x0.astype(np.int64), y0.astype(np.int64)
        xa, xb = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
        ya, yb = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
        im = img.astype(np.float64)
        out = np.zeros((int(f.sum()), 3), dtype=np.uint8)
        for ch in range(3):
            out[:, ch] = _lerp2(im[ya, xa, ch], im[ya, xb, ch], im[yb, xa, ch], im[yb, xb, ch], tx, ty)
        rgb[f] = out
    with np.errstate(all='ignore'):
        uv = np.stack([p['u'], p['v']], 1).astype(np.float32)
    uv[~p['front']] = np.nan
    return state, rgb, uv


def maps(zbuf):
    """-> depth float32 (H, W) (0 where empty), index int32 (H, W) (-1 where empty)"""
    empty = zbuf == EMPTY
    depth = np.where(empty, np.uint64(0), zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = np.where(empty, np.int64(-1), (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return depth, index


def fuse(pc, img, P, radius=0, rel_tol=0.0, abs_tol=0.0, min_depth=0.0, bilinear=True):
    """the batch: pc (B, C, N) float32, img uint8 (B, H, W, 3), P (B, 3, 4) -> dict of stacked state, rgb, uv, depth, index"""
    out = {k: [] for k in ('state', 'rgb', 'uv', 'depth', 'index')}
    for b in range(pc.shape[0]):
        H, W = img[b].shape[:2]
        z = zbuffer(pc[b], P[b], H, W, radius, min_depth)
        s, c, uv = resolve(pc[b], P[b], img[b], z, bilinear, min_depth, rel_tol, abs_tol)
        dm, im = maps(z)
        for k, a in zip(('state', 'rgb', 'uv', 'depth', 'index'), (s, c, uv, dm, im)):
            out[k].append(a)
    return {k: np.stack(a) for k, a in out.items()}


def u8_hwc(img_f):
    """the float (B, 3, H, W) image as the product converts it: truncation, channels last"""
    return np.ascontiguousarray(np.transpose(img_f.astype(np.int64).astype(np.uint8), (0, 2, 3, 1)))
