"""The photometric jitter of sample preparation (csrc/jitter.hip, efgh_amd.data.color_jitter) restated in numpy: torchvision's
`ColorJitter` on PIL images, i.e. Pillow's `Image.blend`, `convert('L')`, `convert('HSV')` / `convert('RGB')` and
`ImageStat.Stat(...).mean`, byte for byte.  numpy only; tests/test_jitter_host.py holds it against Pillow itself (exhaustively
where that is feasible) and against tests/golden/jitter.npz, tests/test_gpu_jitter.py holds the kernels against it.

Images are uint8 arrays whose last axis is (R, G, B).  An op list is what `JitterParams` carries: the op names in the order they
are applied, one factor per op (hue's factor is the hue value in [-0.5, 0.5]; the shift is `hue_shift(factor)`)."""
import numpy as np

OPS = ('brightness', 'contrast', 'saturation', 'hue')
f32, f64 = np.float32, np.float64


def blend(deg, img, f):
    """Pillow `Image.blend(deg, img, f)` per channel (Blend.c).  The factor is a C float there: the two copies and the choice between
    truncation and clipping are decided on float32(f), and t = deg + f * (img - deg) is float32 with a separate multiply and add."""
    deg, img = np.broadcast_arrays(np.asarray(deg), np.asarray(img))
    a = f32(f)
    if a == f32(0.):
        return deg.astype(np.uint8)
    if a == f32(1.):
        return img.astype(np.uint8)
    d = deg.astype(f32)
    t = d + (a * (img.astype(f32) - d)).astype(f32)
    assert t.dtype == f32
    if f32(0.) <= a <= f32(1.):
        return t.astype(np.int32).astype(np.uint8)                   # (uint8)t, truncated; t is inside [0, 255]
    out = np.clip(t, f32(0.), f32(255.)).astype(np.int32)           # 0 where t <= 0, 255 where t >= 255, else truncated
    return out.astype(np.uint8)


def luma(img):
    """`convert('L')`: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    v = np.asarray(img).astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def luma_mean(img):
    """`int(ImageStat.Stat(img.convert('L')).mean[0] + 0.5)`: the quotient in float64, then truncated"""
    L = luma(img)
    return int(float(int(L.astype(np.int64).sum())) / float(L.size) + 0.5)


def rgb_to_hsv(img):
    """`convert('HSV')` of an RGB image (Convert.c:rgb2hsv_row)"""
    v = np.asarray(img).astype(np.int32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    gray = maxc == minc
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - x).astype(f32) / cr for x in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, ((2.0 + rc.astype(f64)) - bc.astype(f64)).astype(f32),
                              ((4.0 + gc.astype(f64)) - rc.astype(f64)).astype(f32)))
        assert s.dtype == f32 and h.dtype == f32
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(gray, 0, H), np.where(gray, 0, S)
    return np.stack([H, S, maxc], axis=-1).astype(np.uint8)


def _round_clip8(x):
    """C `round` (half away from zero) of a float64, clipped to 0 .. 255"""
    return np.clip(np.where(x >= 0., np.floor(x + 0.5), -np.floor(-x + 0.5)), 0., 255.).astype(np.int32)


def hsv_to_rgb(hsv):
    """`convert('RGB')` of an HSV image (Convert.c:hsv2rgb)"""
    a = np.asarray(hsv)
    H, S, V = a[..., 0].astype(f64), a[..., 1].astype(f64), a[..., 2].astype(f64)
    h6 = H * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(f32)
    fs = (S / 255.0).astype(f32)
    p = _round_clip8(V * (1.0 - fs.astype(f64)))
    q = _round_clip8(V * (1.0 - (fs * f).astype(f64)))                     # fs * f is a float32 product, 1.0 - it a double
    t = _round_clip8(V * (1.0 - (fs * (f32(1.0) - f)).astype(f64)))
    v = a[..., 2].astype(np.int32)
    k = i.astype(np.int32) % 6
    table = (((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)))
    out = [np.choose(k, [row[c] for row in table]) for c in range(3)]
    gray = a[..., 1] == 0
    return np.stack([np.where(gray, v, c) for c in out], axis=-1).astype(np.uint8)


def hue_shift(hue):
    """the shift of H for a hue factor: int(hue * 255), truncated toward zero"""
    return int(float(hue) * 255)


def shift_hue(img, k):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(k)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def contrast(img, f):
    return blend(np.full_like(img, luma_mean(img)), img, f)


def hue(img, h):
    return shift_hue(img, hue_shift(h))


def apply(img, order, factors, shift=None):
    """the ops of `order` with their `factors`, one after the other; `shift` overrides the hue shift derived from hue's factor"""
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for op, f in zip(order, factors):
        if op == 'hue':
            out = shift_hue(out, hue_shift(f) if shift is None else shift)
        else:
            out = {'brightness': brightness, 'contrast': contrast, 'saturation': saturation}[op](out, f)
    return out


def all_triplets():
    """all 2^24 byte triplets as a 4096 x 4096 x 3 image: pixel i is (i >> 16, (i >> 8) & 255, i & 255)"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16), (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
