"""Writes tests/golden/jitter.npz: what Pillow itself gives for the photometric jitter (torchvision's ColorJitter on PIL images:
ImageEnhance.Brightness / Contrast / Color, and the HSV round trip of its adjust_hue).  Pillow and numpy only.

    python tests/golden/make_golden_jitter.py

Keys: `pillow_version`; `img/<name>` the inputs; `out/<name>/<op>/<factor>` one op; `cases` a JSON list of the composite cases
[{'order': [...], 'factors': [...]}, ...] and `out/<name>/case<i>` their outputs."""
import json
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
FACTORS = (0, 0.3, 1, 1.4, 2)
HUES = (0, 0.1, -0.1, 0.5, -0.5)
B, C, S, H = 'brightness', 'contrast', 'saturation', 'hue'
# contrast at every position of a four-op order, shorter orders, factors inside and outside [0, 1], and the copies (0 and 1)
CASES = [
    ((C, B, S, H), (0.6, 1.3, 0.7, 0.05)), ((B, C, S, H), (1.3, 0.6, 0.7, 0.05)), ((B, S, C, H), (0.8, 1.6, 1.4, -0.2)),
    ((B, S, H, C), (0.8, 1.6, 0.31, 0.45)), ((H, S, B, C), (-0.37, 0.2, 1.9, 1.7)), ((H, C, S, B), (0.12, 1.25, 0.5, 0.75)),
    ((S, H, C, B), (1.9, 0.5, 0.3, 1.1)), ((C, H), (1.5, -0.5)), ((S, C), (0.0, 0.5)), ((B, C), (0.0, 1.5)),
    ((H, C, B), (0.25, 1.0, 0.9)), ((C, S, B), (2.0, 2.0, 0.5)), ((S, B, H, C), (1.0, 1.0, 0.0, 0.999)),
]


def images():
    rng = np.random.RandomState(20250)
    random = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    # directed cases, one per pixel; [0, 0:2] are two gray pixels whose L mean is exactly 10.5
    px = [(10, 10, 10), (11, 11, 11)]
    px += [(v, v, v) for v in (0, 1, 2, 127, 128, 254, 255)]                                             # gray
    px += [(200, 200, 17), (200, 17, 200), (17, 200, 200), (255, 255, 0), (255, 0, 255), (0, 255, 255),  # two equal maxima
           (1, 1, 0), (90, 90, 89)]
    for v in (0, 1, 100, 254):                                                                          # channels differing by 1
        px += [(v + 1, v, v), (v, v + 1, v), (v, v, v + 1), (v, v + 1, v + 1), (v + 1, v, v + 1), (v + 1, v + 1, v)]
    px += [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]                             # 0 and 255
    px += [(255, 254, 0), (0, 254, 255), (255, 0, 1), (1, 0, 255), (0, 255, 1), (128, 0, 255), (255, 128, 0), (0, 128, 255)]
    while len(px) < 256:                                                                                 # hue sextant borders and near them
        k = len(px)
        px.append(((k * 37) % 256, (k * 91 + 5) % 256, 255 - (k * 13) % 256))
    directed = np.array(px[:256], np.uint8).reshape(16, 16, 3)
    y, x = np.mgrid[0:48, 0:64]
    gradient = np.stack([x * 4, y * 5, (x + y) * 2], axis=-1).astype(np.uint8)
    below = np.full((16, 16, 3), 10, np.uint8)                # 127 gray pixels of 11 among 256: L mean 10.496..., just below 10.5
    below.reshape(-1, 3)[:127] = 11
    return {'random': random, 'directed': directed, 'gradient': gradient, 'mean_half': directed[0:1, 0:2].copy(), 'mean_below': below}


def adjust_hue(im, hue):
    """torchvision.transforms._functional_pil.adjust_hue"""
    h, s, v = im.convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h = np_h + np.array(int(hue * 255)).astype(np.uint8)
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


def one(im, op, f):
    if op == H:
        return adjust_hue(im, f)
    return {B: ImageEnhance.Brightness, C: ImageEnhance.Contrast, S: ImageEnhance.Color}[op](im).enhance(f)


def main():
    out = {'pillow_version': np.array(PIL.__version__),
           'cases': np.array(json.dumps([{'order': list(o), 'factors': list(f)} for o, f in CASES]))}
    for name, arr in images().items():
        out['img/' + name] = arr
        im = Image.fromarray(arr, 'RGB')
        for op in (B, C, S):
            for f in FACTORS:
                out['out/%s/%s/%s' % (name, op, f)] = np.asarray(one(im, op, f))
        for h in HUES:
            out['out/%s/%s/%s' % (name, H, h)] = np.asarray(one(im, H, h))
        for i, (order, factors) in enumerate(CASES):
            cur = im
            for op, f in zip(order, factors):
                cur = one(cur, op, f)
            out['out/%s/case%d' % (name, i)] = np.asarray(cur)
    path = os.path.join(HERE, 'jitter.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes, Pillow', PIL.__version__)


if __name__ == '__main__':
    main()
