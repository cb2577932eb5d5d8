"""Judging a pose without ground truth: one `synthetic.make_sample` pair, the true pose and a perturbed one scored by the mutual
information between a per-point value and the image grey level under the projected point (efgh_amd.common.score).

The synthetic sweep has no reflectance and its image is noise, so the example makes the two sensors agree the way a real pair does:
every point's value is the grey level the TRUE pose finds under it.  The true pose then scores highest; a pose a fraction of a
degree and a few centimetres off scores visibly lower, and `count` says how many points each candidate had in frame (MI of a sparse
histogram is biased upwards for small counts: compare candidates with similar counts).

    python examples/score_synthetic.py --raw 128 256 --points 8192
    python examples/score_synthetic.py --rot-deg 0.5 --trans 0.05 --bins 16

The matrix of the sample's `gt['cam_T_velo']` projects into the camera image at `raw_cam_img_size`; the synthetic sample only has
the half-size input, which is resized up here (a loader has the raw-size frame at hand)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import candidates_around, fuse, score  # noqa: E402
from efgh_amd.data import prepare as P  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', type=int, nargs=2, default=[128, 256])
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--rot-deg', type=float, default=1.0, help='the perturbed pose: this much about every LiDAR axis')
    ap.add_argument('--trans', type=float, default=0.1, help='... and this many metres along every axis')
    ap.add_argument('--bins', type=int, default=16)
    a = ap.parse_args(argv)
    raw = tuple(a.raw)
    s = syn.make_sample(raw, a.points)
    pcd = torch.from_numpy(s['pc']).cuda()[None]
    img = torch.from_numpy(s['img']).cuda()
    cam = P.resize_image(img.to(torch.uint8).permute(1, 2, 0).contiguous(), raw)[None]
    true = torch.from_numpy(s['gt']['cam_T_velo'][:3]).cuda()[None]
    # the grey level under the true projection, as a uint8 value per point (0 where the point is not in frame)
    fused = fuse(pcd, cam, true, bilinear=False, want=('rgb',))
    rgb = fused.rgb.to(torch.int64)
    value = ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 32768) >> 16).to(torch.uint8)
    # candidate 0: the true pose; candidate 1: the corner of the perturbation grid with every axis at +1 step
    around = candidates_around(true, (a.rot_deg,) * 3, (a.trans,) * 3, steps=1)
    poses = torch.stack([around[:, 0], around[:, -1]], 1)
    got = score(pcd, cam, poses, value=value, bins=a.bins)
    mi, nmi, count, best = got.mi[0].tolist(), got.nmi[0].tolist(), got.count[0].tolist(), got.best().tolist()      # the host reads, for the print
    for name, i in (('true pose', 0), ('perturbed by %g deg, %g m' % (a.rot_deg, a.trans), 1)):
        print('%-28s mi %.4f nats   nmi %.4f   %d points in frame' % (name, mi[i], nmi[i], count[i]))
    print('best candidate: %d' % best[0])
    return mi, count


if __name__ == '__main__':
    main()
