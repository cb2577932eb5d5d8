"""What a predicted calibration is for: the synthetic sample through an eval forward, then `fuse` with the prediction - for every
LiDAR point the pixel it falls on, whether the camera sees it, and its colour - the four state counts per sample, and a PLY of the
visible points of sample 0 (any viewer that reads binary PLY shows it: a wrong pose smears colours across depth edges).

    python examples/fuse_synthetic.py --raw 128 256 --points 2048 --out fused.ply
    python examples/fuse_synthetic.py --radius 2 --rel-tol 0.05        # windowed z-buffer: closes the gaps of a sparse foreground

The matrix of `pred['cam_T_velo']` projects into the camera image at `raw_cam_img_size`; the synthetic sample only has the model's
half-size input, which is resized up here (a loader has the raw-size frame at hand)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import fuse  # noqa: E402
from efgh_amd.data import prepare as P  # noqa: E402
from efgh_amd.nets import EFGHBackbone  # noqa: E402

STATES = ('not in front', 'out of frame', 'occluded', 'visible')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', type=int, nargs=2, default=[128, 256])
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--radius', type=int, default=0, help='half width of the window every point covers in the z-buffer (0 .. 8)')
    ap.add_argument('--rel-tol', type=float, default=0.0, help='a point is visible iff depth <= nearest * (1 + rel_tol) + abs_tol')
    ap.add_argument('--abs-tol', type=float, default=0.0)
    ap.add_argument('--out', default='fused.ply')
    a = ap.parse_args(argv)
    raw = tuple(a.raw)
    torch.manual_seed(0)
    model = EFGHBackbone(syn.default_args(raw, 'cuda')).cuda().eval()
    b = syn.make_batch(raw, a.points, a.batch)
    pcd, img, calib, A = (torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A'))
    with torch.no_grad():
        pred = model(pcd, img, calib, A)
    cam = torch.stack([P.resize_image(img[i].to(torch.uint8).permute(1, 2, 0).contiguous(), raw) for i in range(a.batch)])
    fused = fuse(pcd, cam, pred, radius=a.radius, rel_tol=a.rel_tol, abs_tol=a.abs_tol)
    counts = torch.stack([(fused.state == s).sum(1) for s in range(4)], 1).tolist()       # the one host read, for the print
    for i, c in enumerate(counts):
        print('sample %d: %s' % (i, ', '.join('%d %s' % (n, s) for n, s in zip(c, STATES))))
    n = fused.save_ply(a.out, pcd, sample=0)
    print('%s: %d visible points of sample 0 with their colours' % (a.out, n))
    return counts


if __name__ == '__main__':
    main()
