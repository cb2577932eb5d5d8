"""`fuse` behind the model: the synthetic sample through an eval forward (the small configuration of tests/test_gpu_forward.py), the
prediction handed over as the `pred` dict, the result against tests/fuse_contract.py with pred['cam_T_velo'] copied to the host; and
the PLY of the visible points read back."""
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
from test_gpu_fuse import _same  # noqa: E402

pytestmark = pytest.mark.gpu
RAW, NPTS = (128, 256), 2048


def test_fuse_with_the_models_prediction(manifest, tmp_path):
    from efgh_amd.common import fuse
    from efgh_amd.io.formats import read_ply
    from efgh_amd.nets import EFGHBackbone
    m = EFGHBackbone(syn.default_args(RAW, 'cuda'))
    m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1), strict=True)
    m = m.cuda().eval()
    b = syn.make_batch(RAW, NPTS, 2)
    pcd, img, calib, A = (torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A'))
    with torch.no_grad():
        pred = m(pcd, img, calib, A)
    assert tuple(pred['cam_T_velo'].shape) == (2, 3, 4)
    # the matrix projects into the camera image at raw_cam_img_size: the model's half-size input stands in for it, tiled
    cam = img.repeat_interleave(2, 2).repeat_interleave(2, 3)
    keep = pcd.clone(), cam.clone(), pred['cam_T_velo'].clone()
    kw = dict(radius=2, rel_tol=0.05)
    got = fuse(pcd, cam, pred, **kw)
    ref = FC.fuse(b['pc'], FC.u8_hwc(cam.cpu().numpy()), pred['cam_T_velo'].cpu().numpy().astype(np.float64), **kw)
    _same(got, ref)
    assert (ref['state'] == 3).sum() > 50 and (ref['state'] <= 1).sum() > 50
    assert torch.equal(keep[0], pcd) and torch.equal(keep[1], cam) and torch.equal(keep[2], pred['cam_T_velo'])
    # the PLY holds exactly the visible rows of a sample, in order
    path = str(tmp_path / 'fused.ply')
    inten = torch.rand(NPTS, device='cuda')
    n = got.save_ply(path, pcd, sample=1, extra={'intensity': inten})
    vis = ref['state'][1] == 3
    back = read_ply(path)
    assert n == vis.sum() == back['xyz'].shape[0]
    assert (back['xyz'] == b['pc'][1].T[vis]).all() and (back['rgb'] == ref['rgb'][1][vis]).all()
    assert (back['intensity'] == inten.cpu().numpy()[vis]).all() and sorted(back) == ['intensity', 'rgb', 'xyz']
    n = got.save_ply(path, pcd, sample=0, only_visible=False)
    back = read_ply(path)
    assert n == NPTS and (back['state'] == ref['state'][0]).all() and (back['rgb'] == ref['rgb'][0]).all()
