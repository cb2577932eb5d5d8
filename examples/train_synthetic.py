"""End-to-end use of the pieces on synthetic frames: GPU sample preparation (efgh_amd.data, the reference's
`ProcessKITTIODOM` call), EFGHBackbone, EFGHCriterion, the fused-Adam Trainer and the device-side error meter — the
loop of the reference's iterater.py:25-60 with nothing on the CPU between the decoded frame and the optimizer step.

    python examples/train_synthetic.py --iters 3 --raw 128 256 --points 2048
    python examples/train_synthetic.py --iters 3 --batch 4 --accumulate 2        # gradient accumulation over micro-batches
    python examples/train_synthetic.py --iters 3 --transactional                 # a skipped step also restores BatchNorm's state
    python examples/train_synthetic.py --iters 5 --ema 0.999                     # validate the live and the averaged weights
    python examples/train_synthetic.py --iters 3 --groups                        # parameter groups: G at a tenth of the rate, no decay on 1-D parameters
    python examples/train_synthetic.py --iters 3 --accumulate-sweeps 2           # 2 neighbouring sweeps on either side, merged on the GPU
    python examples/train_synthetic.py --iters 3 --accumulate-sweeps 2 --voxel 0.2   # ... thinned on a 0.2 grid before the sub-sampling
    python examples/train_synthetic.py --iters 3 --jitter 0.4 0.4 0.4 0.1        # brightness, contrast, saturation, hue of every frame, on the GPU
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common.metrics import Err  # noqa: E402
from efgh_amd.data import ProcessKITTIODOM, SweepSet, accumulation_indices, accumulation_transform  # noqa: E402
from efgh_amd.losses import EFGHCriterion  # noqa: E402
from efgh_amd.nets import EFGHBackbone  # noqa: E402
from efgh_amd.train import Trainer  # noqa: E402


def raw_frame(raw_hw, seed):
    """a decoded camera frame a bit larger than the network's raw size, and an unfiltered sweep (n,4)"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(raw_hw[0] + 8, raw_hw[1] + 20, 3)).astype(np.uint8)
    return img


def collate(samples, device):
    pc = torch.stack([s[0] for s in samples]).float()
    img = torch.stack([s[1] for s in samples]).float()
    calib = torch.from_numpy(np.stack([s[2] for s in samples])).float().to(device)
    A = torch.from_numpy(np.stack([s[3] for s in samples])).float().to(device)
    gt = {}
    for k in samples[0][4]:
        v = [s[4][k] for s in samples]
        gt[k] = torch.stack(v) if torch.is_tensor(v[0]) else torch.from_numpy(np.stack(v))
    return pc, img, calib, A, gt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--raw', type=int, nargs=2, default=[128, 256])
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--max-grad-norm', type=float, default=None, help='clip the global gradient norm (torch clip_grad_norm_) inside the fused step')
    ap.add_argument('--skip-nonfinite', action='store_true', help='leave weights and Adam moments untouched on a step whose gradient holds inf / NaN')
    ap.add_argument('--transactional', action='store_true',
                    help='implies --skip-nonfinite: a non-finite forward skips the step too, and a skipped step restores BatchNorm\'s '
                         'running statistics and counters')
    ap.add_argument('--accumulate', type=int, default=None, metavar='K',
                    help='cut every batch into K micro-batches and accumulate their gradients: the update of --batch, the memory of --batch / K')
    ap.add_argument('--ema', type=float, default=None, metavar='DECAY',
                    help='keep an exponential moving average of the weights inside the fused step and run the error meter on the last '
                         'batch once with the live and once with the averaged weights')
    ap.add_argument('--groups', action='store_true',
                    help='parameter groups inside the fused step: the ResNet branch G at a tenth of the learning rate, weight '
                         'decay on the rest except BatchNorm weights and biases')
    ap.add_argument('--accumulate-sweeps', type=int, default=0, metavar='N',
                    help='merge up to N neighbouring LiDAR sweeps on either side into every sample (the loaders\' '
                         'accumulation_frame_num; not to be confused with --accumulate, which accumulates gradients)')
    ap.add_argument('--voxel', type=float, default=None, metavar='SIZE',
                    help='thin every cloud on a voxel grid of edge SIZE before it is sub-sampled (first point of a voxel wins, the '
                         'own sweep first); goes together with --accumulate-sweeps')
    ap.add_argument('--jitter', type=float, nargs=4, default=None, metavar=('B', 'C', 'S', 'H'),
                    help='photometric jitter of every frame (torchvision\'s ColorJitter(B, C, S, H), Pillow-exact, on the GPU); 0 leaves '
                         'a component out')
    a = ap.parse_args(argv)
    a.skip_nonfinite = a.skip_nonfinite or a.transactional
    raw = tuple(a.raw)
    args = syn.default_args(raw, 'cuda')
    args.update({'lidar_line': None, 'num_points': a.points, 'test': False,
                 'dclb': {'l_rot_range': 1 / 12., 'l_trs_range': 1.0, 'c_rot_range': 1 / 12.}})
    if a.voxel is not None:
        args['voxel_size'] = a.voxel
    if a.jitter is not None:
        args['color_jitter'] = dict(zip(('brightness', 'contrast', 'saturation', 'hue'), a.jitter))
    torch.manual_seed(0)
    model = EFGHBackbone(args).cuda()
    groups = None
    if a.groups:                                             # first match wins; what nothing matches is the default group
        one_d = {k for k, p in model.named_parameters() if p.dim() <= 1}
        groups = [{'names': ['G.'], 'lr': 1e-5, 'name': 'G'},
                  {'names': lambda k: k in one_d, 'weight_decay': 0.0, 'name': 'bn_and_bias'}]
    trainer = Trainer(model, EFGHCriterion(args), lr=1e-4, weight_decay=1e-2 if a.groups else 0.0, max_grad_norm=a.max_grad_norm,
                      skip_nonfinite=a.skip_nonfinite, transactional=a.transactional, ema_decay=a.ema, param_groups=groups)
    if a.groups:
        print('parameter groups:', ', '.join('%s: %d parameters, lr %g, weight_decay %g' % (g['name'], len(g['params']), g['lr'], g['weight_decay'])
                                             for g in trainer.opt.param_groups))
    prep = ProcessKITTIODOM(args)
    err = Err(args['dataset'])
    calib0, _ = syn.calib_and_A(raw)
    P2 = np.eye(4); P2[:3] = calib0
    hist = []
    for it in range(a.iters):
        samples = []
        for b in range(a.batch):
            seed = it * a.batch + b
            sweep = np.concatenate([syn.lidar_sweep(a.points * 2, seed).T, np.ones((a.points * 2, 1), np.float32)], 1)
            if a.accumulate_sweeps:
                # frame `own` of a 2N+1-frame drive along x: what get_accumulated_pc concatenates, kept as float32 sweeps with
                # one 4x4 each; near the ends of the drive fewer frames are found, as in the loaders
                n_frames, own = 2 * a.accumulate_sweeps + 1, seed % (2 * a.accumulate_sweeps + 1)
                pose = lambda f: np.array([[1., 0, 0, 0.5 * f], [0, 1, 0, 0.02 * f], [0, 0, 1, 0], [0, 0, 0, 1]])
                prev, nxt = accumulation_indices(own, n_frames, a.accumulate_sweeps, 1)
                others = [np.concatenate([syn.lidar_sweep(a.points, 1000 * seed + f).T, np.ones((a.points, 1), np.float32)], 1)
                          for f in prev + nxt]
                sweep = SweepSet([sweep] + others, [accumulation_transform(pose(own), pose(f)) for f in prev + nxt])
            samples.append(prep(sweep, raw_frame(raw, seed), {'P2': P2, 'Tr': np.eye(4)}, np.eye(4), 'f%06d' % seed)[:5])
        pc, img, calib, A, gt = collate(samples, 'cuda')
        if a.accumulate:                                     # one loss over the whole batch, BatchNorm statistics per micro-batch
            losses, preds = trainer.step(pc, img, calib, A, gt, micro_batches=a.accumulate)
            pred = {k: (torch.cat([p[k] for p in preds], 0) if torch.is_tensor(preds[0][k]) and preds[0][k].dim() else preds[0][k]) for k in preds[0]}
        else:
            losses, pred = trainer.step(pc, img, calib, A, gt)
        err.update({'sensor2_T_sensor1': gt['sensor2_T_sensor1'].float().cuda()}, pred)
        hist.append(float(losses['total'].detach()))
        print('iter %d  total %.4f  %s' % (it, hist[-1], '  '.join('%s %.3f' % kv for kv in err.dict.items())))
    if a.max_grad_norm is not None or a.skip_nonfinite:
        print('gradient guard:', trainer.guard_stats())        # the one host read of the guard's state
    if a.ema is not None:
        def validate(tag):
            meter = Err(args['dataset'])
            with torch.no_grad():
                meter.update({'sensor2_T_sensor1': gt['sensor2_T_sensor1'].float().cuda()}, model(pc, img, calib, A))
            print('%-18s %s' % (tag, '  '.join('%s %.3f' % kv for kv in meter.dict.items())))
            return dict(meter.dict)
        model.eval()                                         # (the scope leaves the mode alone)
        live = validate('live weights:')
        with trainer.ema_weights():                          # the averaged weights under the same model, in place
            averaged = validate('averaged weights:')
        model.train()
        return hist, live, averaged
    return hist


if __name__ == '__main__':
    main()
