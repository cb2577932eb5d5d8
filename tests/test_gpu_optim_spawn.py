"""`python -m efgh_amd.run --fused-optimizer <script>`: a script shaped like the reference's main.py + iterater.py (stock
`torch.optim.Adam(...)`, zero_grad / backward / step, a checkpoint with the optimizer's state_dict) runs UNCHANGED on the fused
optimizer, in one process and as two data-parallel ranks sharing the one GPU over gloo."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = '''
# the shape of the reference's entry script and loop (main.py:14-15,126-129,181-183; iterater.py:26-43,82-89), nothing package-specific
import json, os, sys
import numpy as np
import torch, torch.utils.data
import nets
import losses
from efgh_amd import synthetic as syn                 # (stands in for data_loader: synthetic frame-pairs)

args = syn.default_args((128, 256), 'cuda')
args['arch'] = 'EFGH'


class Pairs(torch.utils.data.Dataset):
    def __len__(self):
        return 8

    def __getitem__(self, i):
        s = syn.make_sample((128, 256), 2048, i)
        return s['pc'], s['img'], s['calib'], s['A'], {k: np.asarray(v) for k, v in s['gt'].items()}, 'pair%d' % i


device = torch.device('cuda')
torch.manual_seed(int(os.environ.get('RANK', 0)))     # ranks would start apart without the wrapper's broadcast
model = nets.__dict__[args['arch'] + 'Backbone'](args).to(device)
model = torch.nn.DataParallel(model)
criterion = losses.__dict__[args['arch'] + 'Criterion'](args)
loader = torch.utils.data.DataLoader(Pairs(), batch_size=4, shuffle=True, num_workers=0)
optimizer = torch.optim.Adam([p for _, p in model.named_parameters() if p.requires_grad], lr=1e-4, weight_decay=0)
model.train()
it, last = 0, None
for pcd, img, calib, A, gt, fname in loader:
    for param_group in optimizer.param_groups:        # adjust_learning_rate, common/helper.py:31-34
        param_group['lr'] = 1e-4 * (0.7 ** (it // 50000))
    pcd, img, calib, A = (t.to(device).float() for t in (pcd, img, calib, A))
    pred = model(pcd, img, calib, A, it == 0)
    L, gt = criterion.compute_loss(pcd, img, calib, A, gt, pred)
    optimizer.zero_grad()
    L['total'].backward()
    optimizer.step()
    last = float(L['total'].detach())
    it += 1
torch.cuda.synchronize()
w = torch.cat([p.detach().double().reshape(-1) for p in model.parameters()])
ck = float((w * torch.arange(1, w.numel() + 1, device=w.device, dtype=torch.float64).remainder(977.0)).sum())
torch.save({'iter': it, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()},
           sys.argv[1] + '.ckpt%s' % os.environ.get('RANK', '0'))
import efgh_amd.optim
json.dump({'ck': ck, 'loss': last, 'iters': it, 'optimizer': type(optimizer).__module__ + '.' + type(optimizer).__name__,
           'rebound': torch.optim.Adam is not efgh_amd.optim._TorchAdam, 'launches': 'one flat buffer' if hasattr(optimizer, 'flat') else 'stock'},
          open(sys.argv[1] + '.r%s' % os.environ.get('RANK', '0'), 'w'))
'''


def _run(cmd, timeout, **kw):
    """subprocess.run in a process group of its own: a timeout kills the launcher AND the ranks it started (they hold the GPU)"""
    import signal
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True, **kw)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        raise
    return subprocess.CompletedProcess(cmd, p.returncode, out, err)


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['PYTHONPATH'] = ROOT
    return env


def test_launcher_puts_the_fused_optimizer_under_the_unmodified_loop(tmp_path):
    import math
    import torch
    script = tmp_path / 'main.py'
    script.write_text(SCRIPT)
    out = str(tmp_path / 'out')
    r = _run([sys.executable, '-m', 'efgh_amd.run', '--fused-optimizer', str(script), out], 600, env=_env(), cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    r0 = json.load(open(out + '.r0'))
    assert r0['optimizer'] == 'efgh_amd.optim.Adam' and r0['rebound'] and r0['iters'] == 2 and math.isfinite(r0['loss'])
    # the checkpoint's optimizer entry is torch's layout: it loads into a stock torch.optim.Adam over parameters of those shapes
    sd = torch.load(out + '.ckpt0', map_location='cpu')['optimizer']
    assert len(sd['param_groups']) == 1 and len(sd['state']) == len(sd['param_groups'][0]['params']) > 300
    params = [torch.zeros_like(sd['state'][i]['exp_avg']).requires_grad_(True) for i in sd['param_groups'][0]['params']]
    stock = torch.optim.Adam(params, lr=1.0)
    stock.load_state_dict(sd)
    assert stock.param_groups[0]['lr'] == 1e-4 and float(stock.state[params[0]]['step']) == 2.0
    assert any(float(stock.state[p]['exp_avg_sq'].abs().max()) > 0 for p in params)
    for p in params:
        p.grad = torch.ones_like(p)
    stock.step()                                               # torch steps on from it
    assert float(stock.state[params[0]]['step']) == 3.0


def test_two_ranks_with_the_fused_optimizer_end_on_identical_weights(tmp_path):
    import math
    script = tmp_path / 'main.py'
    script.write_text(SCRIPT)
    out = str(tmp_path / 'out')
    r = _run([sys.executable, '-m', 'efgh_amd.run', '--gpus', '2', '--fused-optimizer', str(script), out], 900, env=_env(),
             cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = json.load(open(out + '.r0')), json.load(open(out + '.r1'))
    assert r0['optimizer'] == r1['optimizer'] == 'efgh_amd.optim.Adam' and r0['iters'] == r1['iters'] == 2
    assert r0['ck'] == r1['ck'] and math.isfinite(r0['loss']) and math.isfinite(r1['loss'])
    assert os.path.exists(out + '.ckpt0') and not os.path.exists(out + '.ckpt1')
