"""CPU-side checks: the C-ABI library loads and exports every symbol include/efgh_hip.h declares,
the host mirror reproduces the reference's module API, and the product refuses to run without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def so_path():
    from efgh_amd import build
    return build.build()


def test_header_symbols_exported(so_path):
    hdr = open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = sorted(set(re.findall(r'\b(efgh_[a-z0-9_]+)\s*\(', hdr)))
    assert len(names) >= 25
    lib = ctypes.CDLL(so_path)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.efgh_version.restype = ctypes.c_int
    want = int(re.search(r'#define\s+EFGH_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert lib.efgh_version() == want == 4  # EFGH_ABI_VERSION (include/efgh_hip.h); the Python binding refuses any other (efgh_amd/_C.py)
    # ABI 4: the one-launch lattice tail is gone.  ABI 3: no hidden hand-off between calls - the round-5 arm / disarm pair is gone, the
    # weight-gradient entry points take `out`
    assert not hasattr(lib, 'efgh_fold_unpack_arm') and not hasattr(lib, 'efgh_fold_unpack_disarm')
    for n in ('efgh_gather_wgrad', 'efgh_thin_wgrad', 'efgh_c4n4_wgrad', 'efgh_c4_wgrad', 'efgh_sc_wgrad', 'efgh_wino_wgrad', 'efgh_wino2d_wfinish'):
        decl = re.search(r'int ' + n + r'\(([^;]*)\);', hdr).group(1)
        assert 'const efgh_wgrad_out_desc *out' in decl, n
    lib.efgh_lattice_hash_capacity.restype = ctypes.c_int64
    assert lib.efgh_lattice_hash_capacity(ctypes.c_int32(131072)) == 1 << 20
    # argument validation happens before any device work: a NULL descriptor is rejected with a message
    lib.efgh_last_error.restype = ctypes.c_char_p
    assert lib.efgh_gather_gemm(None, None) == -1
    assert b'invalid argument' in lib.efgh_last_error()


def test_corr1d_bwd_checks_its_lds_size_before_the_first_launch(so_path):
    """wc * 64 + nj * 4 bytes of LDS must fit 64 KiB: the call is rejected before either of its two kernels is launched, so it
    returns the argument error (not a launch error - there is no device here) and leaves dcam alone"""
    lib = ctypes.CDLL(so_path)
    lib.efgh_last_error.restype = ctypes.c_char_p
    B, h, wc, wp = 1, 1, 1000, 2000                    # 64 000 + 4 004 > 65 536
    f = lambda n, v: (ctypes.c_float * n)(*([v] * n))
    rp, cam, mm, dl = f(h * wp * 16, 1.0), f(h * wc * 16, 1.0), f(2, 0.0), f(wp - wc + 1, 1.0)
    mm[1] = 1.0
    dcam, drp = f(h * wc * 16, -7777.0), f(h * wp * 16, -7777.0)
    rc = lib.efgh_corr1d_bwd(rp, cam, mm, dl, ctypes.c_int32(B), ctypes.c_int32(h), ctypes.c_int32(wc), ctypes.c_int32(wp), dcam, drp,
                             None)
    assert rc == -1
    msg = lib.efgh_last_error()
    assert b'invalid argument' in msg and b'64 * 1024' in msg
    assert all(v == -7777.0 for v in dcam) and all(v == -7777.0 for v in drp)


def test_gemm_desc_layout_matches_header():
    """every struct of the header against its ctypes mirror: one C probe, generated from the mirrors' _fields_, prints sizeof and
    each field's offsetof and size under the header's own field names (LP64).  A renamed, missing or reordered field fails to
    compile or to match"""
    from efgh_amd import _C
    import re, subprocess, tempfile
    hdr = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read(), flags=re.S)
    assert sorted(_C.STRUCTS) == sorted(re.findall(r'\}\s*(efgh_\w+)\s*;', hdr)) and len(_C.STRUCTS) == 8
    lines = []
    for cname, mirror in _C.STRUCTS.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, f[0], cname, f[0]) for f in mirror._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "efgh_hip.h"\nint main(void){\n%s\nreturn 0;}\n' % '\n'.join(lines)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        got = [tuple(map(int, l.split())) for l in subprocess.check_output([os.path.join(d, 'p')]).decode().splitlines()]
    want = []
    for cname, mirror in _C.STRUCTS.items():
        want.append((ctypes.sizeof(mirror),))
        want += [(getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size) for f in mirror._fields_]
    assert got == want


def test_module_api_matches_reference_manifest(manifest):
    from efgh_amd import synthetic as syn
    from efgh_amd.nets import EFGHBackbone
    import efgh_amd.nets as nets
    assert nets.__dict__['EFGH' + 'Backbone'] is EFGHBackbone           # reference main.py:126 lookup
    m = EFGHBackbone(syn.default_args((128, 256)))
    sd = m.state_dict()
    mine = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    assert mine == manifest['state_dict']                                # 637 keys, order, shapes, dtypes
    assert [k for k, _ in m.named_parameters()] == manifest['parameters']
    assert sum(p.numel() for p in m.parameters()) == 47810443
    # DataParallel-style 'module.' prefix round trip (reference main.py:127,136)
    pref = {'module.' + k: v for k, v in sd.items()}
    wrapped = torch.nn.Module()
    wrapped.module = m
    wrapped.load_state_dict(pref, strict=True)
    # init scheme
    assert abs(float(m.G.conv_img2[0].conv1.weight.std()) - 1e-3) < 2e-4
    assert float(m.E.bcn1.blur_conv[0].bias.abs().max()) == 0.0
    assert float(m.H.vgg.features[0].weight.std()) > 0.03                # kaiming fan_out


def test_product_has_no_cpu_path(manifest):
    from efgh_amd import _C, synthetic as syn
    from efgh_amd.nets import EFGHBackbone
    m = EFGHBackbone(syn.default_args((128, 256)))
    b = syn.make_batch((128, 256), 256, 1)
    with pytest.raises(_C.EfghError):
        m(*[torch.from_numpy(b[k]) for k in ('pc', 'img', 'calib', 'A')])


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'efgh_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
                assert '/root/reference' not in src, f


def test_criterion_api_matches_reference():
    """losses.EFGHCriterion: constructor, loss_name order (efghloss.py:13-17), name lookup (main.py:129)"""
    import efgh_amd.losses as losses
    from efgh_amd import synthetic as syn
    c = losses.__dict__['EFGH' + 'Criterion'](syn.default_args((128, 256)))
    assert c.loss_name == ['total', 'e_gn', 'e_gn_sgn', 'e_gn_abs', 'h_hrzn', 'h_hrzn_abs', 'h_hrzn_sgn', 'fov',
                           'g_trs', 'g_depth', 'g_mask']
    assert callable(c.compute_loss)


def test_lr_schedule_and_flat_params_cpu():
    from efgh_amd.train import FlatParams, adjust_learning_rate
    assert adjust_learning_rate(1e-4, 0) == 1e-4
    assert abs(adjust_learning_rate(1e-4, 50000) - 0.7e-4) < 1e-12          # common/helper.py:28-38
    assert abs(adjust_learning_rate(1e-4, 149999) - 0.49e-4) < 1e-12
    m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    f = FlatParams(m)
    assert f.n == 5 * 3 + 3 + 3 * 2 + 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])
    m(torch.randn(4, 5)).sum().backward()
    assert float(f.g.abs().sum()) > 0 and all(p.grad.data_ptr() >= f.g.data_ptr() for p in f.params)


def test_flat_params_shared_parameter_and_rebound_counter_cpu():
    """a parameter consumed by two layers of one forward is never claimed for a direct gradient write (all contributions go
    through autograd, one post-accumulate hook); a BatchNorm counter that no longer aliases the flat vector is counted on
    the module's own buffer"""
    from efgh_amd.nets import fn
    from efgh_amd.train import FlatParams
    m = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4), torch.nn.BatchNorm1d(4))
    f = FlatParams(m)
    w = m[0].weight
    assert f.claim(w, 0) is w.grad
    fn.note_use(w)
    assert f.uses[0] == 1 and f.claim(w, 0) is w.grad
    fn.note_use(w, None, m[0].bias)
    assert f.uses[0] == 2 and f.uses[1] == 1 and f.claim(w, 0) is None
    # counters: both alias f.nbt; rebind the second (what model.to()/.double() does)
    f.tick(0); f.tick(1)
    m[2].num_batches_tracked = m[2].num_batches_tracked.clone()
    f.flush_ticks()
    assert int(m[1].num_batches_tracked) == 1 and int(m[2].num_batches_tracked) == 1
    f.tick(0)
    f.flush_ticks()
    assert int(m[1].num_batches_tracked) == 2 and int(f.nbt[0]) == 2 and int(m[2].num_batches_tracked) == 1


def test_bn_tick_collects_one_add_per_forward():
    """ops.bn_tick: inside a collection (EFGHBackbone.forward) the counters are bumped together at flush time, a layer that
    ran twice counts twice; outside of one the counter moves at once (a sub-network called on its own)"""
    from efgh_amd import ops
    a, b = torch.nn.BatchNorm1d(4), torch.nn.BatchNorm1d(4)
    ops.bn_tick(a)
    assert int(a.num_batches_tracked) == 1
    assert ops.nbt_collect() is True and ops.nbt_collect() is False          # (a nested forward does not own the collection)
    ops.bn_tick(a); ops.bn_tick(b); ops.bn_tick(b)
    assert int(a.num_batches_tracked) == 1 and int(b.num_batches_tracked) == 0
    va = a.num_batches_tracked._version
    ops.nbt_flush()
    assert int(a.num_batches_tracked) == 2 and int(b.num_batches_tracked) == 2
    assert a.num_batches_tracked._version > va            # (layers._bn_eval_affine keys its cache on the version)
    assert ops.TLS.nbt_pending is None
    ops.bn_tick(torch.nn.BatchNorm1d(4, track_running_stats=False))           # no counter: nothing to do


def test_header_is_plain_c():
    """the boundary is a C ABI: include/efgh_hip.h must compile as C99 (no C++ or torch types in the signatures)"""
    import os
    import subprocess
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'efgh_hip.h')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', hdr])


def test_zero_edit_launcher_binds_nets_and_losses(tmp_path):
    """`python -m efgh_amd.run script.py args` (reference main.py:14-15,126-129 unchanged): `import nets, losses` inside the
    script resolve to the MI355X packages, sys.argv / sys.path[0] are what `python script.py args` would see, the process is
    pinned to one device before anything initialises the GPU, and the script's own sibling modules still import"""
    import json
    import subprocess
    import sys
    (tmp_path / 'iterater.py').write_text('MARK = "sibling module of the script"\n')
    (tmp_path / 'main.py').write_text(
        'import os, sys, json\n'
        'import nets\nimport losses\nimport iterater\n'
        'from nets.efghbackbone import EFGHBackbone as B2\n'
        'model_cls = nets.__dict__["EFGH" + "Backbone"]\n'
        'crit_cls = losses.__dict__["EFGH" + "Criterion"]\n'
        'assert B2 is model_cls\n'
        'json.dump({"model": model_cls.__module__, "crit": crit_cls.__module__, "argv": sys.argv, "path0": sys.path[0],\n'
        '           "name": __name__, "sibling": iterater.MARK, "hip": os.environ.get("HIP_VISIBLE_DEVICES")},\n'
        '          open(sys.argv[2], "w"))\n')
    out = tmp_path / 'out.json'
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='3,5')
    env.pop('CUDA_VISIBLE_DEVICES', None)
    subprocess.check_call([sys.executable, '-m', 'efgh_amd.run', '--device', '1', str(tmp_path / 'main.py'), 'cfg.yaml', str(out)],
                          env=env, cwd=str(tmp_path))
    got = json.load(open(out))
    assert got['model'] == 'efgh_amd.nets.efghbackbone' and got['crit'] == 'efgh_amd.losses.efghloss'
    assert got['argv'] == [str(tmp_path / 'main.py'), 'cfg.yaml', str(out)] and got['path0'] == str(tmp_path)
    assert got['name'] == '__main__' and got['sibling'].startswith('sibling') and got['hip'] == '5'
    # --all-devices leaves the visibility alone
    subprocess.check_call([sys.executable, '-m', 'efgh_amd.run', '--all-devices', str(tmp_path / 'main.py'), 'cfg.yaml', str(out)],
                          env=env, cwd=str(tmp_path))
    assert json.load(open(out))['hip'] == '3,5'


def test_dataparallel_replica_is_refused_loudly():
    """torch.nn.DataParallel over more than one device (main.py:127 on a multi-GPU box) marks its per-forward copies with
    `_is_replica`: the backbone refuses them with the one-process-per-GPU recipe instead of running a half-supported schedule"""
    from efgh_amd import _C, synthetic as syn
    from efgh_amd.nets import EFGHBackbone
    m = EFGHBackbone(syn.default_args((128, 256)))
    m._is_replica = True                      # what torch.nn.parallel.replicate sets on every replica
    z = torch.zeros(1)
    with pytest.raises(_C.EfghError, match='ONE PROCESS PER GPU'):
        m(z, z, z, z)


def test_launcher_gpus_n_runs_the_unchanged_script_data_parallel(tmp_path):
    """`python -m efgh_amd.run --gpus 2 script.py`: the reference's multi-GPU mode is `torch.nn.DataParallel(model)` (main.py:127);
    here every GPU gets its own process and the SAME unmodified script.  Plumbing check on CPU ranks (gloo) with a stand-in
    model: `torch.nn.DataParallel` is the process-parallel wrapper (`.module`, `module.`-prefixed state_dict), every rank starts
    from rank 0's weights, a DataLoader without a sampler is sharded (disjoint halves of the epoch, batch_size / world samples
    per step), the gradients are averaged right before `optimizer.step()` (the ranks stay identical although they see
    different data), and only rank 0's `torch.save` writes."""
    import json
    import subprocess
    import sys
    (tmp_path / 'main.py').write_text(
        'import os, sys, json\n'
        'import torch, torch.nn as tnn, torch.utils.data as tud\n'
        'import nets, losses\n'
        'rank = int(os.environ["RANK"])\n'
        'torch.manual_seed(100 + rank)                      # different initial weights per rank: the wrapper must broadcast\n'
        'model = tnn.Sequential(tnn.Linear(4, 3), tnn.BatchNorm1d(3))\n'
        'model = torch.nn.DataParallel(model)\n'
        'opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)\n'
        'data = tud.TensorDataset(torch.arange(32, dtype=torch.float32).repeat(4, 1).t().contiguous())\n'
        'loader = torch.utils.data.DataLoader(data, batch_size=8, shuffle=True)\n'
        'seen = []\n'
        'for epoch in range(2):\n'
        '    for (x,) in loader:\n'
        '        seen.append([int(v) for v in x[:, 0]])\n'
        '        opt.zero_grad(); model(x).pow(2).mean().backward(); opt.step()\n'
        'torch.save({"state_dict": model.state_dict()}, sys.argv[1] + ".ckpt%d" % rank)\n'
        'w = torch.cat([p.detach().reshape(-1) for p in model.parameters()])\n'
        'json.dump({"cls": type(model).__name__, "keys": list(model.state_dict().keys()), "w": w.tolist(), "seen": seen,\n'
        '           "model_cls": nets.__dict__["EFGHBackbone"].__module__}, open(sys.argv[1] + ".r%d" % rank, "w"))\n')
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='', EFGH_DIST_BACKEND='gloo')
    env.pop('CUDA_VISIBLE_DEVICES', None)
    subprocess.check_call([sys.executable, '-m', 'efgh_amd.run', '--gpus', '2', str(tmp_path / 'main.py'), out], env=env,
                          cwd=str(tmp_path), timeout=300)
    r0, r1 = json.load(open(out + '.r0')), json.load(open(out + '.r1'))
    assert r0['cls'] == 'ProcessDataParallel' and r0['model_cls'] == 'efgh_amd.nets.efghbackbone'
    assert r0['keys'][0].startswith('module.') and r0['keys'] == r1['keys']
    assert r0['w'] == r1['w']                                  # same start (broadcast) + averaged gradients = identical replicas
    for e in range(2):                                         # every epoch: 2 steps of 8 // 2 = 4... 16 samples per rank, disjoint, together all 32
        a = sorted(v for b in r0['seen'][4 * e:4 * e + 4] for v in b)
        b = sorted(v for b_ in r1['seen'][4 * e:4 * e + 4] for v in b_)
        assert len(a) == len(b) == 16 and sorted(a + b) == list(range(32))
    assert all(len(b) == 4 for b in r0['seen'])
    assert r0['seen'][:4] != r0['seen'][4:8]                   # reshuffled in the second epoch
    assert os.path.exists(out + '.ckpt0') and not os.path.exists(out + '.ckpt1')


_MAIN_SHAPED = r'''
# shaped like the reference's main.py:23-209 + common/helper.py:40-61 + iterater.py:25-106 (stand-in model / data; same file,
# prompt, loader, checkpoint and cache calls in the same order)
import os, sys, json, shutil
import torch, torch.nn as tnn, torch.utils.data as tud
import yaml
import nets, losses

def query_yes_no(question):
    sys.stdout.write(question + ' [y/n] ')
    return {'y': True, 'yes': True, 'n': False, 'no': False}[input().lower()]

def save_checkpoint(state, is_best, ckpt_dir, filename='checkpoint.pth.tar', iter_iterval=2):
    torch.save(state, os.path.join(ckpt_dir, filename))
    if state['iter'] % iter_iterval == 0:
        shutil.copyfile(os.path.join(ckpt_dir, filename), os.path.join(ckpt_dir, 'checkpoint_' + str(state['iter']) + '.pth.tar'))
    if is_best:
        shutil.copyfile(os.path.join(ckpt_dir, filename), os.path.join(ckpt_dir, 'model_best.pth.tar'))
    if state['iter'] > 1 * iter_iterval:
        prev = os.path.join(ckpt_dir, 'checkpoint_' + str(state['iter'] - 1 * iter_iterval) + '.pth.tar')
        if os.path.exists(prev):
            os.remove(prev)

with open(sys.argv[1]) as f:
    args = yaml.safe_load(f)
rank = int(os.environ.get('RANK', '0'))
if args['test'] is False and os.path.exists(args['ckpt_dir']):
    if args['resume_path'] is False:
        if query_yes_no('ckpt_dir exists, continue?'):
            for root, dirs, files in os.walk(args['ckpt_dir'], topdown=False):
                for name in files:
                    os.remove(os.path.join(root, name))
                for name in dirs:
                    os.rmdir(os.path.join(root, name))
        else:
            sys.exit(1)
if args['test'] is False:
    os.makedirs(args['ckpt_dir'], mode=0o777, exist_ok=True)
    shutil.copyfile(sys.argv[1], os.path.join(args['ckpt_dir'], 'config.yaml'))
train = tud.TensorDataset(torch.arange(32, dtype=torch.float32).repeat(4, 1).t().contiguous())
val = tud.TensorDataset(torch.arange(100, 112, dtype=torch.float32).repeat(4, 1).t().contiguous())
train_loader = torch.utils.data.DataLoader(train, batch_size=args['batch_size'], shuffle=True, num_workers=0)
val_loader = torch.utils.data.DataLoader(val, batch_size=args['batch_size'], shuffle=False, num_workers=0)
torch.manual_seed(100 + rank)
model = torch.nn.DataParallel(tnn.Sequential(tnn.Linear(4, 3), tnn.BatchNorm1d(3)))
optimizer = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
it, seen_train, seen_val, best = 0, [], [], None
for epoch in range(2):
    for (x,) in train_loader:
        seen_train.append([int(v) for v in x[:, 0]])
        optimizer.zero_grad(); model(x).pow(2).mean().backward(); optimizer.step()
        it += 1
        if it % 2 == 0:
            with torch.no_grad():
                model.eval()
                tot = 0.0
                for (v,) in val_loader:
                    seen_val.append([int(q) for q in v[:, 0]])
                    tot += float(model(v).pow(2).mean())
                model.train()
            is_best = best is None or tot < best
            best = tot if is_best else best
            save_checkpoint({'iter': it, 'state_dict': model.state_dict(), 'min_loss': best, 'optimizer': optimizer.state_dict()},
                            is_best, args['ckpt_dir'])
        torch.cuda.empty_cache()
w = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
json.dump({'w': w.tolist(), 'train': seen_train, 'val': seen_val, 'iters': it}, open(sys.argv[2] + '.r%d' % rank, 'w'))
'''


def _write_main_shaped(tmp_path, test=False):
    import yaml
    ck = tmp_path / 'ckpt'
    (tmp_path / 'main.py').write_text(_MAIN_SHAPED)
    cfg = {'test': 'odom' if test else False, 'ckpt_dir': str(ck), 'resume_path': False, 'pretrained_path': False, 'batch_size': 4}
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    return ck


def test_launcher_gpus_n_on_a_main_py_shaped_script(tmp_path):
    """the round-4 advisor's finding: under `--gpus N` EVERY rank runs the whole unmodified script, so main.py's pre-model section
    (ckpt_dir exists -> prompt on the shared stdin -> wipe -> config copy, main.py:45-75) and `save_checkpoint`'s copies and pruning
    (common/helper.py:40-61) must not race.  Two gloo ranks on a script with exactly those calls: an old file in ckpt_dir is wiped
    once (rank 0 asked, answer 'y' on stdin), config.yaml and the checkpoints rank 0 wrote survive the other rank's pass through the
    same lines and load cleanly, the shuffled (training) loader is sharded while the validation loader stays WHOLE on both ranks,
    the replicas end identical, `torch.cuda.empty_cache()` per iteration is a no-op, exit code 0."""
    import json
    import subprocess
    import sys
    ck = _write_main_shaped(tmp_path)
    ck.mkdir()
    (ck / 'stale.txt').write_text('left over from an earlier run')
    (ck / 'sub').mkdir()
    (ck / 'sub' / 'old.bin').write_text('x')
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='', EFGH_DIST_BACKEND='gloo')
    env.pop('CUDA_VISIBLE_DEVICES', None)
    r = subprocess.run([sys.executable, '-m', 'efgh_amd.run', '--gpus', '2', str(tmp_path / 'main.py'), str(tmp_path / 'cfg.yaml'), out],
                       env=env, cwd=str(tmp_path), input='y\n', capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r0, r1 = json.load(open(out + '.r0')), json.load(open(out + '.r1'))
    assert r0['w'] == r1['w']
    # training loader: 32 samples, global batch 4 -> 2 per rank and step, 8 steps per epoch; disjoint halves
    assert r0['iters'] == r1['iters'] == 16 and all(len(b) == 2 for b in r0['train'] + r1['train'])
    for e in range(2):
        a = sorted(v for b in r0['train'][8 * e:8 * e + 8] for v in b)
        b = sorted(v for b_ in r1['train'][8 * e:8 * e + 8] for v in b_)
        assert sorted(a + b) == list(range(32))
    # validation loader: whole on both ranks, config batch size
    for rr in (r0, r1):
        assert len(rr['val']) == 8 * 3 and all(len(b) == 4 for b in rr['val'])
        assert sorted(v for b in rr['val'][:3] for v in b) == list(range(100, 112))
    names = sorted(os.listdir(ck))
    assert 'stale.txt' not in names and 'sub' not in names and 'config.yaml' in names
    # iterations 2..16 step 2 were checkpointed; save_checkpoint prunes iter - 2: only the last numbered copy + its predecessor's successor remain
    assert 'checkpoint.pth.tar' in names and 'model_best.pth.tar' in names and 'checkpoint_16.pth.tar' in names
    assert 'checkpoint_2.pth.tar' not in names
    for n in ('checkpoint.pth.tar', 'model_best.pth.tar', 'checkpoint_16.pth.tar'):
        sd = torch.load(str(ck / n), map_location='cpu', weights_only=False)
        assert sd['state_dict']['module.0.weight'].shape == (3, 4)
    assert torch.load(str(ck / 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)['iter'] == 16


def test_launcher_gpus_n_first_failing_rank_ends_the_job(tmp_path):
    """a rank that exits early leaves its siblings blocked in a collective: the parent polls, terminates them and returns the
    failing rank's code instead of waiting for rank 0 forever"""
    import subprocess
    import sys
    import time
    (tmp_path / 'main.py').write_text(
        'import os, sys, torch, torch.nn as tnn\n'
        'rank = int(os.environ["RANK"])\n'
        'model = torch.nn.DataParallel(tnn.Linear(4, 3))\n'
        'if rank == 1:\n'
        '    sys.exit(7)\n'
        'opt = torch.optim.Adam(model.parameters(), lr=1e-2)\n'
        'model(torch.ones(2, 4)).sum().backward()\n'
        'opt.step()                      # all-reduce that rank 1 never joins\n')
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='', EFGH_DIST_BACKEND='gloo')
    env.pop('CUDA_VISIBLE_DEVICES', None)
    t0 = time.time()
    r = subprocess.run([sys.executable, '-m', 'efgh_amd.run', '--gpus', '2', str(tmp_path / 'main.py')], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 7, (r.returncode, r.stderr[-1000:])
    assert time.time() - t0 < 120


def test_launcher_refuses_gpus_n_for_a_test_configuration(tmp_path):
    import subprocess
    import sys
    _write_main_shaped(tmp_path, test=True)
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, '-m', 'efgh_amd.run', '--gpus', '2', str(tmp_path / 'main.py'), str(tmp_path / 'cfg.yaml'), 'x'],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and 'single process' in r.stderr


def test_bench_line_is_compact(capsys, tmp_path):
    """the driver keeps a bounded tail of bench.py's stdout (round 5's 20-KB line was recorded as `parsed: null`): the ONE stdout line
    is a short object built by `bench.compact_line` from the full result, which goes to a file.  Run on a committed full object."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_default.json')))
    detail = tmp_path / 'detail.json'
    bench.emit(full, str(detail))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) < 8192
    c = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline', 'roofline_fracs', 'forward_value', 'config_r'):
        assert k in c, k
    assert c['config']['workload'].startswith('BASELINE.json configs[2]') and 'model' not in c['config']
    r = c['roofline']
    assert r['bound'] in ('hbm', 'mfma') and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and 'traffic' in r and r['unit'] == 'TFLOP/s'
    cb = c['cpu_baseline']
    assert cb['kind'] == 'port' and cb['cores'] == 32 and cb['value'] > 0 and cb['sample']
    assert abs(c['value'] - full['value']) < 1e-3 and abs(c['ms_per_step'] - full['ms_per_step']) < 1e-3
    for k in ('bcl', 'gemm', 'wgrad', 'wino', 'wino_wgrad', 'wino2d_gemm', 'hbm_convs', 'resnet_branch', 'mfma_step'):
        assert 0 < c['roofline_fracs'][k] <= 1, k
    assert json.load(open(detail)) == full


def test_bench_plain_line_names_no_side_measurement(capsys, tmp_path, monkeypatch):
    """`--full` is off by default, and the line of a plain run carries the headline and what describes the run - no roofline,
    CPU-baseline, forward-only or config_r entry, which only `--full` measures."""
    import importlib.util
    import json
    import sys
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.full is False and (a.steps, a.warmup, a.dump_outputs) == (7, 2, None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full'])
    assert bench.parse().full is True
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_default.json')))
    head = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
            'data', 'config')
    plain = {k: full[k] for k in head}
    plain.update(full=False, outside_steps_s=4.25)
    bench.emit(plain, str(tmp_path / 'detail.json'))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    c = json.loads(lines[0])
    for k in head:
        assert k in c, k
    assert c['full'] is False and c['outside_steps_s'] == 4.25
    assert abs(c['value'] - full['value']) < 1e-3 and abs(c['ms_per_step'] - full['ms_per_step']) < 1e-3
    assert not [k for k in c if k.startswith(('roofline', 'forward', 'cpu_baseline', 'config_r'))], sorted(c)
