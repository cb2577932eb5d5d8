"""Parameter groups of the fused optimizer, host side: the segment table, every refusal (with the group named), torch's state_dict
numbering for interleaved groups, the launcher's --fused-optimizer flag, and the decoupled recipe of efgh_adam_step_groups restated
in numpy fp32 against torch.optim.AdamW on the CPU.  Nothing here touches a GPU (train.FlatParams / FusedAdam are built over CPU
tensors, as the gloo plumbing tests build them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C
from efgh_amd.io import checkpoint as ck
from efgh_amd.train import FlatParams, FusedAdam, adam_segment_table, named_param_groups

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_contract as contract  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3,), (2, 2), (5,), (1,), (4,)]


def _flat(shapes=SHAPES):
    return FlatParams.from_params([torch.full(s, float(i + 1)).requires_grad_(True) for i, s in enumerate(shapes)])


def test_segment_table_merges_adjacent_parameters_of_a_group():
    # sizes 3, 4, 5, 1, 4 -> ends 3, 7, 12, 13, 17
    assert adam_segment_table([3, 4, 5, 1, 4], [0, 0, 1, 1, 0]) == ([7, 13, 17], [0, 1, 0])
    assert adam_segment_table([3, 4, 5, 1, 4], [2, 2, 2, 2, 2]) == ([17], [2])
    assert adam_segment_table([3, 0, 5], [0, 1, 0]) == ([8], [0])                    # an empty parameter cuts nothing
    assert adam_segment_table([1] * 6, [0, 1, 0, 1, 0, 1]) == ([1, 2, 3, 4, 5, 6], [0, 1, 0, 1, 0, 1])
    with pytest.raises(_C.EfghError, match='segments'):
        adam_segment_table([1] * (_C.ADAM_MAX_SEGMENTS + 1), [i % 2 for i in range(_C.ADAM_MAX_SEGMENTS + 1)])
    adam_segment_table([1] * _C.ADAM_MAX_SEGMENTS, [i % 2 for i in range(_C.ADAM_MAX_SEGMENTS)])      # the cap itself is fine
    opt = FusedAdam(_flat(), groups=[{'params': [0, 1, 4]}, {'params': [2, 3], 'lr': 1e-5}])
    assert opt.seg_table == ([7, 13, 17], [0, 1, 0]) and opt.group_of == [0, 0, 1, 1, 0]
    assert opt._seg_ends.tolist() == [7, 13, 17] and opt._seg_gids.tolist() == [0, 1, 0] and opt._seg_ends.dtype == torch.int64
    assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-5] and [g['decoupled'] for g in opt.param_groups] == [False, False]
    assert FusedAdam(_flat()).param_groups is None                                   # without groups nothing of this exists


def test_groups_by_name_first_match_wins_and_the_rest_is_the_default_group():
    names = ['E.conv.weight', 'E.bn.weight', 'G.conv.weight', 'G.conv.bias', 'H.fc.weight']
    groups = named_param_groups(names, [{'names': ['G.'], 'lr': 1e-4},
                                        {'names': lambda k: k.endswith('.bias') or '.bn.' in k, 'weight_decay': 0.0, 'name': 'no_decay'}])
    assert [g['params'] for g in groups] == [[2, 3], [1], [0, 4]]                    # G.conv.bias went to the first match
    assert [g['name'] for g in groups] == ['G.', 'no_decay', 'default'] and groups[0]['lr'] == 1e-4 and 'lr' not in groups[2]
    assert [g['params'] for g in named_param_groups(names, [{'names': 'E.'}, {'names': ['G.', 'H.']}])] == [[0, 1], [2, 3, 4]]
    with pytest.raises(_C.EfghError, match=r'param_groups\[0\]'):
        named_param_groups(names, [{'lr': 1.0}])


REFUSALS = [
    ([{'params': [i]} for i in range(5)] * 4, r'group 16'),                            # 20 groups
    ([{'params': [0, 1, 2]}, {'params': [2, 3, 4]}], r'group 1: parameter 2 is in group 0'),
    ([{'params': [0, 1, 2]}, {'params': [3]}], r'parameter 4 is in no group'),
    ([{'params': [0, 1, 2, 3, 4]}, {'params': [], 'name': 'heads'}], r'group 1 \(heads\) is empty'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'betas': (0.8, 0.999)}], r'group 1: betas .* shared'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'eps': 1e-6}], r'group 1: eps .* shared'),
    ([{'params': [0, 1, 2, 3, 4], 'amsgrad': True}], r'group 0: amsgrad'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'maximize': True}], r'group 1: maximize'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'lr': float('nan')}], r'group 1: lr'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'lr': -1e-3}], r'group 1: lr'),
    ([{'params': [0, 1, 2, 3]}, {'params': [4], 'lr': float('inf')}], r'group 1: lr'),
    ([{'params': [0, 1, 2, 3], 'weight_decay': -0.1}, {'params': [4]}], r'group 0: weight_decay'),
    ([{'params': [0, 1, 2, 3], 'weight_decay': float('nan')}, {'params': [4]}], r'group 0: weight_decay'),
]


@pytest.mark.parametrize('groups,message', REFUSALS, ids=[m for _, m in REFUSALS])
def test_refusals_name_the_group(groups, message):
    with pytest.raises(_C.EfghError, match=message):
        FusedAdam(_flat(), groups=groups)


def test_optimizer_class_refusals():
    from efgh_amd.optim import Adam, AdamW
    ps = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    for kw in ({'amsgrad': True}, {'maximize': True}, {'foreach': True}, {'fused': True}, {'capturable': True},
               {'differentiable': True}):
        with pytest.raises(_C.EfghError, match=list(kw)[0]):
            Adam([p.detach().clone().requires_grad_(True) for p in ps], **kw)
    with pytest.raises(_C.EfghError, match='group 1'):
        Adam([{'params': [torch.zeros(3, requires_grad=True)]}, {'params': [torch.zeros(2, requires_grad=True)], 'betas': (0.5, 0.9)}])
    with pytest.raises(TypeError):
        Adam([torch.zeros(3, requires_grad=True)], nesterov=True)
    # falsy / None values of torch's switches are accepted, as torch's own call sites pass them
    opt = Adam([torch.zeros(3, requires_grad=True)], lr=1e-3, foreach=None, fused=None, capturable=False, differentiable=False, maximize=False)
    assert isinstance(opt, torch.optim.Optimizer) and opt.param_groups[0]['lr'] == 1e-3 and opt.fused.param_groups is None
    with pytest.raises(_C.EfghError, match='add_param_group'):
        opt.add_param_group({'params': [torch.zeros(1, requires_grad=True)]})
    w = AdamW([torch.zeros(3, requires_grad=True)])
    assert w.param_groups[0]['weight_decay'] == 1e-2 and w.fused.param_groups[0]['decoupled'] is True
    # the flat order is the order of the groups, then of the parameters within each: every group is one segment
    a, b, c = (torch.zeros(k, requires_grad=True) for k in (3, 5, 2))
    two = Adam([{'params': [c, a], 'lr': 1e-2}, {'params': [b]}], lr=1e-3, weight_decay=0.1)
    assert two.flat.params[0] is c and two.flat.params[2] is b and two.fused.seg_table == ([5, 10], [0, 1])
    assert [g['lr'] for g in two.fused.param_groups] == [1e-2, 1e-3]
    assert c.data_ptr() == two.flat.w.data_ptr() and a.data_ptr() == two.flat.w.data_ptr() + 4 * 2


def test_values_written_between_steps():
    """what a loop or a scheduler writes into a param_group: any number float() converts is an lr; changed betas / eps are refused"""
    from efgh_amd.optim import Adam
    from efgh_amd.train import check_group_value
    assert check_group_value('lr', 'group 0', np.float32(0.5)) == 0.5 and check_group_value('lr', 'group 0', torch.tensor(0.25)) == 0.25
    assert check_group_value('lr', 'group 0', np.float64(1e-3)) == 1e-3 and check_group_value('lr', 'group 0', 0) == 0.0
    for bad in (True, 'x', None, float('nan'), np.float32('inf'), -1.0, torch.tensor([1.0, 2.0])):
        with pytest.raises(_C.EfghError, match='group 0: lr'):
            check_group_value('lr', 'group 0', bad)
    opt = Adam([{'params': [torch.zeros(3, requires_grad=True)]}, {'params': [torch.zeros(2, requires_grad=True)], 'lr': 1e-2}])
    opt.param_groups[0]['lr'] = np.float32(0.5)
    opt.param_groups[1]['initial_lr'] = 1e-2                       # (what torch's schedulers add)
    opt._sync_groups()
    assert opt.fused.param_groups[0]['lr'] == np.float32(0.5)
    sd = opt.state_dict()
    assert sd['param_groups'][1]['initial_lr'] == 1e-2 and 'initial_lr' not in sd['param_groups'][0]
    opt.param_groups[1]['betas'] = (0.5, 0.999)
    with pytest.raises(_C.EfghError, match='group 1: betas / eps were changed'):
        opt._sync_groups()
    opt.param_groups[1]['betas'] = (0.9, 0.999)
    opt.param_groups[0]['eps'] = 1e-6
    with pytest.raises(_C.EfghError, match='group 0: betas / eps were changed'):
        opt._sync_groups()
    assert len(opt.state) == 0                                     # the moments live in the flat buffers


def test_decoupled_choice_of_a_checkpoint_must_be_the_optimizers():
    coupled = FusedAdam(_flat(), groups=[{'params': [0, 1, 2]}, {'params': [3, 4]}])
    mixed = FusedAdam(_flat(), groups=[{'params': [0, 1, 2]}, {'params': [3, 4], 'decoupled': True}])
    with pytest.raises(_C.EfghError, match=r'group 1 of the optimizer state has decoupled \(AdamW\) weight decay'):
        ck.load_adam_state(coupled, ck.adam_state_dict(mixed))
    with pytest.raises(_C.EfghError, match=r'group 1 of the optimizer state has coupled \(Adam\) weight decay'):
        ck.load_adam_state(mixed, ck.adam_state_dict(coupled))
    ck.load_adam_state(mixed, ck.adam_state_dict(mixed))
    ps = [torch.zeros(s, requires_grad=True) for s in SHAPES]
    with pytest.raises(_C.EfghError, match='group 0 of the optimizer state has decoupled'):
        ck.load_adam_state(FusedAdam(_flat()), torch.optim.AdamW(ps).state_dict())         # AdamW into the plain coupled step
    ck.load_adam_state(FusedAdam(_flat()), torch.optim.Adam(ps).state_dict())


def _fill(opt, t):
    opt.m.copy_(torch.arange(opt.flat.n, dtype=torch.float32))
    opt.v.copy_(torch.arange(opt.flat.n, dtype=torch.float32) * 10.0)
    opt.t = t


def test_state_dict_numbers_interleaved_groups_group_by_group():
    groups = [{'params': [0, 2, 4], 'lr': 1e-3}, {'params': [1, 3], 'lr': 1e-5, 'weight_decay': 0.1, 'decoupled': True}]
    opt = FusedAdam(_flat(), lr=1e-4, groups=groups)
    _fill(opt, 2)
    sd = ck.adam_state_dict(opt)
    assert [g['params'] for g in sd['param_groups']] == [[0, 1, 2], [3, 4]]
    assert [g['lr'] for g in sd['param_groups']] == [1e-3, 1e-5] and [g['weight_decay'] for g in sd['param_groups']] == [0.0, 0.1]
    assert [g['decoupled_weight_decay'] for g in sd['param_groups']] == [False, True]
    order = [0, 2, 4, 1, 3]                                        # state_dict number j is flat parameter order[j]
    for j, i in enumerate(order):
        off, k = opt.flat.offsets[i]
        assert tuple(sd['state'][j]['exp_avg'].shape) == SHAPES[i] and float(sd['state'][j]['step']) == 2.0
        assert sd['state'][j]['exp_avg'].reshape(-1).tolist() == list(range(off, off + k))
    # torch loads it over the same groups, and what torch saves comes back to the same places
    ps = [torch.zeros(s, requires_grad=True) for s in SHAPES]
    stock = torch.optim.Adam([{'params': [ps[0], ps[2], ps[4]]}, {'params': [ps[1], ps[3]]}])
    stock.load_state_dict(sd)
    assert stock.state[ps[3]]['exp_avg_sq'].reshape(-1).tolist() == [10.0 * opt.flat.offsets[3][0]]
    assert stock.param_groups[1]['lr'] == 1e-5 and stock.param_groups[1]['decoupled_weight_decay'] is True
    back = FusedAdam(_flat(), lr=1e-4, groups=[{'params': [0, 2, 4]}, {'params': [1, 3], 'decoupled': True}])
    ck.load_adam_state(back, stock.state_dict())
    assert torch.equal(back.m, opt.m) and torch.equal(back.v, opt.v) and back.t == 2
    assert [g['lr'] for g in back.param_groups] == [1e-3, 1e-5] and back.param_groups[1]['weight_decay'] == 0.1
    # mismatches are named
    with pytest.raises(_C.EfghError, match=r'2 parameter group\(s\), this optimizer 1'):
        ck.load_adam_state(FusedAdam(_flat()), sd)
    with pytest.raises(_C.EfghError, match=r'group 0 .* holds 3 parameters, this optimizer\'s 2'):
        ck.load_adam_state(FusedAdam(_flat(), groups=[{'params': [0, 2]}, {'params': [1, 3, 4]}]), sd)
    # without groups: today's dict, key for key
    plain = FusedAdam(_flat(), lr=1e-3, weight_decay=0.01)
    _fill(plain, 1)
    one = ck.adam_state_dict(plain)
    assert list(one) == ['state', 'param_groups'] and len(one['param_groups']) == 1
    assert list(one['param_groups'][0]) == ['lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable',
                                            'differentiable', 'fused', 'params']
    assert one['param_groups'][0]['params'] == [0, 1, 2, 3, 4] and sorted(one['state']) == [0, 1, 2, 3, 4]
    again = FusedAdam(_flat())
    ck.load_adam_state(again, one)
    assert again.lr == 1e-3 and again.wd == 0.01 and torch.equal(again.m, plain.m) and again.t == 1


def test_trainer_schedule_multiplies_every_groups_own_base_rate():
    from efgh_amd.train import Trainer
    model = torch.nn.Sequential()
    model.add_module('E', torch.nn.Linear(2, 2))
    model.add_module('G', torch.nn.Linear(2, 1))
    tr = Trainer(model, None, lr=1e-3, param_groups=[{'names': ['G.'], 'lr': 1e-4}])
    assert [g['params'] for g in tr.opt.param_groups] == [[2, 3], [0, 1]] and tr.group_base_lr == [1e-4, 1e-3]
    tr.it = 100000
    tr._begin('step')
    assert [g['lr'] for g in tr.opt.param_groups] == [1e-4 * 0.7 ** 2, 1e-3 * 0.7 ** 2]
    sd = ck.adam_state_dict(tr.opt)
    assert [g['params'] for g in sd['param_groups']] == [[0, 1], [2, 3]]
    with pytest.raises(_C.EfghError, match=r'group 0 \(F\.\) is empty'):
        Trainer(torch.nn.Sequential(torch.nn.Linear(2, 2)), None, param_groups=[{'names': ['F.']}])


def test_launcher_flags_are_taken_in_front_of_parse():
    from efgh_amd import run
    opts, rest = run.take_optimizer_flags(['--gpus', '2', '--fused-optimizer', '--max-grad-norm', '5', '--skip-nonfinite',
                                           'main.py', 'cfg.yaml', '--fused-optimizer'])
    assert opts == {'fused': True, 'max_grad_norm': 5.0, 'skip_nonfinite': True}
    assert rest == ['--gpus', '2', 'main.py', 'cfg.yaml', '--fused-optimizer']         # what follows the script is the script's
    assert run.parse(rest) == (0, True, 2, 'main.py', ['cfg.yaml', '--fused-optimizer'], None)
    opts, rest = run.take_optimizer_flags(['--fp32-precision', 'high', '--max-grad-norm=0.5', '--fused-optimizer', '--device=1', 'm.py'])
    assert opts == {'fused': True, 'max_grad_norm': 0.5, 'skip_nonfinite': False}
    assert run.parse(rest) == (1, True, 1, 'm.py', [], 'high')
    opts, rest = run.take_optimizer_flags(['--device', '1', 'main.py', 'cfg.yaml'])
    assert opts == {'fused': False, 'max_grad_norm': None, 'skip_nonfinite': False} and rest == ['--device', '1', 'main.py', 'cfg.yaml']
    assert len(run.parse(rest)) == 6
    for bad in (['--skip-nonfinite', 'm.py'], ['--fused-optimizer', '--max-grad-norm', '-1', 'm.py'],
                ['--fused-optimizer', '--max-grad-norm', 'x', 'm.py'], ['--fused-optimizer', '--max-grad-norm']):
        with pytest.raises(SystemExit):
            run.take_optimizer_flags(bad)


def test_launcher_rebinds_torch_optim_only_with_the_flag(tmp_path):
    (tmp_path / 'main.py').write_text(
        'import json, sys\n'
        'import torch\n'
        'import efgh_amd.optim\n'
        'opt = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=1e-2)\n'
        'json.dump({"adam": issubclass(torch.optim.Adam, efgh_amd.optim.Adam), "adamw": issubclass(torch.optim.AdamW, efgh_amd.optim.AdamW),\n'
        '           "is": torch.optim.Adam is efgh_amd.optim.Adam, "guarded": getattr(getattr(opt, "fused", None), "guarded", None),\n'
        '           "max_grad_norm": getattr(getattr(opt, "fused", None), "max_grad_norm", None)}, open(sys.argv[1], "w"))\n')
    out = tmp_path / 'out.json'
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='')
    env.pop('CUDA_VISIBLE_DEVICES', None)

    def launch(*flags):
        subprocess.check_call([sys.executable, '-m', 'efgh_amd.run'] + list(flags) + [str(tmp_path / 'main.py'), str(out)], env=env,
                              cwd=str(tmp_path), timeout=300)
        return json.load(open(out))
    assert launch() == {'adam': False, 'adamw': False, 'is': False, 'guarded': None, 'max_grad_norm': None}
    assert launch('--fused-optimizer') == {'adam': True, 'adamw': True, 'is': True, 'guarded': False, 'max_grad_norm': None}
    got = launch('--fused-optimizer', '--max-grad-norm', '2.5', '--skip-nonfinite')
    assert got == {'adam': True, 'adamw': True, 'is': False, 'guarded': True, 'max_grad_norm': 2.5}


def test_decoupled_recipe_in_numpy_fp32_is_adamw():
    """the decoupled group's recipe of efgh_adam_step_groups (include/efgh_hip.h) restated in numpy fp32, one step from zero moments
    on the contract inputs, against torch.optim.AdamW on the CPU in fp32.  The two round differently (torch forms lr / bc1 and
    sqrt(bc2) in float64, and its addcdiv is not a fused multiply-add), so they are held to a bound, not to equal bits:
      decay  both multiply w by the SAME fp32 factor with one fp32 product: no difference
      u      the update term lr / bc1 * m / (sqrt(v) / bc2_sqrt + eps) goes through at most 8 fp32 roundings on either side (two
             products for m, two for v, the root, two quotients, the sum with eps): 16 * 2^-24 = 2^-20 of |u| between the two,
             doubled for second-order terms
      w - u  one rounding on either side: 2^-24 |w| each
      subnormal products: a product that lands below 2^-126 is rounded to a multiple of 2^-149 (absolute error 2^-150).  torch's
             addcdiv forms step_size * m BEFORE the division by denom, the recipe forms m = (1 - b1) * g and scales the quotient by
             lr / bc1 afterwards: either error is divided by denom, 2^-150 (1 + lr / bc1) / denom together, doubled"""
    f32 = np.float32
    n, lr, wd, b1, b2, eps = 4096, 1e-3, 1e-2, f32(0.9), f32(0.999), f32(1e-8)
    w, g = contract.inputs(n, 11)
    decay = f32(1.0 - lr * wd)
    bc1 = f32(1.0) - b1 ** f32(1.0)
    bc2_sqrt = np.sqrt(f32(1.0) - b2 ** f32(1.0), dtype=f32)
    with np.errstate(under='ignore'):
        w1 = w * decay
        gr = g * f32(1.0) + f32(0.0) * w1                             # grad_scale = 1, weight_decay = 0 in the coupled expressions
        m = (f32(1.0) - b1) * gr                                      # fma(b1, 0, a) = a
        v = ((f32(1.0) - b2) * gr) * gr
        denom = np.sqrt(v, dtype=f32) / bc2_sqrt + eps
        q = m / denom
        lrb = f32(lr) / bc1
        got = (w1.astype(np.float64) - lrb.astype(np.float64) * q.astype(np.float64)).astype(f32)      # the fused multiply-add
    p = torch.from_numpy(w.copy()).requires_grad_(True)
    p.grad = torch.from_numpy(g.copy())
    torch.optim.AdamW([p], lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8).step()
    want = p.detach().numpy()
    u = np.abs(w1.astype(np.float64) - want.astype(np.float64))
    tol = 2.0 ** -23 * np.abs(want.astype(np.float64)) + 2.0 ** -19 * u + 2.0 ** -149 * (1.0 + float(lrb)) / denom.astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all() and (err <= tol).all(), float((err / tol).max())
    assert (got != w).mean() > 0.5                                    # the step moved the weights
