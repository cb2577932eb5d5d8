"""Checkpoint interchange with the reference.

The reference saves `{'iter', 'state_dict', 'min_loss', 'optimizer'}` with `torch.save`
(common/helper.py:40-61, iterater.py:82-89); `state_dict` comes from the DataParallel-wrapped model,
so every key carries a `module.` prefix (main.py:127,136), and `optimizer` is
`torch.optim.Adam.state_dict()` over `named_parameters()` order (main.py:178-183).  These helpers read
and write exactly that layout, so checkpoints move freely between the reference and this path."""
import os
import shutil

import torch

from .._C import EfghError


def strip_module_prefix(sd):
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}


def load_model_state(model, ckpt, strict=True):
    """ckpt: path | checkpoint dict | bare state_dict (with or without the `module.` prefix)"""
    if isinstance(ckpt, (str, os.PathLike)):
        ckpt = torch.load(ckpt, map_location='cpu')
    sd = ckpt['state_dict'] if isinstance(ckpt, dict) and 'state_dict' in ckpt else ckpt
    return model.load_state_dict(strip_module_prefix(sd), strict=strict)


def update_dict_filter(pretrained_dict, convert_dict, model_dict):
    """main.py:212-225: rename keys (every `convert_dict` key that occurs as a substring is replaced; a key matched by several
    entries yields one renamed copy per entry, as in the reference), then keep what the model has"""
    update = {}
    for k, v in pretrained_dict.items():
        converted = False
        for old, new in convert_dict.items():
            if old in k:
                update[k.replace(old, new)] = v
                converted = True
        if not converted:
            update[k] = v
    return {k: v for k, v in update.items() if k in model_dict}


def grad_false_keys_filter(model, grad_false_keys):
    """main.py:227-235: parameters whose name contains one of the keys are frozen (requires_grad = False)"""
    for k, p in model.named_parameters():
        if any(key in k for key in grad_false_keys):
            p.requires_grad = False
    return model


def load_pretrained(model, ckpt, convert_dict=None, grad_false_keys=None):
    """the `pretrained_path` branch of main.py:162-176: partial, renamed, non-strict load + freezing.  The optimizer must be
    built afterwards over the parameters that still require a gradient (main.py:178-183; train.Trainer / FlatParams do)."""
    if isinstance(ckpt, (str, os.PathLike)):
        ckpt = torch.load(ckpt, map_location='cpu')
    sd = ckpt['state_dict'] if isinstance(ckpt, dict) and 'state_dict' in ckpt else ckpt
    wrapped = all(k.startswith('module.') for k in sd)
    model_dict = model.state_dict()
    if wrapped:                                      # a checkpoint of the DataParallel-wrapped reference model
        model_dict = {'module.' + k: v for k, v in model_dict.items()}
    update = update_dict_filter(sd, convert_dict or {}, model_dict)
    res = model.load_state_dict(strip_module_prefix(update) if wrapped else update, strict=False)
    grad_false_keys_filter(model, grad_false_keys or [])
    return res


def _torch_group(lr, betas, eps, wd, params):
    return {'lr': lr, 'betas': tuple(betas), 'eps': eps,
            'weight_decay': wd, 'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False,
            'differentiable': False, 'fused': None, 'params': params}


def adam_numbering(opt):
    """flat parameter indices in torch's state_dict numbering: group by group, in each group's own order (the identity without
    parameter groups, and whenever every group is one contiguous run of the flat order)"""
    if getattr(opt, 'param_groups', None) is None:
        return list(range(len(opt.flat.params)))
    return [i for g in opt.param_groups for i in g['params']]


def adam_state_dict(opt, lr=None):
    """`torch.optim.Adam.state_dict()`-compatible view of a train.FusedAdam (one entry per parameter).  With parameter groups: one
    entry of `param_groups` per group, `params` numbered group by group as torch numbers them, every group with its own lr /
    weight_decay and `decoupled_weight_decay` (torch.optim.Adam's key for AdamW's decay)."""
    flat = opt.flat
    state = {}
    t = opt.t           # read ONCE: with the gradient guard's skip_nonfinite the count of APPLIED steps lives on the device
    order = adam_numbering(opt)
    for j, i in enumerate(order):
        p, (off, k) = flat.params[i], flat.offsets[i]
        if t > 0:
            state[j] = {'step': torch.tensor(float(t)),
                        'exp_avg': opt.m[off:off + k].view(p.shape).detach().clone(),
                        'exp_avg_sq': opt.v[off:off + k].view(p.shape).detach().clone()}
    if getattr(opt, 'param_groups', None) is None:
        return {'state': state, 'param_groups': [_torch_group(opt.lr if lr is None else lr, opt.betas, opt.eps, opt.wd, order)]}
    groups, j = [], 0
    for g in opt.param_groups:
        group = _torch_group(g['lr'], opt.betas, opt.eps, g['weight_decay'], list(range(j, j + len(g['params']))))
        group['decoupled_weight_decay'] = bool(g['decoupled'])
        groups.append(group)
        j += len(g['params'])
    return {'state': state, 'param_groups': groups}


def load_adam_state(opt, sd):
    """inverse of adam_state_dict: accepts the reference's optimizer state (main.py:190-198) or any torch.optim.Adam / AdamW
    state_dict built over the same groups.  Every group's lr / weight_decay is taken over; betas and eps, shared by design, from
    the first; the coupled / decoupled choice must be the optimizer's own.  EfghError naming the mismatch when the number of
    groups, a group's size or its decoupled choice differs."""
    flat = opt.flat
    mine = opt.param_groups if getattr(opt, 'param_groups', None) is not None else [{'params': list(range(len(flat.params)))}]
    theirs = sd['param_groups']
    if len(theirs) != len(mine):
        raise EfghError('the optimizer state has %d parameter group(s), this optimizer %d' % (len(theirs), len(mine)))
    for k, (a, b) in enumerate(zip(theirs, mine)):
        if len(a['params']) != len(b['params']):
            raise EfghError('parameter group %d of the optimizer state holds %d parameters, this optimizer\'s %d'
                            % (k, len(a['params']), len(b['params'])))
    order = adam_numbering(opt)
    ids = [j for a in theirs for j in a['params']]
    grouped = getattr(opt, 'param_groups', None) is not None
    for k, (a, b) in enumerate(zip(theirs, mine)):
        # torch.optim.Adam's key for AdamW's decay (absent in older files: coupled); an ungrouped FusedAdam is coupled
        saved, own = bool(a.get('decoupled_weight_decay', False)), bool(b.get('decoupled', False))
        if saved != own and (saved or grouped):
            raise EfghError('parameter group %d of the optimizer state has %s weight decay, this optimizer\'s group %s: build the '
                            'optimizer with the same choice' % (k, 'decoupled (AdamW)' if saved else 'coupled (Adam)',
                                                                 'decoupled (AdamW)' if own else 'coupled (Adam)'))
    g = theirs[0]
    opt.betas, opt.eps = tuple(g['betas']), g['eps']
    if getattr(opt, 'param_groups', None) is None:
        opt.lr, opt.wd = g['lr'], g.get('weight_decay', 0.0)
    else:
        for a, b in zip(theirs, mine):
            if tuple(a['betas']) != opt.betas or a['eps'] != opt.eps:
                raise EfghError('the optimizer state\'s groups differ in betas / eps: they are shared by all groups here')
            b['lr'], b['weight_decay'] = float(a['lr']), float(a.get('weight_decay', 0.0))
    steps = []
    for j, i in zip(ids, order):
        st = sd['state'].get(j)
        if st is None:
            continue
        off, k = flat.offsets[i]
        opt.m[off:off + k].copy_(st['exp_avg'].reshape(-1))
        opt.v[off:off + k].copy_(st['exp_avg_sq'].reshape(-1))
        steps.append(int(st['step']))
    opt.t = max(steps) if steps else 0          # (a property: with skip_nonfinite it also sets the device-side count)


def _ema_named(ema, model):
    """[(name, averaged view)] of the trainable parameters a train.WeightEma averages, under their names in `model`"""
    avg = {id(p): v for p, v in ema.views()}
    named = [(name, avg[id(p)]) for name, p in model.named_parameters() if id(p) in avg]
    if len(named) != len(avg):
        raise EfghError('the weight average holds %d parameters, %d of them are parameters of this model' % (len(avg), len(named)))
    return named


def ema_state(ema, model):
    """the 'ema' entry of a checkpoint: decay, warm-up flag and the averaged trainable parameters under the reference's key names"""
    return {'decay': ema.decay, 'warmup': ema.warmup,
            'state_dict': {'module.' + name: v.detach().cpu().clone() for name, v in _ema_named(ema, model)}}


def check_ema_state(ema, model, entry):
    """EfghError unless `entry` (a checkpoint's 'ema') holds exactly the trainable parameters of `model`, with their shapes"""
    sd = strip_module_prefix(entry['state_dict']) if isinstance(entry, dict) and 'state_dict' in entry else None
    if sd is None:
        raise EfghError("the checkpoint's 'ema' entry has no 'state_dict'")
    named = _ema_named(ema, model)
    want = [name for name, _ in named]
    if sorted(sd) != sorted(want):
        missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
        raise EfghError("the checkpoint's weight average does not match the trainable parameters: missing %s, unexpected %s"
                        % (missing[:5], extra[:5]))
    for name, v in named:
        if tuple(sd[name].shape) != tuple(v.shape):
            raise EfghError("the checkpoint's weight average has shape %s for %s, the model %s"
                            % (tuple(sd[name].shape), name, tuple(v.shape)))
    return sd, named


def load_ema_state(ema, model, entry):
    """inverse of ema_state: the averaged values go into the WeightEma's buffer (its decay and warm-up flag stay its own)"""
    sd, named = check_ema_state(ema, model, entry)
    for name, v in named:
        v.copy_(sd[name])


def ema_checkpoint(ckpt):
    """a checkpoint saved with a weight average -> a checkpoint in the reference's layout (`iter`, `state_dict`, `min_loss`,
    `optimizer`) whose `state_dict` carries the AVERAGED trainable parameters, every other entry (frozen parameters, buffers) as
    saved: what the reference's test branch loads with strict=True to evaluate the averaged model"""
    if isinstance(ckpt, (str, os.PathLike)):
        ckpt = torch.load(ckpt, map_location='cpu')
    if not isinstance(ckpt, dict) or 'ema' not in ckpt or 'state_dict' not in ckpt:
        raise EfghError("ema_checkpoint: the checkpoint has no weight average (save it with save_checkpoint(..., ema=trainer.ema))")
    avg = ckpt['ema']['state_dict']
    sd = dict(ckpt['state_dict'])
    for name, v in avg.items():
        if name not in sd or tuple(sd[name].shape) != tuple(v.shape):
            raise EfghError("ema_checkpoint: the weight average's %s is not an entry of the checkpoint's state_dict of that shape" % name)
        sd[name] = v
    out = {k: v for k, v in ckpt.items() if k != 'ema'}
    out['state_dict'] = sd
    return out


def save_checkpoint(ckpt_dir, model, opt, it, min_loss, is_best=False, iter_interval=1000,
                    filename='checkpoint.pth.tar', ema=None):
    """common/helper.py:40-61 semantics: rolling file, periodic copies, best copy, pruning after 5 intervals.  `ema`: a
    train.WeightEma (Trainer.ema) - one more key 'ema' (ema_state); None: exactly the reference's keys"""
    os.makedirs(ckpt_dir, exist_ok=True)
    state = {'iter': it, 'state_dict': {'module.' + k: v.detach().cpu() for k, v in model.state_dict().items()},
             'min_loss': min_loss, 'optimizer': adam_state_dict(opt)}
    if ema is not None:
        state['ema'] = ema_state(ema, model)
    path = os.path.join(ckpt_dir, filename)
    torch.save(state, path)
    if it % iter_interval == 0:
        shutil.copyfile(path, os.path.join(ckpt_dir, 'checkpoint_%d.pth.tar' % it))
    if is_best:
        shutil.copyfile(path, os.path.join(ckpt_dir, 'model_best.pth.tar'))
    if it > 5 * iter_interval:
        old = os.path.join(ckpt_dir, 'checkpoint_%d.pth.tar' % (it - 5 * iter_interval))
        if os.path.exists(old):
            os.remove(old)
    return path
