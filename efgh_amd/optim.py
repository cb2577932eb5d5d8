"""`torch.optim.Adam` / `torch.optim.AdamW` drop-ins on the fused step: the optimizer the reference's own loop builds and drives
(`torch.optim.Adam(model_named_params, lr=..., weight_decay=...)`, main.py:178-183; `optimizer.zero_grad()`, `backward()`,
`optimizer.step()`, iterater.py:41-43) with the flat buffers, the direct gradient writes and the one-launch step that
`efgh_amd.train.Trainer` has.  `python -m efgh_amd.run --fused-optimizer` puts these classes in place of torch's for a run.

What the loop sees is torch's interface: `param_groups` (a list of dicts with the parameter tensors; `param_group['lr']` written by
`adjust_learning_rate`, common/helper.py:31-34, is read at every step), `state_dict()` / `load_state_dict()` in torch's layout -
loadable into a stock `torch.optim.Adam` / `AdamW` built over the same groups, and the other way round - `zero_grad()` and `step()`.

What it does underneath: construction re-homes every parameter and its gradient in ONE flat buffer each (train.FlatParams.from_params;
the flat order is the order of the groups, then of the parameters within each, so every group is one contiguous segment);
`zero_grad()` zeroes the flat gradient with one launch and re-arms the layer backwards' direct writes into it; `step()` is
train.FusedAdam's: one launch (efgh_adam_step, or efgh_adam_step_groups when there are several groups or a decoupled one), three with
the gradient guard (`max_grad_norm=` / `skip_nonfinite=True`: clip_grad_norm_ and the skipping of non-finite steps decided on the
device, nothing read back; `guard_stats()` reads the result).

Shared by all groups BY DESIGN: betas and eps (one pair of moment buffers, one bias correction, one step count).  Not supported:
amsgrad, maximize, foreach / fused / capturable / differentiable set to anything true, `add_param_group` after construction (the
flat layout is fixed then).  `optimizer.state` stays empty: the moments live in two flat buffers (`optimizer.fused.m` / `.v`) and
reach torch's per-parameter form through `state_dict()` only.  Of what the loop writes into a `param_group` after construction, `lr`
and `weight_decay` are read at every step (anything float() converts); changed betas / eps are refused at the next step; other
keys (a scheduler's `initial_lr`) are kept and carried by `state_dict()`.  The transactional step and the weight average need
hooks around the forward, which an optimizer does not see: they stay with train.Trainer."""
import torch

from . import _C, ops
from .io import checkpoint as ck
from .train import FlatParams, FusedAdam, check_group_value

_TorchAdam, _TorchAdamW = torch.optim.Adam, torch.optim.AdamW          # (the launcher may rebind the names in torch.optim)
_REFUSED = ('foreach', 'fused', 'capturable', 'differentiable', 'maximize')


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, amsgrad) on the fused step; see the module docstring.
    `decoupled=True` gives every group torch.optim.AdamW's decay (a group dict may set its own `decoupled` /
    `decoupled_weight_decay`).  `max_grad_norm` / `skip_nonfinite`: the device-side gradient guard of train.FusedAdam."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, decoupled=False,
                 max_grad_norm=None, skip_nonfinite=False, **torch_kwargs):
        for key, value in torch_kwargs.items():
            if key == 'decoupled_weight_decay':
                decoupled = bool(value) or decoupled
            elif key not in _REFUSED:
                raise TypeError('%s() got an unexpected keyword argument %r' % (type(self).__name__, key))
            elif value:
                raise _C.EfghError('%s=%r is not supported by the fused optimizer (leave it unset)' % (key, value))
        if amsgrad:
            raise _C.EfghError('amsgrad is not supported by the fused optimizer')
        if torch.is_tensor(lr):
            raise _C.EfghError('a tensor lr is not supported by the fused optimizer (it is read on the host at every step)')
        self._built = False
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)
        groups, i = [], 0
        for k, g in enumerate(self.param_groups):
            for key in _REFUSED + ('amsgrad',):
                if g.get(key):
                    raise _C.EfghError('group %d: %s=%r is not supported by the fused optimizer' % (k, key, g[key]))
            dec = bool(g.pop('decoupled')) if 'decoupled' in g else bool(g['decoupled_weight_decay'])
            g['decoupled_weight_decay'] = dec
            groups.append({'params': list(range(i, i + len(g['params']))), 'lr': g['lr'], 'weight_decay': g['weight_decay'],
                           'decoupled': dec, 'betas': g['betas'], 'eps': g['eps']})
            i += len(g['params'])
        self.flat = FlatParams.from_params([p for g in self.param_groups for p in g['params']])
        plain = len(groups) == 1 and not groups[0]['decoupled']          # torch.optim.Adam over one list: FusedAdam as it always was
        self.fused = FusedAdam(self.flat, lr=groups[0]['lr'] if plain else lr, betas=tuple(betas), eps=eps,
                               weight_decay=groups[0]['weight_decay'] if plain else weight_decay, max_grad_norm=max_grad_norm,
                               skip_nonfinite=skip_nonfinite, groups=None if plain else groups)
        self.grad_scale = 1.0             # 1 / world once the launcher's data-parallel hook has summed flat.g over the ranks
        self._built = True

    def add_param_group(self, param_group):
        if getattr(self, '_built', False):
            raise _C.EfghError('add_param_group after construction: the flat layout of the fused optimizer is fixed (build the '
                               'optimizer over all groups at once)')
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none=True):
        """flat.zero_grad() whatever the argument: the flat gradient is zeroed (one launch) and the direct gradient writes of the
        layer backwards are re-armed; `.grad` stays a view of the flat buffer (never None)"""
        self.flat.zero_grad()

    def _sync_groups(self):
        """the loop's writes into torch's `param_groups` reach the fused step: lr and weight_decay are taken over at every step;
        betas, eps and the decoupled choice are fixed at construction (shared moment buffers, one bias correction), so a changed
        value is refused here rather than ignored"""
        f = self.fused
        for k, g in enumerate(self.param_groups):
            if tuple(float(b) for b in g['betas']) != tuple(float(b) for b in f.betas) or float(g['eps']) != float(f.eps):
                raise _C.EfghError('group %d: betas / eps were changed after construction (%r, %r); they are shared by all groups '
                                   'and fixed at %r, %r' % (k, tuple(g['betas']), g['eps'], tuple(f.betas), f.eps))
            own = f.param_groups[k]['decoupled'] if f.param_groups is not None else False
            if bool(g.get('decoupled_weight_decay', False)) != own:
                raise _C.EfghError('group %d: decoupled_weight_decay was changed after construction' % k)
            for key in _REFUSED + ('amsgrad',):
                if g.get(key):
                    raise _C.EfghError('group %d: %s=%r is not supported by the fused optimizer' % (k, key, g[key]))
        if f.param_groups is None:
            g = self.param_groups[0]
            f.lr, f.wd = check_group_value('lr', 'group 0', g['lr']), check_group_value('weight_decay', 'group 0', g['weight_decay'])
            return
        for mine, theirs in zip(f.param_groups, self.param_groups):
            mine['lr'], mine['weight_decay'] = theirs['lr'], theirs['weight_decay']

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        flat = self.flat
        ops.join_side_streams(flat.g)             # weight gradients are written on side streams that no autograd node orders
        self._sync_groups()
        self.fused.step(grad_scale=self.grad_scale)             # (bumps the content epoch of the flat weights)
        # the forward counts of a shared parameter's consumers end HERE, not in zero_grad: the loop's order is forward, zero_grad,
        # backward, step - clearing the counts of the forward that was just run would let the first consumer claim the slice
        flat.uses = [0] * len(flat.params)
        return loss

    def guard_stats(self):
        """train.FusedAdam.guard_stats(): one device read; EfghError when the guard is off"""
        return self.fused.guard_stats()

    def state_dict(self):
        """torch's layout: `state[i] = {step, exp_avg, exp_avg_sq}`, `param_groups` with `params` numbered group by group.  Keys
        that others keep in the groups (a scheduler's `initial_lr`) are carried along, as torch carries them."""
        self._sync_groups()
        sd = ck.adam_state_dict(self.fused)
        for out, g in zip(sd['param_groups'], self.param_groups):
            out['decoupled_weight_decay'] = bool(g['decoupled_weight_decay'])
            for key, value in g.items():
                if key != 'params' and key not in out:
                    out[key] = value
        return sd

    def load_state_dict(self, state_dict):
        """a state_dict of this class or of a stock torch.optim.Adam / AdamW over the same groups (main.py:198); EfghError naming
        the mismatch when the number of groups, a group's size or its coupled / decoupled choice differs"""
        ck.load_adam_state(self.fused, state_dict)
        f = self.fused
        for g, theirs in zip(self.param_groups, state_dict['param_groups']):
            for key, value in theirs.items():
                if key not in ('params', 'betas', 'eps', 'decoupled_weight_decay') + _REFUSED + ('amsgrad',):
                    g[key] = value
            g['weight_decay'] = theirs.get('weight_decay', 0.0)
            g['betas'], g['eps'] = tuple(f.betas), f.eps


class AdamW(Adam):
    """torch.optim.AdamW on the fused step: Adam above with decoupled=True and weight_decay=1e-2"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, decoupled=True,
                 max_grad_norm=None, skip_nonfinite=False, **torch_kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, decoupled=decoupled,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, **torch_kwargs)


def bind_defaults(max_grad_norm=None, skip_nonfinite=False):
    """(Adam, AdamW) subclasses whose constructors default to these guard options: what the launcher binds to torch.optim.Adam /
    torch.optim.AdamW for a run (the script's own call passes neither)"""
    def bound(base):
        class Bound(base):
            def __init__(self, params, *args, **kwargs):
                kwargs.setdefault('max_grad_norm', max_grad_norm)
                kwargs.setdefault('skip_nonfinite', skip_nonfinite)
                super().__init__(params, *args, **kwargs)
        Bound.__name__, Bound.__qualname__, Bound.__doc__ = base.__name__, base.__qualname__, base.__doc__
        return Bound
    if max_grad_norm is None and not skip_nonfinite:
        return Adam, AdamW
    return bound(Adam), bound(AdamW)
