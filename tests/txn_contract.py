"""The transactional BatchNorm state's contract restated in numpy (helper of test_txn_host.py / test_gpu_txn*.py; no test in here).
`probe` is the count rule and the first_bad rule of efgh_txn_probe, `resolve` the veto and restore rule of efgh_txn_resolve on a
mirror of the guard block (a dict with the fields the veto touches)."""
import numpy as np


def probe(live, shadow, starts, losses=()):
    """-> (forward_nonfinite, first_bad).
    count: the elements that are inf / NaN in `live` AND finite in `shadow` (an element that was already non-finite at the snapshot
    counts nothing), plus one per non-finite loss scalar.
    first_bad: the smallest buffer index s with such an element in [starts[s], starts[s + 1]), or -1 (losses name no buffer)."""
    live, shadow = np.asarray(live, np.float32), np.asarray(shadow, np.float32)
    new = ~np.isfinite(live) & np.isfinite(shadow)
    count = int(new.sum()) + int((~np.isfinite(np.asarray(losses, np.float32))).sum())
    first = -1
    if new.any():
        first = int(np.searchsorted(np.asarray(starts, np.int64), int(np.flatnonzero(new)[0]), side='right')) - 1
    return count, first


def bias_corrections(applied, b1=0.9, b2=0.999):
    """bc1 = 1 - beta1^applied and bc2_sqrt = sqrt(1 - beta2^applied) as the decide launch forms them: the power in float64 on the
    fp32 betas, rounded once to fp32, the rest in fp32 (the recipe tests/test_gpu_grad_guard.py::_bias_corrections_ok checks the
    guard against, with its tolerance for the power's last bit)"""
    b1, b2 = np.float64(np.float32(b1)), np.float64(np.float32(b2))
    bc1 = np.float32(1) - np.float32(b1 ** applied)
    bc2_sqrt = np.sqrt(np.float32(1) - np.float32(b2 ** applied), dtype=np.float32)
    return bc1, bc2_sqrt


def resolve(guard, forward_nonfinite, txn=None, b1=0.9, b2=0.999):
    """guard: dict(skip, applied, skipped, bc1, bc2_sqrt, ...) as the decide launch left it (with skip_nonfinite on);
    txn: dict(vetoed, vetoed_total, rolled_back).  -> (guard', txn', restore)
    veto:    forward_nonfinite != 0 and skip == 0 -> skip = 1, applied - 1, skipped + 1, the bias corrections of the un-advanced
             `applied`, vetoed = 1, vetoed_total + 1; every other field of the guard block (coef, scale, norm, sums, counts) stays.
             forward_nonfinite == 0: the guard block is unchanged.
    restore: the final skip is 1 -> live = shadow (floats and counters), rolled_back + 1; otherwise live is not written."""
    g = dict(guard)
    t = dict(txn or {'vetoed': 0, 'vetoed_total': 0, 'rolled_back': 0})
    if forward_nonfinite != 0 and not g['skip']:
        g['skip'], g['applied'], g['skipped'] = 1, g['applied'] - 1, g['skipped'] + 1
        g['bc1'], g['bc2_sqrt'] = bias_corrections(g['applied'], b1, b2)
        t['vetoed'], t['vetoed_total'] = 1, t['vetoed_total'] + 1
    restore = bool(g['skip'])
    if restore:
        t['rolled_back'] += 1
    return g, t, restore
