"""Gradient accumulation over micro-batches restated in numpy (helper of test_grad_accum_host.py / test_gpu_grad_accum.py; no
test in here).  Three rules:
  sequential_sum   what GradAccumulator leaves in `acc` after k drains: ((g1 + g2) + g3) + ... in fp32, one IEEE add per element
  depth_weights    w_i = n_i / mean(n) in float64, rounded once to fp32; 1 everywhere when the mean is 0 (no valid pixel at all)
  grad_scale       1 / (k * world): what the optimizer kernels multiply the (all-reduced) sum by - fed into the Adam recipe of
                   tests/grad_guard_contract.py by `adam_on_sum`"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_contract as guard  # noqa: E402


def sequential_sum(grads):
    """fp32 arrays g1..gk -> ((g1 + g2) + g3) + ... in fp32.  The first gradient is COPIED (its -0 stays -0)."""
    acc = np.array(grads[0], dtype=np.float32, copy=True)
    with np.errstate(all='ignore'):
        for g in grads[1:]:
            acc = (acc + np.asarray(g, np.float32)).astype(np.float32)
    return acc


def depth_weights(counts, own=None):
    """counts: valid pixels of ALL micro-batches of all ranks (integers); own: the ones whose weights are wanted (default: all)
    -> fp32 weights n_i / mean(counts), or ones when mean(counts) == 0"""
    counts = np.asarray(counts, np.int64).reshape(-1)
    own = counts if own is None else np.asarray(own, np.int64).reshape(-1)
    mean = np.float64(counts.sum()) / np.float64(counts.size)
    if not mean > 0:
        return np.ones(own.size, np.float32)
    return (own.astype(np.float64) / mean).astype(np.float32)


def grad_scale(k, world=1):
    return 1.0 / (k * world)


def adam_on_sum(w, m, v, acc, k, world, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """one Adam step (number t) on the accumulated SUM `acc` of k micro-batches x world ranks: float64 (w, m, v) -> new ones"""
    return guard.adam(np.asarray(w, np.float64), np.asarray(m, np.float64), np.asarray(v, np.float64),
                      np.asarray(acc, np.float64), grad_scale(k, world), t, lr, betas, eps, wd)
