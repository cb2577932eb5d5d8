"""torch.autograd.Function shims over the HIP forward/backward kernels (training path).

torch's autograd engine is used only as the tape (plumbing); every forward and backward
computation inside these Functions runs in libefgh_hip.so.  Tensors are "row matrices":
shape [..., C] with unit stride on the last axis and a uniform row stride (channel slices of a
contiguous channels-last buffer qualify), addressed as (data_ptr, ld).
"""
import torch

from .. import ops
from ..ops import ACT_NONE, ceil4


def rows_ok(t):
    if t.stride(-1) != 1:
        return False
    ld = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
    exp = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            return False
        exp *= t.shape[d]
    return ld % 4 == 0 and t.data_ptr() % 16 == 0


def as_rows(t):
    return t if rows_ok(t) else t.contiguous()


def ld_of(t):
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


class LayerSpec:
    """Description of one GEMM layer, built once by its layer function in layers.py and run by either path: the no-tape executor
    (layers._run) or GemmLayerFn.

    N, C, T, mode, table: the gather-GEMM's (N the real output channel count, C the padded input one, c_real the real one);
    launches: [(geom | None, M_launch)] forward launches (several for a transposed conv), layouts: one ops.WeightLayout per launch
    (pack(weight) -> its packed forward weight, unpack / fold_args: where its packed weight gradient belongs);
    M, out_shape: rows and leading shape of the output; bn, train, act, slope: the epilogue.
    What only the tape path reads is set by for_tape()."""
    dgrad = custom_forward = custom_wgrad = None
    takes_bnsrc = passthrough = pool = defer_act = bwd_fusable = False

    def __init__(self, N, C, T, mode, launches, layouts, M, out_shape, bn=None, train=False, act=ACT_NONE, slope=0.0, table=None,
                 c_real=None):
        self.N, self.C, self.T, self.mode, self.M = N, C, T, mode, M
        self.launches, self.layouts, self.out_shape = launches, layouts, out_shape
        self.bn, self.train, self.act, self.slope, self.table = bn, train, act, slope, table
        self.c_real = c_real if c_real is not None else C

    def for_tape(self, dgrad, takes_bnsrc=False, custom_forward=None, custom_wgrad=None, passthrough=False, pool=False,
                 defer_act=False, bwd_fusable=False):
        # dgrad(spec, weight, draw, x[, add=]) -> gradient w.r.t. x; takes_bnsrc: it also takes bnsrc= (the BnSrc of the layer that
        # produced x) and pre_v=
        self.dgrad, self.takes_bnsrc = dgrad, takes_bnsrc
        # optional replacements of the launch loop / weight gradient (e.g. transposed conv as GEMM + col2im)
        self.custom_forward, self.custom_wgrad = custom_forward, custom_wgrad
        # passthrough: forward also returns an alias of x for a skip connection; the gradient arriving on that alias is added
        # in the dgrad kernel's epilogue (`dgrad(..., add=)`) instead of by a separate elementwise pass
        self.passthrough = passthrough
        # pool: the layer is followed by MaxPool2d(2,2); BatchNorm + activation + pooling run as one pass over the raw output and
        # the full-resolution activation is never stored (backward recomputes the window from raw)
        self.pool = pool
        # defer_act: the caller guarantees that this layer's activation has ONE consumer and that it is a 2-D Winograd layer
        # (ops.lazy_capable): the normalise + activate pass is not run, the raw output is returned carrying an ops.LazyAct
        self.defer_act = defer_act
        # bwd_fusable: the layer's data AND weight gradient both run on the 2-D Winograd path, so the BatchNorm backward's apply
        # pass can ride in their gradient-side transforms (ops.wino2d_bwd_transforms); its dgrad takes pre_v=
        self.bwd_fusable = bwd_fusable
        return self


def run_launches(spec, x, lda, weight, out, ldo, bias, want_stats, a_off=0, out_off=0, lazy=None, pool=False, keep_on=None, **epilogue):
    """the launch stage of both paths: pack each launch's weight and run the launches of `spec` (or its custom_forward) into `out`.
    want_stats: train-mode BatchNorm follows - the per-column statistics [G][2][Np] are returned, taken in the launches' epilogues or,
    for the kernels without one (ops.no_stats_epilogue) and for a custom_forward, by one ops.col_stats pass over the output;
    the caller then passes no `epilogue` (scale / shift / residual / act: the raw output is wanted).
    keep_on: tape path only - the layer's node, when its own weight gradient will be asked for: a 2-D Winograd launch whose weight
    gradient runs on that path too leaves B^T x B of its input there (ops.gather_gemm keep_v=), as keep_on.kept_v[launch index] - a
    plain attribute (x itself is among the saved tensors, which catch an in-place edit of it) that lives as long as the layer's graph
    does and that GemmLayerFn._backward takes"""
    Np = ceil4(spec.N)
    wps = [lay.pack(weight) for lay in spec.layouts]
    custom = spec.custom_forward
    stats, thin = None, False
    if want_stats:
        thin = custom is not None or ops.no_stats_epilogue(spec.mode, spec.C, Np, spec.T, spec.launches)
        if not thin:
            gs = [ops.stats_rows(spec.mode, spec.C, Np, g, m) for g, m in spec.launches]
            stats = torch.empty((sum(gs), 2, Np), dtype=torch.float32, device=x.device)
    if custom is not None:
        custom(x, weight, out)
    g0 = 0
    for li, (geom, m) in enumerate(spec.launches if custom is None else ()):
        T = ops.taps_of(spec.T, geom)
        st = None
        if stats is not None:
            st = stats[g0:g0 + gs[li]]
            g0 += gs[li]
        slot = None if keep_on is None else []
        ops.gather_gemm(x, lda, spec.C, T, wps[li], Np, m, out, ldo, mode=spec.mode, geom=geom, table=spec.table, bias=bias, stats=st,
                        a_off=a_off, out_off=out_off, flops=2.0 * m * spec.N * T * spec.c_real, lazy=lazy, pool=pool, keep_v=slot,
                        **epilogue)
        if slot and ops.wgrad_route(spec.mode, spec.C, Np, T, geom) == 'wino2d':      # (else nobody will ask for it: freed here)
            if keep_on.kept_v is None:
                keep_on.kept_v = {}
            keep_on.kept_v[li] = slot[0]
    if thin:
        stats, _ = ops.col_stats(out, spec.M, Np, ldo, x_off=out_off)
    return stats


def bn_batch_stats(bn, stats, Np, count, save=False):
    """the batch-statistics stage of both paths: train-mode BatchNorm from the column statistics of the raw output
    -> (scale, shift, mean, invstd), the last two None without `save`.  Ticks num_batches_tracked and updates the running
    statistics in place - through padded temporaries when the channel count was padded to Np (tiny layers)"""
    N = bn.num_features
    ops.bn_tick(bn)          # num_batches_tracked += 1, batched per forward / per step
    momentum = bn.momentum if bn.momentum is not None else 0.1
    rm, rv = ops.pad_vec(bn.running_mean, Np), ops.pad_vec(bn.running_var, Np, 1.0)
    res = ops.bn_finalize(stats, stats.shape[0], Np, count, ops.pad_vec(bn.weight, Np), ops.pad_vec(bn.bias, Np), rm, rv, momentum,
                          bn.eps, save=save)
    if Np != N:
        bn.running_mean.copy_(rm[:N])
        bn.running_var.copy_(rv[:N])
    return res


def materialize(x, lazy):
    """act(x*scale + shift) of a raw BatchNorm output with a pending activation, for a consumer that cannot apply it itself"""
    M = x.numel() // x.shape[-1]
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ops.scale_shift_act(x, ld_of(x), lazy.scale, lazy.shift, y, x.shape[-1], M, x.shape[-1], lazy.act, lazy.slope)
    return y


def claim_grad(p):
    """(flat gradient view, deliver()) when parameter `p` lives in a train.FlatParams whose slice may be overwritten by this
    backward, else (None, None): the backward then returns the gradient to autograd as usual."""
    slot = getattr(p, '_efgh_flat', None) if p is not None else None
    if slot is None:
        return None, None
    flat, i = slot
    g = flat.claim(p, i)
    if g is None:
        return None, None
    return g, (lambda stream=None: flat.deliver(i, stream))


def note_use(*params):
    """forward-side count of a FlatParams parameter's consumers in this step (train.FlatParams.uses)"""
    for p in params:
        slot = getattr(p, '_efgh_flat', None) if p is not None else None
        if slot is not None:
            slot[0].uses[slot[1]] += 1


def _bias_grad_behind_bn(ctx, p_bias, draw, M, Np, N, train_bn, delivered):
    """gradient of a conv / conv1d bias that feeds a BatchNorm.  Train mode: the batch mean absorbs the bias, so
    d/dbias = sum_m draw = coef * (sum dpre - M * mean(dpre) - mean(dpre * xhat) * sum xhat) = 0 exactly (sum xhat = 0); a column-sum
    pass over draw only measures rounding noise (which is what the reference's autograd returns, `tests/test_oracle_e2e.py`), so the
    exact zero is returned without touching draw.  Eval-mode statistics (frozen BatchNorm with autograd on): the real column sum."""
    if not ctx.needs_input_grad[2]:
        return None
    if not train_bn:
        return ops.col_sum(draw, M, Np)[:N]
    g, done = claim_grad(p_bias)
    if g is not None:                      # the flat gradient slice is already zero (FlatParams.zero_grad)
        delivered.append(done)
        return None
    return torch.zeros(N, dtype=torch.float32, device=ctx.saved_tensors[0].device)


class BnSrc:
    """what the BatchNorm backward of a layer needs besides dy, attached (`_efgh_bnsrc`) to the activation the layer returns: the
    consumer of that activation hands it to its data-gradient kernel, which then takes the layer's two column sums in its epilogue
    (ops.gather_gemm bn_bwd) and tags the gradient it returns (`_efgh_bnsums`); the layer's own backward finds the tag on its dy
    and skips the reduction pass over dy and raw.  Any detour of the gradient through autograd (several consumers summed by the
    engine, a view, a clone) arrives as another tensor object without the tag: the layer then reduces as before."""
    __slots__ = ('raw', 'y', 'psc', 'psh', 'mean', 'invstd', 'act', 'slope', 'M', 'N')

    def __init__(self, raw, y, psc, psh, mean, invstd, act, slope, M, N):
        self.raw, self.y, self.psc, self.psh, self.mean, self.invstd = raw, y, psc, psh, mean, invstd
        self.act, self.slope, self.M, self.N = act, slope, M, N

    def fits(self, M, N):
        return self.M == M and self.N == N


TRACE = None          # debug aid (tools/layer_census.py): list of per-layer records appended by GemmLayerFn.backward


# ---- the tails of a GEMM layer: what runs between the GEMM output and the returned activation, and its mirror between dy and draw.
# GemmLayerFn._forward chooses one (_choose_tail) and records its name as ctx.tail; the backward runs that tail's head (TAILS).
#   forward(ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target) -> (y, what the head reads: saved behind x and weight)
#   head(ctx, spec, dy, sums, saved, gs1, gs2, delivered) -> (draw, pre_v, pre_gy, dbeta, dgamma, dbias, dres)
# What a head needs to know besides the saved tensors its forward writes to ctx as plain values: ctx.mask - where the activation
# mask comes from: 'bits' (sign bits left by the forward), 'y' (the activation), 'affine' (re-derived from raw * scale + shift);
# ctx.fused_pool (bn_pool).  ctx.train_bn (train-mode statistics) is common to all.
def _c4_layer(spec, x, weight, b):
    """the ops.C4PoolLayer of a pooled 4-channel layer (b: its padded bias), for the choice, the forward and the backward alike"""
    return ops.C4PoolLayer(x, ld_of(x), spec.layouts[0].pack(weight), ceil4(spec.N), spec.launches[0][0], spec.launches[0][1], b)


def _choose_tail(spec, x, weight, b, lazy, res, needs_grad):
    assert not spec.pool or (spec.bn is not None and res is None), 'the pool rides in the BatchNorm pass of a layer without residual'
    if not spec.pool:
        return 'plain' if spec.bn is None else 'bn'
    # a pooled 4-channel input layer (train-mode BatchNorm + ReLU, stride 1) under a recording tape: the full-resolution raw map is
    # neither written nor saved (ops.C4_POOL_RECOMPUTE).  Its sums are those of ops.pool_bn_bwd's pooled reduction, so it follows
    # that switch
    if (ops.C4_POOL_RECOMPUTE and ops.POOL_REDUCE_FROM_Y and spec.train and spec.act == ops.ACT_RELU and ceil4(spec.N) == spec.N
            and lazy is None and spec.custom_forward is None and len(spec.launches) == 1 and x.shape[-1] == spec.C and needs_grad
            and ops.c4_pool_recompute_ok(_c4_layer(spec, x, weight, b), spec.mode, spec.C)):
        return 'bn_pool_c4'
    return 'bn_pool'


def _fuse_bwd(ctx, spec):
    """may the apply pass of the BatchNorm backward run inside the gradient-side transforms of a 2-D Winograd layer (draw is never
    stored)?  (spec.bwd_fusable is the forward's answer; the weight gradient's route is asked again here: with a switch flipped between
    forward and backward the layer takes the two-pass form instead of handing pre_gy to a kernel that cannot take it)"""
    return (ops.W2_BWD_FUSED and spec.bwd_fusable and ctx.train_bn and ceil4(spec.N) == spec.N and ctx.needs_input_grad[0]
            and ctx.needs_input_grad[1] and spec.custom_wgrad is None and ctx.mask != 'y' and len(spec.out_shape) == 3
            and ops.wgrad_lazy_capable(spec.mode, spec.C, spec.N, spec.launches[0][0]))


def _reduce_apply(ctx, spec, dy, sums, raw, mean, invstd, scale, shift, mask, gs1, gs2, fuse_bwd, delivered):
    """the generic backward head: the two column sums over dy (or `sums`, taken by the kernel that produced dy), then the apply pass
    into draw (+ dres) or, fuse_bwd, into the layer's two gradient-side transforms.  mask: the tensor ctx.mask speaks of"""
    has_bias, has_bn, has_res = ctx.has
    N, Np, M = spec.N, ceil4(spec.N), spec.M
    psc, psh = (scale, shift) if ctx.mask == 'affine' else (None, None)
    ldy = Np if mask is None else 0 if ctx.mask == 'bits' else ld_of(mask)      # (sign bits: `y` with ldy = 0, see efgh_act_bn_bwd_reduce)
    draw = pre_v = pre_gy = dbeta = dgamma = dbias = dres = None
    part = torch.empty((ops.bwd_groups(M), 2, Np), dtype=torch.float64, device=dy.device)      # float64 column sums (see backward.hip)
    s1, s2, m1, m2 = ops.bwd_sums(Np, dy.device, gs1, gs2, means=ctx.train_bn)
    if sums is not None and ctx.train_bn:
        # the kernel that produced dy took the two column sums in its epilogue: fold its per-block partials
        s1, s2, m1, m2 = ops.bwd_finalize_f32(sums[0], Np, float(M))
        if gs1 is not None:
            s1, s2 = gs1.copy_(s1), gs2.copy_(s2)
    else:
        ops.act_bn_bwd_reduce(dy, ld_of(dy), mask, ldy, raw, Np, mean, invstd, M, Np, spec.act, spec.slope, part, s1, s2, m1, m2,
                              pscale=psc, pshift=psh)
    if has_bn and gs1 is None:
        # (s1 / s2 are this backward's own tensors: handed to autograd as they are when there is no padding to cut off)
        dbeta, dgamma = (s1, s2) if Np == N else (s1[:N].clone(), s2[:N].clone())
    if has_bias and not has_bn and gs1 is None:
        dbias = s1 if Np == N else s1[:N].clone()
    if fuse_bwd:
        pre_v, pre_gy, dres = ops.wino2d_bwd_transforms(dy, ld_of(dy), raw, Np, mask, psc, psh, mean, invstd, scale, m1, m2, Np,
                                                        *spec.out_shape, spec.act, spec.slope, has_res)
    else:
        draw = torch.empty(tuple(spec.out_shape) + (Np,), dtype=torch.float32, device=dy.device)
        dres = torch.empty_like(draw) if has_res else None
        ops.act_bn_bwd_apply(dy, ld_of(dy), mask, ldy, raw, Np, mean if ctx.train_bn else None, invstd if ctx.train_bn else None, scale,
                             m1, m2, M, Np, spec.act, spec.slope, draw, Np, dres, Np, pscale=psc, pshift=psh)
    if has_bias and has_bn:          # bias in front of BatchNorm: d/dbias = column sums of draw
        dbias = _bias_grad_behind_bn(ctx, ctx.params[1], draw, M, Np, N, ctx.train_bn, delivered)
    return draw, pre_v, pre_gy, dbeta, dgamma, dbias, dres


def _pooled_sums(ctx, spec, draw, s1, s2, gs1, delivered):
    """what a fused-pool head returns behind ops.pool_bn_bwd / ops.c4_pool_bn_bwd (train-mode BatchNorm, no padding, no residual)"""
    dbias = _bias_grad_behind_bn(ctx, ctx.params[1], draw, spec.M, spec.N, spec.N, True, delivered) if ctx.has[0] else None
    return (s1, s2, dbias, None) if gs1 is None else (None, None, dbias, None)


def _own_wgrad(ctx, spec):
    """ctx when this layer's weight gradient will be asked for and is the layer's own (run_launches keep_on=), else None"""
    return ctx if (ctx.needs_input_grad[1] and spec.custom_wgrad is None) else None


def _plain_fwd(ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target):
    """bias (+ residual) (+ activation) straight in the GEMM epilogue"""
    Np = ceil4(spec.N)
    y = torch.empty(tuple(spec.out_shape) + (Np,), dtype=torch.float32, device=x.device)
    run_launches(spec, x, ld_of(x), weight, y, Np, b, False, lazy=lazy, keep_on=_own_wgrad(ctx, spec), residual=res,
                 ldr=0 if res is None else ld_of(res), act=spec.act, slope=spec.slope)
    ctx.mask = 'y'
    return y, (y,)


def _plain_bwd(ctx, spec, dy, sums, saved, gs1, gs2, delivered):
    has_bias, _, has_res = ctx.has
    if not (spec.act != ACT_NONE or has_res or has_bias):      # no pre-activation gradient is needed
        return dy, None, None, None, None, None, None
    return _reduce_apply(ctx, spec, dy, sums, None, None, None, None, None, saved[2], gs1, gs2, False, delivered)


def _bn_raw(ctx, spec, x, weight, b, gamma, beta, lazy):
    """-> raw, scale, shift, mean, invstd: the raw GEMM output of a BatchNorm layer and its affine map - from the batch statistics
    taken with it in train mode, from the running ones otherwise"""
    bn, Np = spec.bn, ceil4(spec.N)
    raw = torch.empty(tuple(spec.out_shape) + (Np,), dtype=torch.float32, device=x.device)
    stats = run_launches(spec, x, ld_of(x), weight, raw, Np, b, spec.train, lazy=lazy, keep_on=_own_wgrad(ctx, spec))
    if spec.train:
        return (raw,) + tuple(bn_batch_stats(bn, stats, Np, float(spec.M), save=True))
    with torch.no_grad():
        invstd = ops.pad_vec(torch.rsqrt(bn.running_var + bn.eps), Np)
        mean = ops.pad_vec(bn.running_mean.clone(), Np)
        scale = ops.pad_vec(gamma.detach(), Np) * invstd
        shift = ops.pad_vec(beta.detach(), Np) - mean * scale
    return raw, scale, shift, mean, invstd


def _bn_fwd(ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target):
    N, Np, M = spec.N, ceil4(spec.N), spec.M
    raw, scale, shift, mean, invstd = _bn_raw(ctx, spec, x, weight, b, gamma, beta, lazy)
    # layers without a residual re-derive the activation mask from raw * scale + shift in backward
    ctx.mask, mask = 'affine', None
    if (spec.defer_act and ops.LAZY_ACT and spec.train and res is None and Np == N and out_target is None
            and spec.custom_forward is None):
        # the single consumer (a 2-D Winograd layer) normalises and activates inside its input transform: no pass here, no
        # activation tensor (an ALIAS object of raw, not raw itself: the BnSrc tag below refers to raw, and y referring to something
        # that refers to y would be a cycle - a step's activations would wait for the garbage collector instead of their reference
        # counts)
        y = raw.detach()
        y._efgh_lazy = ops.LazyAct(scale, shift, spec.act, spec.slope)
    else:
        # out_target = (buffer [..][Ct], channel offset): the activation is written straight into that channel slice (the
        # training-path form of the decoder's torch.cat, see ConcatFn); the returned tensor is a view of the buffer
        y = None
        if out_target is not None and Np == N:
            tb, toff = out_target
            if tuple(tb.shape[:-1]) == tuple(raw.shape[:-1]) and toff % 4 == 0 and toff + N <= tb.shape[-1]:
                y = tb[..., toff:toff + N]
        if y is None:
            y = torch.empty_like(raw)
        # a residual layer's activation mask cannot be re-derived from raw alone: its backward used to read the activation back in
        # both passes; the forward pass leaves the SIGN BITS instead (M*N/32 words)
        if res is not None:
            ctx.mask, mask = 'y', y
            if spec.train and ops.BN_MASK_BITS and Np % 32 == 0 and spec.act != ACT_NONE and any(ctx.needs_input_grad):
                ctx.mask, mask = 'bits', torch.empty(M * Np // 32, dtype=torch.int32, device=x.device)
        ops.scale_shift_act(raw, Np, scale, shift, y, ld_of(y), M, Np, spec.act, spec.slope, res=res,
                            ldr=0 if res is None else ld_of(res), bits=mask if ctx.mask == 'bits' else None)
    if spec.train and Np == N and any(ctx.needs_input_grad):
        # (y.detach(): an alias object - y itself carrying a reference to something that refers to y would be a cycle, and a step's
        # activations would wait for the garbage collector instead of being freed by reference count)
        ctx.bnsrc = y._efgh_bnsrc = BnSrc(raw, y.detach() if res is not None else None, scale, shift, mean, invstd,
                                          spec.act, spec.slope, M, Np)
    # coef = gamma * invstd of the BatchNorm backward is the forward's `scale`
    return y, (raw, mean, invstd, scale, shift if res is None else None, mask)


def _bn_bwd(ctx, spec, dy, sums, saved, gs1, gs2, delivered):
    raw, mean, invstd, scale, shift, mask = saved[2:]
    return _reduce_apply(ctx, spec, dy, sums, raw, mean, invstd, scale, shift, mask, gs1, gs2, _fuse_bwd(ctx, spec), delivered)


def _bn_pool_fwd(ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target):
    """BatchNorm + activation + MaxPool2d(2,2) as one pass over raw; the full-resolution activation is never stored"""
    raw, scale, shift, mean, invstd = _bn_raw(ctx, spec, x, weight, b, gamma, beta, lazy)
    y = ops.maxpool2_affine(raw, scale, shift, spec.act, spec.slope)
    ctx.mask = 'affine'
    ctx.c4 = False                            # (True: the tail below, raw not stored - for whoever inspects the node, as the tests do)
    # fused: the BatchNorm backward runs straight from the pooled gradient (ops.pool_bn_bwd), which reads the pooled y
    ctx.fused_pool = spec.train and ceil4(spec.N) == spec.N
    return y, (raw, mean, invstd, scale, shift, y if ctx.fused_pool else None)


def _bn_pool_bwd(ctx, spec, dy, sums, saved, gs1, gs2, delivered):
    raw, mean, invstd, scale, shift, y = saved[2:]
    if not ctx.fused_pool:    # pooled gradient -> full resolution (window recomputed from raw*scale+shift), then as an un-pooled layer
        dy = as_rows(ops.maxpool2_bwd_affine(raw, scale, shift, spec.act, spec.slope, dy.contiguous()))
        return _reduce_apply(ctx, spec, dy, sums, raw, mean, invstd, scale, shift, None, gs1, gs2, False, delivered)
    # (no full-resolution dy is ever written; transforms: neither is draw)
    fuse = _fuse_bwd(ctx, spec) and ops.W2_BWD_FUSED_POOL
    draw, s1, s2 = ops.pool_bn_bwd(dy.contiguous(), raw, mean, invstd, scale, scale, shift, spec.act, spec.slope, s1=gs1, s2=gs2,
                                   transforms=fuse, y_pool=y)
    (pre_v, pre_gy), draw = (draw, None) if fuse else ((None, None), draw)
    return (draw, pre_v, pre_gy) + _pooled_sums(ctx, spec, draw, s1, s2, gs1, delivered)


def _bn_pool_c4_fwd(ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target):
    """... and without the raw map: statistics pass, batch statistics, pooled pass.  raw_win (pooled size) and the padded bias the
    backward's convolution re-runs with are saved in its place"""
    c4 = _c4_layer(spec, x, weight, b)
    scale, shift, mean, invstd = bn_batch_stats(spec.bn, ops.c4_pool_stats(c4), c4.N, float(spec.M), save=True)
    y, raw_win = ops.c4_pool_forward(c4, scale, shift, mean, invstd)
    ctx.c4 = True
    return y, (y, raw_win, mean, invstd, scale, shift, b)


def _bn_pool_c4_bwd(ctx, spec, dy, sums, saved, gs1, gs2, delivered):
    """the sums from the pooled tensors and raw_win, draw from the recomputed convolution"""
    x, weight, y, raw_win, mean, invstd, scale, shift, b = saved
    assert not spec.bwd_fusable              # (a 4-channel layer is never on the 2-D Winograd path)
    draw, s1, s2 = ops.c4_pool_bn_bwd(_c4_layer(spec, x, weight, b), dy.contiguous(), y, raw_win, mean, invstd, scale, scale, shift,
                                      s1=gs1, s2=gs2)
    return (draw, None, None) + _pooled_sums(ctx, spec, draw, s1, s2, gs1, delivered)


TAILS = {'plain': (_plain_fwd, _plain_bwd), 'bn': (_bn_fwd, _bn_bwd), 'bn_pool': (_bn_pool_fwd, _bn_pool_bwd),
         'bn_pool_c4': (_bn_pool_c4_fwd, _bn_pool_c4_bwd)}


class GemmLayerFn(torch.autograd.Function):
    """y = act(BN(gemm(x, W) + bias) + residual)   with hand-written backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, residual, spec, out_target=None):
        # the plane-GEMM precision (ops.planes_split_active) is resolved ONCE per layer and step: the backward restores it, so the
        # forward and backward of a step use one mode even if torch's switch changes in between
        ctx.planes_split = ops.planes_split_active()
        old, ops.TLS.planes_split = ops.TLS.planes_split, ctx.planes_split
        try:
            return GemmLayerFn._forward(ctx, x, weight, bias, gamma, beta, residual, spec, out_target)
        finally:
            ops.TLS.planes_split = old

    @staticmethod
    def _forward(ctx, x, weight, bias, gamma, beta, residual, spec, out_target=None):
        ctx.set_materialize_grads(False)      # an unused passthrough alias must arrive as None, not as a zero tensor to add
        ctx.xsrc = getattr(x, '_efgh_bnsrc', None)           # the BatchNorm layer that produced x (BnSrc), if any
        lazy = getattr(x, '_efgh_lazy', None)                # x is a RAW BatchNorm output whose activation this layer applies itself
        x = as_rows(x)
        if lazy is not None and not (spec.custom_forward is None and len(spec.launches) == 1 and not spec.passthrough
                                     and x.shape[-1] == spec.C
                                     and ops.lazy_capable(spec.mode, spec.C, ceil4(spec.N), spec.launches[0][0])):
            x, lazy = materialize(x, lazy), None              # (a consumer the producer was not told about: never wrong, only slower)
        ctx.lazy = lazy
        b = None if bias is None else ops.pad_vec(bias.detach(), ceil4(spec.N))
        res = None if residual is None else as_rows(residual)
        assert spec.custom_forward is None or (spec.bn is not None and bias is None)
        ctx.train_bn = spec.bn is not None and spec.train
        ctx.bnsrc = None                      # (the `bn` tail tags what it returns with its BnSrc, `_efgh_bnsrc`)
        ctx.kept_v = None                     # ({launch index: B^T x B of x}, left by run_launches(keep_on=ctx))
        ctx.tail = _choose_tail(spec, x, weight, b, lazy, res, any(ctx.needs_input_grad))
        y, saved = TAILS[ctx.tail][0](ctx, spec, x, weight, b, gamma, beta, res, lazy, out_target)
        if TRACE is not None:
            y._efgh_src = ('bn' if spec.bn is not None else 'plain', spec.N, spec.pool, residual is not None)
        ctx.spec = spec
        ctx.train_step = ops.TLS.train_step      # (backward runs on autograd's device thread: it restores the caller's switch)
        ctx.has = (bias is not None, gamma is not None, residual is not None)
        ctx.params = (weight, bias, gamma, beta)      # the Parameter objects themselves (claim_grad), not saved copies
        if any(ctx.needs_input_grad[1:5]):
            note_use(weight, bias, gamma, beta)
        ctx.save_for_backward(x, weight, *saved)
        return (y, x.view_as(x)) if spec.passthrough else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        old, ops.TLS.train_step = ops.TLS.train_step, ctx.train_step
        old_split, ops.TLS.planes_split = ops.TLS.planes_split, ctx.planes_split
        try:
            return GemmLayerFn._backward(ctx, dy, dskip)
        finally:
            ops.TLS.train_step = old
            ops.TLS.planes_split = old_split

    @staticmethod
    def _backward(ctx, dy, dskip=None):
        spec = ctx.spec
        sums = getattr(dy, '_efgh_bnsums', None) if dy is not None else None
        if sums is not None and (sums[1] is not ctx.bnsrc or sums[2] != dy._version):
            sums = None
        saved = ctx.saved_tensors
        x, weight = saved[:2]
        dev = x.device
        if dy is None:                        # (only the alias was used downstream)
            dy = torch.zeros(tuple(spec.out_shape) + (ceil4(spec.N),), dtype=torch.float32, device=dev)
        has_bias, has_bn, has_res = ctx.has
        N, Np, M = spec.N, ceil4(spec.N), spec.M
        if TRACE is not None:
            g0, m0 = spec.launches[0] if spec.launches else (None, M)
            TRACE.append(dict(M=M, N=N, C=spec.C, T=spec.T, mode=spec.mode, bn=has_bn, res=has_res, pool=spec.pool, act=spec.act,
                              nl=len(spec.launches), route=ops.gemm_route(spec.mode, spec.C, Np, ops.taps_of(spec.T, g0), g0, m0),
                              x_from=getattr(x, '_efgh_src', None), dx=bool(ctx.needs_input_grad[0]),
                              in_elems=int(x.numel()), custom=spec.custom_forward is not None))
        dy = as_rows(dy)
        p_w, p_bias, p_gamma, p_beta = ctx.params
        delivered = []
        # per-channel sums go straight into the flat gradient slices when the parameters live in a FlatParams (no padding)
        gs1 = gs2 = None
        if Np == N and has_bn and ctx.needs_input_grad[3] and ctx.needs_input_grad[4]:
            gs1, d1 = claim_grad(p_beta)
            gs2, d2 = claim_grad(p_gamma) if gs1 is not None else (None, None)
            if gs2 is None:
                gs1 = None
            else:
                delivered += [d1, d2]
        elif Np == N and has_bias and not has_bn and ctx.needs_input_grad[2]:
            gs1, d1 = claim_grad(p_bias)
            if gs1 is not None:
                delivered.append(d1)
        draw, pre_v, pre_gy, dbeta, dgamma, dbias, dres = TAILS[ctx.tail][1](ctx, spec, dy, sums, saved, gs1, gs2, delivered)
        # ---- dgrad is on the critical path of backward and is enqueued first; the weight gradient only needs draw and x, and
        # nothing in this backward pass waits for it: when it can be written straight into the flat gradient buffer it goes to the
        # weight-gradient stream BEHIND this layer's dgrad, so that it runs underneath the HBM-bound BatchNorm passes of the next
        # layer instead of competing with the dgrad for the matrix pipes (measured: waiting only for draw costs 3 ms per step)
        own_wgrad = ctx.needs_input_grad[1] and spec.custom_wgrad is None
        gW = dw_done = side = None
        if own_wgrad:
            gW, dw_done = claim_grad(p_w)
            side = ops.wgrad_stream(dev) if (gW is not None and ops.WGRAD_SIDE) else None
        dx = None
        if ctx.needs_input_grad[0]:
            kw = {}
            if dskip is not None:
                kw['add'] = as_rows(dskip)
            if ctx.xsrc is not None and spec.takes_bnsrc:
                kw['bnsrc'] = ctx.xsrc
            if pre_v is not None:
                kw['pre_v'] = pre_v
            dx = spec.dgrad(spec, weight, draw, x, **kw)
        # ---- wgrad
        dW = None
        if ctx.needs_input_grad[1] and spec.custom_wgrad is not None:
            dW = spec.custom_wgrad(x, weight, draw)
        elif own_wgrad:
            dW = gW if gW is not None else torch.empty_like(weight)

            xw, lazy_w = x, ctx.lazy
            if lazy_w is not None and not ops.wgrad_lazy_capable(spec.mode, spec.C, Np, spec.launches[0][0]):
                xw, lazy_w = materialize(x, lazy_w), None      # (a switch flipped between forward and backward: never wrong, only slower)

            # the forward's input transforms are taken off the node: freed when the weight gradient has been enqueued, and a second
            # backward over a retained graph transforms again
            kept, ctx.kept_v = ctx.kept_v, None

            def run_wgrad():
                x = xw
                for li, ((geom, m), lay) in enumerate(zip(spec.launches, spec.layouts)):
                    T = ops.taps_of(spec.T, geom)
                    xv = kept.pop(li, None) if kept else None
                    if xv is not None and ops.wgrad_route(spec.mode, spec.C, Np, T, geom) != 'wino2d':
                        xv = None            # (a switch flipped between forward and backward: dropped, like the fallback above)
                    dWp = torch.empty((Np, T, spec.C), dtype=torch.float32, device=dev)
                    ua = lay.fold_args()            # (ops.gather_wgrad(unpack=...): fold + unpack in one launch)
                    done = ops.gather_wgrad(x, ld_of(x), spec.C, T, Np, m, draw, Np, dWp, mode=spec.mode, geom=geom,
                                            table=spec.table, unpack=None if ua is None else (dW,) + ua,
                                            lazy=lazy_w, pre_gy=pre_gy, pre_v=xv)
                    if not done:             # (a single row chunk, or a path with a transform behind its fold)
                        lay.unpack(dWp, dW)
            if side is None:
                run_wgrad()
            else:
                side.wait_stream(torch.cuda.current_stream())
                x.record_stream(side)
                (draw if draw is not None else pre_gy).record_stream(side)
                for v in kept.values() if kept else ():      # (made on the forward's stream)
                    v.record_stream(side)
                if lazy_w is not None:       # (read by efgh_wino2d_input_act on the side stream when the kept transform is missing)
                    lazy_w.scale.record_stream(side)
                    lazy_w.shift.record_stream(side)
                with torch.cuda.stream(side):
                    run_wgrad()
            if gW is not None:
                dW = None
                delivered.append(dw_done if side is None else (lambda: dw_done(side)))
        if dres is not None and Np != N:
            dres = dres[..., :N]
        for done in delivered:               # after the writes are enqueued: the all-reduce bucket countdown
            done()
        return dx, dW, dbias, dgamma, dbeta, dres, None, None


# ---------------------------------------------------------------------------------------------
class ConcatFn(torch.autograd.Function):
    """torch.cat(parts, -1) of activations that their producers ALREADY wrote into adjacent channel slices of `buf`
    (GemmLayerFn's out_target): no copy forward, channel-slice views of the gradient backward.  `concat()` falls back to
    torch.cat when a part lives elsewhere (cropped decoder outputs of odd-height maps, layers without an out_target)."""

    @staticmethod
    def forward(ctx, buf, *parts):
        ctx.widths = [p.shape[-1] for p in parts]
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        outs, off = [], 0
        for w in ctx.widths:
            outs.append(g[..., off:off + w])
            off += w
        return (None,) + tuple(outs)


def concat(buf, parts):
    off, ok = 0, buf is not None
    for p in parts:
        ok = ok and p.shape[:-1] == buf.shape[:-1] and p.stride() == buf.stride() and \
            p.data_ptr() == buf.data_ptr() + 4 * off
        off += p.shape[-1]
    if ok and off == buf.shape[-1]:
        return ConcatFn.apply(buf, *parts)
    return torch.cat(parts, -1)


class MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.maxpool2(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, H, W, C = x.shape
        dx = torch.zeros_like(x) if (H % 2 or W % 2) else torch.empty_like(x)
        ops.maxpool2_bwd(x, dy.contiguous(), dx)
        return dx


class SegmentColMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg, nseg, C):
        x = as_rows(x)
        y, arg = ops.segment_colmax(x, ld_of(x), C, seg, nseg, want_arg=True)
        ctx.save_for_backward(arg)
        ctx.shape = (tuple(x.shape), C, nseg)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        shape, C, nseg = ctx.shape
        dx = torch.zeros(shape, dtype=torch.float32, device=dy.device)
        ops.segment_colmax_bwd(dy.contiguous(), arg, nseg, C, dx, shape[-1])
        return dx, None, None, None


class SegmentColMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, P, nseg, C):
        x = as_rows(x)
        ctx.meta = (tuple(x.shape), P, nseg, C)
        return ops.segment_colmean(x, ld_of(x), C, P, nseg)

    @staticmethod
    def backward(ctx, dy):
        shape, P, nseg, C = ctx.meta
        dx = torch.zeros(shape, dtype=torch.float32, device=dy.device)
        ops.segment_colmean_bwd(dy.contiguous(), P, nseg, C, dx, shape[-1])
        return dx, None, None, None


class SplatFn(torch.autograd.Function):
    """BCL splat + density normalisation of one lattice level; the level's rows are [el_minus_gr | feat[:, :Cf]]; the lattice
    arrays carry no gradient (generate_data.py:119)."""

    @staticmethod
    def forward(ctx, feat, lv, Cf, use_emg=True, normalize=True):
        feat = as_rows(feat)
        splat, wsum = ops.splat_fwd(lv, feat, Cf, use_emg, normalize)
        ctx.save_for_backward(wsum)
        ctx.meta = (lv, Cf, feat.shape[-1], use_emg, normalize)
        return splat

    @staticmethod
    def backward(ctx, g):
        (wsum,) = ctx.saved_tensors
        lv, Cf, ldf, use_emg, normalize = ctx.meta
        gfeat = torch.zeros((lv.n_in, ldf), dtype=torch.float32, device=g.device) if ldf != Cf else \
            torch.empty((lv.n_in, Cf), dtype=torch.float32, device=g.device)
        ops.splat_bwd(lv, g.contiguous(), wsum, Cf, gfeat, use_emg, normalize)
        return gfeat, None, None, None, None


class SliceFn(torch.autograd.Function):
    """slice step of a BCL (bilateralNN.py:248-263) onto `pts` (lattice.OutPoints): rows [H][ld] -> [n_out][C], plus the bias;
    bary / off carry no gradient (generate_data.py:119)."""

    @staticmethod
    def forward(ctx, feat, bias, pts, C):
        feat = as_rows(feat)
        ctx.meta = (pts, C, feat.shape[-1], bias)
        return ops.slice_fwd(pts, feat, C, None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, g):
        pts, C, ldf, bias = ctx.meta
        want_b = bias is not None and ctx.needs_input_grad[1]
        gfeat = torch.zeros((pts.H, ldf), dtype=torch.float32, device=g.device) if ldf != C else None
        gfeat, gbias = ops.slice_bwd(pts, as_rows(g), C, 0, want_b, gfeat)
        return (gfeat if ctx.needs_input_grad[0] else None), gbias, None, None


class Softmax2ToNchwFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = ops.softmax2_to_nchw(x)
        ctx.save_for_backward(y)
        ctx.ld = x.shape[-1]
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        B, _, H, W = y.shape
        dx = torch.empty((B, H, W, ctx.ld), dtype=torch.float32, device=dy.device)
        ops.softmax2_bwd(y, dy.contiguous(), dx)
        return dx


class HeadsToNchwFn(torch.autograd.Function):
    """G's depth and mask heads carried as one 4-channel map (layers.run_convt_heads) -> g_depth, g_mask (gnet.py:121-124)"""
    @staticmethod
    def forward(ctx, x):
        depth, mask = ops.heads_to_nchw(x.contiguous())
        ctx.save_for_backward(mask)
        ctx.set_materialize_grads(False)
        return depth, mask

    @staticmethod
    def backward(ctx, gd, gm):
        (mask,) = ctx.saved_tensors
        return ops.heads_bwd(mask, None if gm is None else gm.contiguous(), None if gd is None else gd.contiguous())


class NhwcToNchwFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Cs):
        ctx.meta = (tuple(x.shape), Cs)
        return ops.nhwc_to_nchw(x.contiguous(), Cs)

    @staticmethod
    def backward(ctx, dy):
        shape, Cs = ctx.meta
        return ops.nchw_to_nhwc(dy.contiguous(), shape[-1]), None


class RangeImageFn(torch.autograd.Function):
    """range image of e_l.[pc;1]; gradient w.r.t. e_l through the rasterised VALUES (x,y,z,r) only
    (indices are truncated integers), every rasterised point receives grad_img[u,v] (oracle note)."""

    @staticmethod
    def forward(ctx, pc, e_l, H, W, fov_up, fov_down):
        img, pix = ops.range_image(pc, e_l, H, W, fov_up, fov_down)
        ctx.save_for_backward(pc, e_l, pix)
        ctx.hw = (H, W)
        return img

    @staticmethod
    def backward(ctx, g):
        pc, e_l, pix = ctx.saved_tensors
        H, W = ctx.hw
        B, _, N = pc.shape
        ge = ops.raster_pose_bwd(pix, g.contiguous(), pc, e_l.detach(), B, N, H * W, 0).view(B, 4, 4)
        return None, ge, None, None, None, None


class DepthImageFn(torch.autograd.Function):
    """depth image; only the 4th channel (w) depends on cam_T_velo (row 2)."""

    @staticmethod
    def forward(ctx, pc, P, H, W):
        img, pix = ops.depth_image(pc, P, H, W)
        ctx.save_for_backward(pc, pix)
        ctx.hw = (H, W)
        return img

    @staticmethod
    def backward(ctx, g):
        pc, pix = ctx.saved_tensors
        H, W = ctx.hw
        B, _, N = pc.shape
        gP = ops.raster_pose_bwd(pix, g.contiguous(), pc, None, B, N, H * W, 1).view(B, 3, 4)
        return None, gP, None, None


class CorrHeadFn(torch.autograd.Function):
    """fnet.py:57,64,78-81 incl. the (max-min) normalisation and the mirror/circular pad."""

    @staticmethod
    def forward(ctx, cam, rng):
        cam, rng = cam.contiguous(), rng.contiguous()
        score, logit, rp, cam_mm, rng_mm = ops.corr_head(cam, rng, want_logit=True, want_aux=True)
        ctx.save_for_backward(cam, rng, rp, cam_mm, rng_mm, score)
        return score

    @staticmethod
    def backward(ctx, ds):
        cam, rng, rp, cam_mm, rng_mm, score = ctx.saved_tensors
        B, h, wc, C = cam.shape
        wr = rng.shape[2]
        off = int(wr / 8)
        dl = (ds * score * (1 - score) / 16.0).contiguous()                  # d/dlogit, incl. the 1/C scale
        dcam_n, drp = ops.corr1d_bwd(rp, cam, cam_mm, dl, B, h, wc, wr + 2 * off)
        drng_n = ops.corr_unpad(drp, B, h, wr, C, off)

        return ops.norm_bwd(cam, dcam_n.contiguous(), cam_mm), ops.norm_bwd(rng, drng_n.contiguous(), rng_mm)


class GImageLossFn(torch.autograd.Function):
    """(l_depth, l_mask) of Gloss over the full-resolution depth / mask images (loss_utils.py:186-199), one HIP sweep each way"""

    @staticmethod
    def forward(ctx, pred_depth, pred_mask, gdep4, img_mask):
        pred_depth, pred_mask = pred_depth.contiguous(), pred_mask.contiguous()
        out3, gt_depth, gt_mask = ops.gimg_loss_fwd(pred_depth, pred_mask, gdep4, img_mask)
        ctx.save_for_backward(pred_depth, pred_mask, gt_depth, img_mask, out3)
        n_valid = out3[2].detach().clone()             # pixels the masked depth mean was taken over (data-parallel weighting)
        ctx.mark_non_differentiable(gt_depth, gt_mask, n_valid)
        return out3[0], out3[1], gt_depth, gt_mask, n_valid

    @staticmethod
    def backward(ctx, g_dep, g_msk, _a, _b, _c):
        pred_depth, pred_mask, gt_depth, img_mask, out3 = ctx.saved_tensors
        d_depth, d_mask = ops.gimg_loss_bwd(pred_depth, pred_mask, gt_depth, img_mask, out3,
                                            g_dep.reshape(1).float().contiguous(), g_msk.reshape(1).float().contiguous())
        return d_depth, d_mask, None, None
