"""What csrc/refine.hip computes, restated in numpy operation by operation (include/efgh_hip.h states it in words): the pose
P = Pstart D(z * scale), the chain rule from dMI/dP to the six rigid parameters, Adam, the best-so-far bookkeeping, and the
selection of the `keep` largest of K values.  numpy's float64 add, multiply, divide and sqrt are IEEE operations rounded on their
own, which is what the kernel is built for (-ffp-contract=off), so the device differs from this file only where its sin, cos, sqrt
and division differ from the host's; the bounds below say by how much at most.  They are derived, never fitted to an output, and
written generously enough (every rounding of a stage counted, k 2^-53 sum |terms|) to hold an implementation that sums in another
order too - torch.optim.Adam and autograd, which tests/test_refine_multi_host.py compares with.

Layout: G, Pstart, P (B,S,3,4); the state z, m, v (B,S,6), or (1,S,6) when the batch shares its parameters (pool); mi, best_mi,
best_iter (B,S) or (1,S)."""
import math

import numpy as np

# Largest errors of the device's float64 sin, cos, sqrt and division in ulp.  ASSUMED, all four: the ROCm math accuracy table is not
# in the toolchain at hand (sin and cos 2 ulp as the OpenCL double-precision profile allows at most 4; sqrt and the division are
# expanded by the compiler to correctly rounded sequences as far as is known, 1 ulp leaves room).  U_HOST: numpy's own sin and cos
# (the C library's, below 1 ulp); its sqrt and division are correctly rounded and are given the same allowance.
U_SIN = 2
U_COS = 2
U_SQRT = 1
U_DIV = 1
U_HOST = 1
EPS = 2.0 ** -53
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8       # torch.optim.Adam's defaults; lr = 1
MAX_K, MAX_KEEP = 4096, 64
MARGIN = 2.0                                     # over every bound: second-order terms, and this file's own roundings


def bias_terms(t):
    """Adam's two bias terms of step t >= 1 as the host forms them in Python floats -> (step_size, bc2_sqrt)"""
    return 1.0 / (1.0 - BETA1 ** t), math.sqrt(1.0 - BETA2 ** t)


def _trig(p):
    return np.sin(p[..., 0]), np.cos(p[..., 0]), np.sin(p[..., 1]), np.cos(p[..., 1]), np.sin(p[..., 2]), np.cos(p[..., 2])


def rotation(p):
    """p (..., >= 3) -> R (..., 3, 3) = Rz Ry Rx with score._rigid's products in its order"""
    sx, cx, sy, cy, sz, cz = _trig(p)
    R = np.empty(p.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sy, cy * sx, cy * cx
    return R


def rotation_derivatives(p):
    """p (..., >= 3) -> dR (3, ..., 3, 3): the nine entries' derivatives by the angle about x, y and z, written out.  By x: column 1
    becomes column 2 and column 2 minus column 1; by z: row 0 becomes minus row 1 and row 1 row 0; by y the products are formed"""
    sx, cx, sy, cy, sz, cz = _trig(p)
    R = rotation(p)
    d = np.zeros((3,) + R.shape)
    d[0][..., 1], d[0][..., 2] = R[..., 2], -R[..., 1]
    d[1][..., 0, 0], d[1][..., 0, 1], d[1][..., 0, 2] = -(cz * sy), cz * cy * sx, cz * cy * cx
    d[1][..., 1, 0], d[1][..., 1, 1], d[1][..., 1, 2] = -(sz * sy), sz * cy * sx, sz * cy * cx
    d[1][..., 2, 0], d[1][..., 2, 1], d[1][..., 2, 2] = -cy, -(sy * sx), -(sy * cx)
    d[2][..., 0, :], d[2][..., 1, :] = -R[..., 1, :], R[..., 0, :]
    return d


def _entry_error(dp):
    """how far an entry of R or of a derivative may lie from the device's when the angles differ by dp: an entry is at most two
    products of at most three factors, each a sine or cosine (magnitude <= 1) off by tau = dp + (U + U_HOST) ulp; a product is off by
    3 tau and two roundings, the sum of two rounds once more on a magnitude <= 2"""
    tau = dp + (max(U_SIN, U_COS) + U_HOST) * 2 * EPS
    return 6 * tau + 6 * EPS


def pose(Pstart, z, scale, dz=None):
    """Pstart (B,S,3,4), z (B or 1,S,6) -> (P (B,S,3,4), its bound).  Entry [i][j] = (A[i][0] D[0][j] + A[i][1] D[1][j]) +
    A[i][2] D[2][j], column 3 plus Pstart[i][3]; the zero row of D is not multiplied.  A row whose z is all zero is Pstart itself,
    bit for bit.  dz: how far z may be off (like z), None for an exact z.
    Bound: a rotation entry sum_k |A_ik| (entry error) + 5 eps sum_k |A_ik R_kj| (three products, two sums); column 3 sum_k |A_ik| dt_k
    + 7 eps (sum_k |A_ik t_k| + |A_i3|)"""
    scale = np.asarray(scale, np.float64)
    p = z * scale
    dp = (0.0 if dz is None else dz * scale) + EPS * np.abs(p)
    R, t = rotation(p), p[..., 3:]
    A, c = Pstart[..., :3], Pstart[..., 3]
    P = np.empty_like(Pstart)
    bound = np.empty_like(Pstart)
    eR = _entry_error(dp[..., :3].max(-1))[..., None]
    absA = np.abs(A)
    with np.errstate(all='ignore'):
        for j in range(3):
            P[..., j] = (A[..., 0] * R[..., None, 0, j] + A[..., 1] * R[..., None, 1, j]) + A[..., 2] * R[..., None, 2, j]
            bound[..., j] = absA.sum(-1) * eR + 5 * EPS * (absA * np.abs(R[..., None, :, j])).sum(-1)
        P[..., 3] = ((A[..., 0] * t[..., None, 0] + A[..., 1] * t[..., None, 1]) + A[..., 2] * t[..., None, 2]) + c
        bound[..., 3] = (absA * dp[..., None, 3:]).sum(-1) + 7 * EPS * ((absA * np.abs(t[..., None, :])).sum(-1) + np.abs(c))
    still = np.broadcast_to((z == 0).all(-1), Pstart.shape[:2])
    P[still], bound[still] = Pstart[still], 0.0
    return P, MARGIN * bound


def chain_rule(G, Pstart, z, scale):
    """dMI/dz_a = scale_a sum_b sum_ij G[b,s,i,j] (Pstart[b,s] dD/dp_a)[i,j] at p = z * scale -> (like z, its bound).  For an angle
    the matrix is A dR_a in the three rotation columns (entry (A[i][0] dR[0][j] + A[i][1] dR[1][j]) + A[i][2] dR[2][j]) and 0 in
    column 3; for the translation k it is column k of A in column 3.  The terms of one sample are added in row-major order from
    the first, the samples' sums in index order; a term whose G entry is 0 is 0 whatever Pstart holds; an axis with scale 0 has
    gradient 0 exactly.
    Bound: sum |G_ij| sum_k |A_ik| (entry error) + (10 nb + 2) eps sum |G_ij A_ik dR_kj| for nb samples a row (three products and two
    sums an entry, one product and one sum a term, one sum a sample), times scale_a, + eps |result| for that product"""
    scale = np.asarray(scale, np.float64)
    B = G.shape[0]
    pooled = z.shape[0] == 1 and B > 1
    p = z * scale
    dR = rotation_derivatives(p)
    eR = _entry_error(EPS * np.abs(p[..., :3]).max(-1))
    tot, mag, soft = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
    with np.errstate(all='ignore'):
        for b in range(B):
            zb = 0 if pooled else b
            A, g = Pstart[b], G[b]
            for a in range(6):
                sub = np.zeros(G.shape[1])
                for i in range(3):
                    for j in (range(3) if a < 3 else (3,)):
                        gij = g[:, i, j]
                        if a < 3:
                            M = (A[:, i, 0] * dR[a][zb][:, 0, j] + A[:, i, 1] * dR[a][zb][:, 1, j]) + A[:, i, 2] * dR[a][zb][:, 2, j]
                            full = (np.abs(A[:, i, :3]) * np.abs(dR[a][zb][:, :, j])).sum(-1)
                            loose = np.abs(A[:, i, :3]).sum(-1) * eR[zb]
                        else:
                            M = A[:, i, a - 3]
                            full, loose = np.abs(M), 0.0
                        on = gij != 0
                        sub = np.where(on, sub + gij * M, sub)
                        mag[zb, :, a] += np.where(on, np.abs(gij) * full, 0.0)
                        soft[zb, :, a] += np.where(on, np.abs(gij) * loose, 0.0)
                tot[zb, :, a] = tot[zb, :, a] + sub
        nb = B if pooled else 1
        free = scale != 0
        grad = np.where(free, scale * tot, 0.0)
        bound = np.where(free, scale * (soft + (10 * nb + 2) * EPS * mag) + EPS * np.abs(grad), 0.0)
    return grad, MARGIN * bound


def adam(dmi, ddmi, z, m, v, t):
    """one step of torch.optim.Adam(lr=1, betas=(0.9, 0.999), eps=1e-8) on -mi from the gradient dmi = dMI/dz (off by at most ddmi) and
    the state before it, t >= 1 the step's number -> dict z, m, v and dz, dm, dv, their bounds.
      g = -dmi; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) (g g); denom = sqrt(v) / bc2_sqrt + eps; z = z - step_size (m / denom)
    Bounds, stage by stage: m: (1 - b1) dg + 3 eps (|b1 m| + |(1 - b1) g|).  v: (1 - b2) (2 |g| + dg) dg + 4 eps (|b2 v| + (1 - b2) g^2).
    sqrt: |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / sqrt a), and (U_SQRT + U_HOST) ulp of its own.  The quotient by bc2_sqrt:
    (U_DIV + U_HOST) ulp and two more for the bias term itself (torch forms it as x ** 0.5); + eps for the sum with eps.  The ratio
    m / denom: (dm + |ratio| ddenom) / (denom - ddenom) and (U_DIV + U_HOST) ulp.  z: step_size times that, four roundings on the
    product (two of them the bias term's), one on the difference"""
    step_size, bc2 = bias_terms(t)
    with np.errstate(all='ignore'):
        g, dg = -dmi, ddmi
        m1 = BETA1 * m + (1.0 - BETA1) * g
        dm = (1.0 - BETA1) * dg + 3 * EPS * (np.abs(BETA1 * m) + np.abs((1.0 - BETA1) * g))
        v1 = BETA2 * v + (1.0 - BETA2) * (g * g)
        dv = (1.0 - BETA2) * (2 * np.abs(g) + dg) * dg + 4 * EPS * (np.abs(BETA2 * v) + (1.0 - BETA2) * (g * g))
        sq = np.sqrt(v1)
        dsq = np.minimum(np.sqrt(dv), np.where(sq > 0, dv / np.where(sq > 0, sq, 1.0), np.inf)) + (U_SQRT + U_HOST) * 2 * EPS * sq
        q = sq / bc2
        dq = dsq / bc2 + (U_DIV + U_HOST + 2) * 2 * EPS * q
        denom = q + ADAM_EPS
        dden = dq + EPS * denom
        ratio = m1 / denom
        dratio = (dm + np.abs(ratio) * dden) / (denom - dden) + (U_DIV + U_HOST) * 2 * EPS * np.abs(ratio)
        z1 = z - step_size * ratio
        dz = step_size * dratio + 4 * EPS * np.abs(step_size * ratio) + EPS * np.abs(z1)
    return dict(z=z1, m=m1, v=v1, dz=MARGIN * dz, dm=MARGIN * dm, dv=MARGIN * dv)


def new_state(B, S, pool, iters):
    rows = (1 if pool else B, S)
    return dict(z=np.zeros(rows + (6,)), m=np.zeros(rows + (6,)), v=np.zeros(rows + (6,)), best_mi=np.zeros(rows),
                best_iter=np.zeros(rows, np.int64), best_pose=np.zeros((B, S, 3, 4)), trace=np.zeros((iters,) + rows))


def step(st, G, Pstart, P, mi, scale, it, last=False):
    """efgh_refine_step on the state dict `st` (new_state's keys), in place: the bookkeeping for iterate `it`, which P holds and mi
    (B or 1, S) and G were computed at; then, unless `last`, the chain rule, Adam's step it + 1 and the next pose -> dict with
    `better` (bool, like mi), and unless last `P` (the next pose) and the bounds dz, dm, dv, dP of z, m, v and P"""
    st['trace'][it] = mi
    with np.errstate(invalid='ignore'):
        better = np.ones(mi.shape, bool) if it == 0 else mi > st['best_mi']       # strict: the first of equals stays; a NaN never wins
    st['best_mi'] = np.where(better, mi, st['best_mi'])
    st['best_iter'] = np.where(better, it, st['best_iter']).astype(np.int64)
    st['best_pose'] = np.where(np.broadcast_to(better, P.shape[:2])[:, :, None, None], P, st['best_pose'])
    out = dict(better=better)
    if last:
        return out
    dmi, ddmi = chain_rule(G, Pstart, st['z'], scale)
    a = adam(dmi, ddmi, st['z'], st['m'], st['v'], it + 1)
    st['z'], st['m'], st['v'] = a['z'], a['m'], a['v']
    out['P'], out['dP'] = pose(Pstart, a['z'], scale, a['dz'])
    out.update(dz=a['dz'], dm=a['dm'], dv=a['dv'], dmi=dmi, ddmi=ddmi)
    return out


def refine_multi(scorer, starts, iters, scale, pool=False):
    """the whole loop: scorer(P (B,S,3,4)) -> (mi (B,S) or (S,), dMI/dP (B,S,3,4)); every start climbs on its own -> dict pose
    (B,S,3,4), mi, start_mi, best_iter (B,S) or (S,), trace (iters,B,S) or (iters,S)"""
    starts = np.ascontiguousarray(starts, np.float64)
    B, S = starts.shape[:2]
    st = new_state(B, S, pool, iters)
    P = starts.copy()
    for it in range(iters):
        mi, G = scorer(P)
        out = step(st, G, starts, P, np.asarray(mi, np.float64).reshape(st['best_mi'].shape), scale, it, last=it + 1 == iters)
        if it + 1 < iters:
            P = out['P']
    cut = (lambda a: a[0]) if pool else (lambda a: a)
    return dict(pose=st['best_pose'], mi=cut(st['best_mi']), start_mi=cut(st['trace'][0]), best_iter=cut(st['best_iter']),
                trace=st['trace'][:, 0] if pool else st['trace'])


def best(mi):
    """the start with the largest mi, the first of equals -> like mi without its last axis"""
    return np.argmax(mi, -1)


def select(val, keep):
    """val (rows, K) -> int32 (rows, keep): the keep largest of a row in descending order; equal values (0.0 and -0.0 are equal) by
    ascending index; a NaN ranks below every number, NaNs among themselves by index"""
    val = np.asarray(val, np.float64)
    rows, K = val.shape
    assert 1 <= K <= MAX_K and 1 <= keep <= min(K, MAX_KEEP)
    out = np.empty((rows, keep), np.int32)
    for r in range(rows):
        order = sorted(range(K), key=lambda i: (1, 0.0, i) if math.isnan(val[r, i]) else (0, -val[r, i], i))
        out[r] = order[:keep]
    return out
