"""Expected BCL neighbour tables from a level's vertex keys (test helper; tests/golden/make_golden_bcl_radius.py checks it bit for bit
against the reference's own tables before it stores the keys in place of them).

The reference's build_it (nets/transforms.py:168-180) looks up key(h) + offset[t] through key2int, which has no range check: the
integer of a key outside the sample's [mins, maxs] box can equal that of another vertex - an aliased hit, kept by the reference."""
import numpy as np


def key2int(k, kmin, kmax):
    """transforms.py:62-77 on a [..][4] int64 array"""
    s = kmax.astype(np.int64) - kmin + 1
    d = k.astype(np.int64) - kmin
    return ((d[..., 0] * s[1] + d[..., 1]) * s[2] + d[..., 2]) * s[3] + d[..., 3]


def neighbor_table(keys, kmin, kmax, offsets):
    """keys [H][4] (vertex h's key, in the reference's numbering), the key box, offsets [F][4] ->
    (nbr [F][H] int32 as the reference's pc1_blur_neighbors, aliased hits [n][2] as (h, t))"""
    keys, kmin, kmax = np.asarray(keys, np.int64), np.asarray(kmin, np.int64), np.asarray(kmax, np.int64)
    vi = key2int(keys, kmin, kmax)
    order = np.argsort(vi, kind='stable')
    sv = vi[order]
    nk = keys[:, None, :] + np.asarray(offsets, np.int64)[None, :, :]          # [H][F][4]
    ni = key2int(nk, kmin, kmax)
    pos = np.clip(np.searchsorted(sv, ni), 0, len(sv) - 1)
    found = sv[pos] == ni
    nbr = np.where(found, order[pos], -1).astype(np.int32)
    out_box = ((nk[..., 1:] < kmin[1:]) | (nk[..., 1:] > kmax[1:])).any(-1)
    hs, ts = np.nonzero(found & out_box)
    return np.ascontiguousarray(nbr.T), np.stack([hs, ts], 1).astype(np.int32)
