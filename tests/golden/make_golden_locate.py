"""Golden data of the lattice point query (OutPoints.locate / efgh_lattice_locate): where ARBITRARY points fall on a lattice that
other points built, from the reference's own get_keys_and_barycentric (nets/generate_data.py:56-112), run UNMODIFIED on the CPU
through ref_harness.py.
Run:  python tests/golden/make_golden_locate.py  ->  tests/golden/locate.npz (data only; the scene and the query sets are
regenerated from seeds by tests/locate_contract.py, which also lists the stored arrays).

Per scale of locate_contract.SCALES a single-level lattice GenerateData(3, [[s, 1]], 'cpu') over the scene gives key tuple ->
pc1_lattice_offset; a query set goes through get_keys_and_barycentric at the same scale and every key is looked up in that
dictionary (-1 = absent).  The directed `alias` points: with box extents s2, s3 of key coordinates 2 and 3 and
g = gcd(s3 - 1, s2 s3 - 1), delta = (0, -4 (s3 - 1) / g, 4 (s2 s3 - 1) / g, -(the two)) is a lattice vector (multiples of 4, sum 0)
with key2int(k + delta) = key2int(k); points are placed around the position of k + delta for vertices k and kept when one of
their corners has an inserted key integer but a key that was not inserted (asserted with the reference's own key2int)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import ref_harness as rh            # noqa: E402
import locate_contract as Q         # noqa: E402

torch.set_num_threads(1)
nets, losses, tu = rh.import_reference()
import nets.generate_data as gdm    # noqa: E402
import nets.transforms as trm       # noqa: E402

N_ALIAS = 8


class Lattice:
    """the reference's single-level lattice of the scene at scale s, and its answers for query points"""

    def __init__(self, pc, s):
        self.s = s
        self.gd = gdm.GenerateData(3, [[s, 1]], 'cpu')
        _, gen = self.gd(torch.from_numpy(pc))
        self.H = int(gen[0]['pc1_hash_cnt'])
        self.off = gen[0]['pc1_lattice_offset'][0].numpy()                  # (4, N)
        keys, _ = self.keys(pc)
        self.maxs = keys.max(-1).max(-1).astype(np.int64)                   # generate_data.py:135-136
        self.mins = keys.min(-1).min(-1).astype(np.int64)
        self.row = {}
        for p in range(keys.shape[1]):
            for r in range(4):
                h = int(self.off[r, p])
                assert self.row.setdefault(tuple(keys[:, p, r].tolist()), h) == h
        assert len(self.row) == self.H and sorted(self.row.values()) == list(range(self.H))
        self.ints = {int(trm.key2int(np.array(k, dtype=np.int64), 3, self.maxs, self.mins)) for k in self.row}
        assert len(self.ints) == self.H

    def keys(self, pts):
        """keys (coordinate, point, corner) and barycentric (4, n) of points in the scene's frame (generate_data.py:130-132)"""
        q = torch.from_numpy(np.array(pts, dtype=np.float32, copy=True))
        q[:3, :] *= self.s
        keys, bary, _ = self.gd.get_keys_and_barycentric(q)
        return keys, bary.numpy()

    def locate(self, pts):
        """-> bary [n][4] float32, off [n][4] (-1 absent), out-of-box [n][4] bool, aliased [n][4] bool"""
        keys, bary = self.keys(pts)
        n = keys.shape[1]
        off = np.full((n, 4), -1, dtype=np.int64)
        outbox = np.zeros((n, 4), dtype=bool)
        alias = np.zeros((n, 4), dtype=bool)
        for p in range(n):
            for r in range(4):
                k = keys[:, p, r].astype(np.int64)
                off[p, r] = self.row.get(tuple(k.tolist()), -1)
                outbox[p, r] = bool(((k < self.mins) | (k > self.maxs)).any())
                alias[p, r] = off[p, r] < 0 and int(trm.key2int(k, 3, self.maxs, self.mins)) in self.ints
        assert not (outbox & (off >= 0)).any()
        return np.ascontiguousarray(bary.T), off, outbox, alias

    def alias_points(self):
        """a handful of points with an aliased corner -> (pts (3, n), mask [n][4])"""
        ext = self.maxs - self.mins + 1
        s2, s3 = int(ext[2]), int(ext[3])
        g = math.gcd(s3 - 1, s2 * s3 - 1)
        d1, d2 = -4 * (s3 - 1) // g, 4 * (s2 * s3 - 1) // g
        delta = np.array([0, d1, d2, -d1 - d2], dtype=np.int64)
        k0 = np.array(next(iter(self.row)), dtype=np.int64)
        assert trm.key2int(k0 + delta, 3, self.maxs, self.mins) == trm.key2int(k0, 3, self.maxs, self.mins)
        rs = np.random.RandomState(5)
        verts = np.array(sorted(self.row), dtype=np.int64)
        E = self.gd.elevate_mat.double().numpy()                             # (4, 3): generate_data.py:176-178 takes a key back
        pts, masks = [], []
        for k in verts[rs.permutation(len(verts))]:
            centre = E.T @ ((k + delta) / (self.gd.expected_std * self.s))
            cand = (centre + rs.normal(0, 0.15 / self.s, 3)).astype(np.float32)[:, None]
            _, off, outbox, alias = self.locate(cand)
            if alias.any():
                assert (outbox & alias == alias).all()                       # (an aliased corner lies outside the box)
                pts.append(cand)
                masks.append(alias[0])
            if len(pts) == N_ALIAS:
                break
        assert len(pts) == N_ALIAS, 'no aliased corner could be constructed'
        return np.concatenate(pts, 1), np.array(masks)


def main():
    store = {}
    pc = Q.scene()
    for s in Q.SCALES:
        t = Q.tag(s)
        lat = Lattice(pc, s)
        store[f'{t}.H'] = np.int64(lat.H)
        store[f'{t}.lattice_offset'] = lat.off[:, :Q.N_QUERY].T.astype(np.int16)
        assert lat.H < 2 ** 15
        for name in Q.SETS:
            bary, off, outbox, alias = lat.locate(Q.query_full(name))
            found = (off >= 0).sum(1)
            store[f'{t}.{name}.classes2048'] = np.bincount(found, minlength=5).astype(np.int64)
            store[f'{t}.{name}.outbox2048'] = np.int64(outbox.sum())
            assert not alias.any()          # (chance sets hold no aliased corner: the directed case below is what tests the box)
            n = Q.N_QUERY
            bary, off, outbox, found = bary[:n], off[:n], outbox[:n], found[:n]
            store[f'{t}.{name}.bary'] = bary.astype(np.float32)
            store[f'{t}.{name}.off'] = off.astype(np.int16)
            store[f'{t}.{name}.missing'] = np.array([(off < 0).sum(), (found == 0).sum()], dtype=np.int64)
            print(t, name, 'H', lat.H, 'classes (2048)', store[f'{t}.{name}.classes2048'].tolist(), 'out of box (2048)',
                  int(store[f'{t}.{name}.outbox2048']), 'stored: classes', np.bincount(found, minlength=5).tolist(), 'out of box',
                  int(outbox.sum()))
            if name == 'other' and s == 1.0:
                assert (np.bincount(found, minlength=5) > 0).all()
            if name == 'far':
                assert outbox.any()
            if name == 'self':
                assert (off >= 0).all() and np.array_equal(off, lat.off[:, :n].T)
        pts, mask = lat.alias_points()
        bary, off, outbox, alias = lat.locate(pts)
        assert np.array_equal(alias, mask) and mask.any(1).all() and (off[mask] == -1).all()
        store[f'{t}.alias.pts'] = pts
        store[f'{t}.alias.mask'] = mask.astype(np.int8)
        store[f'{t}.alias.bary'] = bary.astype(np.float32)
        store[f'{t}.alias.off'] = off.astype(np.int16)
        store[f'{t}.alias.missing'] = np.array([(off < 0).sum(), ((off >= 0).sum(1) == 0).sum()], dtype=np.int64)
        print(t, 'alias', 'aliased corners', int(mask.sum()), 'off', off.tolist())
    path = os.path.join(HERE, 'locate.npz')
    np.savez_compressed(path, **store)
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
