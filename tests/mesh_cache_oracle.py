"""numpy oracle of the incremental mesher's dirty rule: which feature rows changed, which nodes those rows make
dirty, and which query-level nodes must be queried again — in the key-shift form the kernels implement and in a brute-force
geometric form that knows nothing about Morton parents.

Slots are featured levels, top-down; slot s + 1 halves the node edge of slot s.  `keys[s]` are Morton keys (x the most significant
bit of every triplet) in insertion order, `ids[s]` the [n, 8] corner rows, `prev[s]` the node count at the previous call and
`flags[s]` one bool per real feature row."""
import numpy as np


def changed_rows(table, snap):
    """table [rows, 8] f32 with the trash row last, snap [snap_rows, 8] f32 -> bool [rows - 1]: beyond the snapshot, or any of the
    32 bytes differs"""
    real = np.ascontiguousarray(table[:-1], np.float32).view(np.uint32)
    old = np.ascontiguousarray(snap, np.float32).reshape(-1, 8).view(np.uint32)
    out = np.ones(len(real), bool)
    n = min(len(real), len(old))
    out[:n] = (real[:n] != old[:n]).any(1)
    return out


def dirty_nodes(ids, prev, flags):
    """bool [n]: the node is new (index >= prev) or one of its eight corner rows is flagged"""
    ids = np.asarray(ids).reshape(-1, 8)
    out = np.asarray(flags, bool)[ids].any(1) if len(ids) else np.zeros(0, bool)
    out[int(prev):] = True
    return out


def dirty_query_nodes(keys, ids, prev, flags, sq):
    """the rule's key-shift form: bool per node of slot sq"""
    L = len(keys)
    nd = [dirty_nodes(ids[s], prev[s], flags[s]) for s in range(L)]
    qk = np.asarray(keys[sq], np.int64)
    out = nd[sq].copy()
    for s in range(sq + 1, L):  # finer: a dirty node marks its ancestor
        anc = np.asarray(keys[s], np.int64)[nd[s]] >> (3 * (s - sq))
        out |= np.isin(qk, anc)
    for s in range(sq):  # coarser: the ancestor, if it exists, is asked
        table = {int(k): bool(d) for k, d in zip(keys[s], nd[s])}
        out |= np.array([table.get(int(k) >> (3 * (sq - s)), False) for k in qk], bool)
    return out


def decode(keys):
    """Morton key -> (x, y, z), bit by bit"""
    keys = np.asarray(keys, np.int64)
    xyz = np.zeros((len(keys), 3), np.int64)
    for b in range(21):
        for a in range(3):
            xyz[:, a] |= ((keys >> (3 * b + 2 - a)) & 1) << b
    return xyz


def boxes(keys, s, L):
    """[n, 3] lower and upper corners of slot s's nodes in units of the finest slot's node edge"""
    size = 1 << (L - 1 - s)
    lo = decode(keys) * size
    return lo, lo + size


def dirty_query_nodes_brute(keys, ids, prev, flags, sq):
    """the same set from geometry alone: a query node is dirty iff some dirty node of any slot overlaps its (open) box"""
    L = len(keys)
    qlo, qhi = boxes(keys[sq], sq, L)
    out = np.zeros(len(qlo), bool)
    for s in range(L):
        nd = dirty_nodes(ids[s], prev[s], flags[s])
        lo, hi = boxes(np.asarray(keys[s])[nd], s, L)
        if len(lo):
            out |= ((qlo[:, None, :] < hi[None]) & (lo[None] < qhi[:, None, :])).all(2).any(1)
    return out


def encode(xyz):
    xyz = np.asarray(xyz, np.int64)
    key = np.zeros(len(xyz), np.int64)
    for b in range(21):
        for a in range(3):
            key |= ((xyz[:, a] >> b) & 1) << (3 * b + 2 - a)
    return key


def random_octree(rng, n_leaves, L=3, span=8):
    """A random octree of L slots: leaves drawn in a span^3 box of the finest slot, every slot's nodes in a shuffled (insertion)
    order, corner rows numbered per slot by corner position.  Returns (keys, ids, rows) with rows[s] the number of real rows."""
    leaves = np.unique(encode(rng.integers(0, span, (n_leaves, 3))))
    keys, ids, rows = [], [], []
    off = np.array([[(j >> 2) & 1, (j >> 1) & 1, j & 1] for j in range(8)], np.int64)
    for s in range(L):
        k = np.unique(leaves >> (3 * (L - 1 - s)))
        rng.shuffle(k)
        corners = (decode(k)[:, None, :] + off[None]).reshape(-1, 3)
        uniq, inv = np.unique(corners, axis=0, return_inverse=True)
        keys.append(k)
        ids.append(inv.reshape(-1, 8).astype(np.int32))
        rows.append(len(uniq))
    return keys, ids, rows
