"""Numpy helpers for the brick-set marching cubes (csrc/shine_mc_sparse.hip): cutting a dense grid into bricks and putting a brick
set back into the dense grid it stands for — value 0 and mask 0 wherever no brick covers a point."""
import numpy as np


def cut(sdf, mask, B, keep_fraction=1.0, seed=0):
    """The bricks (edge B, origins at multiples of B) of a dense grid; the last brick per axis reaches beyond the grid when the
    shape is no multiple of B and is padded with an arbitrary non-zero value there (it must not matter).  A random
    `keep_fraction` of the bricks is kept.  Returns (values [n,B,B,B] f32, mask [n,B,B,B] bool | None, origins [n,3] int64)."""
    X, Y, Z = sdf.shape
    nb = [(s + B - 1) // B for s in (X, Y, Z)]
    pad = [(0, n * B - s) for n, s in zip(nb, (X, Y, Z))]
    v = np.pad(sdf.astype(np.float32), pad, constant_values=7.5)
    v = v.reshape(nb[0], B, nb[1], B, nb[2], B).transpose(0, 2, 4, 1, 3, 5).reshape(-1, B, B, B)
    m = None
    if mask is not None:
        m = np.pad(mask.astype(bool), pad, constant_values=True)
        m = m.reshape(nb[0], B, nb[1], B, nb[2], B).transpose(0, 2, 4, 1, 3, 5).reshape(-1, B, B, B)
    org = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) * B for n in nb], indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    keep = rng.random(len(org)) < keep_fraction if keep_fraction < 1.0 else np.ones(len(org), bool)
    order = rng.permutation(np.flatnonzero(keep))  # (the brick order carries no meaning)
    return np.ascontiguousarray(v[order]), (np.ascontiguousarray(m[order]) if m is not None else None), org[order]


def dense_twin(values, mask, origins, shape):
    """The dense (sdf f32, mask bool) grids a brick set stands for: the bricks' values and masks (mask None: set wherever a brick
    covers the point), 0 / False elsewhere; what reaches beyond `shape` is dropped."""
    X, Y, Z = (int(s) for s in shape)
    B = values.shape[1]
    sdf = np.zeros((X, Y, Z), np.float32)
    msk = np.zeros((X, Y, Z), bool)
    for i, (ox, oy, oz) in enumerate(np.asarray(origins, np.int64)):
        ex, ey, ez = min(B, X - ox), min(B, Y - oy), min(B, Z - oz)
        if ex <= 0 or ey <= 0 or ez <= 0:
            continue
        sdf[ox:ox + ex, oy:oy + ey, oz:oz + ez] = values[i, :ex, :ey, :ez]
        msk[ox:ox + ex, oy:oy + ey, oz:oz + ez] = True if mask is None else mask[i, :ex, :ey, :ez]
    return sdf, msk


def covered_points(origins, B):
    """the set of grid points (as rows) a brick table covers"""
    ax = np.arange(B, dtype=np.int64)
    off = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pts = (np.asarray(origins, np.int64)[:, None, :] + off[None]).reshape(-1, 3)
    return {tuple(p) for p in pts.tolist()}
