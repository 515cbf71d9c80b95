"""Shared by test_sparse_host.py and test_gpu_sparse.py: the sparse, blocked histogram format
restated in numpy from its definition alone.

T texels form B = ceil(T / 64) blocks of 64 consecutive texels. A blob is uint64 off[B + 1] followed by uint64
entry[64 * rows]: off[0] = 0, off[b + 1] - off[b] = r_b = the largest number of non-zero states any texel of block
b has, rows = off[B]; slot j of texel 64 b + l is entry[(off[b] + j) * 64 + l] = state << 54 | count for the
texel's j-th non-zero state in ascending order, 0 where the texel has fewer (or is past T).
"""
import numpy as np

STATES = 1024
COUNT_BITS = 54
COUNT_MASK = (1 << COUNT_BITS) - 1
M64 = (1 << 64) - 1


def blocks(T):
    return (T + 63) // 64


def nbytes(T, rows):
    return 8 * (blocks(T) + 1) + 512 * rows


def pack(dense):
    """dense uint64 [1024, T] (every count < 2^54) -> (blob uint64 [B + 1 + 64 rows], info dict)."""
    dense = np.asarray(dense)
    assert dense.shape[0] == STATES and dense.dtype == np.uint64
    T = dense.shape[1]
    B = blocks(T)
    assert int(dense.max(initial=0)) <= COUNT_MASK
    per_texel = np.zeros(B * 64, np.int64)
    per_texel[:T] = (dense != 0).sum(0)
    r = per_texel.reshape(B, 64).max(1)
    off = np.zeros(B + 1, np.uint64)
    off[1:] = np.cumsum(r).astype(np.uint64)
    rows = int(off[B])
    entry = np.zeros((rows, 64), np.uint64)
    t, s = np.nonzero(dense.T)  # the cells by texel, and within a texel by ascending state
    first = np.concatenate([[0], np.cumsum(per_texel)])[:-1]  # index of every texel's first cell
    j = np.arange(len(t)) - first[t]  # the cell's slot
    entry[off[t // 64].astype(np.int64) + j, t % 64] = (s.astype(np.uint64) << np.uint64(COUNT_BITS)) | dense[s, t]
    info = {"num_texels": T, "num_blocks": B, "rows": rows, "cells": int(per_texel.sum()),
            "deposits": sum(dense[s, t].tolist()) & M64, "too_large": 0}
    blob = np.concatenate([off, entry.reshape(-1)])
    assert blob.nbytes == nbytes(T, rows)
    return blob, info


def cells(blob, T, rows=None):
    """The non-padding entries of the texels below T as lists (texel, state, count), in each block's row order. With
    rows, every offset is clamped to it first (what the kernels do with the host's info.rows); a block whose begin
    is not below its end has no entries."""
    blob = np.asarray(blob, np.uint64)
    B = blocks(T)
    off = [int(v) for v in blob[: B + 1]]
    if rows is not None:
        off = [min(v, rows) for v in off]
    entry = blob[B + 1:].reshape(-1, 64)
    ts, ss, ns = [], [], []
    for b in range(B):
        if off[b] >= off[b + 1]:
            continue
        part = entry[off[b]: off[b + 1]]
        j, l = np.nonzero(part)
        keep = 64 * b + l < T
        v = part[j[keep], l[keep]]
        ts += (64 * b + l[keep]).tolist()
        ss += (v >> np.uint64(COUNT_BITS)).tolist()
        ns += (v & np.uint64(COUNT_MASK)).tolist()
    return ts, ss, ns


def unpack(blob, T, rows=None):
    """blob -> dense uint64 [1024, T]: every non-padding entry adds its count (mod 2^64)."""
    dense = [[0] * T for _ in range(STATES)]
    for t, s, n in zip(*cells(blob, T, rows)):
        dense[s][t] = (dense[s][t] + n) & M64
    return np.array(dense, np.uint64).reshape(STATES, T)


def fold(blob, T, table, rows=None):
    """sum over the blob's entries of count * table[state] mod 2^64 in Python integers: [T][3] (a list of lists)."""
    out = [[0, 0, 0] for _ in range(T)]
    tab = [[int(v) for v in row] for row in np.asarray(table).tolist()]
    for t, s, n in zip(*cells(blob, T, rows)):
        row, o = tab[s], out[t]
        for c in range(3):
            o[c] = (o[c] + n * row[c]) & M64
    return out
