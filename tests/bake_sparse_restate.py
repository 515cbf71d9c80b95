"""Shared by test_bake_sparse_host.py and test_gpu_bake_sparse.py: the sparse histogram of a set of deposit codes,
and the sum of two blobs, restated in numpy from their definitions alone.

A code is texel << 10 | state. A code of 0xFFFFFFFF is a pad; a code whose texel is >= T is skipped and counted.
The histogram's cell (state, texel) holds how often its code occurs; the blob is sparse_restate.pack of the dense
form. The sum of two blobs is pack(unpack(a) + unpack(b)) in uint64.
"""
import numpy as np

import sparse_restate as S

PAD = 0xFFFFFFFF


def code(texel, state):
    return (np.asarray(texel, np.uint64) << np.uint64(10) | np.asarray(state, np.uint64)).astype(np.uint32)


def from_codes(codes, T):
    """codes uint32 [n] -> (blob, info dict, skipped)."""
    codes = np.asarray(codes, np.uint32)
    codes = codes[codes != np.uint32(PAD)]
    texel = codes >> np.uint32(10)
    skipped = int((texel >= T).sum())
    cell, count = np.unique(codes[texel < T], return_counts=True)
    dense = np.zeros((S.STATES, T), np.uint64)
    dense[(cell & np.uint32(1023)).astype(np.int64), (cell >> np.uint32(10)).astype(np.int64)] = count.astype(np.uint64)
    blob, info = S.pack(dense)
    return blob, info, skipped


def info_of(dense):
    """the info of a dense histogram whose counts may reach 2^54 (pack refuses those)"""
    T = dense.shape[1]
    B = S.blocks(T)
    per_texel = np.zeros(B * 64, np.int64)
    per_texel[:T] = (dense != 0).sum(0)
    return {"num_texels": T, "num_blocks": B, "rows": int(per_texel.reshape(B, 64).max(1).sum()),
            "cells": int(per_texel.sum()), "deposits": sum(int(v) for v in dense[dense != 0].tolist()) & S.M64,
            "too_large": int((dense > np.uint64(S.COUNT_MASK)).sum())}


def add(a, b, T):
    """blobs a, b of T texels -> (blob or None if a summed count reaches 2^54, info dict)."""
    dense = S.unpack(a, T) + S.unpack(b, T)  # counts below 2^54 each: no wrap in uint64
    info = info_of(dense)
    if info["too_large"]:
        return None, info
    blob, packed = S.pack(dense)
    assert packed == info
    return blob, info
