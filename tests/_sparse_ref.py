"""numpy restatement of the sparse radiance volume's layout (include/panonerf_hip.h, "sparse radiance volume"): the slot
order, pack and unpack.  Loops over bricks; fp16 rounding is numpy's astype."""
import numpy as np

import _volume_ref as ref

EDGE = ref.BRICK + 1


def table_of(occ):
    """int32 table like occ: slots 0 .. B - 1 in ascending brick index, -1 where absent"""
    flat = occ.reshape(-1) > 0
    return np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32).reshape(occ.shape)


def _blocks(table, res):
    """(slot, slices of the brick's vertices in the grid, slices of the same vertices in the stored brick), ascending"""
    for (bi, bj, bk), slot in np.ndenumerate(table):
        if slot >= 0:
            lo = (8 * bi, 8 * bj, 8 * bk)
            n = tuple(min(l + EDGE, r) - l for l, r in zip(lo, res))
            yield int(slot), tuple(slice(l, l + m) for l, m in zip(lo, n)), tuple(slice(0, m) for m in n)


def pack(data, dtype=np.float32, table=None):
    """(table, pool [B, 9, 9, 9, C] of dtype): the present bricks of data [nx, ny, nz, C], zeros past the grid's end"""
    if table is None:
        table = table_of(ref.occupancy(data))
    pool = np.zeros((int((table >= 0).sum()), EDGE, EDGE, EDGE, data.shape[3]), dtype)
    for slot, grid, local in _blocks(table, data.shape[:3]):
        pool[(slot,) + local] = data[grid].astype(dtype)
    return table, pool


def unpack(table, pool, res):
    """fp32 [nx, ny, nz, C]: each vertex from the present brick of lowest index that holds it, 0 in no present brick"""
    out = np.zeros(tuple(res) + (pool.shape[4],), np.float32)
    for slot, grid, local in reversed(list(_blocks(table, res))):  # descending, so the lowest index writes last
        out[grid] = pool[(slot,) + local].astype(np.float32)
    return out
