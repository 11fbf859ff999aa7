"""CPU-side checks of tests/schedule_reference.py -- the checker of the two dispatch schedules must be able to fail: a correct
synthetic schedule passes, and each single defect (a tile missing, a tile twice, two classes swapped; a block in the wrong band,
filed twice, a counter above the capacity, a wrong class, a block id with column and row swapped) raises -- and of the export the
GPU tests reach the tile-order tables through (include/gsr_debug_layout.h)."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_helpers import compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub
import schedule_reference as S


# ---- synthetic schedules: what a correct device would leave ----
def make_order(cost_table, n_tiles):
    """A correct forward order: the tiles by class, heaviest first, each class in tile order; the tail left as poison."""
    order = np.full(S.FO_MAX_TILES, -77, np.int32)
    order[:n_tiles] = np.argsort(S.fwd_classes(cost_table, n_tiles), kind="stable")
    return order


def cost_table(n_tiles, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(4 * S.FO_MAX_TILES, np.int32)
    t[:4 * n_tiles] = (rng.integers(0, 0x7FFF, 4 * n_tiles) << 16).astype(np.int32)
    return t


def make_block_order(expected, tiles, rng=None):
    """A correct block_order buffer: every id in its queue, in a shuffled order (the device's comes from atomics)."""
    cap = S.bo_cap(tiles)
    o = np.full(S.BO_HEADER + S.BO_QUEUES * cap, -5, np.int32)
    o[:S.BO_HEADER] = 0
    o[S.BO_FLAG] = expected["filed"]
    ids = np.arange(expected["queue"].size)
    if rng is not None:
        ids = rng.permutation(ids)
    for i in ids:
        q = int(expected["queue"][i])
        o[S.BO_HEADER + q * cap + o[q]] = i
        o[q] += 1
    return o


def frame(W, H, seed):
    """A synthetic frame: ranges, n_contrib and mask bytes with block costs spread over many classes."""
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = gx * gy
    length = rng.integers(0, 600, tiles)
    length[rng.integers(0, tiles, max(1, tiles // 8))] = 0            # empty tiles
    end = np.cumsum(length)
    ranges = np.stack([end - length, end], axis=1).astype(np.int32)
    masks = rng.integers(0, 256, int(end[-1]) + 16).astype(np.uint8)
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    per_block = (rng.random((gy, 4, gx, 2)) * (length.reshape(gy, 1, gx, 1) + 1)).astype(np.int64)   # 0 .. length per 8x4 block
    nc += np.repeat(np.repeat(per_block.reshape(gy * 4, gx * 2), 4, axis=0), 8, axis=1)
    return ranges, nc[:H, :W].astype(np.int32), masks, tiles


# ---- the statements themselves ----
def test_wave_cost_decode_and_classes():
    assert S.wave_cost(np.int32(0)) == 0
    assert S.wave_cost(np.array([0x7FFFFFFF], np.int32))[0] == 0x7FFF + 0x7FFF
    assert S.wave_cost(np.array([-1], np.int32))[0] == 0x7FFF + 0x7FFF        # 0xFFFFFFFF: the sign bit is not part of `walked`
    assert S.wave_cost(np.array([5 << 16 | 7], np.int32))[0] == 5 + 3
    t = np.zeros(16, np.int32)
    assert S.fwd_classes(t, 4).tolist() == [63] * 4                            # all zero: mx = 1, every tile in the lightest class
    t[4] = 100 << 16                                                           # tile 1 heavy through ONE of its waves
    t[11] = 50 << 16
    t[12] = 1 << 16
    c = S.fwd_classes(t, 4)
    assert c[1] in (0, 1) and c[0] == 63 and c[2] in (31, 32) and c[3] == 63 and c[1] < c[2] < c[3]
    assert S.fwd_classes(t, 1).tolist() == [63]                                # slots at or past 4 * n_tiles are not read


def test_bo_class_and_capacity_match_the_header():
    assert S.bo_class(np.arange(0, 8)).tolist() == [0] * 8
    assert S.bo_class([8, 9, 10, 11, 12, 14, 15, 16, 31, 32]).tolist() == [1, 1, 2, 2, 3, 4, 4, 5, 8, 9]
    assert S.bo_class([1 << 10, (1 << 11) - 1, 1 << 20]).tolist() == [29, 31, 31]
    for tiles, tpb, cap in ((1, 1, 8), (7, 1, 8), (9, 2, 8), (256, 32, 16), (4096, 512, 256), (2500, 313, 160)):
        assert S.bo_tiles_per_band(tiles) == tpb and S.bo_cap(tiles) == cap
    hdr = open(os.path.join(ROOT, "3dgs-native_amd", "csrc", "gsr_internal.h")).read()
    for text in ("#define GSR_FO_MAX_TILES 4096", "#define GSR_FO_CLASSES 64", "#define GSR_BO_BANDS 8", "#define GSR_BO_CLASSES 32",
                 "#define GSR_BO_SHARDS 16", "#define GSR_BO_MAX_TILES 4096", "#define GSR_BO_HEADER (GSR_BO_QUEUES + 4)"):
        assert text in hdr, text
    assert S.bo_ints(4112, 16) == S.BO_HEADER + S.BO_QUEUES * S.bo_cap(257) and S.bo_ints(272, 3856) == S.BO_HEADER


def test_block_hits_counts_mask_bits_up_to_the_last_contributor():
    # one tile, 20 entries; block 3 (column 1, strip 1: pixels x 8-15, y 4-7) keeps 11 of them
    ranges = np.array([[0, 20]], np.int32)
    nc = np.zeros((16, 16), np.int32)
    nc[5, 9], nc[6, 15] = 11, 4
    nc[0, 0] = 20                                                              # block 0 keeps everything
    masks = np.zeros(36, np.uint8)
    masks[[0, 3, 10, 11, 19]] = 1 << 3
    masks[[1, 19]] |= 1
    kept, hits = S.block_hits(ranges, nc, masks, 16, 16)
    assert kept[0].tolist() == [20, 0, 0, 11, 0, 0, 0, 0]
    assert hits[0].tolist() == [2, 0, 0, 3, 0, 0, 0, 0]                        # entries 0, 3, 10 of [0, 11); entry 11 is past `kept`


# ---- forward order: pass, and every defect raises ----
@pytest.mark.parametrize("n_tiles", [1, 7, 256, 257, 3841, 4096])
def test_a_correct_forward_order_passes(n_tiles):
    for seed in (1, 2):
        t = cost_table(n_tiles, seed)
        S.check_fwd_order(make_order(t, n_tiles), t, n_tiles)
    garbage = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, 4 * S.FO_MAX_TILES).astype(np.int32)
    S.check_fwd_order(make_order(garbage, n_tiles), garbage, n_tiles)
    flat = np.full(4 * S.FO_MAX_TILES, -1, np.int32)
    S.check_fwd_order(make_order(flat, n_tiles), flat, n_tiles)


def test_forward_order_defects_raise():
    n = 300
    t = cost_table(n, 5)
    good = make_order(t, n)
    cls = S.fwd_classes(t, n)[good[:n]]
    assert len(set(cls.tolist())) > 8
    missing = good.copy()
    missing[17] = -77                                                         # the slot was never written
    with pytest.raises(AssertionError, match="no tile of the image"):
        S.check_fwd_order(missing, t, n)
    twice = good.copy()
    twice[17] = twice[18]                                                     # a tile twice (and so another never)
    with pytest.raises(AssertionError, match="never dispatched"):
        S.check_fwd_order(twice, t, n)
    swapped = good.copy()                                                     # two classes swapped: the first run and the second
    edges = np.flatnonzero(np.diff(cls)) + 1
    a, b = int(edges[0]), int(edges[1])
    swapped[:b] = np.concatenate([good[a:b], good[:a]])
    with pytest.raises(AssertionError, match="class sequence decreases"):
        S.check_fwd_order(swapped, t, n)
    # a tile in a wrong class: the statement (from a table in which that tile cost nothing) puts it in the lightest class
    other = t.copy()
    tile = int(good[a - 1])
    other[4 * tile:4 * tile + 4] = 0
    with pytest.raises(AssertionError, match="class"):
        S.check_fwd_order(good, other, n)


# ---- block order: pass, and every defect raises ----
@pytest.mark.parametrize("W,H", [(16, 16), (112, 16), (48, 48), (250, 130), (1023, 1021)])
def test_a_correct_block_order_passes(W, H):
    ranges, nc, masks, tiles = frame(W, H, 7)
    exp = S.expected_block_queues(ranges, nc, masks, W, H)
    assert exp["queue"].size == 8 * tiles
    S.check_block_order(make_block_order(exp, tiles, np.random.default_rng(1)), exp, tiles)
    un = S.unfiled_block_queues()
    S.check_block_order(np.zeros(S.BO_HEADER, np.int32), un, 4097)
    with pytest.raises(AssertionError, match="filed"):
        S.check_block_order(make_block_order(exp, tiles), un, tiles)


def _entry(o, tiles, block):
    """(queue, slot index into o) of a filed block id."""
    cap = S.bo_cap(tiles)
    body = o[S.BO_HEADER:].reshape(S.BO_QUEUES, cap)
    for q in np.flatnonzero(o[:S.BO_QUEUES]):
        hit = np.flatnonzero(body[q, :o[q]] == block)
        if hit.size:
            return int(q), S.BO_HEADER + int(q) * cap + int(hit[0])
    raise KeyError(block)


def _move(o, tiles, block, q_to):
    """Re-file `block` under queue q_to, counters adjusted: the buffer stays self-consistent."""
    cap = S.bo_cap(tiles)
    q, at = _entry(o, tiles, block)
    last = S.BO_HEADER + q * cap + int(o[q]) - 1
    o[at] = o[last]
    o[q] -= 1
    o[S.BO_HEADER + q_to * cap + o[q_to]] = block
    o[q_to] += 1


def test_block_order_defects_raise():
    W, H = 250, 130
    ranges, nc, masks, tiles = frame(W, H, 11)
    exp = S.expected_block_queues(ranges, nc, masks, W, H)
    good = make_block_order(exp, tiles, np.random.default_rng(2))
    cap = S.bo_cap(tiles)
    per_band = S.BO_CLASSES * S.BO_SHARDS
    block = 8 * 40 + 3
    q = int(exp["queue"][block])

    o = good.copy()                                                           # wrong band, same class and shard
    _move(o, tiles, block, (q + per_band) % S.BO_QUEUES)
    with pytest.raises(AssertionError, match="wrong band"):
        S.check_block_order(o, exp, tiles)

    o = good.copy()                                                           # wrong class, same band and shard
    cls = q // S.BO_SHARDS % S.BO_CLASSES
    _move(o, tiles, block, q + S.BO_SHARDS * (1 if cls < S.BO_CLASSES - 1 else -1))
    with pytest.raises(AssertionError, match="wrong class"):
        S.check_block_order(o, exp, tiles)

    o = good.copy()                                                           # filed twice
    q2 = (q + S.BO_SHARDS) % S.BO_QUEUES
    o[S.BO_HEADER + q2 * cap + o[q2]] = block
    o[q2] += 1
    with pytest.raises(AssertionError, match="filed 2 times"):
        S.check_block_order(o, exp, tiles)

    o = good.copy()                                                           # not filed at all
    _, at = _entry(o, tiles, block)
    o[at] = o[S.BO_HEADER + q * cap + o[q] - 1]
    o[q] -= 1
    with pytest.raises(AssertionError, match="not filed"):
        S.check_block_order(o, exp, tiles)

    o = good.copy()                                                           # a counter above the capacity (its ids were dropped)
    o[q] = cap + 1
    with pytest.raises(AssertionError, match="above the capacity"):
        S.check_block_order(o, exp, tiles)

    o = good.copy()                                                           # the flag alone
    o[S.BO_FLAG] = 0
    with pytest.raises(AssertionError, match="`filed` word"):
        S.check_block_order(o, exp, tiles)

    # a forward that takes block k for the rectangle at column k // 4, strip k % 4 (column and row swapped): its ids are filed
    # by the costs of other rectangles than the ones the backward decodes
    _, hits = S.block_hits(ranges, nc, masks, W, H)
    kept_sw = np.zeros_like(hits)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    full = np.zeros((gy * 16, gx * 16), np.int64)
    full[:H, :W] = nc
    kept = full.reshape(gy, 4, 4, gx, 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(tiles, 4, 2)
    for k in range(8):
        kept_sw[:, k] = kept[:, k % 4, k // 4]
    hits_sw = np.zeros_like(hits)
    for k in range(8):
        bit = (k % 4) * 2 + k // 4
        cs = np.concatenate([[0], np.cumsum((masks >> bit) & 1, dtype=np.int64)])
        hits_sw[:, k] = cs[ranges[:, 0] + kept_sw[:, k]] - cs[ranges[:, 0]]
    swapped = {"filed": 1, "queue": S.block_queue(np.repeat(np.arange(tiles), 8), S.bo_class(hits_sw.reshape(-1)), tiles)}
    assert (swapped["queue"] != exp["queue"]).any()
    with pytest.raises(AssertionError, match="wrong class"):
        S.check_block_order(make_block_order(swapped, tiles), exp, tiles)

    S.check_block_order(good, exp, tiles)                                     # (none of the above touched the good one)


# ---- the export the GPU tests find the tables through ----
HDR = os.path.join(ROOT, "include", "gsr_debug_layout.h")


def test_layout_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_debug_layout.h"\n'
                                'int main(void) { int (*f)(int64_t, size_t *, size_t *) = gsr_fwd_order_tables_offset; (void)f;\n'
                                '                 return GSR_FWD_ORDER_MAX_TILES == 4096 && GSR_ABI_VERSION == 7 ? 0 : 1; }\n')


def test_layout_export_is_bound_documented_and_inside_the_workspace(libpath):
    declared = declared_names(HDR)
    assert declared == {"gsr_fwd_order_tables_offset"}
    assert hasattr(C.CDLL(libpath), "gsr_fwd_order_tables_offset")
    _lib = sub("_lib")
    assert set(_lib.DEBUG_LAYOUT_EXPORTS) == declared                          # its own table: gsr.h's stays as it is
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS, _lib.CAMERA_EXPORTS, _lib.DENSIFY_STATS_EXPORTS,
                  _lib.ANTIALIAS_EXPORTS, _lib.FILTER3D_EXPORTS, _lib.EXPOSURE_EXPORTS):
        assert not (declared & set(other))
    assert "gsr_fwd_order_tables_offset" not in open(os.path.join(ROOT, "include", "gsr.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gsr_fwd_order_tables_offset" in doc and "gsr_debug_layout.h" in doc
    L = _lib.lib()
    assert L.gsr_abi_version() == 7 and _lib.FWD_ORDER_MAX_TILES == S.FO_MAX_TILES
    cost, order = C.c_size_t(0), C.c_size_t(0)
    last = -1
    for N in (0, 1, 255, 3000, 6000, 1 << 20):
        assert L.gsr_fwd_order_tables_offset(N, C.byref(cost), C.byref(order)) == _lib.GSR_OK
        assert cost.value % 256 == 0 and order.value == cost.value + 16 * S.FO_MAX_TILES     # four ints per tile, then the order
        assert order.value + 4 * S.FO_MAX_TILES <= L.gsr_geom_workspace_bytes(N)
        assert cost.value > last                                              # behind everything that grows with N
        last = cost.value
    assert L.gsr_fwd_order_tables_offset(10, None, C.byref(order)) == _lib.GSR_E_NULL
    assert L.gsr_fwd_order_tables_offset(10, C.byref(cost), None) == _lib.GSR_E_NULL
    assert L.gsr_fwd_order_tables_offset(-1, C.byref(cost), C.byref(order)) == _lib.GSR_E_DIMS
