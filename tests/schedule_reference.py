"""The two dispatch schedules as integer numpy statements (test infrastructure; nothing in the package imports this, and it
never calls the library): the forward blend's tile order (csrc/fwd_order.h, gsr_internal.h "forward tile order") and the backward
blend's block order (blend_fwd.hip file_blocks, gsr_internal.h "block order").  Each check_* names the invariant it found broken.

Forward tile order.  fwd_cost holds four ints per tile, one per wave of last frame's blend.  A wave's cost is
walked + (staged >> 1) with walked = (v >> 16) & 0x7FFF and staged = v & 0xFFFF; a tile costs the largest of its four; the
classes are 63 - min(63, int(float32(cost) * (float32(63) / float32(mx)))) with mx = max(1, every tile's cost), class 0 the
heaviest.  fwd_order[:n_tiles] lists the tiles class by class, heaviest first.  The order INSIDE a class is not part of the
contract (it comes from LDS atomics inside a wave) and is not asserted.  Slots of the cost table at or past 4 * n_tiles are
never read.

Block order.  Which tiles reach file_blocks: EVERY tile of a frame that is filed, all four waves of it.  The call sits behind
the blend loop of blend_forward_kernel, outside every condition but `block_order != NULL`: a tile with an empty range skips the
loop (its blocks have kept = 0, hence hits = 0, class 0), a wave that leaves its tile early (all 64 pixels saturated) or whose
tile ends early (the last block saturated) breaks out of the loop and falls through to the call, and a block that lies wholly
outside a partial image has n_contrib 0 on every lane (class 0 again).  So a filed frame files exactly 8 * tiles ids, each once.
A frame is filed when the forward got block masks and a block_order, the image has at most 4096 tiles and the frame's backward
will run 8x4 blocks (gsr_bwd_block_px); otherwise the header is all zero (`filed` = 0) and the queues are not touched.
Block `blk` of a tile is the 8 x 4 pixel rectangle at column (blk % 2) * 8, row (blk // 2) * 4 of the tile -- the mapping the
backward decodes from the id tile * 8 + blk.
"""
import numpy as np

FO_MAX_TILES, FO_CLASSES = 4096, 64
BO_BANDS, BO_CLASSES, BO_SHARDS = 8, 32, 16
BO_QUEUES = BO_BANDS * BO_CLASSES * BO_SHARDS
BO_FLAG, BO_HEADER, BO_MAX_TILES = BO_QUEUES, BO_QUEUES + 4, 4096
TILE = 16


# ---- forward tile order ----
def wave_cost(v):
    v = np.asarray(v).astype(np.int64) & 0xFFFFFFFF
    return ((v >> 16) & 0x7FFF) + ((v & 0xFFFF) >> 1)


def fwd_classes(cost_table, n_tiles):
    """Class (0 = heaviest .. 63) of each of the first n_tiles tiles of a cost table of int32 [>= 4 * n_tiles]."""
    t = np.asarray(cost_table).reshape(-1)[:4 * n_tiles].reshape(n_tiles, 4)
    cost = wave_cost(t).max(axis=1)
    mx = max(1, int(cost.max()))
    scale = np.float32(63) / np.float32(mx)                       # float32, as the kernel: one division, one product per tile
    scaled = (cost.astype(np.float32) * scale).astype(np.int64)   # (int) truncates; the product is >= 0
    return (FO_CLASSES - 1 - np.minimum(FO_CLASSES - 1, scaled)).astype(np.int64)


def check_fwd_order(order, cost_table, n_tiles):
    """order: int32 [>= n_tiles] as read back; cost_table: what the table held when the order was made."""
    assert 0 < n_tiles <= FO_MAX_TILES
    o = np.asarray(order).reshape(-1)[:n_tiles].astype(np.int64)
    outside = o[(o < 0) | (o >= n_tiles)]
    assert outside.size == 0, f"forward order: {outside.size} entries are no tile of the image (first {outside[:4].tolist()} of {n_tiles} tiles)"
    seen = np.bincount(o, minlength=n_tiles)
    missing, twice = np.flatnonzero(seen == 0), np.flatnonzero(seen > 1)
    assert missing.size == 0, f"forward order: tile(s) {missing[:8].tolist()} never dispatched ({missing.size} missing, {twice.size} duplicated)"
    assert twice.size == 0, f"forward order: tile(s) {twice[:8].tolist()} dispatched more than once"
    cls = fwd_classes(cost_table, n_tiles)
    along = cls[o]
    drop = np.flatnonzero(np.diff(along) < 0)
    assert drop.size == 0, (f"forward order: class sequence decreases at slot {int(drop[0]) + 1} "
                            f"(class {int(along[drop[0]])} then {int(along[drop[0] + 1])}): a lighter class ran before a heavier one")
    # a non-decreasing sequence over a permutation holds every class's tiles in one run of the right length: the multisets agree
    want = np.bincount(cls, minlength=FO_CLASSES)
    got = np.bincount(along, minlength=FO_CLASSES)
    assert np.array_equal(want, got), "forward order: per-class tile counts differ from the statement's"
    for c in np.flatnonzero(want):
        a = int(want[:c].sum())
        assert np.array_equal(np.sort(o[a:a + want[c]]), np.flatnonzero(cls == c)), f"forward order: class {c} holds other tiles than the statement's"


# ---- block order ----
def bo_tiles_per_band(tiles):
    return (tiles + BO_BANDS - 1) // BO_BANDS


def bo_cap(tiles):
    return 8 * ((bo_tiles_per_band(tiles) + BO_SHARDS - 1) // BO_SHARDS)


def bo_ints(W, H):
    """gsr_block_order_ints: the header alone for images the forward never files."""
    tiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    return BO_HEADER if tiles > BO_MAX_TILES else BO_HEADER + BO_QUEUES * bo_cap(tiles)


def bo_class(hits):
    """gsr_bo_class: four classes per octave from 8 entries up, class 0 below 8, capped at 31."""
    hits = np.asarray(hits, dtype=np.int64)
    h = np.maximum(hits, 8)
    lg = np.floor(np.log2(h)).astype(np.int64)
    lg = np.where((1 << lg) > h, lg - 1, lg)                      # (log2 of an exact integer below 2^31 does not round across)
    lg = np.where((1 << (lg + 1)) <= h, lg + 1, lg)
    c = 1 + 4 * (lg - 3) + ((h >> (lg - 2)) & 3)
    return np.where(hits < 8, 0, np.minimum(c, BO_CLASSES - 1))


def block_queue(tile, cls, tiles):
    """Queue index (band, class, shard) of a tile's block of class `cls`."""
    tile = np.asarray(tile, dtype=np.int64)
    tpb = bo_tiles_per_band(tiles)
    band = tile // tpb
    return (band * BO_CLASSES + cls) * BO_SHARDS + ((tile - band * tpb) & (BO_SHARDS - 1))


def block_hits(ranges, n_contrib, masks, W, H):
    """(kept, hits), each int64 [tiles, 8]: per 8x4 block the largest n_contrib of its pixels inside the image, and how many of the
    tile's list entries [start, start + kept) carry the block's bit in their mask byte."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = gx * gy
    ranges = np.asarray(ranges).reshape(tiles, 2).astype(np.int64)
    masks = np.asarray(masks).reshape(-1).astype(np.uint8)
    nc = np.zeros((gy * TILE, gx * TILE), np.int64)
    nc[:H, :W] = np.asarray(n_contrib).reshape(H, W)
    # rows = (tile row, 4-row strip, row in strip), columns = (tile column, 8-pixel column, pixel): block = strip * 2 + column
    kept = nc.reshape(gy, 4, 4, gx, 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(tiles, 8)
    start, length = ranges[:, 0], ranges[:, 1] - ranges[:, 0]
    assert (kept <= np.maximum(length, 0)[:, None]).all(), "n_contrib exceeds its tile's list length"
    hits = np.zeros((tiles, 8), np.int64)
    for blk in range(8):
        cs = np.concatenate([[0], np.cumsum((masks >> blk) & 1, dtype=np.int64)])
        hits[:, blk] = cs[start + kept[:, blk]] - cs[start]
    return kept, hits


def expected_block_queues(ranges, n_contrib, masks, W, H):
    """What a filed frame's block order must hold: {"filed": 1, "queue": int64 [8 * tiles] queue index of id tile * 8 + blk}."""
    tiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    assert tiles <= BO_MAX_TILES
    _, hits = block_hits(ranges, n_contrib, masks, W, H)
    tile = np.repeat(np.arange(tiles, dtype=np.int64), 8)
    return {"filed": 1, "queue": block_queue(tile, bo_class(hits.reshape(-1)), tiles)}


def unfiled_block_queues():
    """A frame the forward does not file (more than 4096 tiles, 8x8 backward blocks): a cleared header, nothing else."""
    return {"filed": 0, "queue": np.zeros(0, np.int64)}


def _where(q):
    return f"(band {q // (BO_CLASSES * BO_SHARDS)}, class {q // BO_SHARDS % BO_CLASSES}, shard {q % BO_SHARDS})"


def check_block_order(order_ints, expected, tiles):
    """order_ints: the int32 block_order buffer as read back (gsr_block_order_ints elements)."""
    o = np.asarray(order_ints).reshape(-1).astype(np.int64)
    cap = bo_cap(tiles)
    assert o.size >= BO_HEADER
    assert int(o[BO_FLAG]) == expected["filed"], f"block order: `filed` word is {int(o[BO_FLAG])}, expected {expected['filed']}"
    counts = o[:BO_QUEUES]
    want_q = expected["queue"]
    want_counts = np.bincount(want_q, minlength=BO_QUEUES)
    over = np.flatnonzero(counts > cap)
    assert over.size == 0, f"block order: counter of queue {_where(int(over[0]))} is {int(counts[over[0]])}, above the capacity {cap}"
    assert (counts >= 0).all(), "block order: negative counter"
    if not expected["filed"]:
        assert not counts.any(), "block order: an unfiled frame has nonzero counters"
        return
    assert o.size >= BO_HEADER + BO_QUEUES * cap, "block order: buffer shorter than its queues"
    ids = o[BO_HEADER:BO_HEADER + BO_QUEUES * cap].reshape(BO_QUEUES, cap)
    live = np.arange(cap)[None, :] < counts[:, None]
    got_id, got_q = ids[live], np.repeat(np.arange(BO_QUEUES), counts)
    n_ids = 8 * tiles
    bad = got_id[(got_id < 0) | (got_id >= n_ids)]
    assert bad.size == 0, f"block order: filed id {int(bad[0])} is no block of the image ({n_ids} blocks)"
    seen = np.bincount(got_id, minlength=n_ids)
    twice, missing = np.flatnonzero(seen > 1), np.flatnonzero(seen == 0)
    assert twice.size == 0, f"block order: block {int(twice[0])} (tile {int(twice[0]) // 8}) is filed {int(seen[twice[0]])} times ({twice.size} such)"
    assert missing.size == 0, f"block order: block {int(missing[0])} (tile {int(missing[0]) // 8}) is not filed ({missing.size} such)"
    where = np.empty(n_ids, np.int64)
    where[got_id] = got_q
    wrong = np.flatnonzero(where != want_q)
    if wrong.size:
        b, g, w = int(wrong[0]), int(where[wrong[0]]), int(want_q[wrong[0]])
        part = "band" if g // (BO_CLASSES * BO_SHARDS) != w // (BO_CLASSES * BO_SHARDS) else "class" if g // BO_SHARDS != w // BO_SHARDS else "shard"
        raise AssertionError(f"block order: block {b} (tile {b // 8}, block {b % 8}) is filed under {_where(g)}, expected {_where(w)}: "
                             f"wrong {part} ({wrong.size} blocks misfiled)")
    assert np.array_equal(counts, want_counts), "block order: counters differ from the expected counts"
