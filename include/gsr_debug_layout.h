/*
 * gsr_debug_layout.h -- where the forward's tile-order tables lie inside the geom workspace (for tests and tools).
 *
 * gsr_forward_count keeps two tables at the tail of `geom_ws` (gsr.h, the hint at gsr_forward_count): what every wave of the
 * previous frame's forward blend cost, and the order in which this frame's blend dispatches its tiles, made from those costs.
 *     fwd_cost   int32 [4 * GSR_FWD_ORDER_MAX_TILES]   four per tile, one per wave: (life in ticks, 15 bits) << 16 | (staged, 16 bits)
 *     fwd_order  int32 [GSR_FWD_ORDER_MAX_TILES]       launch slot -> tile; the first (tiles of the image) entries are written
 * A caller never needs them: every output of the forward is the same whatever they hold.  A test that wants to SEE the order, or
 * to set the costs it is made from, asks here for the byte offsets of the two tables instead of restating the workspace's layout.
 *
 * Contract
 *   - Host arithmetic only: no HIP call, no allocation.  The offsets are those gsr_forward_count, gsr_forward_render and
 *     gsr_forward_capacity use for a workspace of N Gaussians; both tables lie inside gsr_geom_workspace_bytes(N), 256-byte aligned.
 *   - The tables are read and written only for images of at most GSR_FWD_ORDER_MAX_TILES tiles; larger images leave them alone.
 *   - Errors: GSR_E_NULL (an output pointer is null), GSR_E_DIMS (N < 0 or N > 2^31 - 1).
 *   - Nothing else changes: gsr.h, its structs, GSR_ABI_VERSION, workspace sizes and every existing entry point are as before.
 */
#ifndef GSR_DEBUG_LAYOUT_H
#define GSR_DEBUG_LAYOUT_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_FWD_ORDER_MAX_TILES 4096

int gsr_fwd_order_tables_offset(int64_t N, size_t *fwd_cost_offset, size_t *fwd_order_offset);

#ifdef __cplusplus
}
#endif

#endif /* GSR_DEBUG_LAYOUT_H */
