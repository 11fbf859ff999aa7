/*
 * gsr_capacity.h -- capacity-mode forward of libgsr_hip.so: the whole forward enqueued without the host wait for D.
 *
 * The sized forward (gsr.h: gsr_forward_count, then gsr_forward_render) stops the host in the middle of every frame: the
 * count of (tile, Gaussian) pairs D has to be read back before the caller can size point_list, block_masks and the binning
 * workspace.  A caller that can bound D -- a trainer whose views come back every few hundred iterations, a viewer whose
 * camera moves smoothly -- passes a capacity K instead and buffers sized for K pairs.  The library then enqueues
 * preprocess, scan, depth sort, expansion, tile sort and blend back to back; nothing in the call waits on the device.
 *
 * Contract
 *   - binning->D holds the capacity K, 0 <= K <= GSR_MAX_RENDERED.  binning->point_list and block_masks hold K entries
 *     (block_masks rounded up to a multiple of 16 bytes, as in gsr.h), bin_ws holds gsr_binning_workspace_bytes(N, K, W, H)
 *     bytes, geom_ws gsr_geom_workspace_bytes(N).  The other buffers are those of gsr_forward_render.
 *   - The real D is left on the device, in geom->point_offsets[N-1] (N > 0; D = 0 for N = 0).  Every kernel that depends on D
 *     works on min(D, K) pairs, read on the device.  The caller reads D later (a non-blocking copy of that word and an event)
 *     and compares it with K.
 *   - Overflow is reported after the fact, not prevented.  If D > K the frame's outputs -- point_list, ranges, the image,
 *     n_contrib, final_T, block_masks -- are untrusted, and so is everything computed from them downstream (a backward, an
 *     optimizer step, a densification statistic).  Every write still stays inside the K-sized buffers.  Render the frame
 *     again with the sized path, or with a larger K.
 *   - For D <= K the outputs are those of the sized path, bit for bit: point_list[0 .. D), ranges, n_contrib, the image,
 *     the inverse depth, final_T, block_masks[0 .. D).  Entries D .. K of point_list and block_masks are undefined.
 *   - A frame with min(D, K) = 0 gives what gsr_forward_render gives for D = 0: zeros, not background (quirk Q10), and the
 *     accumulator clear of binning->backward_ws when one is handed over.
 *   - shape_hint: the last D the caller knows (0 if none).  The host still makes one choice from D, the backward's blend
 *     block shape (8x4 or 8x8 pixels), and with it whether this forward files the 8x4 blocks by cost; the hint stands in
 *     for D there.  A gsr_backward on a capacity-mode frame is called with binning->D = the same hint (at least 1 when
 *     K > 0: with 0 it skips the blend) and with point_list / block_masks of K entries.  Forward and backward then agree
 *     on the block shape; a hint far from the real D costs time, never correctness.
 *   - All four depth-sort passes are launched (the sized path launches as many as the last frame on geom_ws needed); the
 *     passes the frame's depth range does not need return at once on the device.
 *   - No readback slot is leased and the count gsr_forward_render checks (GSR_E_CAPACITY) is not touched: a geom_ws used
 *     here must be counted again by gsr_forward_count before the sized path renders from it.
 *   - The count is a 32-bit scan, as in the sized path: a frame whose true D reaches 2^31 is outside the contract.
 *
 * Errors, all checked before anything is enqueued: GSR_E_OVERFLOW (K or shape_hint < 0 or > GSR_MAX_RENDERED), GSR_E_NULL
 * (K > 0 and point_list NULL, or a required pointer of gsr_forward_render), GSR_E_ALIGN (any array or workspace pointer
 * not 16-byte aligned), GSR_E_WORKSPACE (geom_ws or bin_ws missing or too small), GSR_E_DIMS (as gsr_forward_count).
 */
#ifndef GSR_CAPACITY_H
#define GSR_CAPACITY_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_forward_capacity(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                         const GsrImage *image, void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes,
                         int64_t shape_hint, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_CAPACITY_H */
