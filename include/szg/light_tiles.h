/*
 * szg/light_tiles.h — C-ABI of the lights pass's per-tile light masks (a debug view; the pass needs no call from here).
 *
 * szg_deferred_record_lights with at least one spot light runs k_light_tiles in front of k_lights: per 64 x 64-pixel tile of
 * the LOCAL image (the rows of this rank's row tile) the G-buffer positions are reduced to an axis-aligned box, every light
 * record is tested against the box, and one 64-bit word per tile and per 64 records says which lights k_lights has to visit
 * there (bit i of word b: record 64 b + i; records run directional lights [skip, count), then the spot lights). A bit is
 * clear only where the per-pixel early-out of the light loop would fire for every position of the box
 * (syzygy_amd/csrc/szg_light_tiles.hpp). The storage belongs to the pipeline and is sized at creation.
 */
#ifndef SZG_LIGHT_TILES_H
#define SZG_LIGHT_TILES_H

#include "szg/abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The words the last szg_deferred_record_lights call with spot lights wrote: *out_tiles_x x *out_tiles_y tiles, row-major,
 * *out_batches words each (all three 0 when there was no such call yet). When out_words is not NULL the words are copied to
 * host memory behind the work recorded on `stream`, and the call waits for the copy; capacity_words is the room at
 * out_words (SZG_ERR_CAPACITY when it is too small).
 * The storage holds one pass's words at a time, and the geometry reported is that of the last call with spot lights: call
 * this right behind that szg_deferred_record_lights, on the SAME stream, before any other lights pass of the pipeline is
 * recorded (a later pass with spot lights overwrites the words; one recorded on another stream may do so while they are
 * copied). A later pass without spot lights leaves words and geometry as they were. */
int szg_deferred_debug_light_tile_masks(szg_deferred_t* p, void* stream, uint64_t* out_words, uint64_t capacity_words,
                                        uint32_t* out_tiles_x, uint32_t* out_tiles_y, uint32_t* out_batches);

#ifdef __cplusplus
}
#endif

#endif
