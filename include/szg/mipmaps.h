/*
 * szg/mipmaps.h — C-ABI of mip-mapped material textures: a chain builder that runs when an asset is loaded, and the
 * trilinear sampler of the G-buffer raster pass (szg/raster.h "textures" describes the default, one level).
 *
 * The reference's material sampler is ALREADY trilinear: VK_SAMPLER_MIPMAP_MODE_LINEAR, mipLodBias 0, no anisotropy,
 * minLod 0, maxLod 1.0 (renderer/vulkanstructs.cpp:147-183, used at renderer/material.cpp:115-120). Only its images have
 * one level (renderer/image.cpp:86), so the mip mode never shows. This header is "what that sampler does once an image has
 * levels": SZG_SAMPLER_MAX_LOD_REFERENCE reproduces its maxLod (a quirk: levels above 1 are never read),
 * SZG_SAMPLER_MAX_LOD_NONE lifts it.
 *
 * Vulkan leaves the LOD computation and the filter's precision to the implementation ("parity unpinned", like
 * szg/raster.h). The rules below are Vulkan's "texel filtering" pinned to exact operations, so that the CPU model
 * (tests/mipmap_model.py) and the kernels agree bit for bit. Every floating-point operation named is ONE IEEE binary32
 * operation, rounded to nearest even, never fused with its neighbour.
 *
 * CHAIN LAYOUT  Level 0 is the image itself (szg_texture: any pitch). Level k >= 1 has
 *               w_k = max(1, W >> k), h_k = max(1, H >> k), RGBA8, pitch w_k * 4. Levels 1, 2, ... lie back to back in one
 *               device allocation of szg_mip_chain_bytes(W, H) bytes; a full chain has
 *               szg_mip_level_count(W, H) = floor(log2(max(W, H))) + 1 levels, the last one 1 x 1.
 *
 * GENERATION    szg_record_generate_mipmaps, one kernel launch per level (k_mip_downsample, kernels_mipmaps.hip). Each
 *               level is made from the STORED 8-bit texels of the level before it. Texel (x, y) of level k averages the
 *               2 x 2 texels of columns min(2x, w - 1), min(2x + 1, w - 1) and rows min(2y, h - 1), min(2y + 1, h - 1) of
 *               level k - 1 (w, h its size): a box filter. Where a size is odd its last column or row is dropped
 *               (w_k = w >> 1 never reaches it); where a size is 1 the single column or row is used twice. Polyphase
 *               filters for odd sizes are out of scope. With t00, t10 the texels of the upper row and t01, t11 of the
 *               lower one:
 *                 srgb == 0   every channel, alpha included: (t00 + t10 + t01 + t11 + 2) >> 2 in integers
 *                 srgb == 1   R, G, B: each code decoded as the sampler decodes it (c = float(code) / 255.0f;
 *                             c <= 0.04045f ? c / 12.92f : szg_powf((c + 0.055f) / 1.055f, 2.4f)), summed as
 *                             l = ((t00 + t10) + (t01 + t11)) * 0.25f, encoded with the expression of szg_record_oetf's
 *                             SZG_OETF_SRGB (e = l <= 0.0031308f ? 12.92f * l
 *                             : szg_powf(l, (float)(1.0 / 2.4)) * 1.055f - 0.055f), and stored as
 *                             (int)floorf(e * 255.0f + 0.5f) clamped to 0..255. Alpha takes the integer rule.
 *               A uniform texture keeps its code at every level under both rules.
 *
 * SAMPLER       in k_raster_tile, for each of the three maps of a surface whose level-0 pointer is registered with
 *               L = level_count levels (szg_deferred_set_texture_mips), with the fine quad derivatives dUvDx, dUvDy of
 *               szg/raster.h "derivatives" and W x H the size of level 0:
 *                 mux = dUvDx.x * W;  mvx = dUvDx.y * H;  muy = dUvDy.x * W;  mvy = dUvDy.y * H
 *                 r2  = fmaxf(mux * mux + mvx * mvx, muy * muy + mvy * mvy)       (products first, then the sum)
 *                 lam = !(r2 > 0) ? 0 : 0.5f * (szg_logf(r2) * 1.44269504f)       (NaN and 0 -> level 0; +inf -> clamped)
 *                 lam = fminf(fmaxf(lam, 0), fminf(max_lod, (float)(L - 1)))
 *                 d   = (int)floorf(lam);  f = lam - (float)d
 *                 f == 0 :  result = bilinear(level d)                             (exactly; level d + 1 is not fetched)
 *                 else   :  result = (1.0f - f) * bilinear(level d) + f * bilinear(level d + 1)      per channel
 *               bilinear(level k) is the one-level rule of szg/raster.h "textures" with w_k, h_k. No LOD bias, no
 *               anisotropy (vulkanstructs.cpp:147-183). A magnified pixel (lam == 0), a texture without a table entry
 *               and an entry with level_count == 1 give the one-level value bit for bit. A pipeline without a table
 *               launches the kernel it launched before this header existed. (Anisotropy is opt-in sampler state of its own:
 *               szg/anisotropy.h; at its default this rule is all there is.)
 *
 * The table is keyed by the level-0 DEVICE POINTER, which plays the role the image handle plays in Vulkan: width, height
 * and srgb still come from the surface's szg_texture. The shadow raster reads no texture and is untouched.
 *
 * Additive: SZG_ABI_VERSION does not move; szg_texture, szg_material, szg_surface and szg_mesh_instanced keep their
 * size and layout.
 */
#ifndef SZG_MIPMAPS_H
#define SZG_MIPMAPS_H

#include <stddef.h>

#include "szg/raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference sampler's maxLod (renderer/vulkanstructs.cpp:147-183: minLod 0, maxLod 1.0, mipLodBias 0). */
#define SZG_SAMPLER_MAX_LOD_REFERENCE 1.0f
/* Vulkan's VK_LOD_CLAMP_NONE: every registered level is reachable. */
#define SZG_SAMPLER_MAX_LOD_NONE 1000.0f

/* floor(log2(max(w, h))) + 1; 0 if w or h is 0 */
uint32_t szg_mip_level_count(uint32_t w, uint32_t h);
/* bytes of levels 1 .. L-1 of a full chain, packed (CHAIN LAYOUT); 0 for a 1 x 1 image or an empty one */
size_t szg_mip_chain_bytes(uint32_t w, uint32_t h);

/* Enqueue the generation of the full chain of `level0` (DEVICE memory) into `d_chain` on `stream` and return.
 * SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, nothing launched, nothing written) for: a NULL level0 or
 * level0->data; a width or height of 0 or above 32768; a pitch smaller than a row or not a multiple of 4; a level0->data
 * or d_chain that is not aligned to 4 bytes (texels are read and written as dwords);
 * chain_bytes < szg_mip_chain_bytes(width, height); a NULL d_chain when the chain has bytes. A 1 x 1 image is a no-op
 * that returns SZG_OK. */
int szg_record_generate_mipmaps(void* stream, const szg_texture* level0, void* d_chain, size_t chain_bytes);

typedef struct szg_texture_mips
{
    const void* level0_data; /* == szg_texture.data of the image these belong to */
    const void* d_chain;     /* levels 1..level_count-1, packed as above (may be NULL when level_count == 1) */
    uint32_t level_count;    /* 1..szg_mip_level_count(w, h); 1 = no extra level */
} szg_texture_mips;

/* Replace the pipeline's table by a copy of `entries`; count == 0 clears it. `max_lod` is the sampler's maxLod for every
 * entry. SZG_ERR_INVALID_ARGUMENT (table unchanged) for: a NULL pipeline; NULL `entries` with count > 0; an entry with a
 * NULL level0_data, with level_count == 0, with level_count > 1 and a NULL d_chain, or with a level0_data or d_chain that is
 * not aligned to 4 bytes; two entries with the same
 * level0_data; max_lod negative or NaN. szg_deferred_record_gbuffer_raster (and _draw_commands_meshes) then refuses a
 * surface whose texture has an entry with level_count above szg_mip_level_count of that texture's size. */
int szg_deferred_set_texture_mips(szg_deferred_t* p, const szg_texture_mips* entries, uint32_t count, float max_lod);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_MIPMAPS_H */
