/*
 * szg/anisotropy.h — C-ABI of anisotropic filtering for the material sampler of the G-buffer raster pass: one more piece of
 * sampler state beside max_lod (szg/mipmaps.h "SAMPLER").
 *
 * The reference's sampler has the switch and leaves it off: anisotropyEnable = VK_FALSE, maxAnisotropy = 1.0F
 * (renderer/vulkanstructs.cpp:171-172). szg/mipmaps.h is "what that sampler does once an image has levels"; this header is
 * what it does once maxAnisotropy is above 1. SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE, the value of a new pipeline, reproduces
 * the reference: every frame is then bit for bit what it is without this header, from the kernels it was made by before.
 *
 * Why: the trilinear rule picks its level from the LONGER axis of the pixel's footprint alone. On a floor or a wall seen at a
 * grazing angle the footprint is long in one screen direction and short in the other, and the level that is right for the
 * long axis is several levels too coarse for the short one. The anisotropic rule picks the level from the longer axis
 * divided by the (clamped) ratio of the two, and covers the long axis with up to 16 trilinear taps along it.
 *
 * The rule is Vulkan's anisotropic "scale factor and level-of-detail operation" with the tap placement of
 * VK_EXT / GL_EXT_texture_filter_anisotropic, which the specification leaves to the implementation like the rest of the
 * filter. It is pinned here to exact operations, so that the CPU model (tests/aniso_model.py) and the kernel agree bit for
 * bit. Every floating-point operation named is ONE IEEE binary32 operation, rounded to nearest even, never fused with its
 * neighbour; division and sqrtf are correctly rounded; szg_logf is szg/fpmath.h.
 *
 * SAMPLER       in k_raster_tile_aniso, for each of the three maps of a surface whose level-0 pointer is registered with
 *               L = level_count > 1 levels (szg_deferred_set_texture_mips), with mux, mvx, muy, mvy, max_lod and
 *               bilinear(level k, st) as in szg/mipmaps.h "SAMPLER", st the interpolated uv of the pixel, dUvDx, dUvDy the
 *               fine quad derivatives of szg/raster.h "derivatives" and A = max_anisotropy:
 *                 px2 = mux * mux + mvx * mvx;  py2 = muy * muy + mvy * mvy      (products first, then the sum)
 *                 r2  = fmaxf(px2, py2);        s2  = fminf(px2, py2)            (a NaN operand is dropped, as in mipmaps.h)
 *                 if (A == 1 || !(r2 > 0) || r2 == +inf)   -> the SAMPLER rule of mipmaps.h, unchanged
 *                 eta = fminf(sqrtf(r2 / s2), A)          (s2 == 0 and an overflowing quotient give +inf -> A; 1 <= eta <= A)
 *                 N   = (int)ceilf(eta)                                          (1 .. 16)
 *                 if (N == 1)                              -> the SAMPLER rule of mipmaps.h, unchanged
 *                 lam = 0.5f * (szg_logf(r2) * 1.44269504f) - szg_logf(eta) * 1.44269504f
 *                 lam = fminf(fmaxf(lam, 0), fminf(max_lod, (float)(L - 1)));   d = (int)floorf(lam);   f = lam - (float)d
 *                 major = (px2 >= py2) ? dUvDx : dUvDy                           (a tie goes to x)
 *                 for i = 1 .. N:
 *                   t_i   = (float)i / (float)(N + 1) - 0.5f
 *                   st_i  = (st.x + t_i * major.x,  st.y + t_i * major.y)        (product, then sum)
 *                   tap_i = f == 0 ? bilinear(level d, st_i)                     (exactly; level d + 1 is not fetched)
 *                                  : (1.0f - f) * bilinear(level d, st_i) + f * bilinear(level d + 1, st_i)
 *                 result = (((tap_1 + tap_2) + tap_3) + ... + tap_N) / (float)N  per channel: the sum starts from tap_1,
 *                                                                                 one division at the end
 *               The N taps divide the major axis of the footprint, centred on st, into N + 1 equal parts and sit on the
 *               inner division points. Every tap has weight 1 / N. The levels d and d + 1 are the same for every tap.
 *
 *               "Unchanged" means bit for bit: a pipeline at A == 1, an isotropic or nearly isotropic footprint (eta == 1),
 *               a footprint that is NaN (both axes), zero or infinite, a map without a table entry and an entry with
 *               level_count == 1 give exactly the value they gave before this header existed. A map WITHOUT a table
 *               entry with level_count > 1 keeps the one-level rule of szg/raster.h "textures" whatever A is: anisotropy
 *               for maps without a chain is out of scope. A pipeline that never calls szg_deferred_set_sampler_anisotropy
 *               with a value above 1, and a record call none of whose draws carries a chain, launch exactly the kernels
 *               they launched before (k_raster_tile<false>, k_raster_tile<true>).
 *
 *               An axis with a NaN (px2 or py2 NaN, the other finite and positive) gives r2 == s2, eta == 1: the SAMPLER
 *               rule of mipmaps.h. An infinite footprint is not spread over taps: 0 * inf would put NaN into st_i.
 *
 * The value is sampler state of the PIPELINE, like max_lod: it applies to every map of every draw that has a table entry
 * with level_count > 1, and it survives szg_deferred_set_texture_mips. The shadow raster reads no texture and is untouched.
 *
 * Additive: SZG_ABI_VERSION does not move; every struct of szg/raster.h and szg/mipmaps.h keeps its size and layout.
 */
#ifndef SZG_ANISOTROPY_H
#define SZG_ANISOTROPY_H

#include "szg/mipmaps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference sampler's maxAnisotropy (renderer/vulkanstructs.cpp:171-172: anisotropyEnable VK_FALSE, maxAnisotropy 1.0F). */
#define SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE 1.0f   /* vulkanstructs.cpp:171-172 */
/* The largest ratio the sampler spreads over taps (VkPhysicalDeviceLimits::maxSamplerAnisotropy of current hardware). */
#define SZG_SAMPLER_MAX_ANISOTROPY_LIMIT 16.0f

/* Set the sampler's maxAnisotropy; a new pipeline has SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE. SZG_ERR_INVALID_ARGUMENT (with a
 * szg_last_error() text, the pipeline's value unchanged) for: a NaN; a value below 1; a value above
 * SZG_SAMPLER_MAX_ANISOTROPY_LIMIT; a NULL pipeline. Takes effect with the next szg_deferred_record_gbuffer_raster (and
 * _draw_commands_meshes). */
int szg_deferred_set_sampler_anisotropy(szg_deferred_t* p, float max_anisotropy);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_ANISOTROPY_H */
