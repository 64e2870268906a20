/*
 * szg/multiscatter_sky.h — C-ABI of multiple scattering in the sky-view LUT and the aerial-perspective LUT: the consumer of
 * the multi-scattering LUT of szg/abi.h ("Multi-scattering LUT", szg_skyview_record_multiscatter_lut).
 *
 * The reference's sky is single scattering only: computeLuminanceScatteringIntegral (atmosphere/common.glinl:364-424) sums
 * the sunlight scattered once towards the eye. That is the model of the parity frame and of a new pipeline. With a MODE set
 * on a pipeline, the same 32-step loop also sums Hillaire's second and higher orders (Hillaire 2020, section 5.5), read from
 * the multi-scattering LUT the pipeline holds. Opt-in: SZG_MULTISCATTER_OFF, the mode of a new pipeline, launches exactly the
 * kernels that were launched before this header existed (k_skyview, k_aerial_lut) and every result is bit for bit what it was.
 *
 * THE RULE      in every step of the loop (marchLoop of syzygy_amd/csrc/szg_march.hpp), from values the step already has, each
 *               operation ONE IEEE binary32 operation rounded to nearest even, the division correctly rounded:
 *                 su  = clamp(0.5f + 0.5f * s_musun, 0, 1)
 *                       s_musun: the sun cosine of the step's sample, stepRadiusMu(origin, t).mu_sun (common.glinl:329-331, :389)
 *                 sv  = clamp(altitude / (atmosphereRadius - planetRadius), 0, 1)
 *                       altitude: that of `begin`, where the step samples the extinction (common.glinl:390-393)
 *                 Psi = the multi-scattering LUT at (su, sv) by the library's LINEAR / CLAMP_TO_EDGE LUT sampler:
 *                       u = su * 32 - 0.5, v = sv * 32 - 0.5, i0 = floor(u), j0 = floor(v), a = u - i0, b = v - j0, the four
 *                       indices clamped to the edge AFTER the weights are taken,
 *                       tap = w11 * t11 + (w01 * t01 + (w10 * t10 + w00 * t00)), w00 = (1 - a)(1 - b), w10 = a (1 - b),
 *                       w01 = (1 - a) b, w11 = a b (contraction classes SZG_C_TEXCOORD and SZG_C_BILINEAR, as every LUT tap)
 *                 ms  = fma3(((scatteringRayleigh + scatteringMie) * Psi) * integral, T_begin, ms)      per channel
 *                       (contraction class SZG_C_ACCUM; ms starts at +0)
 *               integral = (1 - T_path) / extinction and T_begin = transmittanceToBegin are the values the single-scattering
 *               term of the same step uses. clamp(x, 0, 1) = fminf(fmaxf(x, 0), 1): a NaN coordinate reads texel 0. Every
 *               product not named above is rounded by itself, whatever SZG_CONTRACT says.
 *               Texel (tx, ty) of the multi-scattering LUT lies at sun cosine 2 (tx + .5) / 32 - 1 and at altitude
 *               (ty + .5) / 32 of the shell, so (su, sv) are that LUT's normalised coordinates. Pairing `begin`'s altitude
 *               with the sample's sun cosine is what the single-scattering term of the step does.
 *
 *               The result of the integral is
 *                 SZG_MULTISCATTER_OFF    luminance                    (the reference's sum, from the operations it came from before)
 *                 SZG_MULTISCATTER_ADD    luminance + ms               (one binary32 addition per channel)
 *                 SZG_MULTISCATTER_ONLY   ms                           (diagnostic: the higher orders alone, for the texture viewer)
 *               `luminance` comes out of exactly the operations it comes out of in mode OFF, in all three bodies of the loop
 *               (generic, LEAN, LEAN + INNER), and the value of ms for a ray does not depend on which body its wave took:
 *               it reads only values that the three bodies form alike.
 *
 * WHERE         szg_skyview_record_skyview_lut, szg_skyview_record_skyview_lut_rows and szg_skyview_record_aerial_lut launch
 *               k_skyview_ms / k_aerial_lut_ms (syzygy_amd/csrc/kernels_lut_ms.hip) when the pipeline's mode is not OFF. These
 *               read the multi-scattering LUT the pipeline holds; if none has been recorded
 *               (szg_skyview_record_multiscatter_lut) or handed out (szg_skyview_multiscatter_lut) on this pipeline, the call
 *               is refused with SZG_ERR_INVALID_ARGUMENT and a text that names szg_skyview_record_multiscatter_lut.
 *               szg_skyview_record_draw_commands records transmittance, multi-scatter, sky-view and composite, in this
 *               order, when the mode is not OFF. The sky-view LUT's status dword ("some texel is not finite") is kept by
 *               k_skyview_ms as k_skyview keeps it. The aerial LUT's transmittance volume is the same in every mode.
 *
 * LUT REUSE     (szg/abi.h "LUT reuse across frames"): a change of mode marks the sky-view LUT as stale, and so does
 *               szg_skyview_multiscatter_lut while a mode is set, because it hands out writable texels like the other two
 *               accessors. szg_skyview_record_multiscatter_lut does not: its texels are a function of the atmosphere block
 *               and the transmittance LUT, which the reuse key covers. (The one exception follows from the same reasoning: the
 *               first such record after the texels were handed out replaces texels the caller may have written, which were a
 *               function of nothing the key knows, so with a mode set it marks the sky-view LUT as stale once.)
 *
 * OUT OF SCOPE  - The exact composite's inline marches stay single scattering: the aerial perspective on geometry pixels
 *                 and sampleGround. k_composite is held at 4 waves per SIMD without scratch by a test, and a third
 *                 accumulator there is a separate piece of work.
 *               - A frame that wants consistent higher orders on geometry uses the aerial LUT with
 *                 szg_skyview_record_composite_fast, which reads the new volume unchanged.
 *               - k_multiscatter, the oracle and every parity figure are unchanged.
 *
 * Additive: SZG_ABI_VERSION does not move; no struct changes.
 */
#ifndef SZG_MULTISCATTER_SKY_H
#define SZG_MULTISCATTER_SKY_H

#include "szg/abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SZG_MULTISCATTER_OFF 0u  /* single scattering only: the reference's model, the mode of a new pipeline */
#define SZG_MULTISCATTER_ADD 1u  /* single scattering + the higher orders */
#define SZG_MULTISCATTER_ONLY 2u /* the higher orders alone (diagnostic) */

/* Set / read the pipeline's mode. SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, the mode unchanged) for a NULL
 * pipeline, a NULL `mode` of the getter, or a mode above SZG_MULTISCATTER_ONLY. Takes effect with the next record call. */
int szg_skyview_set_multiscatter(szg_skyview_t* p, uint32_t mode);
int szg_skyview_get_multiscatter(const szg_skyview_t* p, uint32_t* mode);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_MULTISCATTER_SKY_H */
