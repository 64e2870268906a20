/*
 * szg/present.h — C-ABI of the present pass: the blit that ends the reference's frame. Editor::endFrame
 * (editor/editor.cpp:263-360) encodes the scene texture in place (:303-340, szg_record_oetf) and then copies
 * `sourceSubregion` of it onto the whole swapchain image (:355-361) with
 *
 *   recordCopyImageToImage(cmd, src, dst, VkRect2D srcSize, VkRect2D dstSize)   renderer/imageoperations.cpp:87-119
 *     -> vkCmdBlitImage2, VK_FILTER_LINEAR (:45-85): scales the source rectangle onto the destination rectangle and
 *        converts RGBA16_UNORM to the swapchain's format, one of A2B10G10R10_UNORM_PACK32, R8G8B8A8_UNORM,
 *        B8G8R8A8_UNORM (editor/swapchain.cpp:99-103)
 *   recordCopyImageToImage(cmd, src, dst, aspectMask, ...)                       imageoperations.cpp:141-176
 *     -> the same blit with VK_FILTER_NEAREST, behind Image::recordCopyEntire / recordCopyRect
 *        (renderer/image.cpp:185-229)
 *
 * rebuilt as HIP kernels (syzygy_amd/csrc/kernels_present.hip). This is the one entry point that HONOURS the offset
 * of a szg_rect: every record_* pass refuses a non-zero offset (szg/abi.h, szg_rect), because the reference's passes
 * ignore it; the reference's blit does not.
 *
 * Vulkan fixes a blit's coordinate mapping and leaves the filter's precision and the conversion's rounding to the
 * implementation, so this pass has no bit-level reference ("parity unpinned", like szg/raster.h and szg/debuglines.h).
 * The rule below is stated completely so that the CPU model (tests/present_model.py) and the kernels agree bit for
 * bit. Every floating-point operation named is ONE IEEE binary32 operation, rounded to nearest even, never fused
 * with its neighbour: this site belongs to none of the classes of szg/contraction.h, so libszg_hip.so and
 * libszg_hip_literal.so produce the same bytes.
 *
 * REGIONS     src_region lies inside the allocated source image, dst_region inside the allocated destination image;
 *             offsets are honoured. Neither image may be wider or higher than SZG_PRESENT_MAX_EXTENT (keeps the
 *             integers below inside int32). A szg_rect has no negative extent: no flips.
 *
 * COORDINATES per axis, independently. Destination index k in [0, n) of a region of n texels, mapped onto the source
 *             texels [s0, s0 + sw): Vulkan's u = (k + 0.5) * sw / n + s0, evaluated in integers (an fp32 u moves
 *             5e-3 of the channels of a 1000x700 -> 1337x911 blit by one code):
 *               num   = (2k + 1) * sw + (2 * s0 - 1) * n          (= (u - 0.5) * 2n, negative for k = 0, s0 = 0)
 *               den   = 2n
 *               i0    = floor(num / den)                          (towards minus infinity)
 *               alpha = float(num - i0 * den) / float(den)        (both operands exact, one rounding)
 *             The taps are i0 and i0 + 1, EACH CLAMPED TO [0, image extent - 1]: to the IMAGE, not to the region.
 *             That is Vulkan's blit rule (CLAMP_TO_EDGE addressing of the whole image), kept on purpose: a scaled blit
 *             of a subregion reads the one row / column of texels next to the region where the image has them.
 *
 * LINEAR      texel channel t = float(code) / 65535.0f, as every UNORM16 load of this library. With alpha from x,
 *             beta from y, t00/t10 the taps of row j0 at columns i0/i1, t01/t11 those of row j1:
 *               top = t00 * (1 - alpha) + t10 * alpha
 *               bot = t01 * (1 - alpha) + t11 * alpha
 *               r   = top * (1 - beta) + bot * beta
 *             (1 - alpha), each product and each sum a separately rounded operation.
 *
 * NEAREST     the texel s0 + floor((2k + 1) * sw / (2n)) per axis (clamped to the image; it cannot leave the region),
 *             r = t.
 *
 * STORE       for a channel of b bits: clamp r to [0, 1], multiply by 2^b - 1, round to nearest even: what the
 *             library's UNORM16 store does for b = 16. Alpha takes the same filter and the same conversion.
 *               SZG_FORMAT_RGBA8_UNORM         4 B/texel, bytes R, G, B, A
 *               SZG_FORMAT_BGRA8_UNORM         4 B/texel, bytes B, G, R, A
 *               SZG_FORMAT_A2B10G10R10_UNORM   one little-endian dword: R bits 0-9, G 10-19, B 20-29, A 30-31
 *             The source is SZG_FORMAT_RGBA16_UNORM.
 *
 * ENCODE      SZG_PRESENT_ENCODE_NONE, or a transfer function of szg_record_oetf (SZG_OETF_PURE_GAMMA, SZG_OETF_SRGB)
 *             applied to R, G, B of every TAP before the filter, each tap quantised to UNORM16 exactly as the in-place
 *             pass stores it (the same 65 536-entry table). The result is bit-identical to szg_record_oetf over the
 *             whole source image followed by a plain present, and the source keeps its linear values.
 *
 * 1:1         when both regions have the same extent every alpha and beta is 0 and r = t00: a conversion without a
 *             filter. The kernels take a shorter path there; its bytes are the rule's.
 *
 * Everything outside dst_region, pitch padding included, keeps its bytes. The source is never written.
 * HBM traffic at 1:1: 8 B read + 4 B written per texel.
 */
#ifndef SZG_PRESENT_H
#define SZG_PRESENT_H

#include "szg/abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SZG_PRESENT_MAX_EXTENT 16384u

/* VkFilter: VK_FILTER_NEAREST = 0, VK_FILTER_LINEAR = 1 */
#define SZG_FILTER_NEAREST 0u
#define SZG_FILTER_LINEAR 1u

/* `encode`: one of SZG_OETF_PURE_GAMMA / SZG_OETF_SRGB (szg/abi.h), or no encoding */
#define SZG_PRESENT_ENCODE_NONE 0xFFFFFFFFu

typedef struct szg_present_info
{
    szg_rect src_region; /* editor.cpp:355-361 sourceSubregion */
    szg_rect dst_region; /* editor.cpp:360 VkRect2D{.extent = swapchain.extent()} */
    uint32_t filter;     /* SZG_FILTER_* */
    uint32_t encode;     /* SZG_PRESENT_ENCODE_NONE or SZG_OETF_* */
} szg_present_info;

/* Enqueue the blit on `stream` and return. SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, nothing launched,
 * nothing written) for: a NULL image, info or data pointer; a source format other than RGBA16_UNORM or a destination
 * format other than the three above; a region that leaves its image; a pitch smaller than a row or not a multiple of
 * the texel size, or data not aligned to the texel size; an image extent above SZG_PRESENT_MAX_EXTENT; an unknown
 * filter or encode; source and destination images that overlap in memory. A region without texels is a no-op that
 * returns SZG_OK. */
int szg_record_present(void* stream, const szg_image* src, const szg_image* dst, const szg_present_info* info);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_PRESENT_H */
