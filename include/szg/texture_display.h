/*
 * szg/texture_display.h — C-ABI of the editor's Texture Viewer (editor/editor.cpp:485-505, :684-692; ui/texturedisplay.cpp):
 * the one GPU action of the reference's frame besides the passes of the other headers.
 *
 *   TextureDisplay::create      texturedisplay.cpp:23-145: a display image, R16G16B16A16_SFLOAT at TEXTURE_MAX = 4096^2
 *                               (editor.cpp:47, :487-494), cleared to opaque black by an immediate submit (:147-162) and
 *                               registered with ImGui through a NEAREST / CLAMP_TO_BORDER (opaque black) sampler and an image
 *                               view with components.a = VK_COMPONENT_SWIZZLE_ONE (:69-80, :104-120, :297-304).
 *   picking a texture           texturedisplay.cpp:164-195 -> Image::recordCopyEntire (renderer/image.cpp:191-206) ->
 *                               recordCopyImageToImage(cmd, src, dst, aspectMask, ...) (renderer/imageoperations.cpp:141-176):
 *                               vkCmdBlitImage2 with VK_FILTER_NEAREST of the whole asset image, R8G8B8A8_SRGB or
 *                               R8G8B8A8_UNORM (assets.cpp:706-715), onto the whole display image.
 *   picking "None"              recordClearColorImage (renderer/rendercommands.cpp:25) to opaque black.
 *   drawing                     ImGui::Image of the display image: a quad of the UI layer pass (szg/ui_layer.h).
 *
 * Three entry points: the copy, the clear, and a texture registration of the UI layer that takes a component mapping and
 * half-float images. With them any RGBA16_SFLOAT image of the frame (a G-buffer plane) and the scene colour can be put on
 * screen through the UI pass.
 *
 * Vulkan leaves the conversions of a blit to the implementation, so the copy has no bit-level reference ("parity unpinned",
 * like szg/present.h). The rules are stated completely so that the CPU model (tests/texture_display_model.py) and the kernels
 * (syzygy_amd/csrc/kernels_image_copy.hip, kernels_ui_layer.hip) agree bit for bit. Every floating-point operation named is
 * ONE IEEE binary32 operation, rounded to nearest even, never fused with its neighbour: these sites belong to none of the
 * classes of szg/contraction.h, so libszg_hip.so and libszg_hip_literal.so produce the same bytes.
 *
 * ---- szg_record_copy_image ----
 *
 * REGIONS     as szg/present.h: src_region inside the allocated source image, dst_region inside the allocated destination
 *             image, offsets honoured, no image wider or higher than SZG_PRESENT_MAX_EXTENT, no flips.
 *
 * COORDINATES the NEAREST rule of szg/present.h, per axis and in integers: destination index k in [0, n) of a region of n
 *             texels reads source texel s0 + floor((2k + 1) * sw / (2n)) of the region [s0, s0 + sw), clamped to the image
 *             (it cannot leave the region).
 *
 * LOAD        the source texel as four floats, by the source's format:
 *               SZG_FORMAT_RGBA8_UNORM    float(byte) / 255.0f
 *               SZG_FORMAT_RGBA8_SRGB     R, G, B: c = float(byte) / 255.0f, then c <= 0.04045f ? c / 12.92f :
 *                                         szg_powf((c + 0.055f) / 1.055f, 2.4f) (szg/fpmath.h): decode8(b, true) of the
 *                                         material sampler (szg/raster.h "textures") and of the mip builder (szg/mipmaps.h).
 *                                         Alpha: float(byte) / 255.0f.
 *               SZG_FORMAT_RGBA16_UNORM   float(code) / 65535.0f
 *               SZG_FORMAT_RGBA16_SFLOAT  the bits (see STORE)
 *
 * STORE       the destination is SZG_FORMAT_RGBA16_SFLOAT. Each channel is the fp32 value of LOAD rounded to binary16, to
 *             nearest even: the quotient is rounded to fp32 FIRST and that value to binary16 (two roundings; the kernels keep
 *             the compiler from folding the producing operation into the conversion). RGBA16_SFLOAT -> RGBA16_SFLOAT copies
 *             the 8 bytes of the texel unchanged, NaN payloads, denormals and signed zeros included.
 *
 * Everything outside dst_region keeps its bytes, pitch padding included. The source is never written.
 * HBM traffic: 8 B written per destination texel; the source is read once per destination texel and, magnified, from cache.
 *
 * ---- szg_record_clear_color_image ----
 *
 * CLEAR       every texel of the whole ALLOCATED extent width x height becomes `color`, never a byte of pitch padding.
 *               SZG_FORMAT_RGBA16_SFLOAT  STORE above: inf, NaN and values outside [0, 1] are kept as binary16 has them
 *               SZG_FORMAT_RGBA16_UNORM   the library's UNORM16 store: clamp to [0, 1] (NaN -> 0), * 65535, round to nearest
 *                                         even
 *
 * ---- szg_ui_layer_add_texture_view: two additions to the rules of szg/ui_layer.h ----
 *
 * SAMPLING    (addition) a texture may be SZG_FORMAT_RGBA16_SFLOAT. A binary16 channel is its value converted exactly to
 *             fp32: denormals are kept, inf and NaN stay as they are. Filtering and addressing are unchanged; FRAGMENT's clamp
 *             already turns NaN into 0.
 *
 * MAPPING     (new, between SAMPLING and FRAGMENT) the view's swizzle is applied to the FILTERED sample r, not to the taps:
 *             channel i of the texel FRAGMENT sees is r[i] (IDENTITY), 0.0f, 1.0f, r.r, r.g, r.b or r.a. Border taps
 *             (0, 0, 0, 1) go through the filter like any tap. The order is observable for ZERO and ONE under LINEAR: mapped
 *             taps would give 1 * (1 - alpha) + 1 * alpha. For every alpha in [0, 1) that is 1 in fp32 (the rounding error of
 *             1 - alpha is at most 2^-25 and the sum rounds back to 1), but a non-finite coordinate makes alpha = x - floor(x)
 *             a NaN, and the mapped taps would then give NaN, which FRAGMENT turns into 0, where the rule gives 1.
 *
 * Out of scope: the widget itself (list box, regex search, property table, file dialog); LINEAR copies; destinations other than
 * RGBA16_SFLOAT; sRGB textures sampled directly by the UI pass (copy them into a display image first, as the reference does);
 * row tiles (szg_rowtile) are not supported, as for szg/ui_layer.h.
 *
 * The step is additive: three symbols and one format value behind the old ones; SZG_ABI_VERSION does not move. Every entry
 * point of the other headers refuses SZG_FORMAT_RGBA8_SRGB as it refuses any format it does not name, and
 * szg_ui_layer_add_texture still refuses RGBA16_SFLOAT.
 */
#ifndef SZG_TEXTURE_DISPLAY_H
#define SZG_TEXTURE_DISPLAY_H

#include "szg/abi.h"
#include "szg/present.h"
#include "szg/ui_layer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VkComponentSwizzle */
#define SZG_SWIZZLE_IDENTITY 0u
#define SZG_SWIZZLE_ZERO 1u
#define SZG_SWIZZLE_ONE 2u
#define SZG_SWIZZLE_R 3u
#define SZG_SWIZZLE_G 4u
#define SZG_SWIZZLE_B 5u
#define SZG_SWIZZLE_A 6u

/* VkComponentMapping of an image view: swizzle[0..3] produce R, G, B, A */
typedef struct szg_ui_texture_view
{
    uint32_t swizzle[4]; /* SZG_SWIZZLE_* */
} szg_ui_texture_view;

/* The blit behind Image::recordCopyEntire / recordCopyRect. Enqueues the copy on `stream` and returns: asynchronous, no host
 * wait. SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, nothing launched, nothing written) for: a NULL image or data
 * pointer; a source format other than RGBA8_UNORM, RGBA8_SRGB, RGBA16_UNORM, RGBA16_SFLOAT or a destination format other than
 * RGBA16_SFLOAT; a region that leaves its image; a pitch smaller than a row or not a multiple of the texel size, or data not
 * aligned to the texel size; an image extent above SZG_PRESENT_MAX_EXTENT; source and destination images that overlap in
 * memory. A region without texels is a no-op that returns SZG_OK. */
int szg_record_copy_image(void* stream, const szg_image* src, const szg_image* dst, szg_rect src_region, szg_rect dst_region);

/* recordClearColorImage: CLEAR above on `stream`, asynchronous. SZG_ERR_INVALID_ARGUMENT as above for a NULL image, data or
 * colour pointer, a format other than RGBA16_SFLOAT or RGBA16_UNORM, a malformed pitch or alignment, an extent above
 * SZG_PRESENT_MAX_EXTENT. An image without texels is a no-op that returns SZG_OK. */
int szg_record_clear_color_image(void* stream, const szg_image* image, const float color[4]);

/* szg_ui_layer_add_texture with an image view: `image` may be RGBA8_UNORM, RGBA16_UNORM or RGBA16_SFLOAT, `view` maps its
 * components (NULL: identity). Returns an ordinary handle for szg_ui_draw_cmd::texture and szg_ui_layer_remove_texture; with
 * an identity view of an 8- or 16-bit UNORM image it draws the bytes of a szg_ui_layer_add_texture handle. Refused: what
 * szg_ui_layer_add_texture refuses, any other format, a swizzle value above SZG_SWIZZLE_A. */
int szg_ui_layer_add_texture_view(szg_ui_layer_t* layer, const szg_image* image, szg_ui_sampler sampler,
                                  const szg_ui_texture_view* view, szg_ui_texture_t** out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_TEXTURE_DISPLAY_H */
