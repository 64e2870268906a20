// api_texture_display.cpp — the image copy and clear of the texture viewer behind the C-ABI (include/szg/texture_display.h):
// Image::recordCopyEntire / recordCopyRect (renderer/image.cpp:185-229) and recordClearColorImage (rendercommands.cpp:25).
// szg_ui_layer_add_texture_view, the header's third entry point, lives with the layer's textures in api_ui_layer.cpp.

#include "api_common.hpp"

using namespace szg;

static_assert(SZG_FORMAT_RGBA8_SRGB == 8, "szg/abi.h: the format values are part of the ABI");

extern "C" {

int szg_record_copy_image(void* stream, const szg_image* src, const szg_image* dst, szg_rect src_region, szg_rect dst_region)
{
    static const char* const me = "szg_record_copy_image";
    if (!check_pass_image(me, "source", src, {SZG_FORMAT_RGBA8_UNORM, SZG_FORMAT_RGBA8_SRGB, SZG_FORMAT_RGBA16_UNORM, SZG_FORMAT_RGBA16_SFLOAT},
                          "the source must be RGBA8_UNORM, RGBA8_SRGB, RGBA16_UNORM or RGBA16_SFLOAT", &src_region) ||
        !check_pass_image(me, "destination", dst, {SZG_FORMAT_RGBA16_SFLOAT}, "the destination must be RGBA16_SFLOAT", &dst_region))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (images_overlap(*src, *dst))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: source and destination images overlap in memory", me);
    }
    if (src_region.width == 0u || src_region.height == 0u || dst_region.width == 0u || dst_region.height == 0u)
    {
        return SZG_OK; // nothing to read or nothing to cover
    }
    SZG_HIP(szg::launch_image_copy(static_cast<hipStream_t>(stream), *src, *dst, src_region, dst_region));
    return SZG_OK;
}

int szg_record_clear_color_image(void* stream, const szg_image* image, const float color[4])
{
    static const char* const me = "szg_record_clear_color_image";
    if (image == nullptr || image->data == nullptr || color == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: image, its data or the colour is NULL", me);
    }
    if (image->format != SZG_FORMAT_RGBA16_SFLOAT && image->format != SZG_FORMAT_RGBA16_UNORM)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: image format %u, must be RGBA16_SFLOAT or RGBA16_UNORM", me, image->format);
    }
    // the NULL and format refusals above have this call's own wording; what is left here is the extent cap and the layout
    if (!check_pass_image(me, "the", image, {SZG_FORMAT_RGBA16_SFLOAT, SZG_FORMAT_RGBA16_UNORM}, "", nullptr))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    SZG_HIP(szg::launch_image_clear(static_cast<hipStream_t>(stream), *image, color));
    return SZG_OK;
}

} // extern "C"
