// api_texture_display.cpp — the image copy and clear of the texture viewer behind the C-ABI (include/szg/texture_display.h):
// Image::recordCopyEntire / recordCopyRect (renderer/image.cpp:185-229) and recordClearColorImage (rendercommands.cpp:25).
// szg_ui_layer_add_texture_view, the header's third entry point, lives with the layer's textures in api_ui_layer.cpp.

#include "api_common.hpp"

using namespace szg;

static_assert(SZG_FORMAT_RGBA8_SRGB == 8, "szg/abi.h: the format values are part of the ABI");

namespace
{
// One image of the copy or the clear: present, not above the extent cap, rows inside the pitch, texels naturally aligned.
// The format is the caller's to check first. Everything here runs on the host, before anything is launched.
bool check_layout(const char* me, const szg_image* im, const char* name)
{
    if (im->width > SZG_PRESENT_MAX_EXTENT || im->height > SZG_PRESENT_MAX_EXTENT)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s image %ux%u exceeds %u texels", me, name, im->width, im->height, SZG_PRESENT_MAX_EXTENT);
        return false;
    }
    unsigned const tb = texel_bytes(im->format);
    if ((size_t)im->pitch_bytes < (size_t)im->width * tb || im->pitch_bytes % tb != 0u || reinterpret_cast<uintptr_t>(im->data) % tb != 0u)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s pitch %u / alignment invalid for %u texels of %u bytes", me, name, im->pitch_bytes, im->width,
             tb);
        return false;
    }
    return true;
}

bool check_copy_image(const szg_image* im, const szg_rect& r, bool isSource, const char* name)
{
    static const char* const me = "szg_record_copy_image";
    if (im == nullptr || im->data == nullptr)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s image or its data is NULL", me, name);
        return false;
    }
    bool const formatOk = isSource ? (im->format == SZG_FORMAT_RGBA8_UNORM || im->format == SZG_FORMAT_RGBA8_SRGB ||
                                      im->format == SZG_FORMAT_RGBA16_UNORM || im->format == SZG_FORMAT_RGBA16_SFLOAT)
                                   : im->format == SZG_FORMAT_RGBA16_SFLOAT;
    if (!formatOk)
    {
        fail(SZG_ERR_INVALID_ARGUMENT,
             isSource ? "%s: %s format %u, the source must be RGBA8_UNORM, RGBA8_SRGB, RGBA16_UNORM or RGBA16_SFLOAT"
                      : "%s: %s format %u, the destination must be RGBA16_SFLOAT",
             me, name, im->format);
        return false;
    }
    if (!check_layout(me, im, name))
    {
        return false;
    }
    if (r.x < 0 || r.y < 0 || (uint64_t)r.x + r.width > im->width || (uint64_t)r.y + r.height > im->height)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s region (%d, %d) %ux%u leaves the %ux%u image", me, name, r.x, r.y, r.width, r.height, im->width,
             im->height);
        return false;
    }
    return true;
}

// the bytes an image's texels occupy: [begin, end)
void image_range(const szg_image& im, uintptr_t& begin, uintptr_t& end)
{
    begin = reinterpret_cast<uintptr_t>(im.data);
    size_t const bytes = im.height == 0u ? 0u : (size_t)(im.height - 1u) * im.pitch_bytes + (size_t)im.width * texel_bytes(im.format);
    end = begin + bytes;
}
} // namespace

extern "C" {

int szg_record_copy_image(void* stream, const szg_image* src, const szg_image* dst, szg_rect src_region, szg_rect dst_region)
{
    if (!check_copy_image(src, src_region, true, "source") || !check_copy_image(dst, dst_region, false, "destination"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    uintptr_t sb, se, db, de;
    image_range(*src, sb, se);
    image_range(*dst, db, de);
    if (sb < de && db < se)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_copy_image: source and destination images overlap in memory");
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
    if (!check_layout(me, image, "the"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    SZG_HIP(szg::launch_image_clear(static_cast<hipStream_t>(stream), *image, color));
    return SZG_OK;
}

} // extern "C"
