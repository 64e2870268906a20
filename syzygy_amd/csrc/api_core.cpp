// api_core.cpp — the part of the extern "C" boundary (include/szg/abi.h) that belongs to no pipeline: version and build
// id, the calling thread's error text, the argument checks the other api_*.cpp units share (api_common.hpp), and the
// row-tile arithmetic with its composer.
//
// The api_*.cpp units together are the host-side mirror of renderer/pipelines/skyview.cpp:713-965 and
// renderer/pipelines/deferred.cpp:145-337, :435-792 with Vulkan, VMA and
// descriptor plumbing replaced by HIP device pointers and one stream. Every
// record_* call validates shapes on the host, enqueues, and returns; in-stream
// order replaces the reference's full barriers (imageoperations.cpp:18-33).

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "api_common.hpp"
#ifdef SZG_LITERAL
#define SZG_CONTRACT SZG_CONTRACT_NONE
#endif
#include "szg/contraction.h"

namespace
{
thread_local char g_error[512] = "";
}

namespace szg
{
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    fprintf(stderr, "[szg] error: %s\n", g_error);
    return code;
}
int fail_hip(hipError_t e, const char* what)
{
    return fail(e == hipErrorOutOfMemory ? SZG_ERR_OUT_OF_MEMORY : SZG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
void set_last_error(const char* message)
{
    snprintf(g_error, sizeof g_error, "%s", message != nullptr ? message : "");
    fprintf(stderr, "[szg] error: %s\n", g_error);
}

unsigned texel_bytes(unsigned fmt)
{
    switch (fmt)
    {
    case SZG_FORMAT_RGBA16_SFLOAT:
    case SZG_FORMAT_RGBA16_UNORM:
        return 8;
    case SZG_FORMAT_RGBA32_SFLOAT:
        return 16;
    case SZG_FORMAT_D32_SFLOAT:
    case SZG_FORMAT_RGBA8_UNORM:
    case SZG_FORMAT_BGRA8_UNORM:
    case SZG_FORMAT_A2B10G10R10_UNORM:
    case SZG_FORMAT_RGBA8_SRGB:
        return 4;
    default:
        return 0;
    }
}

bool rows_aligned(const void* data, unsigned pitch_bytes, unsigned bytes)
{
    return pitch_bytes % bytes == 0u && reinterpret_cast<uintptr_t>(data) % bytes == 0u;
}
bool layout_ok(const void* data, unsigned width, unsigned pitch_bytes, unsigned texel)
{
    return (size_t)pitch_bytes >= (size_t)width * texel && rows_aligned(data, pitch_bytes, texel);
}
bool image_layout_ok(const szg_image& im) { return layout_ok(im.data, im.width, im.pitch_bytes, texel_bytes(im.format)); }
bool extents_ok(const szg_image& im, unsigned min)
{
    return im.width >= min && im.height >= min && im.width <= SZG_PRESENT_MAX_EXTENT && im.height <= SZG_PRESENT_MAX_EXTENT;
}
bool rect_inside(const szg_rect& r, const szg_image& im)
{
    return r.x >= 0 && r.y >= 0 && (uint64_t)r.x + r.width <= im.width && (uint64_t)r.y + r.height <= im.height;
}
// the bytes an image's texels occupy: [begin, end)
static void image_range(const szg_image& im, uintptr_t& begin, uintptr_t& end)
{
    begin = reinterpret_cast<uintptr_t>(im.data);
    end = begin + (im.height == 0u ? 0u : (size_t)(im.height - 1u) * im.pitch_bytes + (size_t)im.width * texel_bytes(im.format));
}
bool images_overlap(const szg_image& a, const szg_image& b)
{
    uintptr_t ab, ae, bb, be;
    image_range(a, ab, ae);
    image_range(b, bb, be);
    return ab < be && bb < ae;
}

bool check_image(const szg_image& im, unsigned fmt, unsigned w, unsigned h, const char* name)
{
    unsigned const tb = texel_bytes(fmt);
    if (im.data == nullptr)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: data is NULL", name);
        return false;
    }
    if (im.format != fmt)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: format %u, expected %u", name, im.format, fmt);
        return false;
    }
    if (im.width < w || im.height < h)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %ux%u smaller than the required %ux%u", name, im.width, im.height, w, h);
        return false;
    }
    if (!image_layout_ok(im))
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: pitch %u / alignment invalid for %u-byte texels", name, im.pitch_bytes, tb);
        return false;
    }
    return true;
}

bool check_image_format(const char* me, const char* name, const szg_image* im, std::initializer_list<unsigned> formats, const char* must)
{
    if (im == nullptr || im->data == nullptr)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s image or its data is NULL", me, name);
        return false;
    }
    if (std::find(formats.begin(), formats.end(), im->format) == formats.end())
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s format %u, %s", me, name, im->format, must);
        return false;
    }
    return true;
}

bool check_image_layout(const char* me, const char* name, const szg_image& im)
{
    if (!image_layout_ok(im))
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s pitch %u / alignment invalid for %u texels of %u bytes", me, name, im.pitch_bytes, im.width,
             texel_bytes(im.format));
        return false;
    }
    return true;
}

bool check_pass_image(const char* me, const char* name, const szg_image* im, std::initializer_list<unsigned> formats, const char* must,
                      const szg_rect* region)
{
    if (!check_image_format(me, name, im, formats, must))
    {
        return false;
    }
    if (!extents_ok(*im, 0u))
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s image %ux%u exceeds %u texels", me, name, im->width, im->height, SZG_PRESENT_MAX_EXTENT);
        return false;
    }
    if (!check_image_layout(me, name, *im))
    {
        return false;
    }
    if (region != nullptr && !rect_inside(*region, *im))
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s region (%d, %d) %ux%u leaves the %ux%u image", me, name, region->x, region->y, region->width,
             region->height, im->width, im->height);
        return false;
    }
    return true;
}

bool check_gbuffer(const szg_gbuffer* g, unsigned w, unsigned h)
{
    if (g == nullptr)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "gbuffer is NULL");
        return false;
    }
    return check_image(g->diffuse, SZG_FORMAT_RGBA16_SFLOAT, w, h, "gbuffer.diffuse") &&
           check_image(g->specular, SZG_FORMAT_RGBA16_SFLOAT, w, h, "gbuffer.specular") &&
           check_image(g->normal, SZG_FORMAT_RGBA16_SFLOAT, w, h, "gbuffer.normal") &&
           check_image(g->worldPosition, SZG_FORMAT_RGBA32_SFLOAT, w, h, "gbuffer.worldPosition") &&
           check_image(g->occlusionRoughnessMetallic, SZG_FORMAT_RGBA16_SFLOAT, w, h, "gbuffer.occlusionRoughnessMetallic");
}

bool check_scene(const szg_scene_texture* s, unsigned w, unsigned h, bool needDepth)
{
    if (s == nullptr)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "scene_texture is NULL");
        return false;
    }
    if (!check_image(s->color, SZG_FORMAT_RGBA16_UNORM, w, h, "scene_texture.color"))
    {
        return false;
    }
    if (needDepth && !check_image(s->depth, SZG_FORMAT_D32_SFLOAT, w, h, "scene_texture.depth"))
    {
        return false;
    }
    if (s->debug_color.data != nullptr && !check_image(s->debug_color, SZG_FORMAT_RGBA32_SFLOAT, w, h, "scene_texture.debug_color"))
    {
        return false;
    }
    return true;
}

bool resolve_tile(const szg_rowtile* tile, unsigned drawH, szg::TileArgs& out)
{
    if (tile == nullptr || tile->nranks <= 1u)
    {
        out = szg::TileArgs{1u, 0u, 1u, drawH};
        return true;
    }
    if (tile->block_rows == 0u || tile->rank >= tile->nranks)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "rowtile: block_rows %u rank %u nranks %u", tile->block_rows, tile->rank, tile->nranks);
        return false;
    }
    unsigned const expect = szg_rowtile_local_rows(drawH, tile->block_rows, tile->rank, tile->nranks);
    if (tile->local_rows != expect)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "rowtile: local_rows %u, expected %u for a %u-row frame", tile->local_rows, expect, drawH);
        return false;
    }
    out = szg::TileArgs{tile->block_rows, tile->rank, tile->nranks, tile->local_rows};
    return true;
}

int select_device(int device)
{
    int count = 0;
    hipError_t const e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
    {
        return fail(SZG_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device < 0 || device >= count)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "device %d out of range [0, %d)", device, count);
    }
    SZG_HIP(hipSetDevice(device));
    return SZG_OK;
}

bool check_rect(const szg_rect& r, const char* what)
{
    if (r.x != 0 || r.y != 0)
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: draw_rect offset (%d, %d) must be (0, 0): passes cover the top-left extent only", what, r.x, r.y);
        return false;
    }
    return true;
}

szg_image make_image(void* data, unsigned w, unsigned h, unsigned fmt)
{
    szg_image im;
    im.data = data;
    im.width = w;
    im.height = h;
    im.pitch_bytes = w * texel_bytes(fmt);
    im.format = fmt;
    return im;
}
} // namespace szg

using namespace szg;

extern "C" {

int szg_abi_version(void) { return SZG_ABI_VERSION; }

#ifndef SZG_SOURCE_HASH
#define SZG_SOURCE_HASH "unknown"
#endif
const char* szg_build_id(void)
{
    static char text[64];
    static std::once_flag once;
    std::call_once(once, [] { snprintf(text, sizeof text, "%s contract=0x%04x", SZG_SOURCE_HASH, (unsigned)(SZG_CONTRACT)); });
    return text;
}
const char* szg_last_error(void) { return g_error; }

int szg_device_count(void)
{
    int count = 0;
    hipError_t const e = hipGetDeviceCount(&count);
    if (e != hipSuccess)
    {
        return fail(SZG_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return count;
}

uint32_t szg_rowtile_local_rows(uint32_t height, uint32_t block_rows, uint32_t rank, uint32_t nranks)
{
    if (nranks <= 1u)
    {
        return height;
    }
    if (block_rows == 0u || rank >= nranks)
    {
        return 0u;
    }
    uint32_t const nblocks = (height + block_rows - 1u) / block_rows;
    uint32_t rows = 0;
    for (uint32_t b = rank; b < nblocks; b += nranks)
    {
        uint32_t const begin = b * block_rows;
        uint32_t const end = begin + block_rows < height ? begin + block_rows : height;
        rows += end - begin;
    }
    return rows;
}

int szg_compose_rowtiles(void* stream, const void* gathered, size_t tile_stride_bytes, uint32_t nranks, uint32_t block_rows,
                         const szg_image* dst, uint32_t width, uint32_t height)
{
    if (gathered == nullptr || dst == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compose_rowtiles: NULL argument");
    }
    if (nranks == 0u || block_rows == 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compose_rowtiles: nranks/block_rows must be > 0");
    }
    if (!check_image(*dst, SZG_FORMAT_RGBA16_UNORM, width, height, "compose dst"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if ((width * 8u) % 16u != 0u || tile_stride_bytes % 16u != 0u || reinterpret_cast<uintptr_t>(gathered) % 16u != 0u ||
        !rows_aligned(dst->data, dst->pitch_bytes, 16u))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compose_rowtiles: rows must be 16-byte multiples and 16-byte aligned");
    }
    size_t maxRows = 0;
    for (uint32_t r = 0; r < nranks; r++)
    {
        size_t const rows = szg_rowtile_local_rows(height, block_rows, r, nranks);
        if (rows > maxRows)
        {
            maxRows = rows;
        }
    }
    if (maxRows * width * 8u > tile_stride_bytes)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compose_rowtiles: tile stride %zu smaller than the largest tile %zu",
                    tile_stride_bytes, maxRows * width * 8u);
    }
    SZG_HIP(szg::launch_compose_rowtiles(static_cast<hipStream_t>(stream), gathered, tile_stride_bytes, nranks, block_rows, *dst,
                                         width, height));
    return SZG_OK;
}

} // extern "C"
