// api_image_passes.cpp — the passes over one image that need no pipeline object: OETF, present, compute collection.

#include <mutex>

#include "api_common.hpp"

using namespace szg;

static_assert(SZG_COMPUTE_COLLECTION_MAX_EXTENT == SZG_PRESENT_MAX_EXTENT, "extents_ok (api_core.cpp) holds both passes to one cap");

namespace
{
// Per-device OETF tables (one per transfer function), built on first use by k_oetf_table and kept for the life of
// the process. `ready` orders later uses on other streams behind the build.
struct OetfTables
{
    std::mutex lock;
    unsigned short* table[16][2] = {};
    hipEvent_t ready[16][2] = {};
};
OetfTables g_oetf;

int oetf_table(hipStream_t s, unsigned function, const unsigned short** out)
{
    int device = 0;
    SZG_HIP(hipGetDevice(&device));
    if (device < 0 || device >= 16)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_oetf: device %d outside the table cache", device);
    }
    std::lock_guard<std::mutex> guard(g_oetf.lock);
    if (g_oetf.table[device][function] == nullptr)
    {
        unsigned short* t = nullptr;
        SZG_HIP(hipMalloc(reinterpret_cast<void**>(&t), 65536u * sizeof(unsigned short)));
        hipEvent_t e = nullptr;
        hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (err == hipSuccess)
        {
            err = szg::launch_oetf_table(s, t, function);
        }
        if (err == hipSuccess)
        {
            err = hipEventRecord(e, s);
        }
        if (err != hipSuccess)
        {
            (void)hipFree(t);
            if (e != nullptr)
            {
                (void)hipEventDestroy(e);
            }
            return fail_hip(err, "szg_record_oetf: building the transfer table");
        }
        g_oetf.table[device][function] = t;
        g_oetf.ready[device][function] = e;
    }
    else
    {
        SZG_HIP(hipStreamWaitEvent(s, g_oetf.ready[device][function], 0));
    }
    *out = g_oetf.table[device][function];
    return SZG_OK;
}

// What ShaderReflectionData::PushConstant holds for the four programs of renderer.cpp:238-243. Static tables; their truth is
// checked against the reference's binaries by tests/test_compute_collection_reflection.py, not trusted.
#define SZG_CC_PREFIX_MEMBERS                                                                                                  \
    {"drawOffset", 0u, 8u, 8u, SZG_CC_COMPONENT_FLOAT, 2u, 1u}, { "drawExtent", 8u, 8u, 8u, SZG_CC_COMPONENT_FLOAT, 2u, 1u }
const szg_cc_reflection g_ccReflection[SZG_COMPUTE_COLLECTION_SHADER_COUNT] = {
    {"booleanpush", 80u, 80u, 0u, {16u, 16u, 1u}, 6u,
     {SZG_CC_PREFIX_MEMBERS,
      {"row1", 16u, 16u, 16u, SZG_CC_COMPONENT_BOOL, 4u, 1u},
      {"row2", 32u, 16u, 16u, SZG_CC_COMPONENT_BOOL, 4u, 1u},
      {"row3", 48u, 16u, 16u, SZG_CC_COMPONENT_BOOL, 4u, 1u},
      {"row4", 64u, 16u, 16u, SZG_CC_COMPONENT_BOOL, 4u, 1u}}},
    {"gradient_color", 48u, 48u, 0u, {16u, 16u, 1u}, 4u,
     {SZG_CC_PREFIX_MEMBERS,
      {"topColor", 16u, 16u, 16u, SZG_CC_COMPONENT_FLOAT, 4u, 1u},
      {"bottomColor", 32u, 16u, 16u, SZG_CC_COMPONENT_FLOAT, 4u, 1u}}},
    {"sparse_push_constant", 80u, 80u, 0u, {16u, 16u, 1u}, 6u,
     {SZG_CC_PREFIX_MEMBERS,
      {"topRG", 16u, 8u, 16u, SZG_CC_COMPONENT_FLOAT, 2u, 1u},
      {"topBA", 32u, 8u, 16u, SZG_CC_COMPONENT_FLOAT, 2u, 1u},
      {"bottomRG", 48u, 8u, 16u, SZG_CC_COMPONENT_FLOAT, 2u, 1u},
      {"bottomBA", 64u, 8u, 16u, SZG_CC_COMPONENT_FLOAT, 2u, 1u}}},
    {"matrix_color", 208u, 208u, 0u, {16u, 16u, 1u}, 5u,
     {SZG_CC_PREFIX_MEMBERS,
      {"red", 16u, 64u, 64u, SZG_CC_COMPONENT_FLOAT, 4u, 4u},
      {"green", 80u, 64u, 64u, SZG_CC_COMPONENT_FLOAT, 4u, 4u},
      {"blue", 144u, 64u, 64u, SZG_CC_COMPONENT_FLOAT, 4u, 4u}}},
};
#undef SZG_CC_PREFIX_MEMBERS
} // namespace

extern "C" {

int szg_record_oetf(void* stream, const szg_image* image, uint32_t width, uint32_t height, uint32_t transfer_function)
{
    if (image == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_oetf: image is NULL");
    }
    if (transfer_function != SZG_OETF_PURE_GAMMA && transfer_function != SZG_OETF_SRGB)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_oetf: unknown transfer function %u", transfer_function);
    }
    if (width == 0u || height == 0u)
    {
        return SZG_OK;
    }
    if (!check_image(*image, SZG_FORMAT_RGBA16_UNORM, width, height, "oetf image"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (!rows_aligned(image->data, image->pitch_bytes, 16u))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_oetf: image rows must be 16-byte aligned");
    }
    const unsigned short* table = nullptr;
    SZG_TRY_RC(oetf_table(static_cast<hipStream_t>(stream), transfer_function, &table));
    SZG_HIP(szg::launch_oetf(static_cast<hipStream_t>(stream), *image, width, height, table));
    return SZG_OK;
}

// ---------------------------------------------------------------------------
// Present pass (include/szg/present.h): editor.cpp:355-361 -> imageoperations.cpp:45-119
// ---------------------------------------------------------------------------

int szg_record_present(void* stream, const szg_image* src, const szg_image* dst, const szg_present_info* info)
{
    if (info == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_present: info is NULL");
    }
    static const char* const me = "szg_record_present";
    if (!check_pass_image(me, "source", src, {SZG_FORMAT_RGBA16_UNORM}, "the source must be RGBA16_UNORM", &info->src_region) ||
        !check_pass_image(me, "destination", dst, {SZG_FORMAT_RGBA8_UNORM, SZG_FORMAT_BGRA8_UNORM, SZG_FORMAT_A2B10G10R10_UNORM},
                          "the destination must be RGBA8_UNORM, BGRA8_UNORM or A2B10G10R10_UNORM", &info->dst_region))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (info->filter != SZG_FILTER_NEAREST && info->filter != SZG_FILTER_LINEAR)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_present: unknown filter %u", info->filter);
    }
    if (info->encode != SZG_PRESENT_ENCODE_NONE && info->encode != SZG_OETF_PURE_GAMMA && info->encode != SZG_OETF_SRGB)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_present: unknown encode %u", info->encode);
    }
    if (images_overlap(*src, *dst))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_present: source and destination images overlap in memory");
    }
    if (info->src_region.width == 0u || info->src_region.height == 0u || info->dst_region.width == 0u || info->dst_region.height == 0u)
    {
        return SZG_OK; // nothing to sample or nothing to cover
    }
    const unsigned short* table = nullptr;
    if (info->encode != SZG_PRESENT_ENCODE_NONE)
    {
        SZG_TRY_RC(oetf_table(static_cast<hipStream_t>(stream), info->encode, &table));
    }
    SZG_HIP(szg::launch_present(static_cast<hipStream_t>(stream), *src, *dst, *info, table));
    return SZG_OK;
}

// ---------------------------------------------------------------------------
// Compute-collection pipeline (include/szg/compute_collection.h): renderer.cpp:431-438 -> pipelines.cpp:223-368
// ---------------------------------------------------------------------------

uint32_t szg_compute_collection_shader_count(void) { return SZG_COMPUTE_COLLECTION_SHADER_COUNT; }

int szg_compute_collection_reflect(uint32_t index, szg_cc_reflection* out)
{
    if (out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compute_collection_reflect: out is NULL");
    }
    if (index >= SZG_COMPUTE_COLLECTION_SHADER_COUNT)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_compute_collection_reflect: shader index %u, the collection has %u programs", index,
                    SZG_COMPUTE_COLLECTION_SHADER_COUNT);
    }
    *out = g_ccReflection[index];
    return SZG_OK;
}

int szg_record_compute_collection(void* stream, uint32_t shader_index, const void* push_constant_bytes, uint32_t byte_count,
                                  const szg_image* color, uint32_t width, uint32_t height)
{
    // everything here runs on the host, before anything is launched
    if (push_constant_bytes == nullptr || color == nullptr || color->data == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: push-constant bytes, colour image or its data is NULL");
    }
    if (shader_index >= SZG_COMPUTE_COLLECTION_SHADER_COUNT)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: shader index %u, the collection has %u programs", shader_index,
                    SZG_COMPUTE_COLLECTION_SHADER_COUNT);
    }
    szg_cc_reflection const& program = g_ccReflection[shader_index];
    if (byte_count != program.padded_size_bytes)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: %u bytes, the block of %s has %u", byte_count, program.name,
                    program.padded_size_bytes);
    }
    if (color->format != SZG_FORMAT_RGBA16_UNORM)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: colour format %u, must be RGBA16_UNORM", color->format);
    }
    if (!extents_ok(*color, 0u))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: colour image %ux%u exceeds %u texels", color->width,
                    color->height, SZG_COMPUTE_COLLECTION_MAX_EXTENT);
    }
    if (!image_layout_ok(*color))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: pitch %u / alignment invalid for %u texels of 8 bytes",
                    color->pitch_bytes, color->width);
    }
    if (width == 0u || height == 0u || width > color->width || height > color->height)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_compute_collection: extent %ux%u is empty or leaves the %ux%u image", width,
                    height, color->width, color->height);
    }
    // pipelines.cpp:319-344: a copy of the bytes, its first 16 overwritten with offset (0, 0) and the extent as floats
    szg::CCBlock block{};
    std::memcpy(block.w, push_constant_bytes, byte_count);
    float const prefix[4] = {0.0f, 0.0f, static_cast<float>(width), static_cast<float>(height)};
    static_assert(sizeof prefix == SZG_COMPUTE_COLLECTION_PREFIX_BYTES, "prefix layout");
    std::memcpy(block.w, prefix, sizeof prefix);
    SZG_HIP(szg::launch_compute_collection(static_cast<hipStream_t>(stream), shader_index, block, *color, width, height));
    return SZG_OK;
}

} // extern "C"
