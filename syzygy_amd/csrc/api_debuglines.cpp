// api_debuglines.cpp — DebugLineGraphicsPipeline behind the C-ABI (include/szg/debuglines.h).

#include <new>

#include "api_common.hpp"

using namespace szg;

struct szg_debug_lines
{
    int device = 0;
    uint32_t vertexCapacity = 0;
    DeviceBuffer<DebugLineRec> recs;
    DeviceBuffer<unsigned long long> steps, offsets;
    DeviceBuffer<void> scanTemp;
    DebugLineBuffers b{}; // the view of the four the launch interface takes
};

extern "C" {

// pipelines.cpp:382-461 (the pipeline) + the line list's device memory: scratch for vertex_capacity / 2 lines, sized once
int szg_debug_lines_create(szg_debug_lines_t** out, uint32_t vertex_capacity, int device)
{
    if (out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_debug_lines_create: NULL argument");
    }
    *out = nullptr;
    if (vertex_capacity == 0u || vertex_capacity > SZG_DEBUG_LINES_MAX_CAPACITY)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_debug_lines_create: vertex capacity %u outside [1, %u]", vertex_capacity,
                    SZG_DEBUG_LINES_MAX_CAPACITY);
    }
    SZG_TRY_RC(select_device(device));
    szg_debug_lines* p = new (std::nothrow) szg_debug_lines();
    if (p == nullptr)
    {
        return fail(SZG_ERR_OUT_OF_MEMORY, "szg_debug_lines_create: host allocation failed");
    }
    p->device = device;
    p->vertexCapacity = vertex_capacity;
    size_t const lines = vertex_capacity / 2u;
#define SZG_TRY(expr) SZG_HIP_OR(expr, szg_debug_lines_destroy(p), "szg_debug_lines_create")
    SZG_TRY(debug_lines_scan_temp_bytes((unsigned)lines, p->b.scanTempBytes));
    SZG_TRY(p->recs.alloc(lines > 0u ? lines : 1u));
    SZG_TRY(p->steps.alloc(lines + 1u));
    SZG_TRY(p->offsets.alloc(lines + 1u));
    SZG_TRY(p->scanTemp.alloc(p->b.scanTempBytes > 0u ? p->b.scanTempBytes : 1u));
#undef SZG_TRY
    p->b.recs = p->recs;
    p->b.steps = p->steps;
    p->b.offsets = p->offsets;
    p->b.scanTemp = p->scanTemp;
    *out = p;
    return SZG_OK;
}

// pipelines.cpp:584-589 DebugLineGraphicsPipeline::cleanup
void szg_debug_lines_destroy(szg_debug_lines_t* p)
{
    if (p == nullptr)
    {
        return;
    }
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

// pipelines.cpp:463-581 recordDrawCommands, called as renderer.cpp:445-476 does (reuseDepthAttachment = false; the
// depth attachment is dropped, debuglines.h)
int szg_debug_lines_record(szg_debug_lines_t* p, void* stream, float line_width, szg_rect draw_rect, const szg_rowtile* tile,
                           const szg_scene_texture* scene_texture, uint32_t camera_index, const szg_camera_packed* d_cameras,
                           const szg_vertex_packed* d_vertices, uint32_t vertex_count)
{
    if (p == nullptr || scene_texture == nullptr || (vertex_count >= 2u && (d_cameras == nullptr || d_vertices == nullptr)))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_debug_lines_record: NULL argument");
    }
    if (!check_rect(draw_rect, "szg_debug_lines_record"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    // !(w <= cap) also refuses NaN
    if (!(line_width >= 0.0f && line_width <= SZG_DEBUG_LINES_MAX_WIDTH))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_debug_lines_record: line_width %g outside [0, %g]", (double)line_width,
                    (double)SZG_DEBUG_LINES_MAX_WIDTH);
    }
    if (vertex_count > p->vertexCapacity)
    {
        return fail(SZG_ERR_CAPACITY, "szg_debug_lines_record: %u vertices, capacity %u", vertex_count, p->vertexCapacity);
    }
    if (draw_rect.width > 32768u || draw_rect.height > 32768u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_debug_lines_record: draw extent above 32768");
    }
    DeviceGuard const guard(p->device);
    szg::TileArgs t{};
    if (!resolve_tile(tile, draw_rect.height, t) || !check_scene(scene_texture, draw_rect.width, t.local_rows, false))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (vertex_count < 2u || draw_rect.width == 0u || draw_rect.height == 0u)
    {
        return SZG_OK; // renderer.cpp:455: nothing to draw
    }
    SZG_HIP(szg::launch_debug_lines(static_cast<hipStream_t>(stream), *scene_texture, draw_rect.width, draw_rect.height, t, d_cameras,
                                    camera_index, d_vertices, vertex_count / 2u, line_width, p->b));
    return SZG_OK;
}

} // extern "C"
