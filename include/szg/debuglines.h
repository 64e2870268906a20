/*
 * szg/debuglines.h — C-ABI of the debug-line pass: the "Debug Lines" overlay of Renderer::recordDraw
 * (renderer.cpp:287 clears the list, :355-365 pushes one box per mesh-instance transform, :417-423 the shadow-bounds box,
 * :425-427 + :445-476 draw it over the scene colour after the sky-view composite; editor switch engineui.cpp:95-109,
 * DebugLines::enabled, default off), rebuilt as a HIP compute line rasteriser.
 *
 *   pipeline state  renderer/pipelines.cpp:382-461: line list, polygon fill, no culling, dynamic lineWidth, no blending
 *                   (pipelines.hpp:96), depth test on with compare ALWAYS
 *   draw            pipelines.cpp:463-581: colour LOAD/STORE on the RGBA16 UNORM scene colour; viewport and scissor = the
 *                   draw rect, depth 0..1; depth attachment cleared to 0; vkCmdDraw(indices.deviceSize(), 1, 0, 0): a
 *                   NON-indexed draw, vertex i is endpoint i, line k is (v[2k], v[2k+1]); the index buffer is never read
 *   shaders         shaders/debug/debugline.vert: gl_Position = camera.projection * camera.view * vec4(position, 1);
 *                   debugline.frag writes the constant (0, 1, 0, 1): vertex colour and uv never reach the image
 *
 * The depth attachment is dropped. Its compare op is ALWAYS, so it cannot change a single colour value, and the image it
 * writes (Renderer::m_sceneDepthTexture, renderer.cpp:445-476, not sceneTexture.depth()) is private to the renderer and
 * never read. The pass's only observable output is the colour; scene_texture->depth is neither read nor written.
 *
 * Vulkan leaves line rasterisation to the implementation, so this pass has no bit-level reference: "parity unpinned", like
 * the triangle raster (szg/raster.h). The rules below are stated exactly so that the CPU model (tests/debuglines_model.py)
 * and the kernels (syzygy_amd/csrc/kernels_debuglines.hip) agree bit for bit. Every operation is one IEEE binary32
 * operation, round to nearest even, evaluated in the order written; nothing is contracted into an FMA (the contraction
 * rule of szg/contraction.h does not apply here: the product and the literal library give identical bits).
 *
 *   vertex      PV = projection * view of camera `camera_index`: column j of PV is
 *               ((P[0]*V[j][0] + P[1]*V[j][1]) + P[2]*V[j][2]) + P[3]*V[j][3] (P[c] = column c of P);
 *               clip = ((PV[0]*x + PV[1]*y) + PV[2]*z) + PV[3]*1 for position (x, y, z) (OpMatrixTimesMatrix then
 *               OpMatrixTimesVector of debugline.vert.spv; pinned by tests/golden/debugline_vectors.npz).
 *   assembly    line k = (v[2k], v[2k+1]) for k < vertex_count / 2; an odd last vertex draws nothing. A line with a
 *               non-finite clip component draws nothing.
 *   clipping    only the depth planes of Vulkan's clip volume, first 0 <= z (d = z), then z <= w (d = w - z), each
 *               evaluated at the current endpoints a, b. Both d < 0: the line is dropped. Exactly one d < 0:
 *               t = d_a / (d_a - d_b) and the outside endpoint becomes a + t * (b - a), per component (x, y, z, w), with
 *               a and b the endpoints before this plane. d >= 0 (also -0) is inside. x and y are not clipped: the scissor
 *               bounds them (guard band).
 *   viewport    x_f = (x / w + 1) * (W * 0.5), y_f = (y / w + 1) * (H * 0.5), W x H = the draw-rect extent. A line with
 *               a non-finite x_f or y_f, or one of magnitude above SZG_DEBUG_LINES_GUARD_BAND (2^24 px), draws nothing
 *               (the end of the guard band).
 *   coverage    the strict-line rectangle of width line_width centred on the segment, no end caps. For pixel centre
 *               c = (px + 0.5, py + 0.5): dx = x_b - x_a, dy = y_b - y_a, ex = c.x - x_a, ey = c.y - y_a,
 *               u = ex*dx + ey*dy, v = dx*ey - dy*ex, L2 = dx*dx + dy*dy (each a sum of two rounded products);
 *               covered iff L2 > 0 and 0 <= u and u <= L2 and (4*v)*v <= (line_width*line_width) * L2.
 *   output      covered pixels inside the draw rect (and, with a row tile, inside the rank's rows) get
 *               (0, 65535, 0, 65535) in scene_texture->color and, when debug_color.data != NULL, (0, 1, 0, 1) there.
 *               No other byte of any plane is read or written. Every line writes the same value: primitive order does
 *               not matter and overlaps are harmless.
 */
#ifndef SZG_DEBUGLINES_H
#define SZG_DEBUGLINES_H

#include "szg/abi.h"
#include "szg/raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* renderer.hpp:103 DEBUGLINES_CAPACITY: the vertex capacity of the reference's list */
#define SZG_DEBUG_LINES_CAPACITY 1000u
/* debuglines.hpp DebugLines::lineWidth default */
#define SZG_DEBUG_LINES_DEFAULT_WIDTH 1.0f
/* the widest line the pass accepts; the editor slider ends at 100 (engineui.cpp:95-109) */
#define SZG_DEBUG_LINES_MAX_WIDTH 256.0f
/* |x_f|, |y_f| above this (pixels) drop the line (viewport rule above) */
#define SZG_DEBUG_LINES_GUARD_BAND 16777216.0f
/* most vertices one pipeline object can hold */
#define SZG_DEBUG_LINES_MAX_CAPACITY (1u << 24)

/* DebugLineGraphicsPipeline (renderer/pipelines.hpp:238-268). Owns its scratch memory, sized from vertex_capacity. */
typedef struct szg_debug_lines szg_debug_lines_t;

/* DebugLineGraphicsPipeline constructor (pipelines.cpp:382-461); vertex_capacity in [1, SZG_DEBUG_LINES_MAX_CAPACITY]. */
int szg_debug_lines_create(szg_debug_lines_t** out, uint32_t vertex_capacity, int device);
/* DebugLineGraphicsPipeline::cleanup (pipelines.cpp:583-589). NULL is allowed. */
void szg_debug_lines_destroy(szg_debug_lines_t* p);

/* DebugLineGraphicsPipeline::recordDrawCommands (pipelines.cpp:463-581) as Renderer::recordDrawDebugLines calls it
 * (renderer.cpp:445-476): `vertex_count` endpoints (szg_vertex_packed, DEVICE memory) of camera `camera_index` of
 * `d_cameras`, drawn into scene_texture->color (and debug_color) over draw_rect. `tile` may be NULL; a non-NULL tile works
 * as in abi.h: the rank rasterises only its rows into its local image. Asynchronous on `stream`, no host round trip.
 * Refused (SZG_ERR_INVALID_ARGUMENT, szg_last_error): a non-zero draw-rect offset, a line_width that is NaN, infinite,
 * negative or above SZG_DEBUG_LINES_MAX_WIDTH, a NULL colour plane; SZG_ERR_CAPACITY: vertex_count above the capacity.
 * vertex_count < 2 returns SZG_OK and launches nothing. */
int szg_debug_lines_record(szg_debug_lines_t* p, void* stream, float line_width, szg_rect draw_rect, const szg_rowtile* tile,
                           const szg_scene_texture* scene_texture, uint32_t camera_index, const szg_camera_packed* d_cameras,
                           const szg_vertex_packed* d_vertices, uint32_t vertex_count);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_DEBUGLINES_H */
