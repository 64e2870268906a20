/*
 * szg/ui_layer.h — C-ABI of the UI layer pass: the draw whose output the reference presents. Editor::run
 * (editor/editor.cpp:720-748) records the scene into the scene texture, then UILayer::recordDraw, then endFrame on
 * uiOutput.texture / uiOutput.renderedSubregion: the OETF and the present blit (szg/present.h) run on the UI OUTPUT texture.
 *
 *   UILayer::recordDraw   editor/uilayer.cpp:513-572: clears the RGBA16_UNORM output texture to opaque black (:285-291) and
 *                         draws the Dear ImGui draw data into it (render area :536-545). The scene viewport is one textured
 *                         quad of that draw data: the scene texture through the scene texture's own sampler, NEAREST with
 *                         CLAMP_TO_BORDER and an opaque-black border (renderer/scenetexture.cpp:104-109, registered with
 *                         ImGui at uilayer.cpp:318-322), at UVs contentExtent / textureCapacity
 *                         (ui/statelesswidgets.cpp:868-885).
 *   the backend           ImGui_ImplVulkan_RenderDrawData (imgui v1.90.6-docking, cmake/dependencies.cmake:49-51, default
 *                         ImDrawVert and 16-bit ImDrawIdx, thirdparty/imgui/imguiconfig.h): fb_width / fb_height, the
 *                         concatenated vertex and index buffers with global offsets, the per-command scissor and texture
 *                         binding, one vkCmdDrawIndexed per ImDrawCmd.
 *                         ImGui_ImplVulkan_SetupRenderState: viewport (0, 0, fb_width, fb_height), scale 2 / DisplaySize and
 *                         translate -1 - DisplayPos * scale (a vertex lands on (pos - DisplayPos) * FramebufferScale px).
 *                         ImGui_ImplVulkan_CreatePipeline: triangle list, polygon fill, cull NONE, no depth, blending
 *                         SRC_ALPHA / ONE_MINUS_SRC_ALPHA on colour and ONE / ONE_MINUS_SRC_ALPHA on alpha, op ADD;
 *                         fragment = vertex colour * texture sample.
 *                         The font sampler (ImGui_ImplVulkan_CreateDeviceObjects): LINEAR, REPEAT. A texture added with
 *                         ImGui_ImplVulkan_AddTexture brings its own sampler: szg_ui_layer_add_texture.
 *
 * Widgets, layout, fonts and ImGui itself are out of scope; the DRAW is the pass. Vulkan leaves triangle rasterisation,
 * filtering and blend precision to the implementation, so this pass has no bit-level reference ("parity unpinned", like
 * szg/raster.h, szg/debuglines.h and szg/present.h). The rules below are stated completely so that the CPU model
 * (tests/ui_layer_model.py) and the kernels (syzygy_amd/csrc/kernels_ui_layer.hip) agree bit for bit. Every floating-point
 * operation named is ONE IEEE binary32 operation, rounded to nearest even, evaluated in the order written, never fused with
 * its neighbour: this site belongs to none of the classes of szg/contraction.h, so libszg_hip.so and libszg_hip_literal.so
 * produce the same bytes.
 *
 * VIEWPORT    fbw = (int)(display_size.x * framebuffer_scale.x), fbh likewise (one product, truncated; a product outside
 *             int32 saturates). The viewport is (0, 0, fbw, fbh) of the output image whatever render_area.offset is: what the
 *             backend sets. render_area only limits what is cleared and written, and is honoured WITH its offset, like the
 *             regions of szg/present.h. A pixel is written only inside render_area ∩ viewport ∩ scissor ∩ image. With
 *             fbw <= 0 or fbh <= 0 the clear still happens and nothing is drawn.
 *
 * VERTEX      p = (pos - display_pos) * framebuffer_scale: one subtraction and one product per axis. Snapped to 8 sub-pixel
 *             bits as a signed integer: X = (int)rint(p.x * 256), Y likewise (rint: to nearest, ties to even). A triangle with
 *             a non-finite p or |p| > SZG_UI_GUARD_BAND (2^20 px) on any axis of any vertex draws nothing: the guard band,
 *             which keeps every integer below inside int64.
 *
 * ASSEMBLY    triangle t of a command is vertices[vtx_offset + indices[idx_offset + 3t + {0, 1, 2}]]. Trailing indices beyond a
 *             multiple of three are ignored. An index range reaching past index_count is truncated first (to
 *             index_count - idx_offset indices, none when idx_offset >= index_count). A vertex index (vtx_offset included)
 *             >= vertex_count drops its triangle. No culling: both windings draw.
 *
 * COVERAGE    pixel centre C = (256 px + 128, 256 py + 128). Edge function, for (i, j, k) cyclic over (0, 1, 2):
 *               E_i = (X_k - X_j)(C_y - Y_j) - (Y_k - Y_j)(C_x - X_j)           exact in int64
 *               det = (X_1 - X_0)(Y_2 - Y_0) - (Y_1 - Y_0)(X_2 - X_0);  det = 0 draws nothing;  s = sign(det)
 *             A pixel is covered when for all three edges s E_i > 0, or s E_i = 0 and edge i is a left or a top edge:
 *               left edge  s a_i > 0 with a_i = -(Y_k - Y_j)
 *               top edge   a_i = 0 and s b_i > 0 with b_i = X_k - X_j
 *             (the words of szg/raster.h). A filled rectangle at integer or half-integer corners, drawn as ImGui draws it
 *             (indices 0 1 2, 0 2 3), covers each pixel with x0 <= px + .5 < x1, y0 <= py + .5 < y1 exactly once, in either
 *             winding; consistently wound triangles sharing an edge or a vertex hit no pixel twice.
 *
 * SCISSOR     per command, as the backend computes it: cmin = (clip_rect.xy - display_pos) * framebuffer_scale, cmax from
 *             .zw; cmin.x < 0 becomes 0 and cmax.x > fbw becomes (float)fbw (y likewise); the command is skipped when
 *             cmax.x <= cmin.x or cmax.y <= cmin.y, and also when cmin or cmax has a non-finite component (the backend's
 *             conversion is undefined there). x0 = (int32)cmin.x, w = (uint32)(cmax.x - cmin.x): the float subtraction first,
 *             then the truncation; y likewise. A pixel is inside when x0 <= px < x0 + w and y0 <= py < y0 + h.
 *
 * INTERPOLATION affine (w = 1): lambda_i = float(s E_i) / float(|det|), each conversion from int64 one rounding to nearest
 *             even, then one division. An attribute is (lambda_0 a_0 + lambda_1 a_1) + lambda_2 a_2, a_i belonging to the
 *             vertex opposite edge i (vertex i). Colour channels are float(byte) / 255.0f before interpolation; `col` holds
 *             the bytes R, G, B, A from the least significant (IM_COL32).
 *
 * SAMPLING    textures are SZG_FORMAT_RGBA8_UNORM (font atlas, material maps) or SZG_FORMAT_RGBA16_UNORM (the scene colour),
 *             one level, W x H texels. A texel channel is float(code) / 255.0f or float(code) / 65535.0f.
 *             NEAREST: x = u W (one product), f = floor(x) is the texel; y likewise with v H.
 *             LINEAR:  x = u W - 0.5, f = floor(x), alpha = x - f; taps f and f + 1.0f (a float sum); beta from y. With
 *                      t00 / t10 the taps of row j0 at columns i0 / i1 and t01 / t11 those of row j1, the products and sums
 *                      of szg/present.h LINEAR: top = t00 (1 - alpha) + t10 alpha, bot = t01 (1 - alpha) + t11 alpha,
 *                      r = top (1 - beta) + bot beta; (1 - alpha), each product and each sum separately rounded.
 *             Addressing, per tap and per axis, of a tap coordinate f (a float holding an integer, or non-finite) over n texels:
 *               REPEAT           the positive modulo as wrapIndex of szg_texture.hpp computes it: m = f - n floor(f / n) in
 *                                fp32; the texel is (int)m when 0 <= m < n, else 0. The second LINEAR tap is the texel
 *                                after the first one, 0 after n - 1.
 *               CLAMP_TO_EDGE    (int)min(max(f, 0), n - 1); a NaN gives 0.
 *               CLAMP_TO_BORDER  as CLAMP_TO_EDGE when 0 <= f <= n - 1; any other f (NaN included) is outside, and a tap
 *                                outside on either axis reads (0, 0, 0, 1), opaque black.
 *
 * FRAGMENT    out = colour * texel per channel; each channel is then clamped to [0, 1], NaN becomes 0.
 *
 * BLEND       d = float(code) / 65535.0f of the destination texel AS STORED (after the clear and after every earlier
 *             fragment the destination holds UNORM16 codes), alpha = out.a:
 *               rgb' = out.rgb * alpha + d.rgb * (1 - alpha)
 *               a'   = out.a + d.a * (1 - alpha)
 *             (1 - alpha), each product and each sum separately rounded. The store is the library's UNORM16 store: clamp to
 *             [0, 1], multiply by 65535, round to nearest even.
 *
 * ORDER       per pixel, fragments blend in submission order: command order, then index order. Results depend on the
 *             order, and the order is the caller's. This is the first pass of the library of which that is true.
 *
 * CLEAR       SZG_UI_LOAD_OP_CLEAR writes clear_color through the same store to every pixel of render_area ∩ image before any
 *             fragment; the reference clears to (0, 0, 0, 1). SZG_UI_LOAD_OP_LOAD keeps the pixels.
 *
 * UNTOUCHED   every byte outside render_area keeps its value, pitch padding included. Textures are never written.
 *
 * HBM traffic: the destination is read once per pixel (not at all under CLEAR) and written once, 8 B + 8 B, plus the
 * texture taps. Row tiles (szg_rowtile) are not supported, as for szg/compute_collection.h.
 *
 * STREAM RULE as in szg/abi.h: a layer owns device scratch that its record calls rewrite in stream order; record on one
 * stream at a time, or order the streams yourself.
 */
#ifndef SZG_UI_LAYER_H
#define SZG_UI_LAYER_H

#include "szg/abi.h"
#include "szg/present.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VkSamplerAddressMode: REPEAT = 0, CLAMP_TO_EDGE = 2, CLAMP_TO_BORDER = 3 (border colour: opaque black, 0 0 0 1) */
#define SZG_UI_ADDRESS_REPEAT 0u
#define SZG_UI_ADDRESS_CLAMP_TO_EDGE 2u
#define SZG_UI_ADDRESS_CLAMP_TO_BORDER 3u

/* VkAttachmentLoadOp: LOAD = 0, CLEAR = 1 */
#define SZG_UI_LOAD_OP_LOAD 0u
#define SZG_UI_LOAD_OP_CLEAR 1u

/* |p| above this (pixels) on a vertex drops its triangle (VERTEX above) */
#define SZG_UI_GUARD_BAND 1048576.0f
/* most triangles / commands one layer can be created for */
#define SZG_UI_MAX_TRIANGLE_CAPACITY (1u << 24)
#define SZG_UI_MAX_COMMAND_CAPACITY (1u << 20)

/* ImDrawVert, 20 bytes; col bytes R, G, B, A from the least significant */
typedef struct szg_ui_draw_vert
{
    float pos[2];
    float uv[2];
    uint32_t col;
} szg_ui_draw_vert;

/* The ImGui Vulkan backend's state behind one UILayer: textures and the scratch of the rasteriser. */
typedef struct szg_ui_layer szg_ui_layer_t;
/* What ImTextureID holds: the VkDescriptorSet of ImGui_ImplVulkan_AddTexture, an image and its sampler. */
typedef struct szg_ui_texture szg_ui_texture_t;

typedef struct szg_ui_sampler
{
    uint32_t filter;  /* SZG_FILTER_NEAREST / SZG_FILTER_LINEAR (szg/present.h) */
    uint32_t address; /* SZG_UI_ADDRESS_*, both axes */
} szg_ui_sampler;

/* ImDrawCmd. vtx_offset and idx_offset are already global: the backend's global_vtx_offset + VtxOffset and
 * global_idx_offset + IdxOffset into the concatenated buffers. A command with a user callback is not a draw: leave it out. */
typedef struct szg_ui_draw_cmd
{
    float clip_rect[4]; /* ImDrawCmd::ClipRect x, y, z, w in ImGui coordinates */
    const szg_ui_texture_t* texture;
    uint32_t vtx_offset, idx_offset, elem_count, reserved; /* reserved: 0 */
} szg_ui_draw_cmd;

/* ImDrawData with its lists concatenated. Vertices and indices are DEVICE memory, the command array is HOST memory (like
 * szg_surface): it is copied before the call returns and may be freed or overwritten at once. */
typedef struct szg_ui_draw_data
{
    float display_pos[2], display_size[2], framebuffer_scale[2];
    const szg_ui_draw_vert* d_vertices;
    uint32_t vertex_count;
    const uint16_t* d_indices;
    uint32_t index_count;
    const szg_ui_draw_cmd* commands;
    uint32_t command_count;
} szg_ui_draw_data;

/* ImGui_ImplVulkan_Init + CreateDeviceObjects: scratch for `triangle_capacity` triangles (in [1,
 * SZG_UI_MAX_TRIANGLE_CAPACITY]) and `command_capacity` commands (in [1, SZG_UI_MAX_COMMAND_CAPACITY]) per record, allocated
 * once. Returns SZG_OK and *out, or a negative status and *out = NULL. */
int szg_ui_layer_create(szg_ui_layer_t** out, uint32_t triangle_capacity, uint32_t command_capacity, int device);
/* ImGui_ImplVulkan_Shutdown; frees the layer's textures too. NULL is allowed. */
void szg_ui_layer_destroy(szg_ui_layer_t* layer);

/* ImGui_ImplVulkan_AddTexture: the handle a command's `texture` names. `image` (RGBA8_UNORM or RGBA16_UNORM, one level,
 * extent in [1, SZG_PRESENT_MAX_EXTENT]) is copied as a description; its texels are read when a draw that names it is
 * RECORDED, in stream order, so the scene texture may be re-rendered every frame. Refused: a NULL or malformed image, another
 * format, an unknown sampler value. */
int szg_ui_layer_add_texture(szg_ui_layer_t* layer, const szg_image* image, szg_ui_sampler sampler, szg_ui_texture_t** out);
/* ImGui_ImplVulkan_RemoveTexture. Refused: a handle that is not this layer's. The caller orders it behind the draws that
 * read the texture, as with Vulkan. */
int szg_ui_layer_remove_texture(szg_ui_layer_t* layer, szg_ui_texture_t* texture);

/* UILayer::recordDraw's render pass (uilayer.cpp:513-572 -> ImGui_ImplVulkan_RenderDrawData): clear or load `render_area` of
 * `output` (RGBA16_UNORM) and draw `draw_data` into it by the rules above. Asynchronous on `stream`: no host round trip and
 * no stream synchronisation (the copy of the command array goes through a ring of pinned buffers; the call waits only when
 * all of them are still in flight). clear_color may be NULL under SZG_UI_LOAD_OP_LOAD.
 * Refused with SZG_ERR_INVALID_ARGUMENT (SZG_ERR_CAPACITY where noted) and a szg_last_error() text, nothing launched and
 * nothing written: a NULL layer, draw data or output image or a malformed one (NULL data, a pitch below a row or not a
 * multiple of 8, data not 8-byte aligned); an output format other than RGBA16_UNORM; an image extent above
 * SZG_PRESENT_MAX_EXTENT; a render area that leaves the image; an unknown load op; a NULL clear colour under CLEAR;
 * non-finite display_pos, display_size or framebuffer_scale; a NULL command array with command_count > 0; a NULL vertex or
 * index array while a command has elem_count > 0; on a command with elem_count > 0 a NULL texture, a texture handle that
 * is not this layer's, or a texture whose memory overlaps the output image; more commands than command_capacity or more
 * triangles (after ASSEMBLY's truncation, summed over the commands) than triangle_capacity: SZG_ERR_CAPACITY.
 * command_count == 0 is SZG_OK: it performs the clear, if one is asked for, and nothing else. */
int szg_ui_layer_record_draw(szg_ui_layer_t* layer, void* stream, const szg_image* output, szg_rect render_area, uint32_t load_op,
                             const float clear_color[4], const szg_ui_draw_data* draw_data);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_UI_LAYER_H */
