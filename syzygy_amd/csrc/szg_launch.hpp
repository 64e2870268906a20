// szg_launch.hpp — internal launch interface between the C-ABI layer (api_*.cpp)
// and the kernel translation units. Not part of the public boundary.
#pragma once

#include <hip/hip_runtime_api.h>

#include "szg/abi.h"
#include "szg/compute_collection.h"
#include "szg/debuglines.h"
#include "szg/present.h"
#include "szg/raster.h"
#include "szg/texture_display.h"
#include "szg/ui_layer.h"

namespace szg
{
// Per-light record produced by the prep kernel, consumed by the lights kernel
// through scalar (wave-uniform) loads. 36 dwords.
struct LightRec
{
    float shadowRows[16];   // TO_TEX_COORD_MAT * projection * view (shadowmap.glinl:19), ROW-major: rows[r*4+c]
    float dir[3];           // normalize(-forward) (lights.comp:67/78)
    float falloffFactor;
    float colorStrength[3]; // color.rgb * strength (lights.comp:68/88)
    float falloffDistance;
    float position[3];
    unsigned isSpot;
    const float* map; // D32F shadow map or nullptr
    unsigned mapWidth, mapHeight;
    unsigned mapPitchFloats;
    unsigned leanOK; // bit 0: falloffDistance / falloffFactor / colour*strength of moderate magnitude (lean exact ops allowed)
    // (bit 0 also says: the light's own factors are finite and non-zero where they divide, so a culled pixel's term is an exact 0)
    // bit 1 (implies bit 0), "tight": |position| <= 2^12, |shadow rows| <= 2^14 and falloffBound in [2^-20, 2^20]. Together with
    // pixel positions <= 2^12 this bounds every operand of the lean ops from ABOVE by construction (|clip| < 2^28, d^2 < 2^28,
    // falloff < 2^48), so that k_lights' optimistic pass only has to track their LOWER bounds (kernels_lights.hip).
    float falloffBound;       // falloffFactor / falloffDistance^2 when leanOK: falloffBound * d^2 ~ the light's falloff at distance d
    float rcpFalloffDistance; // rcpN(falloffDistance) when leanOK: the shared reciprocal of dist / falloffDistance (once per light, not per wave)
};
static_assert(sizeof(LightRec) == 144, "LightRec layout");

// Device-visible shadow-map slot table entry (uploaded by the host).
struct ShadowSlot
{
    const float* map;
    unsigned width, height, pitchFloats, pad;
};
static_assert(sizeof(ShadowSlot) == 24, "ShadowSlot layout");

struct AerialLut
{
    const float* luminance; // nullptr = exact composite
    unsigned W, H, D;
    float maxDistance;
};

// The rows of a draw that this rank owns (szg_rowtile), as resolve_tile (api_core.cpp) hands them to every launch function.
// `local_rows` is the number of rows this rank draws; resolve_tile sets it to the draw height for a single rank.
struct TileArgs
{
    unsigned block_rows, rank, nranks, local_rows;
};

// Transmittance LUT block: W*H RGBA32F texels followed by ONE status dword (16 bytes reserved). The dword is 0 when
// every texel's rgb lies in [2^-50, 2] — the operand domain in which the march may use the lean exact division for
// transmittance ratios (szg_atmosphere.hpp TLut::moderate). launch_transmittance maintains it; launch_lut_range recomputes
// it for texels written by the caller. Every kernel that takes `tlut` reads the dword behind the texels.
inline size_t tlut_block_bytes(unsigned W, unsigned H) { return (size_t)W * H * 16u + 16u; }
hipError_t launch_lut_range(hipStream_t s, float* lut, unsigned W, unsigned H);
// `d_dirty` (may be nullptr): LUT reuse flag written by launch_lut_key; the kernel returns at once when it reads 0.
hipError_t launch_transmittance(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, float* lut, unsigned W,
                                unsigned H, const unsigned* d_dirty = nullptr);
// LUT reuse across frames ("cache the LUTs across frames when atmosphere / sun / camera altitude are unchanged
// (allowed because results are identical)"; the reference recomputes both every frame, skyview.cpp:799-893). The parameter
// blocks live in device memory, so the comparison runs on the device, in stream order, with no host round trip: k_lut_key
// (one wave) compares the atmosphere block (and, for the sky-view LUT, the camera position and the generation of the
// transmittance LUT) bit for bit with what the texels were computed from, records the verdict in state[69 + which] and, when
// dirty, stores the new key and clears the LUT's status dword. The LUT kernel launched behind it exits at once on a clean
// verdict. LUT_KEY_DWORDS dwords of state, zeroed at creation; `force` = the host knows the texels are stale (first use,
// texels handed out for writing, a row-slice launch, an explicit invalidate).
constexpr unsigned LUT_KEY_DWORDS = 72u;
constexpr unsigned SLUT_STATUS_RANKS = 64u; // most ranks szg_skyview_allgather_lut_rows exchanges slice status words of
hipError_t launch_lut_key(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                          unsigned camIndex, unsigned* d_state, unsigned which, bool force, float* lutBlock, unsigned W, unsigned H);
// Sky-view LUT block: W*H RGBA32F texels followed by ONE status dword (16 bytes reserved): 0 when every texel's rgb is a
// finite number of moderate size (|x| <= 2^100). The composite consults it before it leaves a sample of this LUT unevaluated
// (the reflection term of a non-metal pixel is an exact zero only if the sample is finite). launch_skyview over all rows
// maintains it; after a partial launch (row slices of the multi-GPU path, completed by an all-gather) or a write by the
// caller, launch_slut_check recomputes it from the texels.
inline size_t slut_block_bytes(unsigned W, unsigned H) { return (size_t)W * H * 16u + 16u; }
hipError_t launch_slut_check(hipStream_t s, float* lut, unsigned W, unsigned H);
// The N-rank form of the same: the status of this rank's slice goes into d_all[rank] (1 when `known` is false), the caller
// all-gathers d_all (4 bytes per rank), and the LUT's status dword becomes the OR of the nranks words.
hipError_t launch_slut_status_stage(hipStream_t s, unsigned* d_all, unsigned rank, const float* lut, unsigned W, unsigned H, bool known);
hipError_t launch_slut_status_reduce(hipStream_t s, const unsigned* d_all, unsigned nranks, float* lut, unsigned W, unsigned H);
hipError_t launch_skyview(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                          unsigned camIndex, const float* tlut, unsigned tW, unsigned tH, float* lut, unsigned W, unsigned H,
                          unsigned rowBegin, unsigned rowEnd, const unsigned* d_dirty, const void* d_prep);
// Per-frame constants (szg_atmosphere.hpp FramePrep): one-lane kernel in front of the sky-view LUT kernel and the composite, which
// read `d_prep` (frame_prep_bytes() bytes of device memory) instead of deriving the same ~300 instructions' worth in every wave.
size_t frame_prep_bytes();
// `d_sun` (may be null): the directional light whose shadow map the composite samples; its TO_TEX * projection * view goes into
// the block (FramePrep::sunShadow). `d_cam` (may be null), `camIndex`, `drawW`, `drawH`: the composite's camera and draw extent;
// what phase A derives from them and the atmosphere alone goes into the block (FramePrep::Camera).
hipError_t launch_frame_prep(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, unsigned tW, unsigned tH, void* d_prep,
                             const szg_directional_light_packed* d_sun = nullptr, const szg_camera_packed* d_cam = nullptr,
                             unsigned camIndex = 0u, unsigned drawW = 0u, unsigned drawH = 0u);
hipError_t launch_composite(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                            const szg_gbuffer& g, ShadowSlot sunSlot, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                            unsigned camIndex, const szg_directional_light_packed* d_dir, unsigned sunIndex, const float* tlut,
                            unsigned tW, unsigned tH, const float* slut, unsigned sW, unsigned sH, AerialLut aerial, const void* d_prep);
hipError_t launch_aerial_lut(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const szg_camera_packed* d_cam,
                             unsigned camIndex, const float* tlut, unsigned tW, unsigned tH, float* luminance, float* transmittance,
                             unsigned W, unsigned H, unsigned D, float maxDistance);
hipError_t launch_multiscatter(hipStream_t s, const szg_atmosphere_packed* d_atm, unsigned atmIndex, const float* tlut, unsigned tW,
                               unsigned tH, float* out, unsigned dim);
// launch_skyview / launch_aerial_lut with the multi-scattering term of include/szg/multiscatter_sky.h in the march
// (kernels_lut_ms.hip). `mode`: SZG_MULTISCATTER_ADD or _ONLY (anything else: hipErrorInvalidValue); `psi`: the
// SZG_MULTISCATTER_DIM^2 RGBA32F texels of the multi-scattering LUT.
hipError_t launch_skyview_ms(hipStream_t s, unsigned mode, const szg_atmosphere_packed* d_atm, unsigned atmIndex,
                             const szg_camera_packed* d_cam, unsigned camIndex, const float* tlut, unsigned tW, unsigned tH,
                             const float* psi, float* lut, unsigned W, unsigned H, unsigned rowBegin, unsigned rowEnd,
                             const unsigned* d_dirty, const void* d_prep);
hipError_t launch_aerial_lut_ms(hipStream_t s, unsigned mode, const szg_atmosphere_packed* d_atm, unsigned atmIndex,
                                const szg_camera_packed* d_cam, unsigned camIndex, const float* tlut, unsigned tW, unsigned tH,
                                const float* psi, float* luminance, float* transmittance, unsigned W, unsigned H, unsigned D,
                                float maxDistance);

// ---- deferred lights pass (kernels_lights.hip) ----
hipError_t launch_light_prep(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount, unsigned dirSkip,
                             const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_slots,
                             unsigned slotCount, LightRec* d_out);
hipError_t launch_lights(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                         const szg_gbuffer& g, const szg_camera_packed* d_cam, unsigned camIndex, const LightRec* d_lights,
                         unsigned lightCount, const unsigned long long* d_tileMasks);
// Per 64 x 64 tile of the local image and per 64 lights one word into `d_tileMasks` (lightTileMaskWords() of
// szg_light_tiles.hpp sizes it): bit set = k_lights has to visit the light in that tile. launch_lights reads the words when it
// is handed them (nullptr: every light is visited).
hipError_t launch_light_tiles(hipStream_t s, unsigned drawW, unsigned drawH, TileArgs tile, const szg_gbuffer& g,
                              const LightRec* d_lights, unsigned lightCount, unsigned long long* d_tileMasks);

// ---- analytic scene: G-buffer fill and shadow maps (kernels_scene_fill.hip) ----
hipError_t launch_gbuffer_fill(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                               const szg_gbuffer& g, const szg_camera_packed* d_cam, unsigned camIndex, float ground_y,
                               float ground_half_extent, float checker_cell, float ground_roughness,
                               const szg_fill_box* d_boxes, unsigned boxCount);
// Per-slot state for shadow-map generation, built on the device by k_shadow_prep.
struct ShadowGen
{
    float projView[16];
    float invProjView[16];
    float* map; // nullptr = skip
    unsigned dim, pitchFloats, pad;
};
hipError_t launch_shadow_maps(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount,
                              const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_ownedSlots,
                              unsigned slotCount, ShadowGen* d_gen, const szg_fill_box* d_boxes, unsigned boxCount, unsigned maxDim);
hipError_t launch_shadow_prep(hipStream_t s, const szg_directional_light_packed* d_dir, unsigned dirCount,
                              const szg_spot_light_packed* d_spot, unsigned spotCount, const ShadowSlot* d_ownedSlots,
                              unsigned slotCount, ShadowGen* d_gen);

// ---- OETF pass (kernels_oetf.hip) ----
// `table`: 65536 x u16, the OETF of every UNORM16 channel value (launch_oetf_table fills it)
hipError_t launch_oetf_table(hipStream_t s, unsigned short* table, unsigned function);
hipError_t launch_oetf(hipStream_t s, const szg_image& image, unsigned width, unsigned height, const unsigned short* table);

// ---- multi-GPU row-tile compose copy (kernels_rowtile.hip) ----
hipError_t launch_compose_rowtiles(hipStream_t s, const void* gathered, size_t tileStrideBytes, unsigned nranks,
                                   unsigned blockRows, const szg_image& dst, unsigned width, unsigned height);

// ---- compute rasteriser (kernels_raster.hip, include/szg/raster.h) ----
// One vkCmdDrawIndexed of the reference (one surface of one mesh, all its instances), uploaded by the host.
// alignas(128) pads the 172 bytes of fields to sizeof == 256, a power of two (128 B before the mip fields), so that indexing
// the record remains a shift and k_raster_tile<false> keeps the register figures it had. Records are
// value-initialised on the host (collect_draws), so the 84 bytes of tail padding that are uploaded per draw are zeros.
struct alignas(128) RasterDraw
{
    const szg_vertex_packed* vertices;
    const uint32_t* indices;
    const szg_mat4* models;
    const szg_mat4* mits;
    uint32_t vertexCount, firstIndex, triCount, instanceCount;
    uint32_t firstPrim; // submission-order number of this draw's first primitive (instance-major, then triangle)
    uint32_t pad;
    szg_texture tex[3]; // color, normal, ORM (offscreen.frag:19-21)
    // szg/mipmaps.h: the chain registered for each map (nullptr / 1 = none) and the sampler's maxLod; read by k_raster_tile<true> only
    const void* mipChain[3];
    uint32_t mipLevels[3];
    float maxLod;
    // szg/anisotropy.h: the sampler's maxAnisotropy (1..16); read by k_raster_tile_aniso only
    float maxAnisotropy;
};
static_assert(sizeof(RasterDraw) == 256, "RasterDraw layout");
// One assembled primitive: signed homogeneous edge functions + clip z, w per vertex (raster.h "coverage", "depth").
struct PrimRec
{
    float a[3], b[3], c[3];
    float z[3], w[3];
    uint32_t draw, instance, tri;
    // where |e_i| <= noise[i] the sign comes from the exact determinant of the h values (hw is w); noise < 0: never
    float hx[3], hy[3], noise[3];
    float facing; // +1 front, -1 back: the factor a, b, c carry
};
static_assert(sizeof(PrimRec) == 112, "PrimRec layout");
// Device buffers of one raster pass, owned by the pipeline and grown on demand (api_raster.cpp).
struct RasterBuffers
{
    PrimRec* prims = nullptr;       // [capacity] submission order
    uint2* boxes = nullptr;         // [capacity] pixel boxes, submission order (x: min | max << 16, y likewise)
    unsigned* keysA = nullptr;      // [capacity] sort keys / scratch
    unsigned* keysB = nullptr;
    unsigned* valsA = nullptr;      // [capacity] identity order
    unsigned* valsB = nullptr;      // [capacity] sorted order
    uint2* orderedBoxes = nullptr;  // [capacity] boxes in walk order
    uint2* chunkBoxes = nullptr;    // [capacity / 64]
    uint2* superBoxes = nullptr;    // [capacity / 4096 + 1]
    void* sortTemp = nullptr;
    size_t sortTempBytes = 0;
    const unsigned* order = nullptr; // valsA or valsB: set by launch_raster_setup
    size_t capacity = 0;
};
// above this many primitives the boxes are radix-sorted (size class, Morton code) before the hierarchy is built
constexpr unsigned RASTER_SORT_THRESHOLD = 4096u;
// kernels_raster_sort.hip (rocPRIM): temp-storage size for `n` pairs, and the sort itself
hipError_t raster_sort_temp_bytes(unsigned n, size_t& bytes);
hipError_t raster_sort_pairs(hipStream_t s, void* temp, size_t tempBytes, const unsigned* keysIn, unsigned* keysOut,
                             const unsigned* valsIn, unsigned* valsOut, unsigned n);
hipError_t launch_raster_setup(hipStream_t s, bool shadow, const RasterDraw* d_draws, unsigned drawCount, unsigned primCount,
                               const szg_camera_packed* d_cam, unsigned camIndex, const ShadowGen* d_gen, unsigned W, unsigned H,
                               RasterBuffers& b);
hipError_t launch_raster_tile(hipStream_t s, const szg_scene_texture& scene, unsigned drawW, unsigned drawH, TileArgs tile,
                              const szg_gbuffer& g, const RasterDraw* d_draws, const RasterBuffers& b, unsigned primCount,
                              const szg_camera_packed* d_cam, unsigned camIndex, bool mips, bool aniso);
// ---- mip chains (kernels_mipmaps.hip, include/szg/mipmaps.h): arguments already validated ----
hipError_t launch_generate_mipmaps(hipStream_t s, const szg_texture& level0, void* d_chain);
hipError_t launch_shadow_tile(hipStream_t s, const ShadowGen* d_gen, unsigned dim, const RasterBuffers& b, unsigned primCount,
                              float biasConstant, float biasSlope);

// ---- debug-line pass (kernels_debuglines.hip, include/szg/debuglines.h) ----
// One line after setup: viewport endpoints, the coverage terms of the header, and its major-axis pixel range.
struct DebugLineRec
{
    float xa, ya, xb, yb;
    float dx, dy, L2, w2; // coverage terms (w2 = line_width * line_width)
    float half;           // minor-axis candidate half-width around the centre line (pixels)
    float slope;          // d_minor / d_major
    int first;            // first major-axis pixel of the clamped range
    unsigned major;       // 0: x-major, 1: y-major
};
static_assert(sizeof(DebugLineRec) == 48, "DebugLineRec layout");
// Device scratch of one pipeline object, sized at creation from its vertex capacity (api_debuglines.cpp).
struct DebugLineBuffers
{
    DebugLineRec* recs = nullptr;          // [lines]
    unsigned long long* steps = nullptr;   // [lines + 1] step counts, last = 0
    unsigned long long* offsets = nullptr; // [lines + 1] exclusive scan; offsets[lines] = total
    void* scanTemp = nullptr;
    size_t scanTempBytes = 0;
};
hipError_t debug_lines_scan_temp_bytes(unsigned lineCapacity, size_t& bytes);
hipError_t launch_debug_lines(hipStream_t s, const szg_scene_texture& scene, unsigned W, unsigned H, TileArgs tile,
                              const szg_camera_packed* d_cam, unsigned camIndex, const szg_vertex_packed* d_vertices,
                              unsigned lineCount, float lineWidth, DebugLineBuffers& b);

// ---- present pass (kernels_present.hip, include/szg/present.h) ----
// Arguments already validated; `table` is the OETF table of info.encode, or nullptr for SZG_PRESENT_ENCODE_NONE.
hipError_t launch_present(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_present_info& info,
                          const unsigned short* table);

// ---- image copy and clear of the texture viewer (kernels_image_copy.hip, include/szg/texture_display.h) ----
// rows a lane of k_image_copy / k_image_clear walks with the column setup it made once
constexpr unsigned IMAGE_COPY_ROWS_PER_LANE = 8u;
// Arguments already validated (api_texture_display.cpp); regions without texels launch nothing.
hipError_t launch_image_copy(hipStream_t s, const szg_image& src, const szg_image& dst, const szg_rect& srcRegion, const szg_rect& dstRegion);
hipError_t launch_image_clear(hipStream_t s, const szg_image& image, const float color[4]);

// ---- UI layer pass (kernels_ui_layer.hip, include/szg/ui_layer.h) ----
// One ImDrawCmd that can draw, as the host resolved it (api_ui_layer.cpp): the texture and sampler its handle names, the
// pixel box scissor ∩ viewport ∩ render area ∩ image, and its triangles after ASSEMBLY's truncation. Read through scalar loads.
struct UICommand
{
    const void* texData;
    unsigned texWidth, texHeight, texPitch;
    // low half: UI_TEX_RGBA8_UNORM / UI_TEX_RGBA16_UNORM / UI_TEX_RGBA16_SFLOAT; high half: the view's four 3-bit swizzles
    // (szg/texture_display.h MAPPING), slot i at bit 16 + 3 i. A szg_ui_layer_add_texture handle gives 0 or 1, as ever.
    unsigned texFormat;
    unsigned filter, address;
    int clip[4];     // x0, y0, x1, y1 (exclusive)
    unsigned vtxOffset, firstIndex, triCount;
    unsigned firstTri; // submission-order number of the command's first triangle
};
static_assert(sizeof(UICommand) == 64, "UICommand layout");
constexpr unsigned UI_TEX_RGBA8_UNORM = 0u, UI_TEX_RGBA16_UNORM = 1u, UI_TEX_RGBA16_SFLOAT = 2u;
// One triangle after setup, sign-normalised (everything multiplied by s = sign(det)): the edge functions at the centre of
// pixel (0, 0) and their steps per pixel, exact; which edges are left or top; the attributes, vertex i opposite edge i.
struct UIPrim
{
    long long e0[3]; // s E_i at C = (128, 128)
    long long ex[3]; // s E_i(px + 1, py) - s E_i(px, py) = 256 s a_i
    long long ey[3]; // 256 s b_i
    float det;       // float(|det|)
    unsigned topLeft; // bit i: edge i owns its zero
    unsigned command;
    unsigned box[2]; // the pixel box, as in UILayerBuffers::boxes
    unsigned pad;
    float u[3], v[3], r[3], g[3], b[3], a[3];
};
static_assert(sizeof(UIPrim) == 168, "UIPrim layout");
// Device scratch of one layer, sized at creation (api_ui_layer.cpp). A box is x: min | max << 16, y likewise, max exclusive;
// the empty box is min = 0xFFFF, max = 0.
struct UILayerBuffers
{
    UICommand* commands = nullptr; // [commandCapacity]
    UIPrim* prims = nullptr;       // [triangleCapacity] submission order
    uint2* boxes = nullptr;        // [triangleCapacity rounded up to 64]
    uint2* chunkBoxes = nullptr;   // [boxes / 64, rounded up to 64]: 64 consecutive triangles
    uint2* superBoxes = nullptr;   // [chunkBoxes / 64]: 64 consecutive chunks
};
struct UIDrawParams
{
    float displayPos[2], scale[2];
    const szg_ui_draw_vert* vertices;
    const uint16_t* indices;
    unsigned vertexCount, commandCount, triCount;
};
// Arguments already validated. `area`: render area ∩ image, not empty. commands[0..commandCount) are in b.commands already
// (uploaded on `s`).
hipError_t launch_ui_layer(hipStream_t s, const szg_image& output, szg_rect area, bool clear, const float clearColor[4],
                           const UIDrawParams& draw, const UILayerBuffers& b);

// ---- compute-collection pipeline (kernels_compute_collection.hip, include/szg/compute_collection.h) ----
// A push-constant block as the kernels take it, by value: the largest of the four (matrix_color), zero-filled behind the
// bytes of a smaller one.
struct alignas(16) CCBlock
{
    unsigned w[SZG_COMPUTE_COLLECTION_MAX_BLOCK_BYTES / 4u];
};
static_assert(sizeof(CCBlock) == SZG_COMPUTE_COLLECTION_MAX_BLOCK_BYTES, "CCBlock layout");
// Arguments already validated; `block` carries drawOffset = 0 and drawExtent = (width, height) in its first 16 bytes.
hipError_t launch_compute_collection(hipStream_t s, unsigned shaderIndex, const CCBlock& block, const szg_image& color, unsigned width,
                                     unsigned height);
} // namespace szg
