/*
 * szg/compute_collection.h — C-ABI of the compute-collection pipeline: the COMPUTE_COLLECTION branch of
 * Renderer::recordDraw (renderer/renderer.cpp:431-438), which hands the scene colour to
 *
 *   ComputeCollectionPipeline                       renderer/pipelines.hpp:166-235, pipelines.cpp:223-368
 *     "a generic compute pipeline driven entirely by a push constant": one of four small compute shaders, chosen at run
 *     time, in this order (renderer.cpp:238-243):
 *       0 booleanpush            shaders/booleanpush.comp
 *       1 gradient_color         shaders/gradient_color.comp
 *       2 sparse_push_constant   shaders/sparse_push_constant.comp
 *       3 matrix_color           shaders/matrix_color.comp
 *     All four: workgroup 16 x 16, one rgba16 storage image at set 0 binding 0, a push-constant block that begins with
 *     `vec2 drawOffset; vec2 drawExtent;`.
 *
 * rebuilt as HIP kernels (syzygy_amd/csrc/kernels_compute_collection.hip). The collection is the reference's fixed four:
 * arbitrary shader binaries are not loaded. The parameters of a program are a REFLECTED BYTE BLOCK, not a typed struct;
 * szg_compute_collection_reflect() gives the table a front end builds its controls from (what
 * ShaderReflectionData::PushConstant gives the editor, ui/pipelineui.cpp:42-, :382).
 *
 * The CPU model is tests/compute_collection_model.py; tests/golden/compute_collection_vectors.npz pins it to the
 * reference's committed SPIR-V: booleanpush, gradient_color and sparse_push_constant for every invocation, matrix_color
 * for the invocations inside the draw extent (see MATRIX). Every floating-point operation named below is ONE IEEE binary32
 * operation, rounded to nearest even, never fused with its neighbour. The site belongs to NO class of szg/contraction.h:
 * libszg_hip.so and libszg_hip_literal.so write the same bytes (most of the time goes into the stores; fusing buys nothing
 * that would be worth a second set of bytes).
 *
 * BLOCKS      byte layout of the four push-constant blocks; every block starts with drawOffset (vec2, 0) and drawExtent
 *             (vec2, 8). A bool is a 32-bit word, true = non-zero. Matrices are column-major, column stride 16.
 *               booleanpush           80 B   row1, row2, row3, row4 = bvec4 at 16, 32, 48, 64
 *               gradient_color        48 B   topColor, bottomColor = vec4 at 16, 32
 *               sparse_push_constant  80 B   topRG, topBA, bottomRG, bottomBA = vec2 at 16, 32, 48, 64, 8 bytes of padding
 *                                            after each (never read)
 *               matrix_color         208 B   red, green, blue = mat4 at 16, 80, 144
 *
 * RECORD      pipelines.cpp:291-368. The caller's bytes are copied at record time (push-constant semantics: the caller
 *             may change its buffer right after the call) and THE FIRST 16 BYTES ARE OVERWRITTEN with drawOffset = (0, 0)
 *             and drawExtent = (float(width), float(height)) (:330-344): whatever the caller wrote there is ignored. Kept
 *             from the reference on purpose. The objects above this call start every block as zeros (:255-257), as the
 *             reference does: transparent black in gradient_color and sparse_push_constant, opaque black in
 *             matrix_color (its alpha is the constant 1).
 *
 * DISPATCH    ceil(width / 16) x ceil(height / 16) groups of 16 x 16 invocations (:360-367). Invocation (x, y) owns texel
 *             (x, y) (texelCoord = ivec2(vec2(gid) + drawOffset), drawOffset = 0) and its store is guarded BY THE IMAGE
 *             SIZE, NOT BY THE EXTENT. So the pass writes every texel of
 *               [0, min(ceil16(width), image.width)) x [0, min(ceil16(height), image.height))
 *             with ceil16(n) = n rounded up to a multiple of 16: up to 15 columns and rows beyond the draw extent (the
 *             "spill") whenever the scene texture is larger than the subregion (it is 4096 x 4096 in the reference). This is
 *             the reference's behaviour and is kept on purpose. Every byte outside that set, pitch padding included, keeps
 *             its value.
 *
 * UV          u = (float(x) + 0.5f) / float(width), v = (float(y) + 0.5f) / float(height): one addition (exact) and one
 *             division each. In the spill u or v exceeds 1.
 *
 * CELL        cx = int(u * 4.0f), cy = int(v * 4.0f): one multiplication, then truncation. With extents up to
 *             SZG_COMPUTE_COLLECTION_MAX_EXTENT, (k + 0.5) / n < 1 and u * 4 < 4 hold in binary32 for every texel inside
 *             the extent, so cx, cy are 0..3 there; in the spill they reach 4 and more (up to 63).
 *
 * MIX         mix(p, q, a) = p * (1 - a) + q * a: (1 - a), both products and the sum are separately rounded: four
 *             roundings (this library's convention for GLSL's mix, the one its SPIR-V interpreter executes for FMix).
 *
 * GRADIENT    gradient_color: texel channel c = mix(topColor[c], bottomColor[c], v), four channels.
 *             sparse_push_constant: the same with top = (topRG, topBA), bottom = (bottomRG, bottomBA).
 *             Beyond the extent v > 1 extrapolates; the store clamps.
 *
 * MATRIX      matrix_color: (red[cy][cx], green[cy][cx], blue[cy][cx], 1): column cy, row cx of the three matrices, the
 *             float at byte base + 16 * cy + 4 * cx. In the spill cx or cy is 4 or more, an index outside the matrix, which
 *             Vulkan leaves undefined. THIS LIBRARY'S CONVENTION: BOTH INDICES ARE CLAMPED TO 3. (The SPIR-V pin therefore
 *             covers matrix_color inside the extent only.)
 *
 * BOOLEAN     booleanpush: base = white (1, 1, 1, 1) or black (0, 0, 0, 1) by word cx % 4 of row (cy + 1) when cy is
 *             0..3, RED (1, 0, 0, 1) when cy is outside 0..3 (only in the spill rows); the texel is
 *             base * (u, v, 0, 1), four multiplications.
 *
 * STORE       the library's UNORM16 store: clamp to [0, 1] (NaN -> 0), multiply by 65535, round to nearest even; channels
 *             R, G, B, A as four little-endian 16-bit codes, 8 B per texel.
 *
 * Row tiles (szg_rowtile) are not supported by this pass: it always writes the whole set above on one device.
 * HBM traffic: 8 B written per texel, nothing read.
 */
#ifndef SZG_COMPUTE_COLLECTION_H
#define SZG_COMPUTE_COLLECTION_H

#include "szg/abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SZG_COMPUTE_COLLECTION_SHADER_COUNT 4u
#define SZG_COMPUTE_COLLECTION_MAX_EXTENT 16384u /* = SZG_PRESENT_MAX_EXTENT */
#define SZG_COMPUTE_COLLECTION_MAX_BLOCK_BYTES 208u
#define SZG_COMPUTE_COLLECTION_PREFIX_BYTES 16u /* drawOffset + drawExtent, overwritten at record time */
#define SZG_COMPUTE_COLLECTION_MAX_MEMBERS 6u
#define SZG_COMPUTE_COLLECTION_WORKGROUP 16u

/* renderer.cpp:238-243 */
#define SZG_CC_BOOLEANPUSH 0u
#define SZG_CC_GRADIENT_COLOR 1u
#define SZG_CC_SPARSE_PUSH_CONSTANT 2u
#define SZG_CC_MATRIX_COLOR 3u

/* component type of a member */
#define SZG_CC_COMPONENT_FLOAT 0u
#define SZG_CC_COMPONENT_BOOL 1u /* a 32-bit word, true = non-zero */

/* One member of a push-constant block (ShaderReflectionData::Member) */
typedef struct szg_cc_member
{
    const char* name;           /* static storage */
    uint32_t offset_bytes;
    uint32_t size_bytes;
    uint32_t padded_size_bytes; /* distance to the next member, or to the end of the block */
    uint32_t component_type;    /* SZG_CC_COMPONENT_* */
    uint32_t vector_width;      /* components of a vector / rows of a matrix column: 2 or 4 */
    uint32_t column_count;      /* 1 for vectors, 4 for mat4 */
} szg_cc_member;

/* ShaderReflectionData::PushConstant of one program, plus what the four have in common */
typedef struct szg_cc_reflection
{
    const char* name;             /* "booleanpush", ...; static storage */
    uint32_t size_bytes;          /* of the block */
    uint32_t padded_size_bytes;   /* what szg_record_compute_collection takes as byte_count (= size_bytes in all four) */
    uint32_t layout_offset_bytes; /* 0 in all four */
    uint32_t local_size[3];       /* 16, 16, 1 */
    uint32_t member_count;        /* drawOffset and drawExtent included */
    szg_cc_member members[SZG_COMPUTE_COLLECTION_MAX_MEMBERS];
} szg_cc_reflection;

/* Host only, no device needed. */
uint32_t szg_compute_collection_shader_count(void);
/* SZG_ERR_INVALID_ARGUMENT for index >= the shader count or a NULL `out`. */
int szg_compute_collection_reflect(uint32_t index, szg_cc_reflection* out);

/* Enqueue program `shader_index` over the top-left width x height texels of `color` (plus the spill, DISPATCH above) on
 * `stream` and return. Stateless. `push_constant_bytes` is a HOST pointer to `byte_count` bytes, copied before the call
 * returns; their first 16 are ignored (RECORD above). SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, nothing
 * launched, nothing written) for: a NULL bytes, image or data pointer; shader_index >= 4; a byte_count other than the
 * program's padded block size; a colour image that is not RGBA16_UNORM, whose pitch is smaller than a row or not a
 * multiple of 8, or whose data is not 8-byte aligned; an empty extent or one that leaves the image; an image extent above
 * SZG_COMPUTE_COLLECTION_MAX_EXTENT. */
int szg_record_compute_collection(void* stream, uint32_t shader_index, const void* push_constant_bytes, uint32_t byte_count,
                                  const szg_image* color, uint32_t width, uint32_t height);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_COMPUTE_COLLECTION_H */
