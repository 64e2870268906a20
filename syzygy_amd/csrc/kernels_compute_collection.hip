// kernels_compute_collection.hip — the compute-collection pipeline (include/szg/compute_collection.h): the four programs
// of ComputeCollectionPipeline (renderer/pipelines.cpp:223-368; shaders/booleanpush.comp, gradient_color.comp,
// sparse_push_constant.comp, matrix_color.comp), each a pure function of the texel coordinate and a push-constant block,
// stored to the RGBA16_UNORM scene colour. The rule (UV, CELL, MIX, GRADIENT, MATRIX, BOOLEAN, STORE, the spill beyond the
// draw extent) is stated in the header; the CPU model is tests/compute_collection_model.py. Nothing here belongs to a
// contraction class: both libraries compile the same code (-ffp-contract=off keeps every operation on its own).
//
// The block travels BY VALUE as a kernel argument: the kernarg segment is HIP's push constant, and the copy made at launch
// is the record-time copy the push-constant semantics ask for. Indexing it with a run-time index reads the kernarg segment
// (constant address space), not a private copy: no scratch.
//
// One kernel template over the four programs, pure streaming, 8 B per texel written and nothing read. A lane owns 2
// adjacent texels (16 B) of ROWS_PER_LANE rows: what depends on the column (u, the cell column) is computed once per lane,
// what depends on the row (v, the cell row, the gradient's colour) once per row, wave-uniform. As in kernels_present.hip the
// texel pairs are formed by ADDRESS: pair g covers the 16 aligned bytes counted from the 16-B boundary at or below the
// image's first texel, so that a full pair is one aligned 16-B store; a pair that straddles the left or right edge of the
// written set, or a row whose pitch moves it off the 16-B grid, takes one predicated 8-B store per texel.
#include "szg_formats.hpp"
#include "szg_launch.hpp"
#include "szg_vec.hpp"

#include "szg/compute_collection.h"

namespace szg
{
namespace
{
constexpr unsigned ROWS_PER_LANE = 4u; // 2 and 4 measure alike, 8 and 16 slower (fewer waves): DESIGN.md §10

// dword indices into the block (header, BLOCKS)
constexpr unsigned DW_EXTENT = 2u;  // drawExtent at byte 8
constexpr unsigned DW_MEMBERS = 4u; // first member at byte 16

SZG_DEV float block_float(const CCBlock& pc, unsigned dword) { return __uint_as_float(pc.w[dword]); }

// MIX of the header: four roundings
SZG_DEV float mix4(float p, float q, float a, float oneMinusA) { return p * oneMinusA + q * a; }

template <unsigned PROG>
__global__ __launch_bounds__(256) void k_compute_collection(CCBlock pc, unsigned char* __restrict__ dst, unsigned pitch, unsigned cols,
                                                            unsigned rows)
{
    unsigned const lead = ((unsigned)reinterpret_cast<uintptr_t>(dst) & 15u) >> 3; // 0 or 1 texels in front of column 0
    int const c0 = (int)(2u * (blockIdx.x * 256u + threadIdx.x)) - (int)lead;       // -1 only for the first pair
    if (c0 >= (int)cols)
    {
        return;
    }
    bool const full = c0 >= 0 && (unsigned)c0 + 2u <= cols;
    float const extentX = block_float(pc, DW_EXTENT), extentY = block_float(pc, DW_EXTENT + 1u);

    // per column, once per lane (a column outside the written set is computed and never stored)
    float u[2];
    unsigned cx[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        int const c = max(c0 + i, 0);
        u[i] = ((float)c + 0.5f) / extentX; // UV
        cx[i] = (unsigned)(int)(u[i] * 4.0f); // CELL
        if (PROG == SZG_CC_MATRIX_COLOR)
        {
            cx[i] = min(cx[i], 3u); // MATRIX: this library's convention in the spill
        }
        else
        {
            cx[i] &= 3u; // BOOLEAN: cx % 4 (cx >= 0)
        }
    }

    unsigned const yBegin = blockIdx.y * ROWS_PER_LANE;
#pragma unroll
    for (unsigned r = 0; r < ROWS_PER_LANE; r++)
    {
        unsigned const y = yBegin + r;
        if (y >= rows)
        {
            break;
        }
        float const v = ((float)y + 0.5f) / extentY;
        uint2 texel[2];
        if (PROG == SZG_CC_GRADIENT_COLOR || PROG == SZG_CC_SPARSE_PUSH_CONSTANT)
        {
            // GRADIENT: top / bottom at dwords 4..7 / 8..11, or as four vec2 at 4, 8, 12, 16 with their padding skipped
            constexpr bool SPARSE = PROG == SZG_CC_SPARSE_PUSH_CONSTANT;
            constexpr unsigned T0 = 4u, T2 = SPARSE ? 8u : 6u, B0 = SPARSE ? 12u : 8u, B2 = SPARSE ? 16u : 10u;
            float const oneMinusV = 1.0f - v;
            texel[0] = pack_unorm16x4(mix4(block_float(pc, T0), block_float(pc, B0), v, oneMinusV),
                                      mix4(block_float(pc, T0 + 1u), block_float(pc, B0 + 1u), v, oneMinusV),
                                      mix4(block_float(pc, T2), block_float(pc, B2), v, oneMinusV),
                                      mix4(block_float(pc, T2 + 1u), block_float(pc, B2 + 1u), v, oneMinusV));
            texel[1] = texel[0];
        }
        else if (PROG == SZG_CC_MATRIX_COLOR)
        {
            unsigned const cy = min((unsigned)(int)(v * 4.0f), 3u);
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                unsigned const e = DW_MEMBERS + 4u * cy + cx[i]; // column cy, row cx
                texel[i] = pack_unorm16x4(block_float(pc, e), block_float(pc, e + 16u), block_float(pc, e + 32u), 1.0f);
            }
        }
        else
        {
            unsigned const cy = (unsigned)(int)(v * 4.0f);
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                float red = 1.0f, greenBlue = 0.0f; // BOOLEAN: red outside rows 0..3
                if (cy < 4u)
                {
                    red = greenBlue = pc.w[DW_MEMBERS + 4u * cy + cx[i]] != 0u ? 1.0f : 0.0f;
                }
                texel[i] = pack_unorm16x4(red * u[i], greenBlue * v, greenBlue * 0.0f, 1.0f);
            }
        }
        unsigned char* row = dst + (size_t)y * pitch;
        unsigned char* p = row + (ptrdiff_t)c0 * 8;
        if (full && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u)
        {
            *reinterpret_cast<uint4*>(p) = make_uint4(texel[0].x, texel[0].y, texel[1].x, texel[1].y);
        }
        else
        {
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                int const c = c0 + i;
                if (c >= 0 && (unsigned)c < cols)
                {
                    *reinterpret_cast<uint2*>(row + (size_t)c * 8u) = texel[i];
                }
            }
        }
    }
}

template <unsigned PROG>
hipError_t launch_program(hipStream_t s, const CCBlock& block, unsigned char* dst, unsigned pitch, unsigned cols, unsigned rows)
{
    unsigned const pairs = (cols + 1u + 1u) / 2u; // at most 1 leading texel
    dim3 const grid((pairs + 255u) / 256u, (rows + ROWS_PER_LANE - 1u) / ROWS_PER_LANE);
    hipLaunchKernelGGL((k_compute_collection<PROG>), grid, dim3(256), 0, s, block, dst, pitch, cols, rows);
    return hipGetLastError();
}
} // namespace

// Arguments are validated by szg_record_compute_collection (szg_api.cpp); `block` already carries the overwritten prefix.
// The written set (header, DISPATCH) is computed here: the extent rounded up to the workgroup, cut by the image.
hipError_t launch_compute_collection(hipStream_t s, unsigned shaderIndex, const CCBlock& block, const szg_image& color, unsigned width,
                                     unsigned height)
{
    unsigned const g = SZG_COMPUTE_COLLECTION_WORKGROUP;
    unsigned const spillX = (width + g - 1u) / g * g, spillY = (height + g - 1u) / g * g;
    unsigned const cols = spillX < color.width ? spillX : color.width;
    unsigned const rows = spillY < color.height ? spillY : color.height;
    unsigned char* dst = static_cast<unsigned char*>(color.data);
    switch (shaderIndex)
    {
    case SZG_CC_BOOLEANPUSH:
        return launch_program<SZG_CC_BOOLEANPUSH>(s, block, dst, color.pitch_bytes, cols, rows);
    case SZG_CC_GRADIENT_COLOR:
        return launch_program<SZG_CC_GRADIENT_COLOR>(s, block, dst, color.pitch_bytes, cols, rows);
    case SZG_CC_SPARSE_PUSH_CONSTANT:
        return launch_program<SZG_CC_SPARSE_PUSH_CONSTANT>(s, block, dst, color.pitch_bytes, cols, rows);
    case SZG_CC_MATRIX_COLOR:
        return launch_program<SZG_CC_MATRIX_COLOR>(s, block, dst, color.pitch_bytes, cols, rows);
    default:
        return hipErrorInvalidValue;
    }
}
} // namespace szg
