// szg_pixel.hpp — how the full-screen passes address their pixels, each rule stated once: the row of an image, the five
// G-buffer planes as one kernel argument, the workgroup's pixel mapping, and the grid that goes with it.
#pragma once

#include <hip/hip_runtime.h>

#include "szg/abi.h"
#include "szg_vec.hpp"

namespace szg
{
template <typename T> SZG_DEV T* row_ptr(const szg_image& im, unsigned y)
{
    return reinterpret_cast<T*>(static_cast<unsigned char*>(im.data) + (size_t)y * im.pitch_bytes);
}

struct GBufferPtrs
{
    szg_image diffuse, specular, normal, position, orm;
};
inline GBufferPtrs gptrs(const szg_gbuffer& g)
{
    return GBufferPtrs{g.diffuse, g.specular, g.normal, g.worldPosition, g.occlusionRoughnessMetallic};
}

// 256-thread workgroup = 32x8 pixels; each wave an 8x8 patch. Functions of the thread index, so that a kernel may address
// its pixel a second time from a copy of the index the compiler cannot see through (k_composite, phase C).
constexpr unsigned PIXEL_GROUP_W = 32u, PIXEL_GROUP_H = 8u;
// (from the wave and lane numbers, for a kernel that holds the wave number anyway: k_composite, whose diagnostic build stamps per wave)
SZG_DEV unsigned pixel_column(unsigned wave, unsigned lane) { return blockIdx.x * PIXEL_GROUP_W + wave * 8u + (lane & 7u); }
SZG_DEV unsigned pixel_column(unsigned tid) { return pixel_column(tid >> 6, tid & 63u); }
SZG_DEV unsigned pixel_row(unsigned tid) { return blockIdx.y * PIXEL_GROUP_H + ((tid & 63u) >> 3); }
// The same tiling with the rows walked from the bottom of the image upwards (workgroups are dispatched in blockIdx order):
// the cheap workgroups - background texels, sky, at the top of most frames - then come last and fill the tail of the launch.
// pixel_group_bottom_up() is the workgroup's place in that walk: its first row is PIXEL_GROUP_H times that.
SZG_DEV unsigned pixel_group_bottom_up() { return gridDim.y - 1u - blockIdx.y; }
SZG_DEV unsigned pixel_row_bottom_up(unsigned tid) { return pixel_group_bottom_up() * PIXEL_GROUP_H + ((tid & 63u) >> 3); }
// Both coordinates of this thread's pixel through one call, as the lights pass and the analytic fills have always taken them.
// They keep this form because the compiler builds their bounds test `x >= W || y >= rows` another way when the coordinates
// arrive as two returned values: the same results from other machine code (profiles/kernel_units_split.md).
SZG_DEV void pixel_of_thread(unsigned& x, unsigned& y)
{
    unsigned const tid = threadIdx.x;
    x = pixel_column(tid);
    y = pixel_row(tid);
}
SZG_DEV void pixel_of_thread_bottom_up(unsigned& x, unsigned& y)
{
    unsigned const tid = threadIdx.x;
    x = pixel_column(tid);
    y = pixel_row_bottom_up(tid);
}

// the grid of such workgroups over `width` x `rows` pixels
inline dim3 pixel_grid(unsigned width, unsigned rows, unsigned layers = 1u)
{
    return dim3((width + PIXEL_GROUP_W - 1u) / PIXEL_GROUP_W, (rows + PIXEL_GROUP_H - 1u) / PIXEL_GROUP_H, layers);
}
} // namespace szg
