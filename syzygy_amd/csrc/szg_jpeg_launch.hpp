// szg_jpeg_launch.hpp — launch interface between api_jpeg.cpp and kernels_jpeg.hip (include/szg/jpeg.h). Not part of the
// public boundary.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace szg
{
struct JpegPlaneArgs
{
    const int16_t* coefficients; // rule 2 layout, 16-byte aligned
    uint8_t* samples;            // this plane's part of the scratch, pitch blocksW * 8
    unsigned blocksW, blocksH;
    unsigned groupsX; // ceil(blocksW / 8): groups of 8 horizontally adjacent blocks, one wave each
    unsigned hs, vs;  // rule 4
    unsigned ch, wl;
};
struct JpegArgs
{
    JpegPlaneArgs plane[3];
    unsigned planeCount, width, height;
    unsigned ycbcr; // 1: rule 5's conversion; 0: the samples are R, G, B (or one grey plane)
    unsigned rgbaAnd, rgbaOr;
    uint8_t* dst;
    unsigned dstPitch;
};
// k_jpeg_idct over every plane, then k_jpeg_color; arguments already validated
hipError_t launch_jpeg_reconstruct(hipStream_t s, const JpegArgs& args);
} // namespace szg
