// kernels_jpeg.hip — the device half of include/szg/jpeg.h: k_jpeg_idct (rule 3: dequantised coefficients -> 8-bit sample
// planes) and k_jpeg_color (rules 4 and 5: planes -> RGBA8 texels). It runs when an asset is loaded, not per frame. The
// arithmetic is the text of szg_jpeg_rules.hpp, which the host path compiles too.
//
// k_jpeg_idct  A block is 128 contiguous bytes. A wave takes 8 horizontally adjacent blocks, one block row (16 bytes) per
//              lane: its 64 loads are one contiguous 1 KiB run. The column pass needs lane (block b, column c) to hold column
//              c, so the rows go through LDS (144 bytes per block: 128 + 16 of padding puts the eight blocks of a read on
//              distinct banks); the 32-bit intermediates go back through LDS (72 dwords per block) for the row pass, where
//              lane (b, r) reads its row as two 16-byte loads. Each lane stores 8 bytes; the 8 lanes of one row r form a
//              contiguous 64-byte run of the plane. Nothing is indexed dynamically in registers: no scratch.
//              Tail groups (blocks_w no multiple of 8) and the waves past a smaller plane's grid are guarded, not padded:
//              they take part in the barriers, load nothing and store nothing.
// k_jpeg_color One lane per 4 adjacent texels of a row: a 16-byte store where the address allows it, dword stores otherwise
//              and for the row tail. An unsubsampled first plane is read as one dword; every other sample by rule 4.
#include <hip/hip_runtime.h>

#include "szg_jpeg_launch.hpp"
#include "szg_jpeg_rules.hpp"

namespace szg
{
namespace
{
constexpr unsigned IN_STRIDE = 144u; // bytes per block of the int16 tile
constexpr unsigned MID_STRIDE = 72u; // dwords per block of the intermediate tile
} // namespace

__global__ __launch_bounds__(256) void k_jpeg_idct(JpegArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_in[4][8u * IN_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned s_mid[4][8u * MID_STRIDE];
    JpegPlaneArgs const p = a.plane[blockIdx.y];
    unsigned const wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned const group = blockIdx.x * 4u + wave;
    unsigned const by = group / p.groupsX, gx = group - by * p.groupsX;
    unsigned const b = lane >> 3, r = lane & 7u;
    unsigned const bx = gx * 8u + b;
    bool const live = by < p.blocksH && bx < p.blocksW;

    uint4 row = make_uint4(0u, 0u, 0u, 0u);
    if (live)
    {
        row = *reinterpret_cast<const uint4*>(p.coefficients + ((size_t)by * p.blocksW + bx) * 64u + r * 8u);
    }
    *reinterpret_cast<uint4*>(&s_in[wave][b * IN_STRIDE + r * 16u]) = row;
    __syncthreads();

    // column pass: this lane is column r of block b
    unsigned s[8], o[8];
#pragma unroll
    for (unsigned k = 0; k < 8u; k++)
    {
        s[k] = (unsigned)(int)*reinterpret_cast<const short*>(&s_in[wave][b * IN_STRIDE + k * 16u + r * 2u]);
    }
    jpeg::idct1d(s, jpeg::COLUMN_BIAS, o);
#pragma unroll
    for (unsigned k = 0; k < 8u; k++)
    {
        s_mid[wave][b * MID_STRIDE + k * 8u + r] = (unsigned)jpeg::asr(o[k], jpeg::COLUMN_SHIFT);
    }
    __syncthreads();

    // row pass: this lane is row r of block b
    uint4 const lo = *reinterpret_cast<const uint4*>(&s_mid[wave][b * MID_STRIDE + r * 8u]);
    uint4 const hi = *reinterpret_cast<const uint4*>(&s_mid[wave][b * MID_STRIDE + r * 8u + 4u]);
    s[0] = lo.x;
    s[1] = lo.y;
    s[2] = lo.z;
    s[3] = lo.w;
    s[4] = hi.x;
    s[5] = hi.y;
    s[6] = hi.z;
    s[7] = hi.w;
    jpeg::idct1d(s, jpeg::ROW_BIAS, o);
    uint2 out = make_uint2(0u, 0u);
#pragma unroll
    for (unsigned k = 0; k < 4u; k++)
    {
        out.x |= jpeg::shiftClamp255(o[k], jpeg::ROW_SHIFT) << (8u * k);
        out.y |= jpeg::shiftClamp255(o[k + 4u], jpeg::ROW_SHIFT) << (8u * k);
    }
    if (live)
    {
        *reinterpret_cast<uint2*>(p.samples + ((size_t)by * 8u + r) * ((size_t)p.blocksW * 8u) + (size_t)bx * 8u) = out;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_color(JpegArgs a)
{
    unsigned const x0 = (blockIdx.x * 64u + threadIdx.x) * 4u;
    unsigned const j = blockIdx.y * 4u + threadIdx.y;
    if (x0 >= a.width || j >= a.height)
    {
        return;
    }
    unsigned const n = a.width - x0 < 4u ? a.width - x0 : 4u;
    unsigned c[3][4];
#pragma unroll
    for (unsigned k = 0; k < 3u; k++)
    {
        if (k < a.planeCount)
        {
            JpegPlaneArgs const& q = a.plane[k];
            jpeg::Plane const p{q.samples, q.blocksW * 8u, q.hs, q.vs, q.ch, q.wl};
            if (k == 0u && q.hs == 1u && q.vs == 1u)
            {
                // the row is blocksW * 8 >= width rounded up to 8 samples long: the dword lies inside it
                unsigned const four = *reinterpret_cast<const unsigned*>(q.samples + (size_t)j * p.pitch + x0);
#pragma unroll
                for (unsigned i = 0; i < 4u; i++)
                {
                    c[0][i] = (four >> (8u * i)) & 0xFFu;
                }
            }
            else
            {
#pragma unroll
                for (unsigned i = 0; i < 4u; i++)
                {
                    c[k][i] = i < n ? jpeg::upsampled(p, x0 + i, j) : 0u;
                }
            }
        }
        else
        {
#pragma unroll
            for (unsigned i = 0; i < 4u; i++)
            {
                c[k][i] = c[0][i]; // one component: R = G = B = Y
            }
        }
    }
    unsigned t[4];
#pragma unroll
    for (unsigned i = 0; i < 4u; i++)
    {
        t[i] = (jpeg::texel(c[0][i], c[1][i], c[2][i], a.ycbcr != 0u) & a.rgbaAnd) | a.rgbaOr;
    }
    unsigned char* const out = a.dst + (size_t)j * a.dstPitch + (size_t)x0 * 4u;
    if (n == 4u && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u)
    {
        *reinterpret_cast<uint4*>(out) = make_uint4(t[0], t[1], t[2], t[3]);
    }
    else
    {
#pragma unroll
        for (unsigned i = 0; i < 4u; i++)
        {
            if (i < n)
            {
                reinterpret_cast<unsigned*>(out)[i] = t[i];
            }
        }
    }
}

hipError_t launch_jpeg_reconstruct(hipStream_t s, const JpegArgs& args)
{
    unsigned groups = 0;
    for (unsigned k = 0; k < args.planeCount; k++)
    {
        unsigned const g = args.plane[k].groupsX * args.plane[k].blocksH;
        groups = g > groups ? g : groups;
    }
    hipLaunchKernelGGL(k_jpeg_idct, dim3((groups + 3u) / 4u, args.planeCount), dim3(256), 0, s, args);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        return e;
    }
    hipLaunchKernelGGL(k_jpeg_color, dim3((args.width + 255u) / 256u, (args.height + 3u) / 4u), dim3(64, 4), 0, s, args);
    return hipGetLastError();
}
} // namespace szg
