// kernels_debuglines.hip — compute line rasteriser for gfx950: the debug-line pass of Renderer::recordDraw
// (include/szg/debuglines.h states the rules and cites the reference).
//
//   k_dl_setup    one lane per line: vertex stage for both endpoints, depth-plane clipping, viewport, major axis; the
//                 major-axis pixel range is clamped to the scissor (and the tile's rows) and its length written as the
//                 line's step count. A line whose endpoints lie far off-screen costs only the steps inside the scissor.
//   (rocPRIM exclusive scan of the step counts: no host round trip, the total stays on the device)
//   k_dl_raster   one lane per (line, major-axis step), grid-stride over the scanned total read from device memory, so one
//                 long line spreads over many waves and a mix of lengths is balanced. Each lane walks a conservative
//                 minor-axis interval (strip half-width + a rounding margin) and applies the exact coverage test of the
//                 header to every candidate. Covered pixels get one 8-byte colour store (and a 16-byte debug store);
//                 lines overlap only with the same value, so there are no atomics.
//
// Plain binary32 operations in the header's order, nothing contracted: -ffp-contract=off and no SZG_CON here, so the
// product and the literal library are the same code.

#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "szg_launch.hpp"

namespace szg
{
namespace
{
constexpr unsigned DL_BLOCK = 256u;

struct Clip
{
    float x, y, z, w;
};

__device__ __forceinline__ bool finite4(Clip c)
{
    return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w);
}

// debugline.vert: (projection * view) * (position, 1), OpMatrixTimesMatrix then OpMatrixTimesVector, sums left to right
__device__ __forceinline__ void projView(const szg_camera_packed& cam, float pv[16])
{
    const float* P = cam.projection.m;
    const float* V = cam.view.m;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            float acc = P[r] * V[j * 4 + 0];
            acc = acc + P[4 + r] * V[j * 4 + 1];
            acc = acc + P[8 + r] * V[j * 4 + 2];
            acc = acc + P[12 + r] * V[j * 4 + 3];
            pv[j * 4 + r] = acc;
        }
    }
}

__device__ __forceinline__ Clip vertexStage(const float pv[16], const float* p)
{
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        float acc = pv[r] * p[0];
        acc = acc + pv[4 + r] * p[1];
        acc = acc + pv[8 + r] * p[2];
        acc = acc + pv[12 + r] * 1.0f;
        o[r] = acc;
    }
    return Clip{o[0], o[1], o[2], o[3]};
}

__device__ __forceinline__ float lerpTo(float a, float b, float t) { return a + t * (b - a); }

// one depth plane: false = the line is dropped
__device__ __forceinline__ bool clipPlane(Clip& a, Clip& b, bool far)
{
    float const da = far ? a.w - a.z : a.z;
    float const db = far ? b.w - b.z : b.z;
    if (da < 0.0f && db < 0.0f)
    {
        return false;
    }
    if (da < 0.0f || db < 0.0f)
    {
        float const t = da / (da - db);
        Clip const n{lerpTo(a.x, b.x, t), lerpTo(a.y, b.y, t), lerpTo(a.z, b.z, t), lerpTo(a.w, b.w, t)};
        if (da < 0.0f)
        {
            a = n;
        }
        else
        {
            b = n;
        }
    }
    return true;
}

// global row of local row l of a tile / does the rank own global row g (abi.h szg_rowtile)
__device__ __forceinline__ unsigned globalRow(TileArgs t, unsigned l)
{
    return ((l / t.block_rows) * t.nranks + t.rank) * t.block_rows + l % t.block_rows;
}

__device__ __forceinline__ bool covered(const DebugLineRec& L, unsigned px, unsigned py)
{
    float const cx = (float)px + 0.5f;
    float const cy = (float)py + 0.5f;
    float const ex = cx - L.xa;
    float const ey = cy - L.ya;
    float const u = ex * L.dx + ey * L.dy;
    float const v = L.dx * ey - L.dy * ex;
    return L.L2 > 0.0f && 0.0f <= u && u <= L.L2 && (4.0f * v) * v <= L.w2 * L.L2;
}

__device__ __forceinline__ void writePixel(const szg_scene_texture& scene, unsigned px, unsigned localRow, bool debug)
{
    unsigned char* const row = static_cast<unsigned char*>(scene.color.data) + (size_t)localRow * scene.color.pitch_bytes;
    reinterpret_cast<uint2*>(row)[px] = make_uint2(0xFFFF0000u, 0xFFFF0000u); // (0, 65535, 0, 65535)
    if (debug)
    {
        unsigned char* const drow = static_cast<unsigned char*>(scene.debug_color.data) + (size_t)localRow * scene.debug_color.pitch_bytes;
        reinterpret_cast<float4*>(drow)[px] = make_float4(0.0f, 1.0f, 0.0f, 1.0f);
    }
}
} // namespace

__global__ __launch_bounds__(DL_BLOCK) void k_dl_setup(const szg_camera_packed* __restrict__ cameras, unsigned cameraIndex,
                                                        const szg_vertex_packed* __restrict__ vertices, unsigned lineCount,
                                                        unsigned W, unsigned H, TileArgs tile, float lineWidth,
                                                        DebugLineRec* __restrict__ recs, unsigned long long* __restrict__ steps)
{
    unsigned const k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0u)
    {
        steps[lineCount] = 0ull; // the scan's last element is the total
    }
    if (k >= lineCount)
    {
        return;
    }
    DebugLineRec L{};
    unsigned long long count = 0ull;
    float pv[16];
    projView(cameras[cameraIndex], pv);
    Clip a = vertexStage(pv, vertices[2u * k].position);
    Clip b = vertexStage(pv, vertices[2u * k + 1u].position);
    // the tile's global row span (rows between belong to other ranks and are skipped per pixel)
    unsigned const rowFirst = tile.local_rows ? globalRow(tile, 0u) : 1u;
    unsigned const rowLast = tile.local_rows ? globalRow(tile, tile.local_rows - 1u) : 0u;
    if (finite4(a) && finite4(b) && clipPlane(a, b, false) && clipPlane(a, b, true) && rowFirst <= rowLast)
    {
        float const hW = (float)W * 0.5f;
        float const hH = (float)H * 0.5f;
        L.xa = (a.x / a.w + 1.0f) * hW;
        L.ya = (a.y / a.w + 1.0f) * hH;
        L.xb = (b.x / b.w + 1.0f) * hW;
        L.yb = (b.y / b.w + 1.0f) * hH;
        float const G = SZG_DEBUG_LINES_GUARD_BAND;
        // each compared on its own: a NaN fails its comparison (fmaxf would drop it)
        if (fabsf(L.xa) <= G && fabsf(L.ya) <= G && fabsf(L.xb) <= G && fabsf(L.yb) <= G)
        {
            float const m = fmaxf(fmaxf(fabsf(L.xa), fabsf(L.ya)), fmaxf(fabsf(L.xb), fabsf(L.yb)));
            L.dx = L.xb - L.xa;
            L.dy = L.yb - L.ya;
            L.L2 = L.dx * L.dx + L.dy * L.dy;
            L.w2 = lineWidth * lineWidth;
            if (L.L2 > 0.0f)
            {
                // Candidate bounds, conservative: the rectangle reaches at most w/2 past an endpoint along the major axis
                // and at most (w/2) * |d| / |d_major| <= (w/2) * sqrt(2) from the centre line along the minor axis. The
                // margin covers the rounding of the exact test (relative 2^-24 per operation on |e| <= 2 * (m + 2^15),
                // under 2^-19 * (m + 2^15) pixels) and of the centre line below.
                float const margin = 2.0f + (m + 32768.0f) * 0x1p-18f;
                float const hw = lineWidth * 0.5f;
                L.major = fabsf(L.dx) >= fabsf(L.dy) ? 0u : 1u;
                float const pa = L.major ? L.ya : L.xa;
                float const pb = L.major ? L.yb : L.xb;
                float const ext = hw + margin;
                L.half = hw * 1.5f + margin;
                L.slope = L.major ? L.dx / L.dy : L.dy / L.dx;
                float lo = floorf(fminf(pa, pb) - ext);
                float hi = floorf(fmaxf(pa, pb) + ext);
                float const top = L.major ? (float)rowLast : (float)(W - 1u);
                float const bottom = L.major ? (float)rowFirst : 0.0f;
                lo = fmaxf(lo, bottom);
                hi = fminf(hi, top);
                if (lo <= hi)
                {
                    L.first = (int)lo;
                    count = (unsigned long long)((int)hi - (int)lo + 1);
                }
            }
        }
    }
    recs[k] = L;
    steps[k] = count;
}

__global__ __launch_bounds__(DL_BLOCK) void k_dl_raster(szg_scene_texture scene, unsigned W, unsigned H, TileArgs tile,
                                                         const DebugLineRec* __restrict__ recs,
                                                         const unsigned long long* __restrict__ offsets, unsigned lineCount)
{
    unsigned long long const total = offsets[lineCount];
    bool const debug = scene.debug_color.data != nullptr;
    unsigned const rowFirst = tile.local_rows ? globalRow(tile, 0u) : 1u;
    unsigned const rowLast = tile.local_rows ? globalRow(tile, tile.local_rows - 1u) : 0u;
    unsigned long long const stride = (unsigned long long)gridDim.x * blockDim.x;
    // the wave's 64 consecutive items: the first index is wave-uniform, so the outer loop stays uniform
    unsigned long long const lane = threadIdx.x & 63u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < total; base += stride)
    {
        // lines of the wave's first and last item (uniform), then each lane's own within that range
        unsigned long long const lastItem = base + 63u < total ? base + 63u : total - 1u;
        unsigned lo = 0u, hi = lineCount; // offsets[lo] <= base < offsets[hi]
        while (hi - lo > 1u)
        {
            unsigned const mid = (lo + hi) >> 1;
            if (offsets[mid] <= base)
            {
                lo = mid;
            }
            else
            {
                hi = mid;
            }
        }
        unsigned hi2 = lineCount;
        unsigned lo2 = lo;
        while (hi2 - lo2 > 1u)
        {
            unsigned const mid = (lo2 + hi2) >> 1;
            if (offsets[mid] <= lastItem)
            {
                lo2 = mid;
            }
            else
            {
                hi2 = mid;
            }
        }
        unsigned long long const i = base + lane;
        if (i >= total)
        {
            continue;
        }
        unsigned l = lo, h = lo2 + 1u; // offsets[l] <= i < offsets[h]
        while (h - l > 1u)
        {
            unsigned const mid = (l + h) >> 1;
            if (offsets[mid] <= i)
            {
                l = mid;
            }
            else
            {
                h = mid;
            }
        }
        DebugLineRec const L = recs[l];
        int const major = L.first + (int)(i - offsets[l]);
        float const c = (float)major + 0.5f;
        float const pa = L.major ? L.ya : L.xa;
        float const qa = L.major ? L.xa : L.ya;
        float const centre = qa + (c - pa) * L.slope;
        float mlo = floorf(centre - L.half);
        float mhi = floorf(centre + L.half);
        float const top = L.major ? (float)(W - 1u) : (float)rowLast;
        float const bottom = L.major ? 0.0f : (float)rowFirst;
        mlo = fmaxf(mlo, bottom);
        mhi = fminf(mhi, top);
        if (!(mlo <= mhi))
        {
            continue;
        }
        int const from = (int)mlo, to = (int)mhi;
        if (L.major)
        {
            unsigned const gy = (unsigned)major;
            unsigned const blk = gy / tile.block_rows;
            if (blk % tile.nranks != tile.rank)
            {
                continue;
            }
            unsigned const localRow = (blk / tile.nranks) * tile.block_rows + gy % tile.block_rows;
            for (int x = from; x <= to; x++)
            {
                if (covered(L, (unsigned)x, gy))
                {
                    writePixel(scene, (unsigned)x, localRow, debug);
                }
            }
        }
        else
        {
            unsigned const px = (unsigned)major;
            for (int y = from; y <= to; y++)
            {
                unsigned const gy = (unsigned)y;
                unsigned const blk = gy / tile.block_rows;
                if (blk % tile.nranks == tile.rank && covered(L, px, gy))
                {
                    writePixel(scene, px, (blk / tile.nranks) * tile.block_rows + gy % tile.block_rows, debug);
                }
            }
        }
    }
}

hipError_t debug_lines_scan_temp_bytes(unsigned lineCapacity, size_t& bytes)
{
    bytes = 0;
    unsigned long long* none = nullptr;
    return rocprim::exclusive_scan(nullptr, bytes, none, none, 0ull, (size_t)lineCapacity + 1u, rocprim::plus<unsigned long long>(),
                                   hipStream_t{});
}

hipError_t launch_debug_lines(hipStream_t s, const szg_scene_texture& scene, unsigned W, unsigned H, TileArgs tile,
                              const szg_camera_packed* d_cam, unsigned camIndex, const szg_vertex_packed* d_vertices,
                              unsigned lineCount, float lineWidth, DebugLineBuffers& b)
{
    unsigned const setupBlocks = (lineCount + DL_BLOCK - 1u) / DL_BLOCK;
    hipLaunchKernelGGL(k_dl_setup, dim3(setupBlocks), dim3(DL_BLOCK), 0, s, d_cam, camIndex, d_vertices, lineCount, W, H, tile,
                       lineWidth, b.recs, b.steps);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        return e;
    }
    e = rocprim::exclusive_scan(b.scanTemp, b.scanTempBytes, b.steps, b.offsets, 0ull, (size_t)lineCount + 1u,
                                rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess)
    {
        return e;
    }
    // enough waves for every step to have a lane when the lines are short, capped by a few waves per SIMD of the device
    // (the grid-stride loop takes the rest)
    unsigned long long const bound = (unsigned long long)lineCount * (W > H ? W : H);
    unsigned long long const want = (bound + DL_BLOCK - 1u) / DL_BLOCK;
    unsigned const blocks = (unsigned)(want < 4096ull ? want : 4096ull);
    hipLaunchKernelGGL(k_dl_raster, dim3(blocks ? blocks : 1u), dim3(DL_BLOCK), 0, s, scene, W, H, tile, b.recs, b.offsets, lineCount);
    return hipGetLastError();
}
} // namespace szg
