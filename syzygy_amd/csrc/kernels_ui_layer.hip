// kernels_ui_layer.hip — the UI layer pass (include/szg/ui_layer.h): UILayer::recordDraw's render pass
// (editor/uilayer.cpp:513-572 -> ImGui_ImplVulkan_RenderDrawData), an indexed triangle-list draw with a per-command scissor
// and texture, alpha-blended in submission order into the RGBA16_UNORM output texture. The rules (8 sub-pixel bits, exact
// int64 edge functions with the top-left rule, affine fp32 interpolation, the samplers, the blend on UNORM16 codes) are stated
// in the header; the CPU model is tests/ui_layer_model.py. Nothing here belongs to a contraction class: both libraries
// compile the same code.
//
// The structure is the one of kernels_raster.hip, adapted to ordered blending: no sort, no per-tile lists, no atomics.
//   k_ui_setup   one lane per triangle in submission order: its command by binary search over the commands' first triangle,
//                indices, vertices, the snap, det, the sign-normalised edge functions, the unpacked colours, and the pixel box
//                bbox ∩ scissor ∩ render area ∩ viewport (the command's box carries the last three). A dropped triangle gets
//                the empty box. A wave is one chunk of 64 consecutive triangles and reduces its union box.
//   k_ui_super   one lane per chunk: union boxes of 64 consecutive chunks.
//   k_ui_tile    a wave owns an 8x8 pixel patch and walks super-chunks, chunks and triangles in increasing index; the box
//                tests run 64 at a time by ballot, the survivors are shaded one by one, in order, from wave-uniform records
//                (scalar loads). The running destination stays in registers as UNORM16 codes - the blend rule reads the
//                destination as stored - is loaded once (not at all under CLEAR, and under LOAD only by a patch some box
//                reaches) and stored once. No two lanes own the same pixel: the order is the walk's order by construction.
//                Per pixel the edge values are the patch origin's (scalar 64-bit arithmetic) plus lane multiples below 8 of the
//                steps; the 64 x 64-bit products stay out of the lanes.
// UI geometry is spatially coherent in submission order (a window, then its widgets), which keeps the union boxes tight.
#include "szg_image_ops.hpp"
#include "szg_launch.hpp"

#include "szg/texture_display.h"
#include "szg/ui_layer.h"

namespace szg
{
namespace
{
constexpr unsigned UI_EMPTY_BOX_X = 0x0000FFFFu; // min = 0xFFFF, max = 0

SZG_DEV bool boxTouchesPatch(uint2 box, int px0, int py0)
{
    int const x0 = (int)(box.x & 0xFFFFu), x1 = (int)(box.x >> 16);
    int const y0 = (int)(box.y & 0xFFFFu), y1 = (int)(box.y >> 16);
    return x0 < px0 + 8 && x1 > px0 && y0 < py0 + 8 && y1 > py0;
}

// union of the 64 lanes' boxes, in every lane
SZG_DEV uint2 waveUnionBox(uint2 box)
{
    unsigned x0 = box.x & 0xFFFFu, x1 = box.x >> 16, y0 = box.y & 0xFFFFu, y1 = box.y >> 16;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
    {
        x0 = min(x0, (unsigned)__shfl_xor((int)x0, m, 64));
        x1 = max(x1, (unsigned)__shfl_xor((int)x1, m, 64));
        y0 = min(y0, (unsigned)__shfl_xor((int)y0, m, 64));
        y1 = max(y1, (unsigned)__shfl_xor((int)y1, m, 64));
    }
    return make_uint2(x0 | (x1 << 16), y0 | (y1 << 16));
}

// VERTEX of the header: false when the guard band drops the vertex
SZG_DEV bool snapVertex(const szg_ui_draw_vert& vtx, const UIDrawParams& d, int& X, int& Y)
{
    float const px = (vtx.pos[0] - d.displayPos[0]) * d.scale[0];
    float const py = (vtx.pos[1] - d.displayPos[1]) * d.scale[1];
    if (!(fabsf(px) <= SZG_UI_GUARD_BAND) || !(fabsf(py) <= SZG_UI_GUARD_BAND)) // NaN fails both
    {
        return false;
    }
    X = __float2int_rn(px * 256.0f);
    Y = __float2int_rn(py * 256.0f);
    return true;
}

__global__ __launch_bounds__(64) void k_ui_setup(UIDrawParams d, const UICommand* __restrict__ commands, UIPrim* __restrict__ prims,
                                                 uint2* __restrict__ boxes, uint2* __restrict__ chunkBoxes)
{
    unsigned const t = blockIdx.x * 64u + threadIdx.x;
    uint2 box = make_uint2(UI_EMPTY_BOX_X, UI_EMPTY_BOX_X);
    if (t < d.triCount)
    {
        // the last command whose first triangle is <= t (commands without triangles are not in the list)
        unsigned lo = 0u, hi = d.commandCount;
        while (hi - lo > 1u)
        {
            unsigned const mid = (lo + hi) >> 1;
            if (commands[mid].firstTri <= t)
            {
                lo = mid;
            }
            else
            {
                hi = mid;
            }
        }
        UICommand const c = commands[lo];
        unsigned const first = c.firstIndex + 3u * (t - c.firstTri); // inside the index array: the host truncated the range
        int X[3], Y[3];
        szg_ui_draw_vert vtx[3];
        bool keep = true;
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            unsigned long long const vi = (unsigned long long)c.vtxOffset + d.indices[first + (unsigned)k];
            keep = keep && vi < d.vertexCount;
            vtx[k] = d.vertices[keep ? vi : 0ull]; // vertexCount > 0 whenever a triangle exists (checked on the host)
            keep = keep && snapVertex(vtx[k], d, X[k], Y[k]);
        }
        if (keep)
        {
            long long const det = (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (X[2] - X[0]);
            if (det != 0)
            {
                long long const s = det > 0 ? 1 : -1;
                UIPrim p;
                unsigned topLeft = 0u;
#pragma unroll
                for (int i = 0; i < 3; i++)
                {
                    int const j = (i + 1) % 3, k = (i + 2) % 3;
                    long long const a = -(long long)(Y[k] - Y[j]) * s; // s a_i
                    long long const b = (long long)(X[k] - X[j]) * s;  // s b_i
                    p.e0[i] = b * (128 - Y[j]) + a * (128 - X[j]);
                    p.ex[i] = 256 * a;
                    p.ey[i] = 256 * b;
                    if (a > 0 || (a == 0 && b > 0))
                    {
                        topLeft |= 1u << i;
                    }
                    p.u[i] = vtx[i].uv[0];
                    p.v[i] = vtx[i].uv[1];
                    p.r[i] = decode8(vtx[i].col & 0xFFu, false);
                    p.g[i] = decode8((vtx[i].col >> 8) & 0xFFu, false);
                    p.b[i] = decode8((vtx[i].col >> 16) & 0xFFu, false);
                    p.a[i] = decode8(vtx[i].col >> 24, false);
                }
                p.det = (float)(det > 0 ? det : -det);
                p.topLeft = topLeft;
                p.command = lo;
                p.pad = 0u;
                // pixels whose centre 256 p + 128 lies inside [min, max] of the snapped vertices, cut by the command's box
                int const xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
                int const ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
                int const x0 = max((xmin + 127) >> 8, c.clip[0]), x1 = min(((xmax - 128) >> 8) + 1, c.clip[2]);
                int const y0 = max((ymin + 127) >> 8, c.clip[1]), y1 = min(((ymax - 128) >> 8) + 1, c.clip[3]);
                if (x0 < x1 && y0 < y1)
                {
                    box = make_uint2((unsigned)x0 | ((unsigned)x1 << 16), (unsigned)y0 | ((unsigned)y1 << 16));
                }
                p.box[0] = box.x;
                p.box[1] = box.y;
                prims[t] = p;
            }
        }
    }
    boxes[t] = box; // the buffer holds a whole number of chunks
    uint2 const u = waveUnionBox(box);
    if (threadIdx.x == 0u)
    {
        chunkBoxes[blockIdx.x] = u;
    }
}

__global__ __launch_bounds__(64) void k_ui_super(const uint2* __restrict__ chunkBoxes, unsigned chunkCount, uint2* __restrict__ superBoxes)
{
    unsigned const c = blockIdx.x * 64u + threadIdx.x;
    uint2 const box = c < chunkCount ? chunkBoxes[c] : make_uint2(UI_EMPTY_BOX_X, UI_EMPTY_BOX_X);
    uint2 const u = waveUnionBox(box);
    if (threadIdx.x == 0u)
    {
        superBoxes[blockIdx.x] = u;
    }
}

// REPEAT of the header: wrapIndex of szg_texture.hpp without its out-of-range conversion
SZG_DEV int repeatIndex(float f, float fn)
{
    float const m = f - fn * floorf(f / fn);
    return (m >= 0.0f && m < fn) ? (int)m : 0;
}

// One axis of SAMPLING: the texels of the two taps, whether each lies outside (CLAMP_TO_BORDER only), and the weight of the
// second. NEAREST uses tap 0 alone.
struct AxisTaps
{
    int i0, i1;
    bool out0, out1;
    float w;
};
SZG_DEV AxisTaps axisTaps(float coord, unsigned n, unsigned filter, unsigned address)
{
    AxisTaps t;
    float const fn = (float)n, last = fn - 1.0f;
    float x = coord * fn;
    if (filter == SZG_FILTER_LINEAR)
    {
        x = x - 0.5f;
    }
    float const f0 = floorf(x);
    float const f1 = f0 + 1.0f;
    t.w = x - f0;
    t.out0 = false;
    t.out1 = false;
    if (address == SZG_UI_ADDRESS_REPEAT)
    {
        t.i0 = repeatIndex(f0, fn);
        t.i1 = t.i0 + 1 == (int)n ? 0 : t.i0 + 1;
    }
    else
    {
        t.i0 = (int)fminf(fmaxf(f0, 0.0f), last); // NaN -> 0
        t.i1 = (int)fminf(fmaxf(f1, 0.0f), last);
        if (address == SZG_UI_ADDRESS_CLAMP_TO_BORDER)
        {
            t.out0 = !(f0 >= 0.0f && f0 <= last);
            t.out1 = !(f1 >= 0.0f && f1 <= last);
        }
    }
    return t;
}

SZG_DEV V4 fetchTexel(const UICommand& c, int i, int j, bool outside)
{
    if (outside)
    {
        return V4{0.0f, 0.0f, 0.0f, 1.0f};
    }
    const unsigned char* row = static_cast<const unsigned char*>(c.texData) + (size_t)j * c.texPitch;
    unsigned const format = c.texFormat & 0xFFFFu; // per command: wave-uniform
    if (format != UI_TEX_RGBA8_UNORM)
    {
        uint2 const t = *reinterpret_cast<const uint2*>(row + (size_t)i * 8u);
        if (format == UI_TEX_RGBA16_SFLOAT)
        {
            return unpack_half4(t); // exact: denormals kept, inf and NaN as they are
        }
        return unpack_unorm16x4(t);
    }
    unsigned const t = *reinterpret_cast<const unsigned*>(row + (size_t)i * 4u);
    return V4{decode8(t & 0xFFu, false), decode8((t >> 8) & 0xFFu, false), decode8((t >> 16) & 0xFFu, false), decode8(t >> 24, false)};
}

// MAPPING of szg/texture_display.h for one channel of the filtered sample: `s` is a VkComponentSwizzle, `own` the channel's
// own value (IDENTITY)
SZG_DEV float swizzled(V4 r, unsigned s, float own)
{
    return s == SZG_SWIZZLE_IDENTITY ? own
         : s == SZG_SWIZZLE_ZERO     ? 0.0f
         : s == SZG_SWIZZLE_ONE      ? 1.0f
         : s == SZG_SWIZZLE_R        ? r.x
         : s == SZG_SWIZZLE_G        ? r.y
         : s == SZG_SWIZZLE_B        ? r.z
                                     : r.w;
}

SZG_DEV V4 filteredSample(const UICommand& c, float u, float v);

// SAMPLING, then MAPPING. The mapping is per command, hence wave-uniform: a scalar branch that an identity view (every
// szg_ui_layer_add_texture handle) skips.
SZG_DEV V4 sampleUI(const UICommand& c, float u, float v)
{
    V4 const r = filteredSample(c, u, v);
    unsigned const map = c.texFormat >> 16;
    if (map == 0u)
    {
        return r;
    }
    return V4{swizzled(r, map & 7u, r.x), swizzled(r, (map >> 3) & 7u, r.y), swizzled(r, (map >> 6) & 7u, r.z),
              swizzled(r, (map >> 9) & 7u, r.w)};
}

SZG_DEV V4 filteredSample(const UICommand& c, float u, float v)
{
    AxisTaps const tx = axisTaps(u, c.texWidth, c.filter, c.address);
    AxisTaps const ty = axisTaps(v, c.texHeight, c.filter, c.address);
    V4 const t00 = fetchTexel(c, tx.i0, ty.i0, tx.out0 || ty.out0);
    if (c.filter != SZG_FILTER_LINEAR)
    {
        return t00;
    }
    V4 const t10 = fetchTexel(c, tx.i1, ty.i0, tx.out1 || ty.out0);
    V4 const t01 = fetchTexel(c, tx.i0, ty.i1, tx.out0 || ty.out1);
    V4 const t11 = fetchTexel(c, tx.i1, ty.i1, tx.out1 || ty.out1);
    float const na = 1.0f - tx.w, nb = 1.0f - ty.w;
    return blend(blend(t00, t10, na, tx.w), blend(t01, t11, na, tx.w), nb, ty.w);
}

SZG_DEV float saturate01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); } // NaN -> 0

// (area*): render area ∩ image; (gx0, gy0): origin of the patch grid, the area's origin rounded down to 8
template <bool CLEAR>
__global__ __launch_bounds__(256) void k_ui_tile(unsigned char* __restrict__ out, unsigned pitch, int ax0, int ay0, int ax1, int ay1,
                                                 int gx0, int gy0, V4 clearColor, const UICommand* __restrict__ commands,
                                                 const UIPrim* __restrict__ prims, const uint2* __restrict__ boxes,
                                                 const uint2* __restrict__ chunkBoxes, const uint2* __restrict__ superBoxes,
                                                 unsigned triCount)
{
    unsigned const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned const lane = threadIdx.x & 63u;
    int const px0 = gx0 + (int)blockIdx.x * 16 + (int)(wave & 1u) * 8;
    int const py0 = gy0 + (int)blockIdx.y * 16 + (int)(wave >> 1) * 8;
    if (px0 >= ax1 || py0 >= ay1 || px0 + 8 <= ax0 || py0 + 8 <= ay0)
    {
        return;
    }
    int const lx = (int)(lane & 7u), ly = (int)(lane >> 3);
    int const px = px0 + lx, py = py0 + ly;
    bool const inArea = px >= ax0 && px < ax1 && py >= ay0 && py < ay1;
    uint2* const texel = reinterpret_cast<uint2*>(out + (size_t)py * pitch + (size_t)px * 8u);

    // the destination as stored: UNORM16 codes r | g << 16, b | a << 16
    uint2 dst = CLEAR ? pack_unorm16x4(clearColor.x, clearColor.y, clearColor.z, clearColor.w) : make_uint2(0u, 0u);
    bool loaded = CLEAR; // wave-uniform

    unsigned const chunkCount = (triCount + 63u) / 64u;
    unsigned const superCount = (chunkCount + 63u) / 64u;
    for (unsigned s = 0u; s < superCount; s++)
    {
        if (!boxTouchesPatch(superBoxes[s], px0, py0))
        {
            continue;
        }
        unsigned const c = s * 64u + lane;
        unsigned long long chunkMask = __builtin_amdgcn_ballot_w64(c < chunkCount && boxTouchesPatch(chunkBoxes[c < chunkCount ? c : 0u], px0, py0));
        while (chunkMask != 0ull)
        {
            unsigned const chunk = s * 64u + (unsigned)__builtin_ctzll(chunkMask);
            chunkMask &= chunkMask - 1ull;
            unsigned const t = chunk * 64u + lane;
            unsigned long long triMask = __builtin_amdgcn_ballot_w64(t < triCount && boxTouchesPatch(boxes[t < triCount ? t : 0u], px0, py0));
            if (!CLEAR && !loaded && triMask != 0ull)
            {
                if (inArea)
                {
                    dst = *texel;
                }
                loaded = true;
            }
            while (triMask != 0ull)
            {
                unsigned const ti = chunk * 64u + (unsigned)__builtin_ctzll(triMask);
                triMask &= triMask - 1ull;
                UIPrim const& p = prims[ti]; // wave-uniform
                int const bx0 = (int)(p.box[0] & 0xFFFFu), bx1 = (int)(p.box[0] >> 16);
                int const by0 = (int)(p.box[1] & 0xFFFFu), by1 = (int)(p.box[1] >> 16);
                bool cover = inArea && px >= bx0 && px < bx1 && py >= by0 && py < by1;
                long long e[3];
#pragma unroll
                for (int i = 0; i < 3; i++)
                {
                    long long const origin = p.e0[i] + p.ex[i] * px0 + p.ey[i] * py0; // scalar
                    e[i] = origin + p.ex[i] * lx + p.ey[i] * ly;
                    cover = cover && e[i] + (long long)((p.topLeft >> i) & 1u) > 0;
                }
                if (cover)
                {
                    float const l0 = (float)e[0] / p.det, l1 = (float)e[1] / p.det, l2 = (float)e[2] / p.det;
                    float const u = (l0 * p.u[0] + l1 * p.u[1]) + l2 * p.u[2];
                    float const v = (l0 * p.v[0] + l1 * p.v[1]) + l2 * p.v[2];
                    float const cr = (l0 * p.r[0] + l1 * p.r[1]) + l2 * p.r[2];
                    float const cg = (l0 * p.g[0] + l1 * p.g[1]) + l2 * p.g[2];
                    float const cb = (l0 * p.b[0] + l1 * p.b[1]) + l2 * p.b[2];
                    float const ca = (l0 * p.a[0] + l1 * p.a[1]) + l2 * p.a[2];
                    V4 const tex = sampleUI(commands[p.command], u, v);
                    float const fr = saturate01(cr * tex.x), fg = saturate01(cg * tex.y), fb = saturate01(cb * tex.z);
                    float const fa = saturate01(ca * tex.w);
                    V4 const d = unpack_unorm16x4(dst);
                    float const na = 1.0f - fa;
                    dst = pack_unorm16x4(fr * fa + d.x * na, fg * fa + d.y * na, fb * fa + d.z * na, fa + d.w * na);
                }
            }
        }
    }
    if (inArea && loaded)
    {
        *texel = dst;
    }
}
} // namespace

hipError_t launch_ui_layer(hipStream_t s, const szg_image& output, szg_rect area, bool clear, const float clearColor[4],
                           const UIDrawParams& draw, const UILayerBuffers& b)
{
    unsigned const chunkCount = (draw.triCount + 63u) / 64u;
    if (chunkCount > 0u)
    {
        hipLaunchKernelGGL(k_ui_setup, dim3(chunkCount), dim3(64), 0, s, draw, b.commands, b.prims, b.boxes, b.chunkBoxes);
        hipLaunchKernelGGL(k_ui_super, dim3((chunkCount + 63u) / 64u), dim3(64), 0, s, b.chunkBoxes, chunkCount, b.superBoxes);
    }
    else if (!clear)
    {
        return hipSuccess; // LOAD and nothing to draw: every pixel keeps its value
    }
    int const ax0 = area.x, ay0 = area.y, ax1 = area.x + (int)area.width, ay1 = area.y + (int)area.height;
    int const gx0 = ax0 & ~7, gy0 = ay0 & ~7;
    dim3 const grid((unsigned)(ax1 - gx0 + 15) / 16u, (unsigned)(ay1 - gy0 + 15) / 16u);
    unsigned char* out = static_cast<unsigned char*>(output.data);
    if (clear)
    {
        V4 const cc{clearColor[0], clearColor[1], clearColor[2], clearColor[3]};
        hipLaunchKernelGGL(k_ui_tile<true>, grid, dim3(256), 0, s, out, output.pitch_bytes, ax0, ay0, ax1, ay1, gx0, gy0, cc, b.commands,
                           b.prims, b.boxes, b.chunkBoxes, b.superBoxes, draw.triCount);
    }
    else
    {
        hipLaunchKernelGGL(k_ui_tile<false>, grid, dim3(256), 0, s, out, output.pitch_bytes, ax0, ay0, ax1, ay1, gx0, gy0,
                           V4{0.0f, 0.0f, 0.0f, 0.0f}, b.commands, b.prims, b.boxes, b.chunkBoxes, b.superBoxes, draw.triCount);
    }
    return hipGetLastError();
}
} // namespace szg
