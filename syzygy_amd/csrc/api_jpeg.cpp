// api_jpeg.cpp — the device entry points of include/szg/jpeg.h: the scratch size and the recorded reconstruction
// (kernels_jpeg.hip). The frame is validated in full before anything is launched: the kernels' reads and writes are bounded
// by the frame's geometry alone.
#include "api_common.hpp"
#include "szg/jpeg.h"
#include "szg_internal.hpp"
#include "szg_jpeg_launch.hpp"

using namespace szg;

size_t szg_jpeg_scratch_bytes(const szg_jpeg_frame* frame)
{
    if (frame == nullptr || frame->plane_count < 1u || frame->plane_count > 3u)
    {
        return 0;
    }
    // the geometry decides, not the pointers: a frame whose coefficients are not there yet still has a size
    szg_jpeg_frame probe = *frame;
    for (uint32_t p = 0; p < probe.plane_count; p++)
    {
        probe.planes[p].coefficients = reinterpret_cast<const int16_t*>(&probe);
    }
    if (jpeg_frame_problem(probe)[0] != '\0')
    {
        return 0;
    }
    size_t bytes = 0;
    for (uint32_t p = 0; p < frame->plane_count; p++)
    {
        bytes += (size_t)frame->planes[p].blocks_w * frame->planes[p].blocks_h * 64u;
    }
    return bytes;
}

int szg_record_jpeg_reconstruct(void* stream, const szg_jpeg_frame* frame, void* d_scratch, size_t scratch_bytes, uint32_t rgba_and,
                                uint32_t rgba_or, const szg_image* dst)
{
    if (frame == nullptr || d_scratch == nullptr || dst == nullptr || dst->data == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: NULL frame, d_scratch, dst or dst->data");
    }
    const char* const problem = jpeg_frame_problem(*frame);
    if (problem[0] != '\0')
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: %s", problem);
    }
    for (uint32_t p = 0; p < frame->plane_count; p++)
    {
        if (reinterpret_cast<uintptr_t>(frame->planes[p].coefficients) % 16u != 0u)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: the coefficients of plane %u are not aligned to 16 bytes", p);
        }
    }
    if (reinterpret_cast<uintptr_t>(d_scratch) % 16u != 0u || reinterpret_cast<uintptr_t>(dst->data) % 4u != 0u)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: d_scratch must be aligned to 16 bytes and dst->data to 4");
    }
    size_t const need = szg_jpeg_scratch_bytes(frame);
    if (scratch_bytes < need)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: scratch_bytes %zu, the planes of this frame need %zu", scratch_bytes,
                    need);
    }
    if (dst->format != SZG_FORMAT_RGBA8_UNORM)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: dst format %u, expected SZG_FORMAT_RGBA8_UNORM", dst->format);
    }
    if (dst->width < frame->width || dst->height < frame->height)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: dst %ux%u is smaller than the frame %ux%u", dst->width, dst->height,
                    frame->width, frame->height);
    }
    if (!image_layout_ok(*dst)) // (the alignment of dst->data was refused above, under its own sentence)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_record_jpeg_reconstruct: dst pitch %u is smaller than a row of %u texels or no multiple of 4",
                    dst->pitch_bytes, dst->width);
    }
    JpegArgs args{};
    uint8_t* samples = static_cast<uint8_t*>(d_scratch);
    for (uint32_t p = 0; p < frame->plane_count; p++)
    {
        szg_jpeg_plane const& k = frame->planes[p];
        JpegPlaneArgs& q = args.plane[p];
        q.coefficients = k.coefficients;
        q.samples = samples;
        q.blocksW = k.blocks_w;
        q.blocksH = k.blocks_h;
        q.groupsX = (k.blocks_w + 7u) / 8u;
        q.hs = frame->h_max / k.h;
        q.vs = frame->v_max / k.v;
        q.ch = k.height;
        q.wl = (frame->width + q.hs - 1u) / q.hs;
        samples += (size_t)k.blocks_w * k.blocks_h * 64u;
    }
    args.planeCount = frame->plane_count;
    args.width = frame->width;
    args.height = frame->height;
    args.ycbcr = frame->color == SZG_JPEG_YCBCR ? 1u : 0u;
    args.rgbaAnd = rgba_and;
    args.rgbaOr = rgba_or;
    args.dst = static_cast<uint8_t*>(dst->data);
    args.dstPitch = dst->pitch_bytes;
    SZG_HIP(launch_jpeg_reconstruct(static_cast<hipStream_t>(stream), args));
    return SZG_OK;
}
