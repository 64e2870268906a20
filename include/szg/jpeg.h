/*
 * szg/jpeg.h — C-ABI of JPEG material maps: an entropy decoder on the host and the reconstruction (IDCT, chroma upsampling,
 * colour conversion to RGBA8) as HIP kernels that write straight into the texture the raster samples, or as plain C++.
 *
 * glTF 2.0 allows two image encodings, PNG and JPEG. The reference decodes both through its vendored stb_image
 * (assets/assets.cpp:319-364, detail_stbi::loadRGBA: a 4-channel 8-bit request). The rules below are what that decoder
 * computes (thirdparty/stb/include/stb/stb_image.h), written as exact integer operations, so that the numpy model
 * (tests/jpeg_model.py), the host path and the kernels agree bit for bit, and the model agrees with recorded outputs of the
 * reference's decoder (tests/golden/jpeg). OPT-IN: nothing of szg/assets.h changes its behaviour unless one of the flags
 * below is passed; szg_decode_image_rgba still answers a JPEG stream with SZG_ERR_PARSE.
 *
 * 1 ACCEPTED STREAMS  Baseline and extended-sequential Huffman (SOF0, SOF1) and progressive (SOF2) at 8 bits of precision;
 *               1 or 3 components; sampling factors 1..4 that divide the frame's maximum; DRI and restart markers;
 *               interleaved and non-interleaved scans, several scans per frame; 8- and 16-bit quantisation tables; width
 *               and height 1..32768. SZG_ERR_PARSE with a szg_last_error() text for everything else: 12-bit, arithmetic,
 *               lossless and hierarchical streams; larger sizes; 2 or 4 components. DELIBERATE GAP: the reference decodes
 *               4-component CMYK and YCCK files, this library refuses them. A stream that ends before its EOI marker, or
 *               that is shorter than one bit per coefficient block of its frame, is refused as truncated (the reference
 *               pads such a stream with zero bits).
 *
 * 2 COEFFICIENTS  Dequantised on the host: the product of the entropy-decoded value and the 16-bit table entry, TRUNCATED
 *               to int16 (it wraps); for progressive streams after the last scan. Natural (row-major) order within the
 *               block, blocks in raster order over the component's MCU-padded grid: blocks_w = mcus_x * h,
 *               blocks_h = mcus_y * v with mcus_x = ceil(W / (8 h_max)), mcus_y = ceil(H / (8 v_max)). Blocks that no scan
 *               writes are zero.
 *
 * 3 IDCT        The reference's stbi__idct_block, operation for operation. All arithmetic is 32-bit two's complement that
 *               WRAPS (unsigned operations, arithmetic shift of the reinterpreted value). The constants are
 *               (int)(c * 4096 + 0.5) with c read as binary32: 0.5411961 -> 2217, -1.847759065 -> -7567, 0.765366865 ->
 *               3135, 1.175875602 -> 4816, 0.298631336 -> 1223, 2.053119869 -> 8410, 3.072711026 -> 12586, 1.501321110
 *               -> 6149, -0.899976223 -> -3685, -2.562915447 -> -10497, -1.961570560 -> -8034, -0.390180644 -> -1597.
 *               One 8-point pass over s0..s7 with bias B:
 *                 p1 = (s2 + s6) * 2217;  t2 = p1 - s6 * 7567;  t3 = p1 + s2 * 3135
 *                 t0 = (s0 + s4) * 4096;  t1 = (s0 - s4) * 4096
 *                 x0 = t0 + t3 + B;  x3 = t0 - t3 + B;  x1 = t1 + t2 + B;  x2 = t1 - t2 + B
 *                 t0 = s7; t1 = s5; t2 = s3; t3 = s1;  p3 = t0 + t2;  p4 = t1 + t3;  p1 = t0 + t3;  p2 = t1 + t2
 *                 p5 = (p3 + p4) * 4816
 *                 t0 *= 1223;  t1 *= 8410;  t2 *= 12586;  t3 *= 6149
 *                 p1 = p5 - p1 * 3685;  p2 = p5 - p2 * 10497;  p3 = -p3 * 8034;  p4 = -p4 * 1597
 *                 t3 += p1 + p4;  t2 += p2 + p3;  t1 += p2 + p4;  t0 += p1 + p3
 *                 out0, out7 = x0 +- t3;  out1, out6 = x1 +- t2;  out2, out5 = x2 +- t1;  out3, out4 = x3 +- t0
 *               The COLUMN pass comes first, B = 512, every output >> 10. The ROW pass follows on those values,
 *               B = 65536 + (128 << 17), every output >> 17, clamped to 0..255. The reference's shortcut for a column
 *               whose AC entries are all zero gives what the full pass gives ((d * 4096 + 512) >> 10 = 4 d) and does not
 *               exist here as a branch. For extreme coefficients the reference's SIMD build saturates where its scalar
 *               build wraps; the rule is the scalar one.
 *
 * 4 UPSAMPLING  Per component, hs = h_max / h, vs = v_max / v. Its sample extent is cw = ceil(W h / h_max) by
 *               ch = ceil(H v / v_max); the source samples a row needs are wl = ceil(W / hs). Clamps go to ch - 1 and
 *               wl - 1, NEVER into the MCU padding. For output row j: near = min(j / vs, ch - 1); if vs == 2:
 *               far = max(near - 1, 0) for even j, min(near + 1, ch - 1) for odd j. With N, F those two sample rows:
 *                 (1, 1)   out[x] = N[x]
 *                 (1, 2)   out[x] = (3 N[x] + F[x] + 2) >> 2
 *                 (2, 1)   out[0] = N[0];  out[2 wl - 1] = N[wl - 1];
 *                          inner: out[2 s] = (3 N[s] + N[s - 1] + 2) >> 2, out[2 s + 1] = (3 N[s] + N[s + 1] + 2) >> 2
 *                          QUIRK, kept: out[2 wl - 2] = (3 N[wl - 2] + N[wl - 1] + 2) >> 2 — the reference weights
 *                          sample wl - 2 there, not wl - 1. wl == 1: both outputs are N[0].
 *                 (2, 2)   t[s] = 3 N[s] + F[s];  out[0] = (t[0] + 2) >> 2;  out[2 wl - 1] = (t[wl - 1] + 2) >> 2;
 *                          inner: out[2 s] = (3 t[s] + t[s - 1] + 8) >> 4, out[2 s + 1] = (3 t[s] + t[s + 1] + 8) >> 4.
 *                          wl == 1: both outputs are (t[0] + 2) >> 2.
 *                 every other pair: out[x] = N[x / hs] (each near sample replicated hs times; far unused).
 *
 * 5 COLOUR      One component: R = G = B = Y. Three components: taken as R, G, B unconverted when the component ids are
 *               'R', 'G', 'B', or when an Adobe APP14 segment says transform 0 and there is no JFIF APP0 segment; otherwise
 *               YCbCr, with f(x) = ((int)(x * 4096.0f + 0.5f)) << 8 (f(1.40200) = 1470208, f(0.71414) = 748800,
 *               f(0.34414) = 360960, f(1.77200) = 1858048), cb = Cb - 128, cr = Cr - 128:
 *                 yf = (Y << 20) + (1 << 19)
 *                 r = yf + cr * f(1.40200)
 *                 g = yf - cr * f(0.71414) + ((-cb * f(0.34414)) & 0xffff0000)
 *                 b = yf + cb * f(1.77200)
 *               each >> 20 (arithmetic) and clamped to 0..255. Alpha is 255. Last, the texel as a little-endian dword
 *               (R lowest) becomes (texel & rgba_and) | rgba_or: the loader's ORM overrides (szg/assets.h: R := 255 is
 *               and 0xFFFFFF00 or 0x000000FF; G := B := 0 is and 0xFF0000FF or 0).
 *
 * Additive: SZG_ABI_VERSION does not move and no existing struct changes.
 */
#ifndef SZG_JPEG_H
#define SZG_JPEG_H

#include <stddef.h>

#include "szg/abi.h"
#include "szg/assets.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SZG_JPEG_MAX_EXTENT 32768u

#define SZG_JPEG_GREY 0u
#define SZG_JPEG_YCBCR 1u
#define SZG_JPEG_RGB 2u

typedef struct szg_jpeg szg_jpeg; /* opaque; owns the coefficient planes it hands out */

typedef struct szg_jpeg_plane
{
    const int16_t* coefficients; /* rule 2; blocks_w * blocks_h * 64 values. HOST memory from szg_jpeg_get_frame */
    uint32_t h, v;               /* sampling factors */
    uint32_t width, height;      /* cw, ch of rule 4 */
    uint32_t blocks_w, blocks_h; /* the MCU-padded block grid */
} szg_jpeg_plane;

typedef struct szg_jpeg_frame
{
    uint32_t width, height;
    uint32_t plane_count; /* 1 or 3 */
    uint32_t color;       /* SZG_JPEG_GREY / _YCBCR / _RGB (rule 5) */
    uint32_t h_max, v_max;
    uint32_t progressive; /* 1 for SOF2; information only */
    szg_jpeg_plane planes[3];
} szg_jpeg_frame;

/* ---- host side, CPU only ---- */

/* Parse the markers and entropy-decode every scan into dequantised coefficient planes. Any byte string gives SZG_OK and
 * *out, or a negative status, *out = NULL and a szg_last_error() text: SZG_ERR_INVALID_ARGUMENT (NULL argument),
 * SZG_ERR_PARSE (rule 1, or a corrupt stream), SZG_ERR_OUT_OF_MEMORY. */
int szg_jpeg_open(const void* bytes, size_t size, szg_jpeg** out);
void szg_jpeg_destroy(szg_jpeg* jpeg); /* NULL is allowed */
/* The frame with HOST pointers to the coefficients, valid until szg_jpeg_destroy. */
int szg_jpeg_get_frame(const szg_jpeg* jpeg, szg_jpeg_frame* out);
/* Rules 3-5 in plain C++: width x height texels into `rgba`, rows pitch_bytes apart (>= width * 4; the padding is not
 * written). `frame` carries HOST pointers; its geometry is validated as szg_record_jpeg_reconstruct validates it. */
int szg_jpeg_reconstruct_host(const szg_jpeg_frame* frame, uint32_t rgba_and, uint32_t rgba_or, uint8_t* rgba, size_t pitch_bytes);

/* ---- device side ---- */

/* Bytes of the 8-bit sample planes: the sum of blocks_w * blocks_h * 64 over the planes (plane k starts where plane k - 1
 * ends, pitch blocks_w * 8). 0 for a NULL or invalid frame. */
size_t szg_jpeg_scratch_bytes(const szg_jpeg_frame* frame);
/* Enqueue k_jpeg_idct and k_jpeg_color on `stream` and return. `frame` carries DEVICE pointers to the coefficients (the
 * planes of szg_jpeg_get_frame copied to the device), which are only read. `dst` is SZG_FORMAT_RGBA8_UNORM, allocated at
 * least width x height, any pitch that is a multiple of 4; only the frame's width x height texels are written, and only the
 * first szg_jpeg_scratch_bytes(frame) bytes of d_scratch. SZG_ERR_INVALID_ARGUMENT (with a szg_last_error() text, nothing
 * launched, nothing written) for: a NULL frame, d_scratch, dst, dst->data or coefficient pointer; plane_count not 1 or 3;
 * a colour that does not fit the plane count; width or height outside 1..32768; h or v outside 1..4 or not dividing the
 * maximum; h_max, v_max, or a plane's width, height, blocks_w, blocks_h that do not follow from width, height, h, v by
 * rules 2 and 4 (device reads are bounded by this geometry alone); a coefficient pointer not aligned to 16 bytes, a
 * d_scratch not aligned to 16 or a dst->data not aligned to 4; scratch_bytes below szg_jpeg_scratch_bytes(frame); a dst of
 * another format, smaller than the frame, or with a pitch below width * 4 or no multiple of 4. */
int szg_record_jpeg_reconstruct(void* stream, const szg_jpeg_frame* frame, void* d_scratch, size_t scratch_bytes,
                                uint32_t rgba_and, uint32_t rgba_or, const szg_image* dst);

/* ---- loader (szg/assets.h) ---- */

/* The flags SZG_GLTF_DECODE_JPEG and SZG_GLTF_JPEG_FOR_DEVICE of szg_gltf_load_* are defined in szg/assets.h. */

typedef struct szg_jpeg_map
{
    const szg_jpeg* jpeg;       /* NULL: this map is not a JPEG kept for the device; owned by the asset */
    uint32_t rgba_and, rgba_or; /* rule 5: the ORM override of this map, 0xFFFFFFFF / 0 for none */
    uint32_t srgb;
    const char* name;
} szg_jpeg_map;

/* kind: SZG_MAP_COLOR / _NORMAL / _ORM. SZG_ERR_INVALID_ARGUMENT for a NULL argument, an index out of range or an unknown
 * kind. */
int szg_gltf_material_jpeg(const szg_gltf* asset, uint32_t material, int kind, szg_jpeg_map* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SZG_JPEG_H */
