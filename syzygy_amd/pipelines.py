"""Host-side mirror of the reference's render-pass API for the deferred-shading +
atmosphere path, over the C-ABI library.

Names, argument order and meaning follow the reference:
  TStagedBuffer             renderer/buffers.hpp:209-299, buffers.cpp:180-255
  SceneTexture              renderer/scenetexture.hpp:11-81
  DeferredShadingPipeline   renderer/pipelines/deferred.hpp:23-119
  SkyViewComputePipeline    renderer/pipelines/skyview.hpp:24-51
  DebugLines                renderer/pipelines/debuglines.hpp:22-68
  DebugLineGraphicsPipeline renderer/pipelines.hpp:238-268
  record_copy_image_to_image / record_present   renderer/imageoperations.cpp:45-176, editor/editor.cpp:303-361
  ComputeCollectionPipeline renderer/pipelines.hpp:166-235, pipelines.cpp:223-368
  UILayer                   editor/uilayer.hpp:36-114, uilayer.cpp:285-337, :412-450, :513-572 (the draw only: szg/ui_layer.h)
  TextureDisplay, record_copy_image, record_clear_color_image   ui/texturedisplay.cpp, renderer/image.cpp:185-229,
                            rendercommands.cpp:25 (szg/texture_display.h)
with `cmd` (VkCommandBuffer) replaced by a HIP stream handle and Vulkan images by
linear device buffers. torch is used only to own device memory and streams.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import abi, ui
from ._lib import check, lib


def _stream_handle(cmd):
    """`cmd` may be None (current torch stream), a torch.cuda.Stream or a raw handle."""
    if cmd is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(cmd, torch.cuda.Stream):
        return C.c_void_p(cmd.cuda_stream)
    return C.c_void_p(int(cmd))


def _image(tensor, width, height, fmt):
    im = abi.Image()
    im.data = tensor.data_ptr()
    im.width = width
    im.height = height
    im.pitch_bytes = width * abi.TEXEL_BYTES[fmt]
    im.format = fmt
    return im


def rect(width, height):
    return abi.Rect(0, 0, int(width), int(height))


class TStagedBuffer:
    """buffers.hpp:209-299: host staging + device copy of an array of packed structs.

    recordCopyToDevice() is asynchronous: the copy runs in stream order, possibly behind a whole frame of kernels, so the
    pinned memory it reads must stay untouched until it has run. The reference guards its staging memory with the frame
    fences (two frames in flight, framebuffer.cpp:134); here every copy reads its own slot of a small ring of pinned
    buffers, and a slot is rewritten only after the event recorded behind its last copy has completed."""

    SLOTS = 3

    def __init__(self, struct_type, capacity, device="cuda:0"):
        self.struct_type = struct_type
        self.capacity = int(capacity)
        self._staged = []
        self._device_size = 0
        self._dirty = False
        nbytes = C.sizeof(struct_type) * self.capacity
        self._ring = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.SLOTS)]
        self._ring_done = [None] * self.SLOTS
        self._ring_next = 0
        self._device = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def allocate(cls, struct_type, capacity, device="cuda:0"):
        return cls(struct_type, capacity, device)

    def clearStaged(self):
        self._staged = []
        self._dirty = True

    def push(self, value):
        values = value if isinstance(value, (list, tuple)) else [value]
        if len(self._staged) + len(values) > self.capacity:
            raise ValueError("TStagedBuffer: staged size exceeds capacity")
        self._staged.extend(values)
        self._dirty = True

    def stage(self, values):
        self.clearStaged()
        self.push(list(values))

    def pop(self, count):
        del self._staged[len(self._staged) - count:]
        self._dirty = True

    def recordCopyToDevice(self, cmd=None):
        n = len(self._staged)
        size = C.sizeof(self.struct_type)
        if n:
            raw = self._stagedBytes()
            slot = self._ring_next
            self._ring_next = (slot + 1) % self.SLOTS
            if self._ring_done[slot] is not None:
                self._ring_done[slot].synchronize()  # the copy that last read this slot has run
            host = self._ring[slot]
            host[: n * size] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
            stream = torch.cuda.current_stream() if cmd is None else cmd
            with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _NullCtx():
                self._device[: n * size].copy_(host[: n * size], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
            self._ring_done[slot] = done
        self._device_size = n
        self._dirty = False

    def _stagedBytes(self):
        return b"".join(bytes(v) for v in self._staged)

    def deviceAddress(self):
        return self._device.data_ptr()

    def deviceSize(self):
        return self._device_size

    def stagedSize(self):
        return len(self._staged)

    def stagingCapacity(self):
        return self.capacity

    def isDirty(self):
        return self._dirty

    def readValidStaged(self):
        return list(self._staged)


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class SceneTexture:
    """scenetexture.hpp:11-81: colour (RGBA16 UNORM) + depth (D32F), allocated at a
    capacity extent and rendered into a sub-rect at offset (0, 0). `debug=True` adds
    the fp32 pre-quantisation colour plane used by the parity tests."""

    def __init__(self, width, height, device="cuda:0", debug=False):
        self.width, self.height = int(width), int(height)
        self.color = torch.zeros((self.height, self.width, 4), dtype=torch.int16, device=device)
        self.depth = torch.zeros((self.height, self.width), dtype=torch.float32, device=device)
        self.debug = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device=device) if debug else None

    def abi(self):
        st = abi.SceneTexture()
        st.color = _image(self.color, self.width, self.height, abi.SZG_FORMAT_RGBA16_UNORM)
        st.depth = _image(self.depth, self.width, self.height, abi.SZG_FORMAT_D32_SFLOAT)
        if self.debug is not None:
            st.debug_color = _image(self.debug, self.width, self.height, abi.SZG_FORMAT_RGBA32_SFLOAT)
        return st

    def color_numpy(self):
        return self.color.cpu().numpy().view(np.uint16)


def recordOETF(cmd, sceneTexture, width, height, transferFunction=abi.SZG_OETF_SRGB):
    """editor.cpp:303-340: in-place linear -> display encoding of the colour image (sRGB by default,
    editorconfig.hpp:13)."""
    im = sceneTexture.abi().color
    check(lib().szg_record_oetf(_stream_handle(cmd), C.byref(im), int(width), int(height), int(transferFunction)))


# ---------------------------------------------------------------------------
# Mip-mapped material textures (include/szg/mipmaps.h)
# ---------------------------------------------------------------------------
def mip_level_shapes(width, height):
    """[(w_k, h_k)] for k = 0 .. szg_mip_level_count - 1 (mipmaps.h "CHAIN LAYOUT")."""
    return [(max(1, width >> k), max(1, height >> k)) for k in range(lib().szg_mip_level_count(int(width), int(height)))]


def mip_chain_levels(chain, width, height):
    """Views [h_k, w_k, 4] of levels 1.. of a packed chain (tensor or numpy array of bytes) of a width x height image."""
    out, offset = [], 0
    for w, h in mip_level_shapes(width, height)[1:]:
        out.append(chain[offset:offset + w * h * 4].reshape(h, w, 4))
        offset += w * h * 4
    return out


def parse_mipmaps_option(text):
    """The examples' --mipmaps[=MAXLOD] switch -> the sampler's max_lod: 'none' (the switch alone) lifts the clamp, 'reference' is
    the reference sampler's 1.0, else a number >= 0."""
    if text in ("none", "reference"):
        return abi.SZG_SAMPLER_MAX_LOD_NONE if text == "none" else abi.SZG_SAMPLER_MAX_LOD_REFERENCE
    try:
        value = float(text)
    except ValueError:
        value = -1.0
    if not value >= 0.0:
        raise ValueError(f"{text!r}: expected none, reference or a number >= 0")
    return value


def parse_anisotropy_option(text):
    """The examples' --anisotropy A switch -> the sampler's max_anisotropy (include/szg/anisotropy.h): a number in 1 .. 16."""
    try:
        value = float(text)
    except ValueError:
        value = 0.0
    if not abi.SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE <= value <= abi.SZG_SAMPLER_MAX_ANISOTROPY_LIMIT:
        raise ValueError(f"{text!r}: expected a number from 1 to 16")
    return value


def generate_mipmaps(texture, srgb, cmd=None):
    """szg_record_generate_mipmaps: the packed chain (levels 1.., a uint8 CUDA tensor; empty for a 1x1 image) of an RGBA8 image,
    a uint8 CUDA tensor [h, w, 4] whose rows may be strided (a pitch wider than w * 4)."""
    if texture.dtype != torch.uint8 or texture.dim() != 3 or texture.shape[2] != 4 or texture.stride(2) != 1 or texture.stride(1) != 4:
        raise ValueError("generate_mipmaps: expected a uint8 tensor [h, w, 4] with contiguous texels")
    h, w = int(texture.shape[0]), int(texture.shape[1])
    level0 = abi.Texture(texture.data_ptr(), w, h, int(texture.stride(0)) if h > 1 else w * 4, int(bool(srgb)))
    nbytes = lib().szg_mip_chain_bytes(w, h)
    chain = torch.empty(nbytes, dtype=torch.uint8, device=texture.device)
    check(lib().szg_record_generate_mipmaps(_stream_handle(cmd), C.byref(level0), C.c_void_p(chain.data_ptr() if nbytes else None), nbytes))
    return chain


# ---------------------------------------------------------------------------
# JPEG material maps (include/szg/jpeg.h)
# ---------------------------------------------------------------------------
def upload_jpeg_frame(frame, device="cuda"):
    """Copy the coefficient planes of a HOST frame (szg_jpeg_get_frame) to `device`: (abi.JpegFrame with DEVICE pointers, the
    tensors that own them). The copies are complete when this returns, so the szg_jpeg may be destroyed."""
    out = abi.JpegFrame.from_buffer_copy(frame)
    keep = []
    for k in range(frame.plane_count):
        p = frame.planes[k]
        n = p.blocks_w * p.blocks_h * 64
        host = np.ctypeslib.as_array(C.cast(p.coefficients, C.POINTER(C.c_int16)), shape=(n,))
        keep.append(torch.from_numpy(host.copy()).to(device))
        out.planes[k].coefficients = keep[-1].data_ptr()
    return out, keep


def record_jpeg_reconstruct(frame, dst, rgba_and=0xFFFFFFFF, rgba_or=0, cmd=None, scratch=None):
    """szg_record_jpeg_reconstruct of a frame with DEVICE pointers into `dst`, a uint8 CUDA tensor [h, w, 4] whose rows may be
    strided and which may be larger than the frame. Returns the scratch tensor (keep it until the stream has run)."""
    if dst.dtype != torch.uint8 or dst.dim() != 3 or dst.shape[2] != 4 or dst.stride(2) != 1 or dst.stride(1) != 4:
        raise ValueError("record_jpeg_reconstruct: expected a uint8 tensor [h, w, 4] with contiguous texels")
    h, w = int(dst.shape[0]), int(dst.shape[1])
    nbytes = lib().szg_jpeg_scratch_bytes(C.byref(frame))
    if scratch is None:
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dst.device)
    im = abi.Image()
    im.data, im.width, im.height, im.format = dst.data_ptr(), w, h, abi.SZG_FORMAT_RGBA8_UNORM
    im.pitch_bytes = int(dst.stride(0)) if h > 1 else w * 4
    check(lib().szg_record_jpeg_reconstruct(_stream_handle(cmd), C.byref(frame), C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                            int(rgba_and), int(rgba_or), C.byref(im)))
    return scratch


def reconstruct_jpeg(handle, rgba_and=0xFFFFFFFF, rgba_or=0, device="cuda", cmd=None):
    """An open szg_jpeg -> uint8 [h, w, 4] tensor on `device`: coefficient upload, then k_jpeg_idct and k_jpeg_color on `cmd` (the
    current stream by default). The handle is not needed once this returns."""
    frame = abi.JpegFrame()
    check(lib().szg_jpeg_get_frame(handle, C.byref(frame)))
    stream = torch.cuda.current_stream(device) if cmd is None else cmd
    with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _NullCtx():
        d_frame, keep = upload_jpeg_frame(frame, device)
        out = torch.empty((frame.height, frame.width, 4), dtype=torch.uint8, device=device)
        keep.append(record_jpeg_reconstruct(d_frame, out, rgba_and, rgba_or, stream))
    # coefficients and scratch go back to torch's allocator here: it hands them out again in stream order, behind the kernels
    return out


def decode_jpeg(data, rgba_and=0xFFFFFFFF, rgba_or=0, device="cuda", cmd=None):
    """JPEG bytes -> uint8 [h, w, 4] tensor on `device`: szg_jpeg_open on the host (entropy decode), the reconstruction on the
    GPU. (texel & rgba_and) | rgba_or is applied to every texel as a little-endian dword, R lowest (jpeg.h rule 5)."""
    data = bytes(data)
    handle = C.c_void_p()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    check(lib().szg_jpeg_open(C.cast(buf, C.c_void_p), len(data), C.byref(handle)))
    try:
        return reconstruct_jpeg(handle, rgba_and, rgba_or, device, cmd)
    finally:
        lib().szg_jpeg_destroy(handle)


# ---------------------------------------------------------------------------
# Present pass (include/szg/present.h)
# ---------------------------------------------------------------------------
def _as_rect(r):
    """An abi.Rect, or (x, y, width, height)."""
    return r if isinstance(r, abi.Rect) else abi.Rect(int(r[0]), int(r[1]), int(r[2]), int(r[3]))


def _strided_image(tensor, fmt, channels):
    """szg_image over a torch tensor whose rows may be padded: [h, w, channels] (channels > 1) or [h, w]; the pitch is the
    row stride, the texels of a row are contiguous."""
    want = 3 if channels > 1 else 2
    if tensor.dim() != want or (channels > 1 and (tensor.shape[2] != channels or tensor.stride(2) != 1)) or \
            tensor.stride(1) != channels:
        raise ValueError(f"expected a tensor of shape [h, w{', %d' % channels if channels > 1 else ''}] with contiguous rows, "
                         f"got shape {tuple(tensor.shape)} strides {tuple(tensor.stride())}")
    im = abi.Image()
    im.data = tensor.data_ptr()
    im.height, im.width = int(tensor.shape[0]), int(tensor.shape[1])
    im.pitch_bytes = int(tensor.stride(0)) * tensor.element_size() if im.height > 1 else im.width * abi.TEXEL_BYTES[fmt]
    im.format = fmt
    return im


PRESENT_FORMAT_NAMES = {"rgba8": abi.SZG_FORMAT_RGBA8_UNORM, "bgra8": abi.SZG_FORMAT_BGRA8_UNORM,
                        "a2b10g10r10": abi.SZG_FORMAT_A2B10G10R10_UNORM}


def parse_present_option(text):
    """'WxH[:format]' (the examples' --present switch) -> (width, height, szg_format); format defaults to rgba8."""
    extent, _, name = text.partition(":")
    w, _, h = extent.lower().partition("x")
    name = name or "rgba8"
    if not (w.isdigit() and h.isdigit() and int(w) > 0 and int(h) > 0) or name not in PRESENT_FORMAT_NAMES:
        raise ValueError(f"{text!r}: expected WxH[:{'|'.join(PRESENT_FORMAT_NAMES)}]")
    return int(w), int(h), PRESENT_FORMAT_NAMES[name]


def swapchain_image(width, height, fmt=abi.SZG_FORMAT_RGBA8_UNORM, device="cuda:0"):
    """A tensor in the layout of a swapchain image of `fmt`: uint8 [h, w, 4] for the 8-bit formats, int32 [h, w] for
    A2B10G10R10_UNORM. What record_copy_image_to_image / record_present take as destination."""
    if fmt == abi.SZG_FORMAT_A2B10G10R10_UNORM:
        return torch.zeros((int(height), int(width)), dtype=torch.int32, device=device)
    return torch.zeros((int(height), int(width), 4), dtype=torch.uint8, device=device)


def write_presented_ppm(path, presented, fmt):
    """A swapchain image on the host (numpy uint8 [h, w, 4] or int32 [h, w]) as a binary PPM of its R, G, B: maxval 255, or
    1023 (two bytes per sample, most significant first) for A2B10G10R10_UNORM."""
    h, w = presented.shape[:2]
    with open(path, "wb") as f:
        if fmt == abi.SZG_FORMAT_A2B10G10R10_UNORM:
            word = presented.view(np.uint32)
            rgb = np.stack([word & 0x3FF, (word >> 10) & 0x3FF, (word >> 20) & 0x3FF], axis=-1)
            f.write(f"P6 {w} {h} 1023\n".encode())
            f.write(rgb.astype(">u2").tobytes())
        else:
            order = [2, 1, 0] if fmt == abi.SZG_FORMAT_BGRA8_UNORM else [0, 1, 2]
            f.write(f"P6 {w} {h} 255\n".encode())
            f.write(np.ascontiguousarray(presented[..., order]).tobytes())


def present_images(source, destination, dstFormat=None):
    """(szg_image of the RGBA16_UNORM source, szg_image of the destination). `source`: a SceneTexture or an int16 / uint16
    tensor [h, w, 4]. `destination`: a uint8 tensor [h, w, 4] (RGBA8_UNORM, or BGRA8_UNORM with dstFormat) or an int32
    tensor [h, w] (A2B10G10R10_UNORM)."""
    color = source.color if isinstance(source, SceneTexture) else source
    if color.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
        raise ValueError(f"the source must hold 16-bit codes, got {color.dtype}")
    src = _strided_image(color, abi.SZG_FORMAT_RGBA16_UNORM, 4)
    if destination.dtype == torch.uint8:
        fmt = abi.SZG_FORMAT_RGBA8_UNORM if dstFormat is None else int(dstFormat)
        if fmt not in (abi.SZG_FORMAT_RGBA8_UNORM, abi.SZG_FORMAT_BGRA8_UNORM):
            raise ValueError(f"a uint8 destination is RGBA8_UNORM or BGRA8_UNORM, not format {fmt}")
        dst = _strided_image(destination, fmt, 4)
    elif destination.dtype == torch.int32:
        if dstFormat not in (None, abi.SZG_FORMAT_A2B10G10R10_UNORM):
            raise ValueError(f"an int32 destination is A2B10G10R10_UNORM, not format {dstFormat}")
        dst = _strided_image(destination, abi.SZG_FORMAT_A2B10G10R10_UNORM, 1)
    else:
        raise ValueError(f"the destination must be uint8 [h, w, 4] or int32 [h, w], got {destination.dtype}")
    return src, dst


def record_copy_image_to_image(cmd, source, destination, srcRegion=None, dstRegion=None, filter=abi.SZG_FILTER_LINEAR,
                               encode=abi.SZG_PRESENT_ENCODE_NONE, dstFormat=None):
    """imageoperations.cpp:87-119 (LINEAR, the VkRect2D form) and :141-176 (filter=SZG_FILTER_NEAREST, the form behind
    Image::recordCopyEntire / recordCopyRect): blit `srcRegion` of the RGBA16_UNORM `source` onto `dstRegion` of
    `destination`, scaling and converting the format by the rule of include/szg/present.h. Regions are abi.Rect or
    (x, y, width, height), offsets honoured; None is the whole image. `encode` applies a transfer function to the taps and
    leaves the source linear."""
    src, dst = present_images(source, destination, dstFormat)
    info = abi.PresentInfo()
    info.src_region = _as_rect(srcRegion) if srcRegion is not None else abi.Rect(0, 0, src.width, src.height)
    info.dst_region = _as_rect(dstRegion) if dstRegion is not None else abi.Rect(0, 0, dst.width, dst.height)
    info.filter = int(filter)
    info.encode = int(encode)
    check(lib().szg_record_present(_stream_handle(cmd), C.byref(src), C.byref(dst), C.byref(info)))


def record_present(cmd, sceneTexture, sourceSubregion, swapchainImage, gammaFunction=abi.SZG_OETF_SRGB, encodeInBlit=False,
                   dstFormat=None):
    """What Editor::endFrame records after the frame is drawn (editor.cpp:303-361): the OETF in place over the top-left
    DESTINATION extent of the scene texture (the reference dispatches it over the swapchain extent, not over
    sourceSubregion: editor.cpp:328-337; kept on purpose, clamped to the texture as the shader's stores are), then the LINEAR
    blit of `sourceSubregion` onto the whole `swapchainImage`. With encodeInBlit the transfer function is applied to the
    blit's taps instead and the scene texture keeps its linear values (12 B/px at 1:1 instead of 16 + 12)."""
    src, dst = present_images(sceneTexture, swapchainImage, dstFormat)
    if encodeInBlit:
        encode = int(gammaFunction)
    else:
        encode = abi.SZG_PRESENT_ENCODE_NONE
        check(lib().szg_record_oetf(_stream_handle(cmd), C.byref(src), min(dst.width, src.width), min(dst.height, src.height),
                                    int(gammaFunction)))
    info = abi.PresentInfo(_as_rect(sourceSubregion), abi.Rect(0, 0, dst.width, dst.height), abi.SZG_FILTER_LINEAR, encode)
    check(lib().szg_record_present(_stream_handle(cmd), C.byref(src), C.byref(dst), C.byref(info)))


# ---------------------------------------------------------------------------
# Image copy and clear of the texture viewer (include/szg/texture_display.h)
# ---------------------------------------------------------------------------
_UINT16 = getattr(torch, "uint16", torch.int16)


def _tensor_format(tensor, fmt=None, srgb=False):
    """The szg_format of an [h, w, 4] tensor: uint8 is RGBA8_UNORM (RGBA8_SRGB with `srgb`), int16 / uint16 RGBA16_UNORM,
    float16 RGBA16_SFLOAT; `fmt` names it explicitly and must fit the element size."""
    if tensor.dtype == torch.uint8:
        natural = abi.SZG_FORMAT_RGBA8_SRGB if srgb else abi.SZG_FORMAT_RGBA8_UNORM
    elif tensor.dtype in (torch.int16, _UINT16):
        natural = abi.SZG_FORMAT_RGBA16_UNORM
    elif tensor.dtype == torch.float16:
        natural = abi.SZG_FORMAT_RGBA16_SFLOAT
    else:
        raise ValueError(f"an image holds uint8, 16-bit codes or float16, got {tensor.dtype}")
    if fmt is None:
        return natural
    if abi.TEXEL_BYTES.get(int(fmt)) != 4 * tensor.element_size():
        raise ValueError(f"format {fmt} does not fit a tensor of {tensor.dtype}")
    return int(fmt)


def _any_image(image, fmt=None, srgb=False):
    if isinstance(image, abi.Image):  # an image the library owns (a G-buffer plane): described already
        return image
    color = image.color if isinstance(image, SceneTexture) else image
    return _strided_image(color, _tensor_format(color, fmt, srgb), 4)


def record_copy_image(cmd, source, destination, srcRegion=None, dstRegion=None, srgb=False, srcFormat=None):
    """Image::recordCopyEntire / recordCopyRect (image.cpp:185-229 -> imageoperations.cpp:141-176): the NEAREST blit of
    `srcRegion` of `source` onto `dstRegion` of the float16 [h, w, 4] `destination` (RGBA16_SFLOAT), scaling and converting by
    the rule of include/szg/texture_display.h. `source`: uint8 (RGBA8_UNORM, or RGBA8_SRGB with `srgb`), int16 / uint16
    (RGBA16_UNORM) or float16 [h, w, 4], a SceneTexture, or an abi.Image (a plane of DeferredShadingPipeline.gbuffer()). Regions are abi.Rect or (x, y, width, height), offsets honoured;
    None is the whole image."""
    src = _any_image(source, srcFormat, srgb)
    dst = _any_image(destination)
    sr = _as_rect(srcRegion) if srcRegion is not None else abi.Rect(0, 0, src.width, src.height)
    dr = _as_rect(dstRegion) if dstRegion is not None else abi.Rect(0, 0, dst.width, dst.height)
    check(lib().szg_record_copy_image(_stream_handle(cmd), C.byref(src), C.byref(dst), sr, dr))


def record_clear_color_image(cmd, image, color=(0.0, 0.0, 0.0, 1.0)):
    """recordClearColorImage (rendercommands.cpp:25): every texel of the float16 (RGBA16_SFLOAT) or int16 / uint16
    (RGBA16_UNORM) [h, w, 4] tensor or SceneTexture becomes `color`; row padding keeps its bytes."""
    im = _any_image(image)
    check(lib().szg_record_clear_color_image(_stream_handle(cmd), C.byref(im), (C.c_float * 4)(*[float(v) for v in color])))


# ---------------------------------------------------------------------------
# Compute-collection pipeline (include/szg/compute_collection.h)
# ---------------------------------------------------------------------------
CCMember =namedtuple("CCMember", "name offsetBytes sizeBytes paddedSizeBytes componentType vectorWidth columnCount")
CCPushConstant = namedtuple("CCPushConstant", "name sizeBytes paddedSizeBytes layoutOffsetBytes localSize members")


def compute_collection_reflection():
    """The reflection tables of the library (szg_compute_collection_reflect), one CCPushConstant per program in the order
    of renderer.cpp:238-243: what ShaderReflectionData::PushConstant gives the editor. Needs no device."""
    out = []
    for index in range(lib().szg_compute_collection_shader_count()):
        r = abi.CCReflection()
        check(lib().szg_compute_collection_reflect(index, C.byref(r)))
        members = tuple(CCMember(m.name.decode(), m.offset_bytes, m.size_bytes, m.padded_size_bytes, m.component_type,
                                 m.vector_width, m.column_count) for m in r.members[: r.member_count])
        out.append(CCPushConstant(r.name.decode(), r.size_bytes, r.padded_size_bytes, r.layout_offset_bytes,
                                  tuple(r.local_size), members))
    return out


def record_compute_collection(cmd, shaderIndex, pushConstantBytes, color, width, height):
    """szg_record_compute_collection over a torch tensor: `color` is a SceneTexture or an int16 / uint16 tensor [h, w, 4]
    whose rows may be padded (the pitch is the row stride). The bytes are copied before the call returns."""
    tensor = color.color if isinstance(color, SceneTexture) else color
    if tensor.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
        raise ValueError(f"the colour image must hold 16-bit codes, got {tensor.dtype}")
    im = _strided_image(tensor, abi.SZG_FORMAT_RGBA16_UNORM, 4)
    raw = bytes(pushConstantBytes)
    check(lib().szg_record_compute_collection(_stream_handle(cmd), int(shaderIndex), raw, len(raw), C.byref(im), int(width),
                                              int(height)))


class ComputeCollectionPipeline:
    """pipelines.hpp:166-235: "a generic compute pipeline driven entirely by a push constant". Holds one byte block per
    program, zeros at first (pipelines.cpp:255-257), which survive a switch of program; recordDrawCommands copies the current
    one, overwrites its first 16 bytes with the draw extent (pipelines.cpp:330-344) and dispatches. No device work here."""

    def __init__(self):
        self._reflection = compute_collection_reflection()
        self._pushConstants = [bytearray(r.paddedSizeBytes) for r in self._reflection]
        self._shaderIndex = 0

    def recordDrawCommands(self, cmd, sceneTexture, drawExtent):
        """pipelines.cpp:291-368. `drawExtent` is (width, height) or an abi.Rect (its extent is taken, as the reference takes
        sceneSubregion.extent)."""
        if isinstance(drawExtent, abi.Rect):
            drawExtent = (drawExtent.width, drawExtent.height)
        record_compute_collection(cmd, self._shaderIndex, self._pushConstants[self._shaderIndex], sceneTexture,
                                  drawExtent[0], drawExtent[1])

    def mapPushConstantBytes(self):
        """The current program's block, writable in place (a bytearray)."""
        return self._pushConstants[self._shaderIndex]

    def readPushConstantBytes(self):
        return bytes(self._pushConstants[self._shaderIndex])

    def selectShader(self, index):
        """An index outside the table is a warning and leaves the selection where it was (as the reference's selectShader does)."""
        if not 0 <= int(index) < len(self._reflection):
            import warnings

            warnings.warn(f"selectShader({index}): the collection has {len(self._reflection)} programs, selection unchanged")
            return
        self._shaderIndex = int(index)

    def selectShaderByName(self, name):
        names = [r.name for r in self._reflection]
        if name not in names:
            raise ValueError(f"{name!r}: expected one of {names}")
        self._shaderIndex = names.index(name)

    def shaderIndex(self):
        return self._shaderIndex

    def shaderCount(self):
        return len(self._reflection)

    def shaders(self):
        """The reflection of every program (ShaderObjectReflected::reflectionData)."""
        return list(self._reflection)

    def currentShader(self):
        return self._reflection[self._shaderIndex]

    def writePushConstant(self, name, values):
        """Write `values` into member `name` of the current block: floats, or for a bool member 32-bit words (true = 1).
        A mat4 takes its 16 floats column by column."""
        member = next((m for m in self.currentShader().members if m.name == name), None)
        if member is None:
            raise KeyError(f"{self.currentShader().name} has no member {name!r}")
        count = member.vectorWidth * member.columnCount
        values = list(values)
        if len(values) != count:
            raise ValueError(f"{name}: {count} values expected, got {len(values)}")
        dtype = np.uint32 if member.componentType == abi.SZG_CC_COMPONENT_BOOL else np.float32
        raw = np.asarray(values, dtype=dtype).tobytes()
        assert len(raw) == member.sizeBytes
        self._pushConstants[self._shaderIndex][member.offsetBytes: member.offsetBytes + member.sizeBytes] = raw

    def writeExampleValues(self):
        """The visible block of abi.COMPUTE_COLLECTION_EXAMPLE_VALUES for the current program."""
        for name, values in abi.COMPUTE_COLLECTION_EXAMPLE_VALUES[self.currentShader().name].items():
            self.writePushConstant(name, values)

    def cleanup(self):
        pass


def parse_pipeline_option(text):
    """'deferred' or 'compute-collection[:NAME]' (the examples' --pipeline switch) -> (name, shader name or None)."""
    kind, _, shader = text.partition(":")
    if kind == "deferred" and not shader:
        return "deferred", None
    if kind == "compute-collection" and (not shader or shader in abi.COMPUTE_COLLECTION_EXAMPLE_VALUES):
        return "compute-collection", shader or "gradient_color"
    raise ValueError(f"{text!r}: expected deferred or compute-collection[:{'|'.join(abi.COMPUTE_COLLECTION_EXAMPLE_VALUES)}]")


class DeferredShadingPipeline:
    """deferred.hpp:23-119."""

    def __init__(self, dimensionCapacity, max_spot_lights=16, max_shadow_maps=10, shadow_map_dim=0, device_index=0):
        desc = abi.DeferredDesc(int(dimensionCapacity[0]), int(dimensionCapacity[1]), int(max_spot_lights),
                                int(max_shadow_maps), int(shadow_map_dim), 0)
        handle = C.c_void_p()
        check(lib().szg_deferred_create(C.byref(handle), C.byref(desc), int(device_index)))
        self._h = handle
        self.capacity = (int(dimensionCapacity[0]), int(dimensionCapacity[1]))

    def recordDrawCommands(self, cmd, drawRect, sceneTexture, atmosphericDirectionalLightsCount, directionalLights, spotLights,
                           viewCameraIndex, cameras, sceneGeometry, tile=None):
        """deferred.hpp:34-44. `spotLights` is a ctypes array (host span) of SpotLightPacked,
        `sceneGeometry` an abi.FillScene or None (keep the G-buffer as it is)."""
        st = sceneTexture.abi()
        n_spot = len(spotLights) if spotLights is not None else 0
        spots = C.cast(spotLights, C.POINTER(abi.SpotLightPacked)) if n_spot else None
        check(lib().szg_deferred_record_draw_commands(
            self._h, _stream_handle(cmd), drawRect, C.byref(tile) if tile is not None else None, C.byref(st),
            int(atmosphericDirectionalLightsCount), C.c_void_p(directionalLights.deviceAddress()),
            int(directionalLights.deviceSize()), spots, n_spot, int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()),
            C.byref(sceneGeometry) if sceneGeometry is not None else None))

    def recordGBufferFill(self, cmd, drawRect, sceneTexture, viewCameraIndex, cameras, sceneGeometry, tile=None):
        st = sceneTexture.abi()
        check(lib().szg_deferred_record_gbuffer_fill(
            self._h, _stream_handle(cmd), drawRect, C.byref(tile) if tile is not None else None, C.byref(st),
            int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()), C.byref(sceneGeometry)))

    def recordLights(self, cmd, drawRect, sceneTexture, atmosphericDirectionalLightsCount, directionalLights, spotLights,
                     viewCameraIndex, cameras, tile=None):
        st = sceneTexture.abi()
        n_spot = len(spotLights) if spotLights is not None else 0
        spots = C.cast(spotLights, C.POINTER(abi.SpotLightPacked)) if n_spot else None
        check(lib().szg_deferred_record_lights(
            self._h, _stream_handle(cmd), drawRect, C.byref(tile) if tile is not None else None, C.byref(st),
            int(atmosphericDirectionalLightsCount), C.c_void_p(directionalLights.deviceAddress()),
            int(directionalLights.deviceSize()), spots, n_spot, int(viewCameraIndex), C.c_void_p(cameras.deviceAddress())))

    def recordShadowMaps(self, cmd, directionalLights, spotLights, sceneGeometry):
        """render the pipeline-owned shadow maps for the analytic scene."""
        n_spot = len(spotLights) if spotLights is not None else 0
        spots = C.cast(spotLights, C.POINTER(abi.SpotLightPacked)) if n_spot else None
        check(lib().szg_deferred_record_shadow_maps(self._h, _stream_handle(cmd), C.c_void_p(directionalLights.deviceAddress()),
                                                    int(directionalLights.deviceSize()), spots, n_spot, C.byref(sceneGeometry)))

    # -- real scene geometry (include/szg/raster.h); `meshes` is a list of syzygy_amd.meshes.MeshInstanced
    def recordGBufferRaster(self, cmd, drawRect, sceneTexture, viewCameraIndex, cameras, meshes, tile=None, device="cuda"):
        """The G-buffer pass of recordDrawCommands (deferred.cpp:493-713) through the compute rasteriser."""
        from .meshes import mesh_array

        st = sceneTexture.abi()
        arr = mesh_array(meshes, device)
        check(lib().szg_deferred_record_gbuffer_raster(
            self._h, _stream_handle(cmd), drawRect, C.byref(tile) if tile is not None else None, C.byref(st),
            int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()), arr, len(meshes)))

    def recordShadowRaster(self, cmd, directionalLights, spotLights, meshes, device="cuda"):
        """The shadow passes (shadowpass.cpp:188-270) into the pipeline-owned maps."""
        from .meshes import mesh_array

        n_spot = len(spotLights) if spotLights is not None else 0
        spots = C.cast(spotLights, C.POINTER(abi.SpotLightPacked)) if n_spot else None
        arr = mesh_array(meshes, device)
        check(lib().szg_deferred_record_shadow_raster(self._h, _stream_handle(cmd), C.c_void_p(directionalLights.deviceAddress()),
                                                      int(directionalLights.deviceSize()), spots, n_spot, arr, len(meshes)))

    def recordDrawCommandsMeshes(self, cmd, drawRect, sceneTexture, atmosphericDirectionalLightsCount, directionalLights, spotLights,
                                 viewCameraIndex, cameras, meshes, tile=None, device="cuda"):
        """deferred.hpp:34-44 with `sceneGeometry` = real meshes: shadow raster, G-buffer raster, lights."""
        from .meshes import mesh_array

        st = sceneTexture.abi()
        n_spot = len(spotLights) if spotLights is not None else 0
        spots = C.cast(spotLights, C.POINTER(abi.SpotLightPacked)) if n_spot else None
        arr = mesh_array(meshes, device)
        check(lib().szg_deferred_record_draw_commands_meshes(
            self._h, _stream_handle(cmd), drawRect, C.byref(tile) if tile is not None else None, C.byref(st),
            int(atmosphericDirectionalLightsCount), C.c_void_p(directionalLights.deviceAddress()),
            int(directionalLights.deviceSize()), spots, n_spot, int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()),
            arr, len(meshes)))

    def setTextureMips(self, entries, max_lod=abi.SZG_SAMPLER_MAX_LOD_NONE):
        """szg_deferred_set_texture_mips: `entries` = [(level0, chain, level_count)], level0 and chain CUDA tensors (kept alive
        by the pipeline until the table is replaced) or device addresses; an empty list clears the table. `max_lod` is the
        sampler's maxLod: abi.SZG_SAMPLER_MAX_LOD_REFERENCE (1.0, what the reference's sampler has) or _NONE."""
        entries = list(entries)
        table = (abi.TextureMips * max(len(entries), 1))()
        for i, (level0, chain, levels) in enumerate(entries):
            table[i].level0_data = level0.data_ptr() if hasattr(level0, "data_ptr") else level0
            table[i].d_chain = (chain.data_ptr() or None) if hasattr(chain, "data_ptr") else chain
            table[i].level_count = int(levels)
        check(lib().szg_deferred_set_texture_mips(self._h, table if entries else None, len(entries), float(max_lod)))
        self._mip_keep = entries

    def setSamplerAnisotropy(self, max_anisotropy):
        """szg_deferred_set_sampler_anisotropy (include/szg/anisotropy.h): the sampler's maxAnisotropy, 1.0 (the reference's, and
        a new pipeline's) to 16.0; it applies to every map with a registered chain of more than one level."""
        check(lib().szg_deferred_set_sampler_anisotropy(self._h, float(max_anisotropy)))

    def gbuffer(self):
        return lib().szg_deferred_gbuffer(self._h).contents

    def shadowMaps(self):
        return lib().szg_deferred_shadow_maps(self._h).contents

    def setShadowMap(self, index, tensor):
        """Attach a caller-owned D32F map (2-D float32 CUDA tensor whose rows may be padded: the pitch is the row stride) to
        slot `index`, or detach with None."""
        if tensor is None:
            check(lib().szg_deferred_set_shadow_map(self._h, int(index), None))
            return
        if tensor.dtype != torch.float32:
            raise ValueError(f"a shadow map holds float32 depths, got {tensor.dtype}")
        im = _strided_image(tensor, abi.SZG_FORMAT_D32_SFLOAT, 1)
        check(lib().szg_deferred_set_shadow_map(self._h, int(index), C.byref(im)))

    def debugLightTileMasks(self, cmd=None):
        """include/szg/light_tiles.h: the mask words the last lights pass with spot lights wrote, as a uint64 array
        [tiles_y, tiles_x, batches] (bit i of word b set: the tile visits light record 64 b + i); None before any such pass."""
        tx, ty, nb = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().szg_deferred_debug_light_tile_masks(self._h, _stream_handle(cmd), None, 0, C.byref(tx), C.byref(ty), C.byref(nb)))
        n = tx.value * ty.value * nb.value
        if n == 0:
            return None
        words = np.zeros(n, dtype=np.uint64)
        check(lib().szg_deferred_debug_light_tile_masks(self._h, _stream_handle(cmd), words.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                        C.byref(tx), C.byref(ty), C.byref(nb)))
        return words.reshape(ty.value, tx.value, nb.value)

    def getConfiguration(self):
        cfg = abi.DeferredConfiguration()
        check(lib().szg_deferred_get_configuration(self._h, C.byref(cfg)))
        return cfg

    def setConfiguration(self, cfg):
        check(lib().szg_deferred_set_configuration(self._h, C.byref(cfg)))

    def cleanup(self):
        if self._h:
            lib().szg_deferred_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    # -- helpers to move G-buffer planes between host numpy arrays and the device
    def upload_gbuffer(self, planes):
        """planes: dict name -> numpy array [h, w, 4] (float16 planes / float32 position)."""
        g = self.gbuffer()
        names = {"diffuse": g.diffuse, "specular": g.specular, "normal": g.normal, "worldPosition": g.worldPosition,
                 "occlusionRoughnessMetallic": g.occlusionRoughnessMetallic}
        for name, im in names.items():
            arr = np.ascontiguousarray(planes[name])
            h, w = arr.shape[0], arr.shape[1]
            src = torch.from_numpy(arr.view(np.uint8).reshape(h, -1)).cuda()
            _memcpy2d_to(im, src, h)

    def download_gbuffer(self, width, height):
        g = self.gbuffer()
        out = {}
        for name, im, dt in (("diffuse", g.diffuse, np.float16), ("specular", g.specular, np.float16),
                             ("normal", g.normal, np.float16), ("worldPosition", g.worldPosition, np.float32),
                             ("occlusionRoughnessMetallic", g.occlusionRoughnessMetallic, np.float16)):
            raw = _memcpy2d_from(im, width * abi.TEXEL_BYTES[im.format], height)
            out[name] = raw.cpu().numpy().view(dt).reshape(height, width, 4)
        return out


class _RawDeviceArray:
    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 3,
                                         "strides": None}


def _alias_tensor(ptr, shape):
    return torch.as_tensor(_RawDeviceArray(ptr, shape), device="cuda")


def _hip_memcpy2d(dst_ptr, dpitch, src_ptr, spitch, width_bytes, height):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.restype = C.c_int
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    rc = hip.hipMemcpy2D(dst_ptr, dpitch, src_ptr, spitch, width_bytes, height, 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy2D failed: {rc}")


def _memcpy2d_to(im, src, rows):
    _hip_memcpy2d(im.data, im.pitch_bytes, src.data_ptr(), src.shape[1], src.shape[1], rows)


def _memcpy2d_from(im, width_bytes, rows):
    out = torch.empty((rows, width_bytes), dtype=torch.uint8, device="cuda")
    _hip_memcpy2d(out.data_ptr(), width_bytes, im.data, im.pitch_bytes, width_bytes, rows)
    return out


class SkyViewComputePipeline:
    """skyview.hpp:24-51. Use `create()`; it returns None on failure like the reference
    (skyview.cpp:713-740)."""

    def __init__(self, handle, desc):
        self._h = handle
        self.desc = desc

    @staticmethod
    def create(device_index=0, transmittance_extent=(512, 128), skyview_extent=(2048, 1024), flags=0):
        desc = abi.SkyviewDesc(int(transmittance_extent[0]), int(transmittance_extent[1]), int(skyview_extent[0]),
                               int(skyview_extent[1]), int(flags), 0)
        handle = C.c_void_p()
        status = lib().szg_skyview_create(C.byref(handle), C.byref(desc), int(device_index))
        if status != abi.SZG_OK:
            return None
        return SkyViewComputePipeline(handle, desc)

    def recordDrawCommands(self, cmd, sceneTexture, drawRect, gbuffer, shadowMaps, atmosphereIndex, atmospheres,
                           viewCameraIndex, cameras, sunLightIndex, lights, tile=None):
        """skyview.hpp:39-51: transmittance LUT -> sky-view LUT -> camera composite."""
        st = sceneTexture.abi()
        check(lib().szg_skyview_record_draw_commands(
            self._h, _stream_handle(cmd), C.byref(st), drawRect, C.byref(tile) if tile is not None else None,
            C.byref(gbuffer), C.byref(shadowMaps) if shadowMaps is not None else None, int(atmosphereIndex),
            C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()),
            int(sunLightIndex), C.c_void_p(lights.deviceAddress())))

    def recordTransmittance(self, cmd, atmosphereIndex, atmospheres):
        check(lib().szg_skyview_record_transmittance(self._h, _stream_handle(cmd), int(atmosphereIndex),
                                                     C.c_void_p(atmospheres.deviceAddress())))

    def recordSkyViewLUT(self, cmd, atmosphereIndex, atmospheres, viewCameraIndex, cameras):
        check(lib().szg_skyview_record_skyview_lut(self._h, _stream_handle(cmd), int(atmosphereIndex),
                                                   C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex),
                                                   C.c_void_p(cameras.deviceAddress())))

    def recordSkyViewLUTRows(self, cmd, atmosphereIndex, atmospheres, viewCameraIndex, cameras, rowBegin, rowEnd):
        """Multi-GPU extension: texel rows [rowBegin, rowEnd) only (see rowtile.allgather_skyview_lut)."""
        check(lib().szg_skyview_record_skyview_lut_rows(self._h, _stream_handle(cmd), int(atmosphereIndex),
                                                        C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex),
                                                        C.c_void_p(cameras.deviceAddress()), int(rowBegin), int(rowEnd)))

    def lutRowSlice(self, rank, nranks):
        """[begin, end) rows of the sky-view LUT that `rank` of `nranks` computes (szg_skyview_lut_row_slice)."""
        b, e = C.c_uint32(), C.c_uint32()
        check(lib().szg_skyview_lut_row_slice(self._h, int(rank), int(nranks), C.byref(b), C.byref(e)))
        return int(b.value), int(e.value)

    def setLUTReuse(self, enable):
        """Extension (abi.h "LUT reuse across frames"): skip a LUT pass whose parameter blocks are bit-equal to those its
        texels were computed from; compared on the device, identical results. Off by default (the reference recomputes)."""
        check(lib().szg_skyview_set_lut_reuse(self._h, 1 if enable else 0))

    def invalidateLUTs(self, which=abi.SZG_LUT_TRANSMITTANCE | abi.SZG_LUT_SKYVIEW):
        """The caller wrote texels of these LUTs through a pointer / tensor it kept (abi.h szg_skyview_invalidate_luts)."""
        check(lib().szg_skyview_invalidate_luts(self._h, int(which)))

    def skyviewLUT_tensor(self):
        """The sky-view LUT memory the C library owns, aliased (zero copy) as a torch float32 tensor
        [height, width, 4] through __cuda_array_interface__."""
        im = self.skyviewLUT()
        return _alias_tensor(im.data, (im.height, im.width, 4))

    def recordComposite(self, cmd, sceneTexture, drawRect, gbuffer, shadowMaps, atmosphereIndex, atmospheres, viewCameraIndex,
                        cameras, sunLightIndex, lights, tile=None):
        st = sceneTexture.abi()
        check(lib().szg_skyview_record_composite(
            self._h, _stream_handle(cmd), C.byref(st), drawRect, C.byref(tile) if tile is not None else None,
            C.byref(gbuffer), C.byref(shadowMaps) if shadowMaps is not None else None, int(atmosphereIndex),
            C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()),
            int(sunLightIndex), C.c_void_p(lights.deviceAddress())))

    def recordMultiScatterLUT(self, cmd, atmosphereIndex, atmospheres):
        """Extension (no reference counterpart, abi.h): multi-scattering LUT, one wavefront per texel."""
        check(lib().szg_skyview_record_multiscatter_lut(self._h, _stream_handle(cmd), int(atmosphereIndex),
                                                        C.c_void_p(atmospheres.deviceAddress())))

    def multiScatterLUT(self):
        return self._lut(lib().szg_skyview_multiscatter_lut)

    def setMultiScattering(self, mode):
        """Extension (szg/multiscatter_sky.h): abi.SZG_MULTISCATTER_OFF (default: the reference's single scattering), _ADD
        (the sky-view and aerial LUT passes add the higher orders from the multi-scattering LUT) or _ONLY (those alone)."""
        check(lib().szg_skyview_set_multiscatter(self._h, int(mode)))

    def multiScattering(self):
        mode = C.c_uint32()
        check(lib().szg_skyview_get_multiscatter(self._h, C.byref(mode)))
        return int(mode.value)

    def recordAerialLUT(self, cmd, atmosphereIndex, atmospheres, viewCameraIndex, cameras, maxDistanceMm):
        """Extension (no reference counterpart, abi.h): aerial-perspective froxel LUT, exact texel values."""
        check(lib().szg_skyview_record_aerial_lut(self._h, _stream_handle(cmd), int(atmosphereIndex),
                                                  C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex),
                                                  C.c_void_p(cameras.deviceAddress()), C.c_float(maxDistanceMm)))

    def recordCompositeFast(self, cmd, sceneTexture, drawRect, gbuffer, shadowMaps, atmosphereIndex, atmospheres,
                            viewCameraIndex, cameras, sunLightIndex, lights, tile=None):
        """Extension: APPROXIMATE composite (aerial perspective from the froxel LUT). Never part of the parity frame."""
        st = sceneTexture.abi()
        check(lib().szg_skyview_record_composite_fast(
            self._h, _stream_handle(cmd), C.byref(st), drawRect, C.byref(tile) if tile is not None else None,
            C.byref(gbuffer), C.byref(shadowMaps) if shadowMaps is not None else None, int(atmosphereIndex),
            C.c_void_p(atmospheres.deviceAddress()), int(viewCameraIndex), C.c_void_p(cameras.deviceAddress()),
            int(sunLightIndex), C.c_void_p(lights.deviceAddress())))

    def aerialLUT(self):
        lum, tr = abi.Image(), abi.Image()
        check(lib().szg_skyview_aerial_lut(self._h, C.byref(lum), C.byref(tr)))
        return lum, tr

    def _lut(self, getter):
        im = abi.Image()
        check(getter(self._h, C.byref(im)))
        return im

    def transmittanceLUT(self):
        return self._lut(lib().szg_skyview_transmittance_lut)

    def skyviewLUT(self):
        return self._lut(lib().szg_skyview_skyview_lut)

    def download_lut(self, im):
        raw = _memcpy2d_from(im, im.width * 16, im.height)
        return raw.cpu().numpy().view(np.float32).reshape(im.height, im.width, 4)

    def upload_lut(self, im, array):
        arr = np.ascontiguousarray(array, dtype=np.float32).reshape(im.height, im.width * 4)
        src = torch.from_numpy(arr.view(np.uint8).reshape(im.height, -1)).cuda()
        _memcpy2d_to(im, src, im.height)

    def destroy(self):
        if self._h:
            lib().szg_skyview_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# pipelines.hpp:39-44
DrawResultsGraphics = namedtuple("DrawResultsGraphics", ["drawCalls", "verticesDrawn", "indicesDrawn"])


def _f(values, n):
    values = [float(v) for v in values]
    assert len(values) == n, values
    return (C.c_float * n)(*values)


class DebugLineGraphicsPipeline:
    """pipelines.hpp:238-268 over include/szg/debuglines.h: the debug-line pass as a HIP line rasteriser. The depth
    attachment of the reference is dropped (compare ALWAYS, a renderer-private image nothing reads)."""

    def __init__(self, vertexCapacity=abi.SZG_DEBUG_LINES_CAPACITY, device_index=0):
        handle = C.c_void_p()
        check(lib().szg_debug_lines_create(C.byref(handle), int(vertexCapacity), int(device_index)))
        self._h = handle
        self.vertexCapacity = int(vertexCapacity)

    def recordDrawCommands(self, cmd, lineWidth, drawRect, sceneTexture, cameraIndex, cameras, endpoints, tile=None):
        """pipelines.cpp:463-581: draws endpoints.deviceSize() vertices as a line list over the scene colour."""
        st = sceneTexture.abi()
        n = int(endpoints.deviceSize())
        check(lib().szg_debug_lines_record(
            self._h, _stream_handle(cmd), C.c_float(lineWidth), drawRect, C.byref(tile) if tile is not None else None,
            C.byref(st), int(cameraIndex), C.c_void_p(cameras.deviceAddress()), C.c_void_p(endpoints.deviceAddress()), n))
        return DrawResultsGraphics(1, n, n)

    def cleanup(self):
        if self._h:
            lib().szg_debug_lines_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


class DebugLines:
    """debuglines.hpp:22-68: the line list (a TStagedBuffer of VertexPacked, renderer.hpp:103 capacity), the switch and the
    width; the push* builders are the C restatements of debuglines.cpp:23-124 (szg/host.h). Pushing past the capacity
    raises, as TStagedBuffer.push does."""

    def __init__(self, capacity=abi.SZG_DEBUG_LINES_CAPACITY, device="cuda:0", device_index=0):
        self.vertices = TStagedBuffer(abi.VertexPacked, capacity, device)
        self.pipeline = DebugLineGraphicsPipeline(capacity, device_index)
        self.lastFrameDrawResults = DrawResultsGraphics(0, 0, 0)
        self.enabled = False
        self.lineWidth = abi.SZG_DEBUG_LINES_DEFAULT_WIDTH

    def clear(self):
        self.vertices.clearStaged()

    def _push(self, out):
        self.vertices.push(list(out))

    def push(self, start, end):
        out = (abi.VertexPacked * 2)()
        lib().szg_debug_lines_segment(_f(start, 3), _f(end, 3), out)
        self._push(out)

    def pushQuad(self, a, b, c, d):
        out = (abi.VertexPacked * 8)()
        lib().szg_debug_lines_quad(_f(a, 3), _f(b, 3), _f(c, 3), _f(d, 3), out)
        self._push(out)

    def pushRectangleAxes(self, center, extentA, extentB):
        out = (abi.VertexPacked * 8)()
        lib().szg_debug_lines_rectangle_axes(_f(center, 3), _f(extentA, 3), _f(extentB, 3), out)
        self._push(out)

    def pushRectangleOriented(self, center, orientation, extents):
        """`orientation` is a quaternion {x, y, z, w}."""
        out = (abi.VertexPacked * 8)()
        lib().szg_debug_lines_rectangle_oriented(_f(center, 3), _f(orientation, 4), _f(extents, 2), out)
        self._push(out)

    def pushBox(self, *args):
        """pushBox(center, orientation {x, y, z, w}, extents) or pushBox(abi.Transform, abi.AABB)."""
        out = (abi.VertexPacked * 48)()
        if len(args) == 2:
            parent, box = args
            lib().szg_debug_lines_box_transform(C.byref(parent), C.byref(box), out)
        else:
            center, orientation, extents = args
            lib().szg_debug_lines_box(_f(center, 3), _f(orientation, 4), _f(extents, 3), out)
        self._push(out)

    def recordCopy(self, cmd=None):
        self.vertices.recordCopyToDevice(cmd)

    def recordDraw(self, cmd, cameraIndex, sceneTexture, sceneSubregion, cameras, tile=None):
        """Renderer::recordDrawDebugLines (renderer.cpp:445-476): copy and draw only when enabled and the list is not empty."""
        self.lastFrameDrawResults = DrawResultsGraphics(0, 0, 0)
        if self.enabled and self.vertices.stagedSize() > 0:
            self.recordCopy(cmd)
            self.lastFrameDrawResults = self.pipeline.recordDrawCommands(cmd, self.lineWidth, sceneSubregion, sceneTexture,
                                                                         cameraIndex, cameras, self.vertices, tile)
        return self.lastFrameDrawResults

    def cleanup(self):
        self.pipeline.cleanup()


# ---------------------------------------------------------------------------
# UI layer pass (include/szg/ui_layer.h)
# ---------------------------------------------------------------------------
class TStagedArray(TStagedBuffer):
    """A TStagedBuffer staged from one numpy array of records (an ImVector's Data / Size) instead of a list of structs."""

    def __init__(self, dtype, capacity, device="cuda:0"):
        self.dtype = np.dtype(dtype)
        super().__init__(C.c_uint8 * self.dtype.itemsize, capacity, device)

    def stage(self, values):
        values = np.ascontiguousarray(values, self.dtype)
        if len(values) > self.capacity:
            raise ValueError("TStagedArray: staged size exceeds capacity")
        self._staged = values
        self._dirty = True

    def push(self, value):
        raise TypeError("TStagedArray is staged whole: stage(array)")

    def _stagedBytes(self):
        return self._staged.tobytes()


SceneViewport = namedtuple("SceneViewport", "focused texture renderedSubregion")  # uilayer.hpp:23-28
UIOutputImage = namedtuple("UIOutputImage", "texture renderedSubregion")  # uilayer.hpp:30-34


class UILayer:
    """uilayer.hpp:36-114, the part that is a render pass: the scene texture the renderer draws into, the output texture the
    frame is presented from, the textures the draw data may name, and recordDraw. Widgets, layout and ImGui itself are out of
    scope: the draw data comes from Dear ImGui in an engine, or from syzygy_amd.ui here.

    create() allocates both textures at `textureCapacity` (uilayer.cpp:285-328) and registers the scene texture with its own
    sampler, NEAREST / CLAMP_TO_BORDER with an opaque-black border (scenetexture.cpp:104-109, uilayer.cpp:318-322)."""

    def __init__(self, textureCapacity, triangleCapacity=1 << 16, commandCapacity=4096, device="cuda:0", device_index=0):
        w, h = (int(v) for v in textureCapacity)
        handle = C.c_void_p()
        check(lib().szg_ui_layer_create(C.byref(handle), int(triangleCapacity), int(commandCapacity), int(device_index)))
        self._h = handle
        self.triangleCapacity, self.commandCapacity = int(triangleCapacity), int(commandCapacity)
        self._vertices = TStagedArray(ui.DRAW_VERT, 3 * self.triangleCapacity, device)
        self._indices = TStagedArray(np.uint16, 3 * self.triangleCapacity, device)
        self._keep = {}  # handle -> the tensor whose memory the texture names
        self._scene = SceneTexture(w, h, device)
        self._output = SceneTexture(w, h, device)
        self._sceneHandle = self.addTexture(self._scene.color, abi.SZG_FILTER_NEAREST, abi.SZG_UI_ADDRESS_CLAMP_TO_BORDER)
        self._viewport = abi.Rect(0, 0, w, h)

    @classmethod
    def create(cls, textureCapacity, **kwargs):
        return cls(textureCapacity, **kwargs)

    def sceneTexture(self):
        return self._scene

    def outputTexture(self):
        return self._output

    def sceneTextureHandle(self):
        """m_imguiSceneTextureHandle: the ImTextureID of the scene viewport quad"""
        return self._sceneHandle

    def setSceneViewportExtent(self, width, height):
        """What the "Scene Viewport" window (statelesswidgets.cpp:868-885) measures: the content extent the scene is rendered
        at, clamped to the texture's capacity."""
        self._viewport = abi.Rect(0, 0, min(int(width), self._scene.width), min(int(height), self._scene.height))

    def sceneViewportUV(self):
        """statelesswidgets.cpp:868-885: uv_max = contentExtent / textureCapacity of the viewport quad"""
        return (0.0, 0.0), (self._viewport.width / self._scene.width, self._viewport.height / self._scene.height)

    def sceneViewport(self, forceFocus=False):
        """uilayer.cpp:412-448: {focused, texture, renderedSubregion}"""
        return SceneViewport(bool(forceFocus), self._scene, self._viewport)

    def addTexture(self, tensor, filter=abi.SZG_FILTER_LINEAR, address=abi.SZG_UI_ADDRESS_REPEAT):
        """ImGui_ImplVulkan_AddTexture: `tensor` is uint8 [h, w, 4] (RGBA8_UNORM) or int16 / uint16 [h, w, 4] (RGBA16_UNORM);
        returns the ImTextureID (an int) that draw commands name. The tensor is kept alive until removeTexture."""
        fmt = abi.SZG_FORMAT_RGBA8_UNORM if tensor.dtype == torch.uint8 else abi.SZG_FORMAT_RGBA16_UNORM
        if fmt == abi.SZG_FORMAT_RGBA16_UNORM and tensor.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
            raise ValueError(f"a texture holds 8- or 16-bit codes, got {tensor.dtype}")
        im = _strided_image(tensor, fmt, 4)
        out = C.c_void_p()
        check(lib().szg_ui_layer_add_texture(self._h, C.byref(im), abi.UISampler(int(filter), int(address)), C.byref(out)))
        self._keep[out.value] = tensor
        return out.value

    def addTextureView(self, tensor, format=None, filter=abi.SZG_FILTER_LINEAR, address=abi.SZG_UI_ADDRESS_REPEAT, swizzle=None):
        """ImGui_ImplVulkan_AddTexture of an image VIEW (include/szg/texture_display.h): `tensor` may also be float16
        [h, w, 4] (RGBA16_SFLOAT), `swizzle` is four abi.SZG_SWIZZLE_* values producing R, G, B, A (None: identity), applied to
        the filtered sample. Returns an ImTextureID like addTexture."""
        im = _strided_image(tensor, _tensor_format(tensor, format), 4)
        view = abi.UITextureView((abi.U32 * 4)(*[int(v) for v in swizzle])) if swizzle is not None else None
        out = C.c_void_p()
        check(lib().szg_ui_layer_add_texture_view(self._h, C.byref(im), abi.UISampler(int(filter), int(address)),
                                                  C.byref(view) if view is not None else None, C.byref(out)))
        self._keep[out.value] = tensor
        return out.value

    def removeTexture(self, handle):
        check(lib().szg_ui_layer_remove_texture(self._h, C.c_void_p(handle)))
        self._keep.pop(handle, None)

    def recordDraw(self, cmd, drawData, loadOp=abi.SZG_UI_LOAD_OP_CLEAR, clearColor=(0.0, 0.0, 0.0, 1.0)):
        """uilayer.cpp:513-572: the render area is (int32)DisplayPos, (uint32)DisplaySize (:536-545), the output texture is
        cleared to opaque black and the draw data drawn into it. `drawData`: a ui.DrawData (or what its flatten() returns).
        Returns UIOutputImage{texture, renderedSubregion}: what Editor::endFrame presents."""
        flat = drawData.flatten() if hasattr(drawData, "flatten") else drawData
        area = abi.Rect(int(flat.display_pos[0]), int(flat.display_pos[1]), int(flat.display_size[0]), int(flat.display_size[1]))
        self._vertices.stage(flat.vertices)
        self._indices.stage(flat.indices)
        self._vertices.recordCopyToDevice(cmd)
        self._indices.recordCopyToDevice(cmd)
        n = len(flat.commands)
        commands = (abi.UIDrawCmd * max(n, 1))()
        for dst, c in zip(commands, flat.commands):
            dst.clip_rect[:] = [float(v) for v in c.clip_rect]
            dst.texture = c.texture
            dst.vtx_offset, dst.idx_offset, dst.elem_count = int(c.vtx_offset), int(c.idx_offset), int(c.elem_count)
        dd = abi.UIDrawData()
        dd.display_pos[:] = [float(v) for v in flat.display_pos]
        dd.display_size[:] = [float(v) for v in flat.display_size]
        dd.framebuffer_scale[:] = [float(v) for v in flat.framebuffer_scale]
        dd.d_vertices, dd.vertex_count = self._vertices.deviceAddress(), len(flat.vertices)
        dd.d_indices, dd.index_count = self._indices.deviceAddress(), len(flat.indices)
        dd.commands, dd.command_count = commands, n
        out = _strided_image(self._output.color, abi.SZG_FORMAT_RGBA16_UNORM, 4)
        check(lib().szg_ui_layer_record_draw(self._h, _stream_handle(cmd), C.byref(out), area, int(loadOp), _f(clearColor, 4),
                                             C.byref(dd)))
        return UIOutputImage(self._output, area)

    def cleanup(self):
        if self._h:
            lib().szg_ui_layer_destroy(self._h)
            self._h = None
            self._keep = {}

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


class TextureDisplay:
    """ui/texturedisplay.cpp, the part that runs on the GPU (include/szg/texture_display.h): the Texture Viewer's display
    image, RGBA16_SFLOAT at `displaySize` (TEXTURE_MAX = 4096^2 in the editor, editor.cpp:47), cleared to opaque black at once
    as the reference's immediate submit does (:147-162) and registered with the layer NEAREST / CLAMP_TO_BORDER through a
    view with alpha ONE (:69-80, :104-120). select() is the blit of the picked texture onto the whole image
    (Image::recordCopyEntire, :164-195), clear() what picking "None" records. The list box, the search and the property table
    are out of scope: draw `handle` with ui.DrawList.add_image at imageSize()."""

    def __init__(self, uiLayer, displaySize=(4096, 4096), device="cuda:0"):
        w, h = (int(v) for v in displaySize)
        self._layer = uiLayer
        self.width, self.height = w, h
        self.image = torch.empty((h, w, 4), dtype=torch.float16, device=device)
        record_clear_color_image(None, self.image)
        torch.cuda.current_stream().synchronize()
        self.handle = uiLayer.addTextureView(self.image, filter=abi.SZG_FILTER_NEAREST, address=abi.SZG_UI_ADDRESS_CLAMP_TO_BORDER,
                                             swizzle=(abi.SZG_SWIZZLE_IDENTITY,) * 3 + (abi.SZG_SWIZZLE_ONE,))

    def select(self, cmd, tensor, srgb=False, format=None, srcRegion=None):
        """texturedisplay.cpp:164-195: `tensor` (an asset map, uint8 [h, w, 4], sRGB-encoded with `srgb`; or a 16-bit UNORM or
        float16 image of the frame; a SceneTexture; an abi.Image) stretched onto the whole display image; None is "None" and
        clears. `srcRegion` (Image::recordCopyRect) shows a part of an image allocated larger than what was drawn."""
        if tensor is None:
            return self.clear(cmd)
        record_copy_image(cmd, tensor, self.image, srcRegion=srcRegion, srgb=srgb, srcFormat=format)

    def clear(self, cmd):
        record_clear_color_image(cmd, self.image)

    def imageSize(self, contentWidth):
        """texturedisplay.cpp:291-295: (contentWidth, aspectRatio * contentWidth) with aspectRatio = width / height of the
        display image. The reference's expression, right for a square image only; kept."""
        return float(contentWidth), self.width / self.height * float(contentWidth)

    def cleanup(self):
        if self.handle is not None:
            self._layer.removeTexture(self.handle)
            self.handle = None
