"""Images allocated larger than the draw rect, as the reference allocates its scene texture and G-buffer (a capacity extent
of 4096^2, renderer.hpp:93-96, drawn into at the top-left drawExtent): a raw byte buffer [cap_h, pitch_bytes] per image, with
pitch_bytes >= cap_w * texel chosen per image, every byte a per-image sentinel before use. The sentinels are hostile when
read: geometry-looking poison in the G-buffer (diffuse alpha 1.0, NaN everywhere else), a NaN bit pattern in depth and
debug colour, a non-zero code in colour, the nearest possible occluder (1.0) in a shadow map's pitch padding - so a kernel
that reads one column or row too far, or walks rows with the wrong pitch, changes texels INSIDE the rect and fails the
comparison there, and one that writes too far is caught by assert_outside_untouched, pitch padding included.

numpy only until to_device() is called; tests/test_padded_images.py checks the masks without a GPU."""
import numpy as np

from syzygy_amd import abi

# texel layout per format: (component dtype, components)
LAYOUT = {
    abi.SZG_FORMAT_RGBA16_SFLOAT: (np.float16, 4),
    abi.SZG_FORMAT_RGBA32_SFLOAT: (np.float32, 4),
    abi.SZG_FORMAT_RGBA16_UNORM: (np.uint16, 4),
    abi.SZG_FORMAT_D32_SFLOAT: (np.float32, 1),
}

_NAN16 = np.array([0x7E5A], np.uint16).view(np.float16)[0]
_NAN32 = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]
# one texel of each sentinel, as bytes
POISON_DIFFUSE = np.array([_NAN16, _NAN16, _NAN16, np.float16(1.0)], np.float16).tobytes()  # alpha 1.0: "geometry here"
POISON_HALF = np.array([_NAN16] * 4, np.float16).tobytes()
POISON_FLOAT4 = np.array([_NAN32] * 4, np.float32).tobytes()
POISON_DEPTH = np.array([_NAN32], np.float32).tobytes()
POISON_COLOR = np.array([0xBEEF, 0x1234, 0xCAFE, 0x7777], np.uint16).tobytes()
NEAREST_OCCLUDER = np.array([1.0], np.float32).tobytes()  # reverse-Z: 1.0 is the near plane


def extent_of(rect):
    """(width, height) of an abi.Rect or a (width, height) pair."""
    return (int(rect.width), int(rect.height)) if isinstance(rect, abi.Rect) else (int(rect[0]), int(rect[1]))


def outside_mask(cap_w, cap_h, pitch_bytes, texel, rect):
    """bool [cap_h, pitch_bytes]: True for every byte that is not a texel of the top-left rect - the capacity texels right
    of it and below it, and the padding bytes of every row."""
    w, h = extent_of(rect)
    assert w <= cap_w and h <= cap_h and pitch_bytes >= cap_w * texel
    mask = np.ones((cap_h, pitch_bytes), bool)
    mask[:h, : w * texel] = False
    return mask


class PaddedImage:
    """One image of `cap_w` x `cap_h` texels with `pad` texels of row padding, filled with `sentinel` (the bytes of one
    texel). `host` is what the device buffer must hold wherever nobody was allowed to write; write_inside() updates both."""

    def __init__(self, fmt, cap_w, cap_h, pad, sentinel):
        self.fmt, self.cap_w, self.cap_h = fmt, int(cap_w), int(cap_h)
        self.texel = abi.TEXEL_BYTES[fmt]
        assert len(sentinel) == self.texel and any(sentinel)
        self.pitch_bytes = (self.cap_w + int(pad)) * self.texel
        self.host = np.tile(np.frombuffer(sentinel, np.uint8), (self.cap_h, self.cap_w + int(pad))).copy()
        assert self.host.shape == (self.cap_h, self.pitch_bytes)
        self.device = None

    # -- host side (numpy only)
    def outside_mask(self, rect):
        return outside_mask(self.cap_w, self.cap_h, self.pitch_bytes, self.texel, rect)

    def typed(self, raw, rect):
        """The [h, w, c] ([h, w] for depth) view of the draw rect of a byte array shaped like `host`."""
        w, h = extent_of(rect)
        dtype, c = LAYOUT[self.fmt]
        block = np.ascontiguousarray(raw[:h, : w * self.texel]).view(dtype)
        return block.reshape(h, w, c) if c > 1 else block.reshape(h, w)

    def changed_outside(self, raw, rect):
        """(row, byte column) of every byte outside `rect` where `raw` differs from the sentinel state."""
        assert raw.shape == self.host.shape and raw.dtype == np.uint8
        return np.argwhere((raw != self.host) & self.outside_mask(rect))

    # -- device side
    def to_device(self, torch):
        self.torch = torch
        self.device = torch.from_numpy(self.host.copy()).cuda()
        return self

    def write_inside(self, array):
        """Put `array` ([h, w, c] or [h, w], h x w <= capacity) into the top-left texels, on the host copy and the device."""
        a = np.ascontiguousarray(array)
        h, w = a.shape[:2]
        assert a.dtype.itemsize * (a.shape[2] if a.ndim == 3 else 1) == self.texel and w <= self.cap_w and h <= self.cap_h
        self.host[:h, : w * self.texel] = a.view(np.uint8).reshape(h, w * self.texel)
        if self.device is not None:
            self.device.copy_(self.torch.from_numpy(self.host))

    def image(self, width=None, height=None):
        """abi.Image over the device buffer; width / height default to the capacity."""
        return abi.Image(self.device.data_ptr(), self.cap_w if width is None else width, self.cap_h if height is None else height,
                         self.pitch_bytes, self.fmt)

    def read(self):
        self.torch.cuda.synchronize()
        return self.device.cpu().numpy()

    def inside(self, rect):
        return self.typed(self.read(), rect)

    def assert_outside_untouched(self, rect, what=""):
        bad = self.changed_outside(self.read(), rect)
        assert len(bad) == 0, (f"{what}: {len(bad)} bytes outside the {extent_of(rect)} draw rect of a {self.cap_w}x{self.cap_h} image "
                               f"(pitch {self.pitch_bytes}) changed, first (row, byte) {bad[:4].tolist()}")

    def assert_untouched(self, what=""):
        self.assert_outside_untouched((0, 0), what)


class PaddedScene:
    """Colour, depth and debug colour at a capacity extent, each with its own odd row padding."""

    def __init__(self, torch, cap_w, cap_h, pads=(3, 5, 1), debug=True):
        self.color = PaddedImage(abi.SZG_FORMAT_RGBA16_UNORM, cap_w, cap_h, pads[0], POISON_COLOR).to_device(torch)
        self.depth = PaddedImage(abi.SZG_FORMAT_D32_SFLOAT, cap_w, cap_h, pads[1], POISON_DEPTH).to_device(torch)
        self.debug = PaddedImage(abi.SZG_FORMAT_RGBA32_SFLOAT, cap_w, cap_h, pads[2], POISON_FLOAT4).to_device(torch) if debug else None

    def images(self):
        return {"color": self.color, "depth": self.depth, **({"debug_color": self.debug} if self.debug is not None else {})}

    def abi(self):
        st = abi.SceneTexture()
        st.color, st.depth = self.color.image(), self.depth.image()
        if self.debug is not None:
            st.debug_color = self.debug.image()
        return st


GBUFFER_PLANES = (  # (field of szg_gbuffer, format, sentinel)
    ("diffuse", abi.SZG_FORMAT_RGBA16_SFLOAT, POISON_DIFFUSE),
    ("specular", abi.SZG_FORMAT_RGBA16_SFLOAT, POISON_HALF),
    ("normal", abi.SZG_FORMAT_RGBA16_SFLOAT, POISON_HALF),
    ("worldPosition", abi.SZG_FORMAT_RGBA32_SFLOAT, POISON_FLOAT4),
    ("occlusionRoughnessMetallic", abi.SZG_FORMAT_RGBA16_SFLOAT, POISON_HALF),
)


class PaddedGBuffer:
    """A caller-built szg_gbuffer: five planes at a capacity extent, every plane with a different pitch."""

    def __init__(self, torch, cap_w, cap_h, pads=(7, 9, 11, 13, 15)):
        self.planes = {name: PaddedImage(fmt, cap_w, cap_h, pad, sentinel).to_device(torch)
                       for (name, fmt, sentinel), pad in zip(GBUFFER_PLANES, pads)}

    def write_inside(self, planes):
        for name, array in planes.items():
            self.planes[name].write_inside(array)

    def abi(self):
        g = abi.GBuffer()
        for name, im in self.planes.items():
            setattr(g, name, im.image())
        return g


def gbuffer_poison(cap_w, cap_h):
    """The G-buffer sentinels as typed arrays {field: [cap_h, cap_w, 4]}: what DeferredShadingPipeline.upload_gbuffer takes to
    poison the planes a pipeline owns (tight pitch at its capacity)."""
    out = {}
    for name, fmt, sentinel in GBUFFER_PLANES:
        dtype, c = LAYOUT[fmt]
        out[name] = np.tile(np.frombuffer(sentinel, dtype), (cap_h, cap_w, 1)).copy()
    return out
